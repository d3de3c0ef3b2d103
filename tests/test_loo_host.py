"""The host side of PSIS-LOO (literate_amd/loo.py, csrc/lr_loo.hip): the numpy restatement tests/helpers/loo_ref.py on a
case worked by hand, its quantile function against scipy's, its fit on random generalized-Pareto samples, the tail-length
rule, the unsmoothed and the flagged rows, lppd against waic_ref's; the compare tool and its refusals, the flag combinations
the three CLIs refuse before they touch the GPU, the new declarations, the plan and the argument errors of the C ABI
(host arithmetic)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import loo_ref, waic_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_worked_row_of_25_draws_whose_tail_is_five_uniform_quantiles():
    # S = 25: M = min(floor(5), ceil(15)) = 5, m = 30 + floor(sqrt 5) = 32, q = floor(5/4 + 1/2) = 1.
    # Importance ratios exp(r): nineteen draws at 0.25, one at 0.55 (the cutoff: the largest outside the tail) and the tail
    # 0.6, 0.7, 0.8, 0.9, 1.0; rmax = 0, so x = ratio - 0.55 = (0.05, 0.15, 0.25, 0.35, 0.45): the quantiles at
    # p = 0.1 ... 0.9 of the uniform distribution on [0, 0.5], the generalized Pareto with k = -1, sigma = 0.5.
    ratios = np.array([0.25] * 19 + [0.55, 0.6, 0.7, 0.8, 0.9, 1.0])
    perm = np.random.default_rng(1).permutation(25)
    l = -np.log(ratios)[perm]
    row = loo_ref.psis_row(l)
    assert row["M"] == 5 and loo_ref.grid_points(5) == 32
    assert np.array_equal(perm[row["tail"]], [20, 21, 22, 23, 24]) and row["cutoff"] == math.log(0.55)
    # The grid: theta_j = 1/x_5 + (1 - sqrt(32 / (j - 1/2))) / (3 x_1).  j = 1: sqrt(64) = 8, theta_1 = 1/0.45 - 7/0.15 =
    # 2.2222 - 46.6667 = -44.4444; 1 - theta_1 x = (3.2222, 7.6667, 12.1111, 16.5556, 21): k_1 = the mean of their logarithms
    # = (1.17007 + 2.03688 + 2.49413 + 2.80673 + 3.04452) / 5 = 2.31046; ell_1 = 5 (log(44.4444 / 2.31046) - 2.31046 - 1)
    # = 5 (2.95679 - 3.31046) = -1.76836.
    x = [0.05, 0.15, 0.25, 0.35, 0.45]
    theta = [1 / x[4] + (1 - math.sqrt(32 / (j - 0.5))) / (3 * x[0]) for j in range(1, 33)]
    assert math.isclose(theta[0], 1 / 0.45 - 7 / 0.15, rel_tol=1e-15) and math.isclose(theta[0], -44.4444, rel_tol=1e-5)
    kj = [sum(math.log1p(-t * v) for v in x) / 5 for t in theta]
    ell = [5 * (math.log(-t / k) - k - 1) for t, k in zip(theta, kj)]
    assert math.isclose(kj[0], 2.31046, rel_tol=1e-5) and math.isclose(ell[0], -1.76836, rel_tol=1e-5)
    # j = 32: theta_32 = 2.2222 + (1 - 1.007905) / 0.15 = 2.16952 (below 1/x_5: every 1 - theta x stays positive),
    # k_32 = -1.29123, ell_32 = 4.05071, the largest of the grid; its weight is 0.17682 and the weighted mean of the grid is
    # theta^ = 0.963827.  Then k = mean log(1 - 0.963827 x) = -0.292281 and sigma = -k / theta^ = 0.303251; the prior step
    # reports (5 k + 5) / 15 = 0.235906.  (Five points do not pin down k = -1: the estimator is a posterior mean under a
    # prior that reaches far into k > -1.)
    w = [1 / sum(math.exp(b - a) for b in ell) for a in ell]
    theta_hat = sum(t * v for t, v in zip(theta, w))
    assert ell.index(max(ell)) == 31 and math.isclose(w[31], 0.17682, rel_tol=1e-4) and math.isclose(theta_hat, 0.963827, rel_tol=1e-6)
    k = sum(math.log1p(-theta_hat * v) for v in x) / 5
    sigma = -k / theta_hat
    assert math.isclose(k, -0.292281, rel_tol=1e-5) and math.isclose(sigma, 0.303251, rel_tol=1e-5)
    assert math.isclose(float(row["k_fit"]), k, rel_tol=1e-12) and math.isclose(float(row["sigma"]), sigma, rel_tol=1e-12)
    assert math.isclose(float(row["k"]), 0.235906, rel_tol=1e-5) and row["out"][1] == row["k"]
    # The five replaced ratios: sigma ((1 - p)^(-k) - 1) / k at p = 0.1, 0.3, 0.5, 0.7, 0.9 with -k = 0.292281:
    # 0.9^0.292281 = 0.969675 -> 0.303251 (1 - 0.969675) / 0.292281 = 0.031464;  0.7^... -> 0.102715;  0.5^... -> 0.190273;
    # 0.3^... -> 0.307782;  0.1^... -> 0.508209.  Plus exp(c) = 0.55 and the logarithm: -0.542207, -0.426615, -0.300736,
    # -0.153405 and log 1.058209 = +0.056578, which the rule caps at 0.
    want_lw = [-0.542207, -0.426615, -0.300736, -0.153405, 0.0]
    got = row["lw"][perm.argsort()][20:]
    assert np.allclose(got, want_lw, rtol=0, atol=2e-6) and got[4] == 0.0
    assert np.allclose(row["lw"][perm.argsort()][:20], np.log(ratios[:20]), rtol=0, atol=1e-15)          # the others: r - rmax
    # the outputs from these weights, by their definitions
    lw, ll = row["lw"], l
    elpd = math.log(sum(math.exp(a + b) for a, b in zip(ll, lw))) - math.log(sum(math.exp(b) for b in lw))
    wn = np.exp(lw) / np.exp(lw).sum()
    assert math.isclose(row["out"][0], elpd, rel_tol=1e-14) and math.isclose(row["out"][3], 1 / np.sum(wn ** 2), rel_tol=1e-14)
    assert math.isclose(row["out"][2], math.log(np.mean(np.exp(ll))), rel_tol=1e-14)
    ld = loo_ref.psis(l[None, :], np.longdouble)
    assert loo_ref.error_counts(loo_ref.psis(l[None, :])["pointwise"], ld).max() < 8


@pytest.mark.parametrize("k", [-0.4, 0.0, 0.3, 1.2])
def test_quantile_function_against_scipy(k):
    stats = pytest.importorskip("scipy.stats")
    p = np.concatenate(([1e-12, 1e-6], (np.arange(1, 96) - 0.5) / 95, [1 - 1e-6]))
    for sigma in (0.01, 1.0, 37.5):
        want = stats.genpareto.ppf(p, k, loc=0.0, scale=sigma)
        assert np.allclose(loo_ref.qgpd(p, k, sigma), want, rtol=1e-12, atol=0)
        assert np.allclose(loo_ref.qgpd(p.astype(np.longdouble), np.longdouble(k), np.longdouble(sigma)).astype(float), want, rtol=1e-12)


@pytest.mark.parametrize("k0", [-0.3, 0.2, 0.7, 1.2])
def test_fit_recovers_the_shape_of_generalized_pareto_samples(k0):
    N = 2000
    rng = np.random.default_rng(int(100 * (k0 + 1)))
    x = np.sort(loo_ref.qgpd(rng.random(N), k0, 2.5))
    k, sigma = loo_ref.gpdfit(x)
    bound = 4.0 * (1.0 + k0) / math.sqrt(N)                   # four asymptotic standard errors of the MLE
    assert abs(k - k0) <= bound, (k, k0, bound)
    assert abs(sigma / 2.5 - 1.0) < 0.2
    kl, sl = loo_ref.gpdfit(x.astype(np.longdouble))
    assert abs(float(kl) - k) < 1e-10 and abs(float(sl) - sigma) < 1e-10


def test_tail_length_rule_and_grid_points():
    want = {24: 4, 25: 5, 100: 20, 225: 45, 226: 45, 1000: 95, 8192: 272, 2: 0, 4: 0, 5: 1}
    for S, M in want.items():
        assert loo_ref.tail_length(S) == M == min(math.floor(0.2 * S), math.ceil(3 * math.sqrt(S))), S
    # (S = 225: both rules give 45; S = 226: floor(45.2) = 45 against ceil(45.1) = 46)
    assert [loo_ref.grid_points(M) for M in (4, 5, 45, 95, 272)] == [0, 32, 36, 39, 46]


def test_unsmoothed_rows_few_draws_and_identical_draws():
    rng = np.random.default_rng(2)
    for S in (2, 5, 24):
        out = loo_ref.psis(-rng.random((3, S)) * 5.0)
        assert np.isposinf(out["pointwise"][:, 1]).all() and out["totals"][8] == 3 and out["totals"][6] == out["totals"][7] == 0
        assert np.isnan(out["totals"][9])
        # raw importance sampling: elpd_loo = -log mean exp(-l), the harmonic-mean form
        L = -np.arange(1.0, S + 1.0)[None, :] / S
        o = loo_ref.psis(L)["pointwise"][0]
        assert math.isclose(o[0], -math.log(np.mean(np.exp(-L[0]))), rel_tol=1e-13)
    for S in (25, 100):
        L = np.full((2, S), -3.25)
        out = loo_ref.psis(L)
        pw = out["pointwise"]
        assert np.isposinf(pw[:, 1]).all() and np.array_equal(pw[:, 0], pw[:, 2]) and np.array_equal(pw[:, 0], [-3.25, -3.25])
        assert np.array_equal(pw[:, 3], [S, S]) and out["totals"][4] == 0.0 and out["totals"][8] == 2
    # a constant tail above a spread body: unsmoothed all the same
    l = np.concatenate((-np.linspace(0.0, 1.0, 20), np.full(5, -2.0)))
    assert np.isposinf(loo_ref.psis_row(l)["k"])


def test_flag_rule_and_lppd_equal_to_waic_refs():
    ts = np.array([0.5, 1.5, 2.5, 0.25])
    te = np.array([1.5, 2.5, 2.75, 0.75])
    lam = np.full((30, 3), 0.5) + np.random.default_rng(4).random((30, 3))
    mu = np.full((30, 3), 0.25) + np.random.default_rng(5).random((30, 3))
    good = loo_ref.loo(ts, te, 0.0, lam, mu, model=2)
    w = waic_ref.waic(ts, te, 0.0, lam, mu, model=2)
    assert not good["flagged"].any() and np.array_equal(good["pointwise"][:, 2], w["pointwise"][:, 0])
    assert good["totals"][5] == w["totals"][2] and np.isfinite(good["pointwise"]).all()
    mu[1, 1] = 0.0            # draw 1: nobody can die in bin 1 - lineage 0 does (-inf)
    lam[2, 2] = np.nan        # draw 2: lineage 2 is born in bin 2, lineage 1 lives into it
    ref = loo_ref.loo(ts, te, 0.0, lam, mu, model=2)
    assert ref["flagged"].tolist() == [True, True, True, False]
    assert np.isnan(ref["pointwise"][:3]).all() and np.array_equal(ref["pointwise"][3], good["pointwise"][3])
    t = ref["totals"]
    assert t[0] == 1 and t[1] == 3 and np.isnan(t[3]) and t[2] == ref["pointwise"][3, 0] and t[5] == ref["pointwise"][3, 2]
    none = loo_ref.loo(ts[:3], te[:3], 0.0, lam, mu)["totals"]
    assert none[0] == 0 and none[1] == 3 and np.isnan(none[[2, 3, 4, 5, 9]]).all()


def test_smoothed_weights_stay_at_or_below_zero_and_the_tail_stays_sorted():
    rng = np.random.default_rng(6)
    for S, spread in ((25, 1.0), (100, 5.0), (1000, 0.3), (1000, 30.0), (1025, 3.0)):
        for heavy in (False, True):
            r = rng.exponential(size=S) * spread if heavy else rng.normal(size=S) * spread
            row = loo_ref.psis_row(-r)
            assert np.isfinite(row["k"]) and (row["lw"] <= 0.0).all()
            t = row["lw"][row["tail"]]
            assert (np.diff(t) >= 0.0).all()
            assert t[0] >= float(row["cutoff"] - r.max()) - 1e-12       # the tail starts at the cutoff, not below it
            body = np.setdiff1d(np.arange(S), row["tail"])
            assert np.array_equal(row["lw"][body], (r - r.max())[body])
            assert 1.0 <= row["out"][3] <= S and row["out"][0] <= row["out"][2] + 1e-12


def _save(path, elpd, fp, method="psis-loo", k=None):
    extra = {} if method is None else {"method": np.array(method)}
    np.savez(path, elpd=np.asarray(elpd, dtype=np.float64), fingerprint=np.asarray(fp, dtype=np.float64),
             pareto_k=np.zeros(len(elpd)) if k is None else np.asarray(k, dtype=np.float64), **extra)


def test_compare_ranking_and_its_refusals(tmp_path):
    from literate_amd import loo
    rng = np.random.default_rng(3)
    n = 40
    a = -1.0 - rng.random(n)
    b = a - 0.1 * rng.random(n)             # worse everywhere
    b[7] = np.nan                           # one flagged lineage
    kb = rng.random(n)
    kb[3], kb[7] = np.inf, np.nan
    fp = [n, 2.0, 9, 2, 123.5, 456.25]
    names = [str(tmp_path / ("%s_LOO_pointwise.npz" % k)) for k in "abc"]
    _save(names[0], a, fp), _save(names[1], b, fp, k=kb), _save(names[2], a, fp)
    with open(names[1][:-len("_pointwise.npz")] + ".tsv", "w") as f:
        f.write("\t".join(loo.TSV_HEAD) + "\n" + "\t".join(["10", "40", "39", "1", "-60.0", "1.0", "2.5", "-57.5", "120.0", "2.0", "0", "0", "1", "0.9"]) + "\n")
    rows = loo.compare(names)
    want = waic_ref.compare_rows(names, [a, b, a])
    assert [r["model"] for r in rows] == [r["model"] for r in want] == [names[0], names[2], names[1]]
    for r, w in zip(rows, want):
        assert r["elpd_loo"] == w["elpd_waic"] and r["elpd_diff"] == w["elpd_diff"] and r["se_diff"] == w["se_diff"]
    both = np.isfinite(b)
    d = b[both] - a[both]
    assert rows[2]["elpd_diff"] == float(d.sum()) < 0 and rows[2]["lineages_used"] == n - 1 and rows[2]["p_loo"] == 2.5
    assert math.isnan(rows[0]["p_loo"]) and rows[0]["n_k_gt_0.7"] == 0
    assert rows[2]["n_k_gt_0.7"] == int(np.sum(np.isfinite(kb) & (kb > 0.7)))
    text = loo.format_table(rows)
    assert text.splitlines()[0].split("\t") == ["model", "elpd_loo", "p_loo", "elpd_diff", "se_diff", "lineages_used", "n_k_gt_0.7"]
    assert len(text.splitlines()) == 4
    for k in range(6):
        other = list(fp)
        other[k] += 1
        _save(names[2], a if k else np.append(a, -1.0), other)
        with pytest.raises(ValueError, match="fingerprint mismatch \\(%s\\)" % loo.waic.FINGERPRINT[k]):
            loo.compare(names)
    with pytest.raises(ValueError):
        loo.compare(names[:1])
    # a WAIC file (no method), and a file of another method
    for method in (None, "waic"):
        _save(names[2], a, fp, method=method)
        with pytest.raises(ValueError, match="not a PSIS-LOO pointwise file"):
            loo.compare(names)
    np.savez(names[2], elpd=a, fingerprint=np.asarray(fp, dtype=np.float64))                  # exactly what waic.write_files leaves
    out = subprocess.run([sys.executable, "-m", "literate_amd.loo", names[0], names[2]], capture_output=True, text=True,
                         cwd=ROOT, timeout=120)
    assert out.returncode != 0 and "not a PSIS-LOO pointwise file" in out.stderr
    _save(names[2], a, fp)
    out = subprocess.run([sys.executable, "-m", "literate_amd.loo", names[1], names[0], "-o", str(tmp_path / "t.tsv")],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == 3 and lines[1].split("\t")[0] == names[0] and open(tmp_path / "t.tsv").read() == out.stdout
    assert float(lines[2].split("\t")[3]) == float(d.sum())


def test_files(tmp_path):
    from literate_amd import loo
    fp = loo.fingerprint(np.array([1.0, 0.5]), np.array([2.0, 5.5]), 1.0, 7, 2)
    pw = np.array([[-1.25, 0.75, -1.0, 12.5], [np.nan] * 4])
    res = loo.LooResult(30, 2, 1, 1, -1.25, float("nan"), 0.25, -1.0, 2.5, float("nan"), 1, 1, 0, 0.75, pw[:, 0], pw[:, 1], pw, fp,
                        (6, 32, 2, 1), None)
    loo.write_files(str(tmp_path / "x"), res)
    head, row = [l.split("\t") for l in open(tmp_path / "x_LOO.tsv").read().splitlines()]
    assert head == ["draws", "lineages", "lineages_used", "lineages_flagged", "elpd_loo", "se_elpd", "p_loo", "lppd", "looic",
                    "se_looic", "n_k_gt_0.5", "n_k_gt_0.7", "n_unsmoothed", "max_k"]
    assert row == ["30", "2", "1", "1", "-1.25", "nan", "0.25", "-1.0", "2.5", "nan", "1", "1", "0", "0.75"]
    z = np.load(tmp_path / "x_LOO_pointwise.npz")
    assert np.array_equal(z["elpd"], [-1.25, np.nan], equal_nan=True) and np.array_equal(z["pareto_k"], [0.75, np.nan], equal_nan=True)
    assert np.array_equal(z["fingerprint"], fp) and str(z["method"]) == "psis-loo"


def test_arg_error_rules():
    from literate_amd import loo, waic
    assert loo.arg_error(0.2, 1000) is None and loo.arg_error(0.0, 2) is None and loo.arg_error(0.5, 8192) is None
    for args, kw in (((1.0, 100), {}), ((-0.1, 100), {}), ((0.2, 1), {}), ((0.2, 8193), {}), ((0.2, 100), dict(model=1)),
                     ((0.2, 100), dict(rm_first_bin=True)), ((0.2, 100), dict(pyrate_output=True))):
        err = loo.arg_error(*args, **kw)
        assert err and err.startswith("--loo") and "waic" not in err, (args, kw, err)
        if args[1] <= 8192:
            assert waic.arg_error(*args, **kw)                  # the same rules refuse --waic
    assert "[2, 8192]" in loo.arg_error(0.2, 1) and "[2, 8192]" in loo.arg_error(0.2, 8193)


CLI_REFUSALS = [("LiteRateForward", ["--loo", "1.0"]), ("LiteRateForward", ["--loo", "-0.5"]),
                ("LiteRateForward", ["--loo", "0.2", "--loo_draws", "1"]),
                ("LiteRateForward", ["--loo", "0.2", "--loo_draws", "8193"]),
                ("LiteRateForward", ["--loo", "0.2", "-model_BDI", "1"]),
                ("LiteRateForward", ["--loo", "0.2", "-pyrate_output"]),
                ("LiteRateForward", ["--waic", "0.2", "--loo", "1.5"]),
                ("DDRate", ["--loo", "1.0"]), ("DDRate", ["--loo", "0.2", "--loo_draws", "1"]),
                ("DDRate", ["--loo", "0.2", "--loo_draws", "9000"]),
                ("DDRate", ["--loo", "0.2", "-rm_first_bin", "1"]),
                ("trend_rate", ["--loo", "-0.1"]), ("trend_rate", ["--loo", "0.2", "--loo_draws", "0"]),
                ("trend_rate", ["--loo", "0.2", "--loo_draws", "8193"]),
                ("trend_rate", ["--loo", "0.2", "-rm_first_bin", "1"])]


@pytest.mark.parametrize("script,flags", CLI_REFUSALS)
def test_clis_refuse_before_the_gpu_is_touched(script, flags):
    code = ("import sys; sys.path.insert(0, %r)\nimport %s as cli\n"
            "try:\n    cli.main(['-d', 'no_such_file.tsv'] + %r)\nexcept SystemExit as e:\n"
            "    assert 'torch' not in sys.modules, 'torch was imported'\n    print('REFUSED', e)\n" % (ROOT, script, flags))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0 and "REFUSED --loo" in out.stdout, out.stdout + out.stderr


def test_parsers_take_the_flags_and_their_defaults():
    sys.path.insert(0, ROOT)
    import DDRate
    import LiteRateForward
    import trend_rate
    for cli in (LiteRateForward, DDRate, trend_rate):
        a = cli.build_parser().parse_args(["-d", "x"])
        assert a.loo == -1.0 and a.loo_draws == 1000 and a.waic == -1.0
        a = cli.build_parser().parse_args(["-d", "x", "--loo", "0.25", "--loo_draws", "64", "--waic", "0.5"])
        assert a.loo == 0.25 and a.loo_draws == 64 and a.waic == 0.5 and a.waic_draws == 1000


def test_header_declares_and_binding_binds_the_new_entry_points():
    from literate_amd import _hip, build
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        text = f.read()
    for name, n_args in (("lr_loo_workspace_bytes", 4), ("lr_loo_plan", 5), ("lr_loo_pointwise", 16),
                         ("lr_psis_rows_workspace_bytes", 2), ("lr_psis_rows", 8)):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert len(_hip.SIGNATURES[name][1]) == n_args
    assert "LR_LOO_BATCH" in text and "lr_loo.hip" in build.SOURCES


def test_plan_and_argument_errors_need_no_device(monkeypatch):
    """the plan is host arithmetic on (n, n_bins, n_draws, model); every refusal comes before any device call"""
    import ctypes as C
    from literate_amd import _hip
    monkeypatch.delenv("LR_LOO_BATCH", raising=False)
    lib = _hip.load()
    q, qr = lib.lr_loo_workspace_bytes, lib.lr_psis_rows_workspace_bytes

    def plan(n, nb, S, model):
        out = (C.c_int32 * 4)()
        rc = lib.lr_loo_plan(n, nb, S, model, out)
        return rc if rc else tuple(out)

    # 64 MiB / (8 S) lineages per slab, whole tiles of 512: 8388 -> 8192 at 1000 draws, 1024 at the cap, 2097 -> 2048 at 4000
    assert plan(100000, 40, 1000, 2) == (95, 39, 8192, 13)
    assert plan(100000, 40, 4000, 2) == (190, 43, 2048, 49)
    assert plan(30000, 32, 8192, 3) == (272, 46, 1024, 30)
    assert plan(8388, 40, 1000, 2) == (95, 39, 8388, 1) and plan(8389, 40, 1000, 2) == (95, 39, 8192, 2)      # (one slab: no rounding)
    assert plan(5, 20, 2, 2) == (0, 0, 5, 1) and plan(5, 20, 24, 0) == (4, 0, 5, 1) and plan(5, 20, 25, 0) == (5, 32, 5, 1)
    for S in (2, 24, 25, 100, 225, 226, 1000, 1023, 1024, 1025, 8192):
        M, m = plan(7, 20, S, 2)[:2]
        assert M == loo_ref.tail_length(S) and m == loo_ref.grid_points(M), S
    monkeypatch.setenv("LR_LOO_BATCH", "300")
    assert plan(1031, 20, 64, 2) == (12, 33, 300, 4) and plan(200, 20, 64, 2) == (12, 33, 200, 1)
    small = q(1031, 20, 64, 2)
    monkeypatch.delenv("LR_LOO_BATCH")
    align = lambda v: (v + 255) // 256 * 256
    assert plan(1031, 20, 64, 2) == (12, 33, 1031, 1)
    assert q(1031, 20, 64, 2) - small == align(1031 * 64 * 8) - align(300 * 64 * 8)      # the slab is what a smaller batch saves
    for bad, code in (((0, 20, 8, 2), _hip.LR_ERR_SIZE), ((10, 20, 1, 2), _hip.LR_ERR_SIZE), ((10, 20, 8193, 2), _hip.LR_ERR_SIZE),
                      ((10, 0, 8, 2), _hip.LR_ERR_SIZE), ((10, _hip.LR_MAX_BINS + 1, 8, 2), _hip.LR_ERR_SIZE),
                      ((10, 2399, 8, 3), _hip.LR_ERR_SIZE), ((10, 20, 8, 1), _hip.LR_ERR_MODEL), ((10, 20, 8, 4), _hip.LR_ERR_MODEL),
                      ((10, 20, 8, -1), _hip.LR_ERR_MODEL)):
        assert q(*bad) == code and plan(*bad) == code, bad
    assert q(10, 20, 8192, 2) > 0 and q(10, _hip.LR_MAX_BINS, 25, 2) > 0 and q(10, 2398, 25, 3) > 0
    assert lib.lr_loo_plan(10, 20, 8, 2, None) == _hip.LR_ERR_NULL
    assert qr(10, 2) > 0 and qr(10, 8192) >= 10 * 272 * 4 and qr(0, 8) == qr(10, 1) == qr(10, 8193) == qr(2 ** 31, 8) == _hip.LR_ERR_SIZE
    one = C.c_void_p(256)           # never dereferenced: the checks below all fail before a launch
    args = lambda **kw: [kw.get("ts", one), one, kw.get("n", 10), kw.get("t0", 3.0), kw.get("nb", 20), one, one, kw.get("S", 8),
                         kw.get("model", 2), kw.get("br", None), 0.0, one, one, kw.get("ws", one), kw.get("wsb", 1 << 30), None]
    f = lib.lr_loo_pointwise
    assert f(*args(ts=None)) == _hip.LR_ERR_NULL and f(*args(ws=None)) == _hip.LR_ERR_NULL
    assert f(*args(n=0)) == _hip.LR_ERR_SIZE and f(*args(S=1)) == _hip.LR_ERR_SIZE and f(*args(S=8193)) == _hip.LR_ERR_SIZE
    assert f(*args(nb=5000)) == _hip.LR_ERR_SIZE
    assert f(*args(model=1, br=one)) == _hip.LR_ERR_MODEL and f(*args(model=7)) == _hip.LR_ERR_MODEL
    assert f(*args(model=0)) == _hip.LR_ERR_MODEL                               # model 0 without br_length
    assert f(*args(t0=3.5)) == _hip.LR_ERR_T0
    assert f(*args(wsb=q(10, 20, 8, 2) - 1)) == _hip.LR_ERR_WORKSPACE
    g = lib.lr_psis_rows
    rows = lambda **kw: [kw.get("L", one), kw.get("n", 10), kw.get("S", 30), one, kw.get("tot", one), kw.get("ws", one),
                         kw.get("wsb", 1 << 30), None]
    assert g(*rows(L=None)) == _hip.LR_ERR_NULL and g(*rows(tot=None)) == _hip.LR_ERR_NULL and g(*rows(ws=None)) == _hip.LR_ERR_NULL
    assert g(*rows(n=0)) == _hip.LR_ERR_SIZE and g(*rows(S=1)) == _hip.LR_ERR_SIZE and g(*rows(S=8193)) == _hip.LR_ERR_SIZE
    assert g(*rows(wsb=qr(10, 30) - 1)) == _hip.LR_ERR_WORKSPACE
