"""The host side of the pointwise WAIC (literate_amd/waic.py, csrc/lr_waic.hip): the numpy restatement
tests/helpers/waic_ref.py on a case worked by hand, against the oracle's per-draw log-likelihoods under models 0, 2 and 3,
the flag rule, the compare arithmetic and its fingerprint refusals, the flag combinations the three CLIs refuse before
they touch the GPU, the plan and the argument errors of the C ABI (host arithmetic), and the new declarations."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import waic_ref
from oracle import literate_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)


def synthetic(n, n_bins, S, seed, t0=3.0):
    rng = np.random.default_rng(seed)
    ts = t0 - 1.0 + rng.random(n) * (n_bins + 1.5)
    te = ts + rng.random(n) * n_bins * 0.6 + 1e-3
    lam = 0.05 + rng.random((S, n_bins))
    mu = 0.05 + rng.random((S, n_bins))
    return ts, te, lam, mu


def test_hand_worked_two_bins_two_draws_three_lineages():
    # t0 = 0, bins [0, 1) and [1, 2).  Draw A: lam = mu = 1 (log 0, R = 2 per bin); draw B: lam = mu = 1/2 (log -ln 2, R = 1)
    ts = np.array([-1.0, 1.25, 0.5])          # born before the window | in bin 1 at fraction 1/4 | in bin 0 at 1/2
    te = np.array([0.5, 5.0, 1.5])            # dies in bin 0 at 1/2    | extant past the window   | dies in bin 1 at 1/2
    lam = np.array([[1.0, 1.0], [0.5, 0.5]])
    ref = waic_ref.waic(ts, te, 0.0, lam, lam.copy(), model=2)
    # lineage 0: only the death in bin 0 and half a bin of exposure:  A: 0 - 1        B: -ln 2 - 1/2
    # lineage 1: birth in bin 1, exposure 3/4 of it:                  A: 0 - 3/2      B: -ln 2 - 3/4
    # lineage 2: birth, death, one unit of exposure:                  A: 0 + 0 - 2    B: -2 ln 2 - 1
    want = np.array([[-1.0, -LN2 - 0.5], [-1.5, -LN2 - 0.75], [-2.0, -2 * LN2 - 1.0]])
    assert np.allclose(ref["L"], want, rtol=0, atol=4e-16)
    pw = ref["pointwise"]
    for i, (a, b) in enumerate(want):
        assert math.isclose(pw[i, 0], math.log((math.exp(a) + math.exp(b)) / 2), rel_tol=1e-15)
        assert math.isclose(pw[i, 1], (a + b) / 2, rel_tol=1e-15)
        assert math.isclose(pw[i, 2], (a - b) ** 2 / 2, rel_tol=1e-14)
    t = ref["totals"]
    elpd = pw[:, 0] - pw[:, 2]
    assert t[0] == 3 and t[1] == 0 and t[6] == 0
    assert math.isclose(t[2], pw[:, 0].sum()) and math.isclose(t[3], pw[:, 2].sum()) and math.isclose(t[4], elpd.sum())
    assert math.isclose(t[5], math.sqrt(3 * np.var(elpd, ddof=1))) and t[7] == pw[:, 2].max()
    # the error scale: |logB| + |logD| + the whole exposure rate, the larger of the two draws
    assert np.allclose(ref["A"], [4.0, 4.0, 4.0])
    assert np.allclose(ref["spread"], np.abs(want[:, 0] - want[:, 1]))
    ld = waic_ref.waic(ts, te, 0.0, lam, lam.copy(), model=2, dtype=np.longdouble)
    assert waic_ref.error_counts(pw, ld).max() < 4


@pytest.mark.parametrize("model", [0, 2])
def test_column_sums_are_the_oracles_log_likelihood(model):
    ts, te, lam, mu = synthetic(300, 7, 5, 11)
    br = np.array([4.0, 0.0, 2.5, 1.0, 0.0, 7.0, 3.0])             # two bins nobody lived in: their terms are zero
    L, A = waic_ref.matrix(ts, te, 3.0, lam, mu, model, br if model == 0 else None)
    for s in range(5):
        want = lo.per_lineage_loglik(ts, te, 3.0, lam[s], mu[s], model, br if model == 0 else None)
        assert math.isclose(L[:, s].sum(), want, rel_tol=1e-12), (s, L[:, s].sum(), want)
    if model == 0:
        # a lineage born and dead inside a k = 0 bin scores exactly 0 under every draw
        L0, _ = waic_ref.matrix(np.array([4.2]), np.array([4.7]), 3.0, lam, mu, 0, br)
        assert np.array_equal(L0, np.zeros((1, 5)))
    assert (A > 0).all()


def test_model_3_scores_extant_lineages_by_the_birth_process_alone():
    ts, te, lam, mu = synthetic(200, 6, 4, 5)
    end = 8.0
    ts, te = ts[ts < end - 0.01], te[ts < end - 0.01]
    te = np.minimum(te, end)
    extant = te >= end
    assert 10 < extant.sum() < len(ts) - 10
    L3, _ = waic_ref.matrix(ts, te, 3.0, lam, mu, 3, None, end_time=end)
    L2, _ = waic_ref.matrix(ts, te, 3.0, lam, mu, 2)
    assert np.array_equal(L3[~extant], L2[~extant])
    lo_b = 3.0 + np.arange(6.0)
    for s in range(4):
        for i in np.nonzero(extant)[0][:25]:
            ov = np.clip(np.minimum(te[i], lo_b + 1) - np.maximum(ts[i], lo_b), 0, None)
            b = int(np.floor(ts[i] - 3.0))
            want = (math.log(lam[s, b]) if 0 <= b < 6 else 0.0) - float(np.sum(ov * lam[s]))
            assert math.isclose(L3[i, s], want, rel_tol=1e-12, abs_tol=1e-14)


def test_longdouble_and_float64_bin_terms_agree():
    _, _, lam, mu = synthetic(1, 9, 3, 2)
    br = np.array([1.0, 0, 2, 3, 0, 5, 6, 7, 8])
    for model in (0, 2, 3):
        for s in range(3):
            a = waic_ref.bin_terms(lam[s], mu[s], model, br, np.float64)
            b = waic_ref.bin_terms(lam[s], mu[s], model, br, np.longdouble)
            for x, y in zip(a, b):
                assert np.allclose(x, y.astype(np.float64), rtol=4e-16, atol=1e-18)


def test_flag_rule_on_a_zero_and_a_nan_rate():
    ts = np.array([0.5, 1.5, 2.5, 0.25])
    te = np.array([1.5, 2.5, 2.75, 0.75])
    lam = np.full((3, 3), 0.5)
    mu = np.full((3, 3), 0.25)
    mu[1, 1] = 0.0            # draw 1: nobody can die in bin 1 - lineage 0 does (-inf)
    lam[2, 2] = np.nan        # draw 2: lineage 2 is born in bin 2, lineage 1 lives into it (nan through the exposure)
    ref = waic_ref.waic(ts, te, 0.0, lam, mu, model=2)
    assert ref["flagged"].tolist() == [True, True, True, False]
    assert np.isnan(ref["pointwise"][:3]).all() and np.isfinite(ref["pointwise"][3]).all()
    t = ref["totals"]
    assert t[0] == 1 and t[1] == 3 and np.isnan(t[5]) and t[2] == ref["pointwise"][3, 0] and t[7] == ref["pointwise"][3, 2]
    assert waic_ref.waic(ts[:3], te[:3], 0.0, lam, mu)["totals"][0] == 0


def _save(path, elpd, fp):
    np.savez(path, elpd=np.asarray(elpd, dtype=np.float64), fingerprint=np.asarray(fp, dtype=np.float64))


def test_compare_on_three_pointwise_files_and_its_refusals(tmp_path):
    from literate_amd import waic
    rng = np.random.default_rng(3)
    n = 40
    a = -1.0 - rng.random(n)
    b = a - 0.1 * rng.random(n)             # worse everywhere
    b[7] = np.nan                           # one flagged lineage
    fp = [n, 2.0, 9, 2, 123.5, 456.25]
    names = [str(tmp_path / ("%s_WAIC_pointwise.npz" % k)) for k in "abc"]
    _save(names[0], a, fp), _save(names[1], b, fp), _save(names[2], a, fp)
    rows = waic.compare(names)
    want = waic_ref.compare_rows(names, [a, b, a])
    assert [r["model"] for r in rows] == [r["model"] for r in want] == [names[0], names[2], names[1]]
    for r, w in zip(rows, want):
        for k in ("elpd_waic", "elpd_diff", "se_diff"):
            assert r[k] == w[k], (k, r, w)
    assert rows[0]["elpd_diff"] == 0.0 and rows[0]["se_diff"] == 0.0
    assert rows[1]["elpd_diff"] == 0.0 and rows[1]["se_diff"] == 0.0          # the identical model: exactly 0
    both = np.isfinite(b)
    d = b[both] - a[both]
    assert rows[2]["elpd_diff"] == float(d.sum()) < 0 and rows[2]["lineages_used"] == n - 1
    assert math.isclose(rows[2]["se_diff"], math.sqrt((n - 1) * np.var(d, ddof=1)), rel_tol=1e-14)
    text = waic.format_table(rows)
    assert text.splitlines()[0].split("\t") == waic.COMPARE_HEAD and len(text.splitlines()) == 4
    # every field of the fingerprint
    for k in range(6):
        other = list(fp)
        other[k] += 1
        _save(names[2], a if k else np.append(a, -1.0), other)
        with pytest.raises(ValueError, match="fingerprint mismatch \\(%s\\)" % waic.FINGERPRINT[k]):
            waic.compare(names)
    with pytest.raises(ValueError):
        waic.compare(names[:1])
    # the command line
    _save(names[2], a, fp)
    out = subprocess.run([sys.executable, "-m", "literate_amd.waic", names[1], names[0], "-o", str(tmp_path / "t.tsv")],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == 3 and lines[1].split("\t")[0] == names[0] and open(tmp_path / "t.tsv").read() == out.stdout
    assert float(lines[2].split("\t")[3]) == float(d.sum())
    _save(names[2], a, fp[:3] + [0] + fp[4:])
    out = subprocess.run([sys.executable, "-m", "literate_amd.waic", names[0], names[2]], capture_output=True, text=True,
                         cwd=ROOT, timeout=120)
    assert out.returncode != 0 and "fingerprint mismatch (model)" in out.stderr


def test_fingerprint_and_files(tmp_path):
    from literate_amd import waic
    ts, te = np.array([1.0, 1e16, -1e16, 0.5]), np.array([2.0, 3.0, 4.0, 5.5])
    fp = waic.fingerprint(ts, te, 1.0, 7, 2)
    assert fp.tolist() == [4.0, 1.0, 7.0, 2.0, 1.5, 14.5]                     # exact sums: any order of the lineages
    assert np.array_equal(fp, waic.fingerprint(ts[::-1], te[::-1], 1.0, 7, 2))
    assert waic.fingerprint_mismatch(fp, fp) is None
    pw = np.array([[-1.0, -1.5, 0.25], [np.nan] * 3])
    res = waic.WaicResult(10, 2, 1, 1, -1.0, 0.25, -1.25, float("nan"), 2.5, float("nan"), 0, 0.25, pw[:, 0] - pw[:, 2], pw, fp,
                          (512, 7, 1, 1), None)
    waic.write_files(str(tmp_path / "x"), res)
    head, row = [l.split("\t") for l in open(tmp_path / "x_WAIC.tsv").read().splitlines()]
    assert head == ["draws", "lineages", "lineages_used", "lineages_flagged", "lppd", "p_waic", "elpd_waic", "se_elpd", "waic",
                    "se_waic", "n_var_gt_0.4", "max_var"]
    assert row == ["10", "2", "1", "1", "-1.0", "0.25", "-1.25", "nan", "2.5", "nan", "0", "0.25"]
    z = np.load(tmp_path / "x_WAIC_pointwise.npz")
    assert np.array_equal(z["elpd"], [-1.25, np.nan], equal_nan=True) and np.array_equal(z["fingerprint"], fp)


def test_draws_follow_the_ppc_rule():
    from literate_amd import ppc
    for M, n in ((10, 4), (3, 50), (12345, 1000)):
        assert np.array_equal(ppc.draw_indices(M, n), waic_ref.draw_indices(M, n))


CLI_REFUSALS = [("LiteRateForward", ["--waic", "1.0"]), ("LiteRateForward", ["--waic", "-0.5"]),
                ("LiteRateForward", ["--waic", "0.2", "--waic_draws", "1"]),
                ("LiteRateForward", ["--waic", "0.2", "-model_BDI", "1"]),
                ("LiteRateForward", ["--waic", "0.2", "-pyrate_output"]),
                ("DDRate", ["--waic", "1.0"]), ("DDRate", ["--waic", "0.2", "--waic_draws", "1"]),
                ("DDRate", ["--waic", "0.2", "-rm_first_bin", "1"]),
                ("trend_rate", ["--waic", "-0.1"]), ("trend_rate", ["--waic", "0.2", "--waic_draws", "0"]),
                ("trend_rate", ["--waic", "0.2", "-rm_first_bin", "1"])]


@pytest.mark.parametrize("script,flags", CLI_REFUSALS)
def test_clis_refuse_before_the_gpu_is_touched(script, flags):
    code = ("import sys; sys.path.insert(0, %r)\nimport %s as cli\n"
            "try:\n    cli.main(['-d', 'no_such_file.tsv'] + %r)\nexcept SystemExit as e:\n"
            "    assert 'torch' not in sys.modules, 'torch was imported'\n    print('REFUSED', e)\n" % (ROOT, script, flags))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0 and "REFUSED --waic" in out.stdout, out.stdout + out.stderr


def test_parsers_take_the_flags_and_their_defaults():
    sys.path.insert(0, ROOT)
    import DDRate
    import LiteRateForward
    import trend_rate
    for cli in (LiteRateForward, DDRate, trend_rate):
        a = cli.build_parser().parse_args(["-d", "x"])
        assert a.waic == -1.0 and a.waic_draws == 1000
        a = cli.build_parser().parse_args(["-d", "x", "--waic", "0.25", "--waic_draws", "64"])
        assert a.waic == 0.25 and a.waic_draws == 64


def test_header_declares_and_binding_binds_the_new_entry_points():
    from literate_amd import _hip, build
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        text = f.read()
    for name, n_args in (("lr_waic_workspace_bytes", 4), ("lr_waic_plan", 5), ("lr_waic_pointwise", 16)):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert len(_hip.SIGNATURES[name][1]) == n_args
    assert "LR_WAIC_SLICES" in text and "lr_waic.hip" in build.SOURCES


def test_plan_and_argument_errors_need_no_device(monkeypatch):
    """the plan is host arithmetic on (n, n_bins, n_draws, model); every refusal comes before any device call"""
    import ctypes as C
    from literate_amd import _hip
    monkeypatch.delenv("LR_WAIC_SLICES", raising=False)
    lib = _hip.load()
    q = lib.lr_waic_workspace_bytes

    def plan(n, nb, S, model):
        out = (C.c_int32 * 4)()
        rc = lib.lr_waic_plan(n, nb, S, model, out)
        return rc if rc else tuple(out)

    tile, chunk, slices, tiles = plan(100000, 128, 1000, 2)
    assert tile == 512 and tiles == (100000 + 511) // 512 and chunk == 32768 // (2 * 130 * 16) and slices == 3
    assert plan(10 ** 7, 128, 1000, 2) == (512, chunk, 1, (10 ** 7 + 511) // 512)
    assert plan(1031, 20, 64, 3)[1] == 32768 // (4 * 22 * 16)                   # model 3: two table classes
    assert plan(2000, 4094, 8, 2)[1] == 1 and plan(2000, 2398, 8, 3)[1] == 1    # the largest tables: a draw at a time
    assert plan(5, 20, 3, 2)[2] == 1                                            # too few draws to slice
    monkeypatch.setenv("LR_WAIC_SLICES", "7")
    assert plan(100000, 128, 1000, 2)[2] == 7 and plan(5, 20, 3, 2)[2] == 3
    monkeypatch.delenv("LR_WAIC_SLICES")
    for bad, code in (((0, 20, 8, 2), _hip.LR_ERR_SIZE), ((10, 20, 1, 2), _hip.LR_ERR_SIZE), ((10, 0, 8, 2), _hip.LR_ERR_SIZE),
                      ((10, _hip.LR_MAX_BINS + 1, 8, 2), _hip.LR_ERR_SIZE), ((10, 2399, 8, 3), _hip.LR_ERR_SIZE),
                      ((10, 20, 8, 1), _hip.LR_ERR_MODEL), ((10, 20, 8, 4), _hip.LR_ERR_MODEL), ((10, 20, 8, -1), _hip.LR_ERR_MODEL)):
        assert q(*bad) == code and plan(*bad) == code, bad
    for nb, model in ((_hip.LR_MAX_BINS, 2), (_hip.LR_MAX_BINS + 1, 2), (_hip.LR_MAX_BINS, 0), (2398, 3), (2399, 3)):
        assert (q(10, nb, 8, model) > 0) == (lib.lr_bd_loglik_workspace_bytes(10, nb, 8, model) > 0)    # the same bin counts
    assert q(10, 20, 8, 2) > 0 and lib.lr_waic_plan(10, 20, 8, 2, None) == _hip.LR_ERR_NULL
    one = C.c_void_p(256)           # never dereferenced: the checks below all fail before a launch
    args = lambda **kw: [kw.get("ts", one), one, kw.get("n", 10), kw.get("t0", 3.0), kw.get("nb", 20), one, one, kw.get("S", 8),
                         kw.get("model", 2), kw.get("br", None), 0.0, one, one, kw.get("ws", one), kw.get("wsb", 1 << 30), None]
    f = lib.lr_waic_pointwise
    assert f(*args(ts=None)) == _hip.LR_ERR_NULL and f(*args(ws=None)) == _hip.LR_ERR_NULL
    assert f(*args(n=0)) == _hip.LR_ERR_SIZE and f(*args(S=1)) == _hip.LR_ERR_SIZE and f(*args(nb=5000)) == _hip.LR_ERR_SIZE
    assert f(*args(model=1, br=one)) == _hip.LR_ERR_MODEL and f(*args(model=7)) == _hip.LR_ERR_MODEL
    assert f(*args(model=0)) == _hip.LR_ERR_MODEL                               # model 0 without br_length
    assert f(*args(t0=3.5)) == _hip.LR_ERR_T0
    assert f(*args(wsb=q(10, 20, 8, 2) - 1)) == _hip.LR_ERR_WORKSPACE
