"""The host side of trend_rate.py's marginal likelihoods (literate_amd/trend_mlik.py, include/literate_hip_tmlik.h), no GPU:

  (a) the restatement tests/helpers/tmlik_ref.py at beta = 1, s = 1 and win = 0.001 IS oracle/trend_mcmc_oracle.run_trend_mcmc,
      row for row, on the golden statistics - on the Philox draws bit for bit, and on numpy's legacy draws against the rows the
      reference process wrote (tests/golden/trend_trajectories.npz);
  (b) run_vec with the window schedule on the shared problem gives, per model, |pooled log Z - truth| <= 4 REF_SD / sqrt(R) +
      1e-3, the truth by closed form (constant halves) and a 3-D quadrature (EXP halves) that agrees with itself to 1e-3
      between two grid sizes; REF_SD is this very run's sd over the replicates;
  (c) the argument checks, the model selection, the tuning rule, the file writers and the compare tool on multi-model and on
      single-model files; the header against the ctypes binding.
"""
import math
import os
import re

import numpy as np
import pytest

from helpers import mlik_ref
from helpers import tmlik_ref as H
from oracle import trend_mcmc_oracle as tro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden_problem():
    z = np.load(os.path.join(GOLDEN, "ratemaps.npz"))
    return H.Problem(z["N_SPEC"], z["N_EXTI"], z["DT"], z["TREND"])


# ---- (a) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cb,cd", [(False, False), (True, False), (False, True), (True, True)])
def test_a_the_restatement_at_beta_1_is_the_oracles_loop_on_the_philox_draws(cb, cd):
    P = golden_problem()
    n, seed, key = 400, 11, 5
    want = np.array([w[:12] for w in tro.run_trend_mcmc(P.n_spec, P.n_exti, P.DT, P.trends[0], tro.PhiloxDraws(seed, key), n, 1, cb, cd)])
    ch = H.Chain(P, 0, int(cb) + 2 * int(cd), 1.0, 1.0, 0.001)
    rows = H.run_chain(ch, tro.PhiloxDraws(seed, key), n, 1)
    assert rows.shape == (n, H.ROW_W)
    assert np.array_equal(rows[:, H.R_IT], want[:, 0]) and np.array_equal(rows[:, H.R_LIK], want[:, 2])
    assert np.array_equal(rows[:, H.R_PRIOR], want[:, 5]) and np.array_equal(rows[:, H.R_ARGS:H.R_ARGS + 6], want[:, 6:12])
    assert 0.2 * n < sum(ch.accepted) <= sum(ch.proposed) <= n and len(set(rows[:, H.R_LIK])) > 20
    # an additive step that fires for no slope is not counted: none of the null model's, about a quarter where both rates vary
    assert (sum(ch.proposed) == n) == (cb != cd) and (ch.proposed[1] == 0) == (cb and cd)


def test_a_and_the_reference_process_rows_on_numpys_legacy_draws():
    P = golden_problem()
    T = np.load(os.path.join(GOLDEN, "trend_trajectories.npz"))
    keys = sorted({k.split("/")[0] for k in T.files})
    assert len(keys) == 3
    for key in keys:
        cb, cd, seed, n, s = [int(v) for v in T[key + "/meta"]]
        np.random.seed(seed)
        ch = H.Chain(P, 0, cb + 2 * cd, 1.0, 1.0, 0.001)
        rows = H.run_chain(ch, tro.NumpyLegacyDraws(), n, s)
        head = T[key + "/head"]
        assert rows.shape[0] == head.shape[0]
        got = np.column_stack([rows[:, H.R_IT], rows[:, H.R_LIK], rows[:, H.R_PRIOR], rows[:, H.R_ARGS:H.R_ARGS + 6]])
        assert np.allclose(got, np.column_stack([head[:, 0], head[:, 2], head[:, 5], head[:, 6:12]]), rtol=1e-9, atol=1e-9), key


def test_a_the_power_posterior_and_the_windows_enter_where_the_header_says():
    """beta = 0 ignores the likelihood (a move that lowers it by any amount is judged by prior and hastings alone), the window
    scales the additive step and s the multiplier's exponent"""
    P = golden_problem()

    class Fixed:
        def __init__(self, rr):
            self.rr = rr

        def move(self, it):
            return self.rr

        def normal_vec(self, it, f, d):
            return np.array([0, 0, 1, 1, 0, 0]), np.full(6, -2.0) * d

        def multiplier(self, it, f):
            return np.array([1, 1, 0, 0, 1, 1]), np.full(6, 0.75)

        def accept(self, it):
            return 0.5
    a = H.Chain(P, 0, 0, 0.0, 1.0, 0.25)
    H.step(a, 1, Fixed(0.1))
    assert np.array_equal(a.args, [.1, .1, -.5, -.5, 1, 1]) and a.accepted == [0, 1]          # rates floored where t > 0.2
    b = H.Chain(P, 0, 0, 1.0, 1.0, 0.25)
    H.step(b, 1, Fixed(0.1))
    assert b.accepted == [0, 0] and b.proposed == [0, 1], "at beta = 1 the same step is judged by a likelihood that falls"
    c = H.Chain(P, 0, 0, 0.0, 3.0, 0.25)
    H.step(c, 1, Fixed(0.9))
    m = math.exp(3.0 * 2 * math.log(1.1) * 0.25)
    assert np.allclose(c.args, [.1 * m, .1 * m, 0, 0, m, m], rtol=1e-15) and c.proposed == [1, 0]


# ---- (b) --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth():
    fine, halves = H.shared_truth(161)
    coarse, _ = H.shared_truth(121)
    return fine, coarse, halves


def test_b_the_quadrature_agrees_with_itself_and_with_the_issues_figures(truth):
    fine, coarse, halves = truth
    assert np.max(np.abs(np.array(fine) - np.array(coarse))) < 1e-3
    for k, v in dict(birth_exp=-179.1910, death_exp=-96.6630, birth_const=-179.7245, death_const=-92.6059).items():
        assert abs(halves[k] - v) < 1e-3, (k, halves[k])
    # the constant half against a 1-d quadrature of its own
    r = np.linspace(.001, 3.0, 400001)
    f = 40.0 * np.log(r) - r * 300.0 - (r - .001) / 10.0 - math.log(10.0)
    w = np.full(len(r), r[1] - r[0])
    w[0] = w[-1] = w[0] / 2
    assert abs(np.logaddexp.reduce(f + np.log(w)) - H.const_half(40, 300.0)) < 1e-6


def test_b_the_tuned_sampler_finds_the_marginal_likelihoods_of_the_shared_problem(truth):
    fine, _, _ = truth
    P = H.shared_problem()
    betas = H.temperatures(H.T, H.ALPHA)
    scales = H.window_scales(betas, H.WIDEN)
    flags = np.array([int(b) + 2 * int(d) for _, b, d in H.MODELS])
    rows, wins, rate, burn = H.run_vec(P, [m[0] for m in H.MODELS], flags, betas, scales, H.R, H.N_IT, H.S_FREQ, H.BURN,
                                       np.random.default_rng(H.SEED))
    assert rows.shape == (3, 2000, H.R, H.T, H.ROW_W) and burn == 600
    for m in range(3):
        est = mlik_ref.estimate(rows[m], betas, burn)
        pooled, sd = est["pooled"][-1], float(np.std(est["ss"], ddof=1))
        print("%s: pooled %.4f, truth %.4f, sd over the replicates %.4f (REF_SD %.4f)" % (H.MODELS[m], pooled, fine[m], sd, H.REF_SD[m]))
        assert abs(sd - H.REF_SD[m]) < 5e-4, "REF_SD is this run's sd"
        assert abs(pooled - fine[m]) <= 4 * H.REF_SD[m] / math.sqrt(H.R) + 1e-3
    # the schedule: the null model is never tuned; the others end inside the clip's range with the additive move near 30 %
    assert np.all(wins[0] == 0.001)
    assert np.all(wins[1:] > 0.001) and np.all(wins[1:] < 20.0) and np.all(wins[1:, -1] < wins[1:, 0]) and np.isnan(rate[0, :, 1]).all()
    assert np.all(rate[1:, :, 1] >= 0.2) and np.all(rate[1:, :, 1] <= 0.5)
    assert np.array_equal(rows[:, burn:, :, :, H.R_WIN], np.broadcast_to(wins[:, None, None, :], rows[:, burn:, :, :, 0].shape))


# ---- (c) --------------------------------------------------------------------------------------------------------------------
def test_c_argument_checks_and_the_model_selection():
    from literate_amd import trend_mlik as tm
    ok = (0.3, 16, 8, 10000, 10, 0.3, 8.0)
    assert tm.arg_error(*ok) is None and tm.arg_error(*ok, n_bins=512, n_models=64) is None
    assert "512" in tm.arg_error(*ok, n_bins=513)
    assert "burn-in" in tm.arg_error(1.0, *ok[1:]) and "mlik_temps" in tm.arg_error(0.3, 1, *ok[2:])
    assert "mlik_reps" in tm.arg_error(0.3, 16, 0, *ok[3:]) and "samples" in tm.arg_error(0.3, 16, 8, 30, 10, 0.3, 8.0)
    assert "chains" in tm.arg_error(0.3, 128, 1 << 20, 10000, 10, 0.3, 8.0, n_models=64)
    assert tm.select_models("run", "run", 2, False, True, 4) == [(2, False, True)]
    assert tm.select_models("all", "run", 2, False, False, 3) == [(0, False, False), (1, False, False), (2, False, False)]
    assert tm.select_models("1,0", "all", 2, False, False, 3) == [(1, False, False), (1, False, True), (1, True, False),
                                                                 (0, False, False), (0, False, True), (0, True, False)]
    for bad in (("3", "run"), ("-1", "run"), ("x", "run"), ("run", "some")):
        with pytest.raises(ValueError):
            tm.select_models(bad[0], bad[1], 0, False, False, 3)
    assert tm.selection_error("all", "all") is None and tm.selection_error("run", "run", 3) is None and tm.selection_error("0,2", "all") is None
    assert "mlik_columns" in tm.selection_error("x", "run") and "mlik_columns" in tm.selection_error("1,-2", "run")
    assert "mlik_models" in tm.selection_error("all", "some")
    # the null is always there, once, and first; a run of the null alone is the null alone
    assert tm.with_null([(1, False, False), (2, True, True), (1, False, False)]) == [tm.NULL, (1, False, False)]
    assert tm.with_null([(5, True, True)]) == [tm.NULL]
    assert tm.group_size(2000, 16, 16, 1 << 30) == 21 and tm.group_size(10 ** 6, 16, 16, 1 << 30) == 1
    assert tm.group_size(10, 2, 2, 1 << 30) == tm.MAX_MODELS == 64


def test_c_the_tuning_rule():
    from literate_amd import trend_mlik as tm
    assert tm.tune_blocks(6000)[:3] == [0, 300, 600] and tm.tune_blocks(6000)[-1] == 6000 and len(tm.tune_blocks(6000)) == 21
    assert tm.tune_blocks(7) == H.tune_blocks(7) and sorted(set(tm.tune_blocks(7))) == list(range(8))
    win = np.array([[0.001, 0.5, 19.0], [0.001, 0.5, 19.0]])
    acc, prop = np.array([[0.0, 30.0, 100.0]] * 2), np.array([[100.0, 100.0, 100.0]] * 2)
    got = tm.tuned(win, acc, prop, 4, [True, False])
    assert np.array_equal(got[1], win[1]), "a model with both rates constant is never tuned"
    assert got[0, 0] == 0.001 and got[0, 1] == 0.5 and got[0, 2] == 20.0
    one = tm.tuned(win, np.full((2, 3), 50.0), prop, 1, [True, True])
    assert np.allclose(one, np.clip(win * math.exp(4 * 0.2), 0.001, 20.0))
    assert np.array_equal(tm.tuned(win, acc * 0, prop * 0, 1, [True, True]), win), "no proposal, no change"
    assert (tm.WIN0, tm.WIN_MIN, tm.WIN_MAX, tm.TUNE_BLOCKS) == (H.WIN0, H.WIN_MIN, H.WIN_MAX, H.TUNE_BLOCKS)


def _fake_result(tm, seed=0, fp=(5, 1, 2, 3, 4, 0)):
    rng = np.random.default_rng(seed)
    models = []
    for i, (col, cb, cd) in enumerate([tm.NULL, (1, False, False), (2, False, True)]):
        ss = -100.0 - 3.0 * ((i + seed) % 3) + rng.normal(size=4) * 0.1
        fit = {"model": tm.model_name(cb, cd), "column": col, "logZ_ss": float(ss.mean()), "logZ_ss_se": float(ss.std(ddof=1) / 2.0),
               "logZ_ti": float(ss.mean()) - 1.0, "min_lik_ess": 50.0, "accept_mult_min": 0.7, "accept_mult_max": 0.9,
               "accept_add_min": 0.25, "accept_add_max": float("nan") if cb and cd else 0.4}
        temps = [(j, j / 2.0, 1.0 + j, 0.001 * (i + 1), -50.0, 2.0, 40.0, 0.8, 0.3, float("nan") if j == 2 else -1.0) for j in range(3)]
        models.append(tm.ModelResult(col, cb, cd, fit["model"], fit, temps, ss, fit["logZ_ss"], np.full(3, 0.001 * (i + 1))))
    null = models[0]
    for r in models:
        r.fit["two_ln_bf"] = 2.0 * (r.fit["logZ_ss"] - null.fit["logZ_ss"])
        r.fit["two_ln_bf_se"] = 0.0 if r is null else 2.0 * math.hypot(r.fit["logZ_ss_se"], null.fit["logZ_ss_se"])
    settings = dict(temps=3, reps=4, iterations=100, s_freq=10, burnin=0.3, alpha=0.3, widen=8.0, bins=7, samples_kept=7)
    return tm.TrendMlikResult(models, np.array([0, .5, 1.]), np.ones(3), settings, np.array(fp, dtype=float))


def test_c_the_file_writers(tmp_path):
    from literate_amd import trend_mlik as tm
    res = _fake_result(tm)
    stem = str(tmp_path / "run_0")
    tm.write_tables(stem, res, names=["year", "gdp", "sales"])
    with open(stem + "_MLIK.tsv") as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("# logZ_ss") and "3 temperatures x 4 replicates" in lines[0] and lines[1].split("\t") == tm.FIT_HEAD
    fit = tm.read_fit(stem)
    assert len(fit) == 3 and [r["logZ_ss"] for r in fit] == sorted([r["logZ_ss"] for r in fit], reverse=True)
    by = {(r["model"], r["column"]): r for r in fit}
    assert by[("_CONB_COND", 0)]["two_ln_bf"] == 0.0 and by[("_CONB_COND", 0)]["column_name"] == "-"
    assert by[("_EXPB_EXPD", 1)]["column_name"] == "gdp" and by[("_EXPB_COND", 2)]["column_name"] == "sales"
    for r in res.models:
        for k in tm.FIT_HEAD[3:]:
            a, b = by[(r.name, r.col)][k], r.fit[k]
            assert a == b or (math.isnan(a) and math.isnan(b)), k
    with open(stem + "_MLIK_temps.tsv") as f:
        temps = [l.split("\t") for l in f.read().splitlines()]
    assert temps[0] == tm.TEMPS_HEAD and len(temps) == 1 + 3 * 3 and [t[0] for t in temps[1::3]] == [r["model"] for r in fit]
    assert float(temps[1][5]) in (0.001, 0.002, 0.003) and temps[3][-1] == "nan"
    with np.load(stem + "_MLIK.npz") as z:
        assert z["ss"].shape == (3, 4) and z["logZ_ss"].shape == (3,) and z["logZ_ss_se"].shape == (3,) and z["fingerprint"][0] == 5
        assert list(z["names"]) == [tm.label(r) for r in sorted(res.models, key=lambda r: -r.pooled)]
        assert np.array_equal(z["logZ_ss"], np.sort(z["logZ_ss"])[::-1]) and "_CONB_COND" in list(z["names"])


def test_c_a_constant_column_is_refused_by_name(tmp_path):
    from literate_amd import trend_mlik as tm
    from literate_amd.trendrate import normalise_trend
    path = str(tmp_path / "trend.tsv")
    with open(path, "w") as f:
        f.write("year\tgdp\tflat\n")
        for i in range(6):
            f.write("%d\t%g\t%g\n" % (i, (i - 2.5) ** 2, 3.0 if i < 5 else 4.0))
    with pytest.raises(ValueError, match=r"column 2 \(flat\)"):
        tm.read_trends(path, 0)
    trends, names = tm.read_trends(path, 0, cols=[1])
    assert names == ["year", "gdp", "flat"] and trends.shape == (3, 5) and np.all(trends[[0, 2]] == 1.0)
    assert np.array_equal(trends[1], normalise_trend([(i - 2.5) ** 2 for i in range(6)], 0)) and trends[1].min() == 1e-15
    assert np.array_equal(tm.read_trends(path, 1, cols=[0, 1])[0][1], normalise_trend([(i - 2.5) ** 2 for i in range(6)], 1))


def test_c_the_trend_file_is_checked_before_the_run_and_a_null_only_run_needs_no_column(tmp_path):
    from literate_amd import trend_mlik as tm
    path = str(tmp_path / "trend.tsv")
    with open(path, "w") as f:
        f.write("year\tgdp\tflat\n")
        for i in range(6):
            f.write("%d\t%g\t%g\n" % (i, (i - 2.5) ** 2, 3.0))
    # the run's own model is the null (-const_B -const_D, or -const_B -no_death): no column is read, not even a constant one
    for idx in (1, 2):
        trends, names, models = tm.read_selection(path, "run", "run", idx, True, True, 0)
        assert tm.with_null(models) == [tm.NULL] and trends.shape == (3, 5) and np.all(trends == 1.0) and names == ["year", "gdp", "flat"]
    assert tm.read_trends(path, 1, cols=[])[0].shape == (3, 4) and tm.read_trends(path, 0, cols=[])[1] == ["year", "gdp", "flat"]
    trends, names, models = tm.read_selection(path, "0,1", "all", 2, False, False, 0)
    assert len(models) == 6 and np.all(trends[2] == 1.0) and trends[1].min() == 1e-15 and trends[0].max() == 1.0
    for args, word in ((("run", "run", 2, False, False, 0), r"column 2 \(flat\)"), (("all", "run", 1, False, True, 0), r"column 2 \(flat\)"),
                       (("3", "run", 1, False, False, 0), "column 3 is not among the trend file's 3 columns"),
                       (("run", "run", 5, False, False, 0), "column 5 is not among")):
        with pytest.raises(ValueError, match=word):
            tm.read_selection(path, *args)
    with open(path, "w") as f:
        f.write("year\tgdp\n0\t1\n")
    with pytest.raises(ValueError, match="too few rows"):
        tm.read_selection(path, "run", "run", 1, True, True, 0)


def test_c_the_command_line_refuses_the_trend_file_before_the_run(tmp_path):
    """a column that is not there or is constant ends the command at once, on every rank, by name - not after the main run"""
    import subprocess
    import sys
    trend = str(tmp_path / "trend.tsv")
    with open(trend, "w") as f:
        f.write("year\tflat\n" + "".join("%d\t2.5\n" % i for i in range(8)))
    base = [sys.executable, os.path.join(ROOT, "trend_rate.py"), "-d", str(tmp_path / "none.tsv"), "-n", "100", "-s", "10", "--mlik", "0.3",
            "-trend_data", trend]
    for extra, word in ((["-trend_index", "1"], "column 1 (flat)"), (["-trend_index", "0", "--mlik_columns", "0,4"], "column 4 is not among"),
                        (["-trend_index", "0", "--mlik_columns", "all"], "column 1 (flat)")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and word in out.stderr and "Traceback" not in out.stderr and "TrendRate" not in out.stdout, out.stderr[-500:]
    out = subprocess.run(base[:-2] + ["-trend_data", str(tmp_path / "missing.tsv")], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and out.stderr.startswith("--mlik:") and "Traceback" not in out.stderr


def test_c_the_compare_tool_on_multi_model_and_single_model_files(tmp_path):
    from literate_amd import mlik
    from literate_amd import trend_mlik as tm
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    tm.write_tables(a, _fake_result(tm, 0))
    tm.write_tables(b, _fake_result(tm, 1))
    rows = mlik.compare([a + "_MLIK.npz", b + "_MLIK.npz"])
    assert len(rows) == 6 and [r["logZ_ss"] for r in rows] == sorted([r["logZ_ss"] for r in rows], reverse=True)
    assert rows[0]["two_ln_bf"] == 0.0 and rows[0]["two_ln_bf_se"] == 0.0 and all(r["two_ln_bf"] < 0 and r["two_ln_bf_se"] > 0 for r in rows[1:])
    assert {r["model"] for r in rows} == {"_CONB_COND", "_EXPB_EXPD_1", "_EXPB_COND_2"} and {r["name"] for r in rows} == {a + "_MLIK.npz", b + "_MLIK.npz"}
    text = mlik.format_compare(rows).splitlines()
    assert text[0].split("\t") == mlik.COMPARE_HEAD and len(text) == 7
    # files of other data are refused, multi-model or not
    c = str(tmp_path / "c")
    tm.write_tables(c, _fake_result(tm, 2, fp=(6, 1, 2, 3, 4, 0)))
    with pytest.raises(ValueError, match="different data"):
        mlik.compare([a + "_MLIK.npz", c + "_MLIK.npz"])
    # today's single-model files: the table is what it was, byte for byte
    for name, lz, se, model in (("x", -218.25, 0.03125, "_LDDN_MDDN"), ("y", -220.5, 0.0625, "_LC_MC")):
        np.savez(str(tmp_path / name) + "_MLIK.npz", ss=np.array([lz, lz]), logZ_ss=np.float64(lz), logZ_ss_se=np.float64(se),
                 model=np.str_(model), fingerprint=np.array([5., 1, 2, 3, 4, 0]))
    x, y = str(tmp_path / "x_MLIK.npz"), str(tmp_path / "y_MLIK.npz")
    se = 2.0 * math.sqrt(0.0625 ** 2 + 0.03125 ** 2)
    want = ("name\tmodel\tlogZ_ss\tlogZ_ss_se\ttwo_ln_bf\ttwo_ln_bf_se\n%s\t_LDDN_MDDN\t-218.25\t0.03125\t0.0\t0.0\n"
            "%s\t_LC_MC\t-220.5\t0.0625\t-4.5\t%s\n" % (x, y, str(se)))
    assert mlik.format_compare(mlik.compare([y, x])) == want
    mixed = mlik.compare([x, a + "_MLIK.npz"])
    assert len(mixed) == 4 and {r["model"] for r in mixed} >= {"_LDDN_MDDN", "_CONB_COND"}


def test_c_the_header_the_binding_and_the_build_agree():
    import ctypes as C
    from literate_amd import _hip, build, ops
    with open(os.path.join(ROOT, "include", "literate_hip_tmlik.h")) as f:
        text = f.read()
    consts = dict(re.findall(r"#define (LR_TMLIK_\w+) (\d+)", text))
    for k, v in consts.items():
        assert getattr(_hip, k) == int(v), k
    assert set(consts) == {"LR_TMLIK_MAX_BINS", "LR_TMLIK_MAX_TEMPS", "LR_TMLIK_MAX_MODELS", "LR_TMLIK_MOVES", "LR_TMLIK_STATE_W", "LR_TMLIK_ROW_W"}
    assert _hip.LR_TMLIK_ROW_W == _hip.LR_MLIK_ROW_W == len(ops.TMLIK_ROW) == H.ROW_W and ops.TMLIK_ROW.index("lik") == ops.MLIK_ROW.index("lik") == 2
    assert _hip.LR_TMLIK_STATE_W == H.STATE_W == ops.TMLIK_STATE["model"] + 1
    assert (ops.TMLIK_STATE["lik"], ops.TMLIK_STATE["proposed"], ops.TMLIK_STATE["accepted"], ops.TMLIK_STATE["win"]) == (H.S_LIK, H.S_PROPOSED, H.S_ACCEPTED, H.S_WIN)
    body = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decl = {m.group(1): [" ".join(a.split()) for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(lr_tmlik_\w+)\s*\(([^;{}]*?)\)\s*;", body, flags=re.S)}
    assert set(decl) == {"lr_tmlik_init", "lr_tmlik_steps"}
    kinds = {"const lr_tmlik_problem*": C.POINTER(_hip.TmlikProblem), "int64_t": _hip.c_i64, "int32_t": _hip.c_i32, "double*": _hip.c_vp}
    for name, args in decl.items():
        res, got = _hip.SIGNATURES[name]
        assert res is _hip.c_i32 and got == [kinds[a.rsplit(" ", 1)[0]] for a in args], name
        assert args[-1] != "void* stream", "the stream rides in the descriptor"
    # the descriptor, field by field
    struct = re.search(r"typedef struct lr_tmlik_problem \{(.*?)\} lr_tmlik_problem;", body, flags=re.S).group(1)
    fields = []
    for stmt in struct.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            typ, names = re.match(r"(.*?)\s+(\w+(?:\s*,\s*\w+)*)$", stmt).groups()
            fields += [(n.strip(), typ) for n in names.split(",")]
    want = {"int32_t": _hip.c_i32, "uint64_t": C.c_uint64}
    assert [(n, want.get(t, _hip.c_vp)) for n, t in fields] == [(n, t) for n, t in _hip.TmlikProblem._fields_]
    assert fields[-1] == ("stream", "void*")
    assert "lr_tmlik.hip" in build.SOURCES and any(h.endswith("literate_hip_tmlik.h") for h in build.HEADERS)
    with open(os.path.join(ROOT, "literate_amd", "csrc", "lr_tmlik.hip")) as f:
        src = f.read()
    assert "static_assert(sizeof(lr_tmlik_cfg) + sizeof(lr_tmlik_tables)" in src and "< 4096" in src and "atomic" not in src.replace("floating-point atomics", "")


def test_c_the_command_line_checks_its_flags_before_anything_runs(tmp_path):
    """refused at once, by name, before the data are read (a check that enumerated the columns of `all` once took minutes)"""
    import subprocess
    import sys
    import time
    base = [sys.executable, os.path.join(ROOT, "trend_rate.py"), "-d", str(tmp_path / "none.tsv"), "-n", "100", "-s", "10", "--mlik", "0.3"]
    t = time.time()
    for extra, word in ((["--mlik_columns", "all", "--mlik_models", "some"], "--mlik_models takes run or all"),
                        (["--mlik_columns", "a,b"], "--mlik_columns takes run, all or a comma-separated list of column indices"),
                        (["--mlik_temps", "1"], "--mlik_temps must be between 2 and 128"),
                        (["--mlik_columns", "all", "--mlik_models", "all", "--mlik_reps", "0"], "--mlik_reps must be at least 1")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and word in out.stderr, (extra, out.stderr[-500:])
        assert "Traceback" not in out.stderr and "unrecognized arguments" not in out.stderr and "usage:" not in out.stderr
    assert time.time() - t < 40


def test_c_the_docs_no_longer_say_not_built():
    from literate_amd import mlik
    for path in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert "Not built: trend_rate.py" not in text and "trend_mlik" in text, path
    assert "Not built: trend_rate.py" not in mlik.__doc__ and "trend_mlik" in mlik.__doc__
