"""The host side of the simulation study (literate_amd/simstudy.py, include/literate_hip_score.h, tests/helpers/score_ref.py),
no GPU: scenario parsing and every refusal, --from_rtt, the keep and drop rules, Replicates.from_counts, the numpy restatement
of the scoring on hand-made arrays whose answers are written out here, simstudy's own shift arithmetic against it, and the
errors lr_rtt_score returns before a launch, through ctypes with host pointers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import score_ref as R
from literate_amd import simstudy as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the scenario ------------------------------------------------------------------------------------------------------------
def write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_a_scenario_file_is_read_with_its_comments_skipped(tmp_path):
    p = write(tmp_path / "s.tsv", "# a step in the birth rate\nbin\tbirth\tdeath\n0\t0.3\t0.1\n# half way\n1\t0.3\t0.1\n\n2 1.2 0.1\n")
    sc = SS.read_scenario(p)
    assert sc.dtype == np.float64 and sc.tolist() == [[0.3, 0.3, 1.2], [0.1, 0.1, 0.1]]


@pytest.mark.parametrize("text,sentence", [
    ("bin\tbirth\tdeath\n0\t-0.3\t0.1\n1\t0.3\t0.1\n", "a rate is negative"),
    ("bin\tbirth\tdeath\n0\t0.3\tnan\n1\t0.3\t0.1\n", "a rate is not a finite number"),
    ("bin\tbirth\tdeath\n0\tinf\t0.1\n1\t0.3\t0.1\n", "a rate is not a finite number"),
    ("bin\tbirth\tdeath\n0\t0.3\t0.1\n", "1 bins; a scenario needs at least 2 unit bins"),
    ("bin\tbirth\tdeath\n", "0 bins; a scenario needs at least 2 unit bins"),
    ("bin\tbirth\tdeath\n" + "".join("%d\t0.3\t0.1\n" % i for i in range(513)), "513 bins; the replicate sampler holds at most 512"),
    ("time\tbirth\tdeath\n0\t0.3\t0.1\n1\t0.3\t0.1\n", "the header must be `bin birth death`"),
    ("bin\tbirth\tdeath\n0\t0.3\t0.1\n2\t0.3\t0.1\n", "row 1 names bin 2"),
    ("bin\tbirth\tdeath\n0\t0.3\t0.1\n1\t0.3\n", "row 1 is not `bin birth death`"),
    ("bin\tbirth\tdeath\n0\t0.3\t0.1\n1\tx\t0.1\n", "row 1 is not `bin birth death`"),
    ("# nothing\n", "no header line"),
])
def test_every_refusal_of_a_scenario_is_a_sentence(tmp_path, text, sentence):
    with pytest.raises(ValueError, match=re.escape(sentence)):
        SS.read_scenario(write(tmp_path / "s.tsv", text))


def test_512_bins_are_a_scenario():
    assert SS.check_scenario(np.full(512, 0.2), np.zeros(512)).shape == (2, 512)
    with pytest.raises(ValueError, match="3 birth rates but 2 death rates"):
        SS.check_scenario([1, 2, 3], [1, 2])


def test_from_rtt_takes_the_posterior_means_of_a_finished_run(tmp_path):
    from literate_amd import logs
    rates = np.arange(27, dtype=float).reshape(3, 3, 3) / 10.0
    logs.write_rtt_tables(str(tmp_path / "run"), [0.5, 1.5, 2.5], rates, np.zeros((2, 3)), np.ones((2, 32), dtype=np.int64))
    sc = SS.scenario_from_rtt(str(tmp_path / "run_RTT.tsv"))
    assert sc.tolist() == [rates[0, 0].tolist(), rates[1, 0].tolist()]
    with pytest.raises(ValueError, match="no birth_rate and death_rate columns"):
        SS.scenario_from_rtt(str(tmp_path / "run_RTT_K.tsv"))
    p = write(tmp_path / "neg_RTT.tsv", "time\tbirth_rate\tdeath_rate\n0.5\t0.1\t-0.2\n1.5\t0.1\t0.2\n")
    with pytest.raises(ValueError, match="a rate is negative"):
        SS.scenario_from_rtt(p)


def test_the_command_line_wants_exactly_one_scenario(tmp_path):
    with pytest.raises(SystemExit, match="name the scenario"):
        SS.main([])
    with pytest.raises(SystemExit, match="name the scenario"):
        SS.main(["a.tsv", "--from_rtt", "b_RTT.tsv"])
    with pytest.raises(SystemExit, match="a rate is negative"):
        SS.main([write(tmp_path / "s.tsv", "bin\tbirth\tdeath\n0\t-1\t0\n1\t1\t0\n")])
    a = SS.parser().parse_args(["s.tsv"])
    assert (a.steps_per_bin, a.n_start, a.burnin, a.bf, a.bf_reps, a.tol, a.min_lineages) == (100, 100, 0.2, 6.0, 1 << 20, 2, 0)
    assert (a.use_rate_HP, a.Poisson_prior, a.update_fraction, a.block, a.seed) == (1, 0.0, 0.75, 0, 1)


def test_run_refuses_a_group_beyond_the_cap_before_any_device_work():
    sc = np.array([[0.3, 0.3], [0.1, 0.1]])
    with pytest.raises(ValueError, match="scored on 2 to 4096 samples"):
        SS.run(sc, 4, chains_per_rep=2, n_iter=2561 * 10, s_freq=10, burnin=0.2)          # 2 x (2561 - 512) = 4098
    with pytest.raises(ValueError, match="at least 2 replicates"):
        SS.run(sc, 1)


# ---- keep and drop -----------------------------------------------------------------------------------------------------------
def test_the_keep_and_drop_rules_on_hand_made_counts():
    nb = 3
    counts = np.ones((7, 4, nb), dtype=np.int64) * 5
    totals = np.array([[100, 40, 0, -1],       # kept
                       [100, 40, 1, -1],       # overflow
                       [100, 0, 0, 250],       # extinct
                       [100, 40, 0, -1],       # a bin without lineage-steps
                       [9, 40, 0, -1],         # too few
                       [501, 40, 0, -1],       # too many
                       [100, 0, 1, 17]])       # overflow and extinct: the first rule names it
    counts[3, 3, 1] = 0
    reason = SS.keep_replicates(counts, totals, min_lineages=10, max_lineages=500)
    assert [SS.REASONS[r] for r in reason] == ["kept", "overflow", "extinct", "empty_bin", "lineages", "lineages", "overflow"]
    assert SS.keep_replicates(counts, totals).tolist() == [0, 1, 2, 3, 0, 0, 1], "no bounds: only the first three rules"
    assert SS.keep_replicates(counts, totals, min_lineages=100, max_lineages=100)[0] == 0, "the ends are included"
    sp, ex, br = SS.statistics(counts[:1] * np.array([1, 2, 3, 50])[None, :, None], 100)
    assert sp.tolist() == [[5.0] * nb] and ex.tolist() == [[10.0] * nb] and br.tolist() == [[2.5] * nb]
    assert SS.end_time(12) == 12.5


def test_replicates_from_counts():
    from literate_amd.replicates import Replicates
    sp, ex, br = np.arange(6.0).reshape(2, 3), np.ones((2, 3)), np.full((2, 3), 4.0)
    reps = Replicates.from_counts(sp, ex, br, 0.0, 3.5)
    assert (reps.R, reps.n_bins, reps.t0) == (2, 3, 0) and reps.paths == ["replicate0", "replicate1"]
    assert reps.start_time.tolist() == [0.0, 0.0] and reps.end_time.tolist() == [3.5, 3.5] and reps.ex_dead is None
    assert np.array_equal(reps.sp, sp) and reps.sp.flags.c_contiguous and reps.br.dtype == np.float64
    assert reps.empirical(1)[0].tolist() == [0.75, 1.0, 1.25]
    one = Replicates.from_counts(sp[0], ex[0], br[0], [1.25], [4.5], t0=1, paths=["x"])
    assert (one.R, one.n_bins, one.t0, one.paths) == (1, 3, 1, ["x"]) and one.end_time.tolist() == [4.5]
    per = Replicates.from_counts(sp, ex, br, [0.0, 0.25], [3.5, 3.75])
    assert per.start_time.tolist() == [0.0, 0.25]
    for bad, sentence in (((sp, ex[:1], br, 0.0, 3.5), "share their shape"), ((sp, ex, -br, 0.0, 3.5), "finite and not negative"),
                          ((sp, ex, br, 3.5, 3.5), "end_time must lie after"), ((sp, ex, br * np.nan, 0.0, 3.5), "finite and not negative"),
                          ((np.zeros((1, 513)),) * 3 + (0.0, 513.5), "513 time bins")):
        with pytest.raises(ValueError, match=sentence):
            Replicates.from_counts(*bad)
    with pytest.raises(ValueError, match="paths names 1 replicates"):
        Replicates.from_counts(sp, ex, br, 0.0, 3.5, paths=["a"])


# ---- the restatement, answers by hand ----------------------------------------------------------------------------------------
def hand_rates():
    """2 replicates, 2 bins: (mean, lo, hi) of birth, death, net"""
    r = np.zeros((2, 3, 3, 2))
    r[0, 0] = [[0.5, 0.25], [0.25, 0.125], [1.0, 0.5]]        # birth: truth 0.25 sits ON lo in bin 0, ON hi... see below
    r[0, 1] = [[0.25, 0.25], [0.125, 0.125], [0.5, 0.5]]
    r[0, 2] = [[0.25, 0.0], [0.0, -0.25], [0.5, 0.25]]
    r[1, 0] = [[1.0, 0.75], [0.5, 0.5], [1.5, 1.0]]
    r[1, 1] = [[0.5, 0.25], [0.25, 0.1875], [0.75, 0.24999999999999997]]
    r[1, 2] = [[0.5, 0.5], [0.25, 0.25], [1.0, 1.0]]
    return r


def test_coverage_and_the_six_columns_by_hand():
    truth = np.array([[0.25, 0.5], [0.25, 0.25]])          # net: 0.0, 0.25
    cov = R.covered(hand_rates(), truth)
    # replicate 0: birth bin 0 truth == lo (covered), bin 1 truth == hi (covered); death inside; net bin 0 truth == lo, bin 1 == hi
    # replicate 1: birth bin 0 truth 0.25 < lo 0.5 (out), bin 1 truth == lo (covered); death bin 0 truth == lo (covered), bin 1
    #              hi is the double just below 0.25 (just outside); net bin 0 truth 0 < 0.25 (out), bin 1 truth == lo (covered)
    assert cov.dtype == np.int32 and cov.tolist() == [[[1, 1], [1, 1], [1, 1]], [[0, 1], [1, 0], [0, 1]]]
    sc, mag = R.score(hand_rates(), truth)
    # birth, bin 0: errors 0.25, 0.75 -> bias 0.5, mae 0.5, rmse sqrt((0.0625 + 0.5625) / 2), widths 0.75, 1.0
    assert sc[0, 0].tolist() == [2.0, 0.5, 0.5, 0.5, np.sqrt(0.3125), 0.875]
    # birth, bin 1: errors -0.25, 0.25 -> bias 0, mae 0.25, rmse 0.25, widths 0.375, 0.5
    assert sc[0, 1].tolist() == [2.0, 1.0, 0.0, 0.25, 0.25, 0.4375]
    # net, bin 0: errors 0.25, 0.5; covered 1 of 2
    assert sc[2, 0].tolist() == [2.0, 0.5, 0.375, 0.375, np.sqrt((0.0625 + 0.25) / 2), 0.625]
    assert mag[0, 1].tolist() == [0.25, 0.25, 0.0625, 0.4375]
    per_group = np.repeat(truth[None], 2, axis=0)
    assert np.array_equal(R.covered(hand_rates(), per_group), cov) and np.array_equal(R.score(hand_rates(), per_group)[0], sc)
    assert R.truth3(truth).tolist() == [[0.25, 0.5], [0.25, 0.25], [0.0, 0.25]]


def test_the_empirical_baseline_by_hand():
    sp, ex, br = np.array([[2.0, 4.0], [6.0, 4.0]]), np.array([[1.0, 1.0], [1.0, 3.0]]), np.array([[4.0, 8.0], [8.0, 8.0]])
    truth = np.array([[0.5, 0.5], [0.25, 0.25]])
    e = R.empirical(sp, ex, br, truth)
    # birth bin 0: 0.5, 0.75 -> errors 0, 0.25; death bin 1: 0.125, 0.375 -> errors -0.125, 0.125
    assert e[0, 0, [0, 2, 3, 4]].tolist() == [2.0, 0.125, 0.125, np.sqrt(0.03125)] and np.isnan(e[0, 0, [1, 5]]).all()
    assert e[1, 1, [0, 2, 3, 4]].tolist() == [2.0, 0.0, 0.125, 0.125]
    assert np.allclose(SS.empirical_score(sp, ex, br, truth), e, rtol=0, atol=1e-15, equal_nan=True)


def freq_of(two, pi):
    """the sampled frequency whose 2 ln BF against pi is `two`"""
    a = np.exp(two / 2.0) * pi / (1.0 - pi)
    return a / (a + 1.0)


def test_two_ln_bf_and_the_threshold():
    from literate_amd import shift_bf
    assert R.two_ln_bf(0.0, 0.1) == -np.inf and R.two_ln_bf(1.0, 0.1) == np.inf and np.isnan(R.two_ln_bf(0.5, 0.0))
    for f in (0.01, 0.3, 0.9):
        assert R.two_ln_bf(f, 0.05) == pytest.approx(float(shift_bf.two_ln_bf(f, 0.05)), rel=1e-15)
    assert R.two_ln_bf(freq_of(7.0, 0.05), 0.05) == pytest.approx(7.0, rel=1e-12)


def shifts_case():
    """8 bins, 4 replicates.  Birth: true shifts at bin 1 and at the last bin (7); death: none."""
    nb, pi = 8, 0.05
    truth = np.array([[0.2, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8, 0.4], [0.1] * nb])
    hi, lo = freq_of(7.0, pi), freq_of(5.0, pi)          # reported, not reported
    f = np.full((4, 2, nb), lo)
    f[0, 0, 0] = hi          # birth, replicate 0: bin 0 - within tol of bin 1 (the window reaches past the start)
    f[1, 0, 3] = hi          # replicate 1: bin 3 - within tol 2 of bin 1, not of bin 7, and not far from a true one
    f[2, 0, 4] = hi          # replicate 2: bin 4 - farther than 2 from 1 and from 7: a false positive
    f[2, 0, 7] = hi          #              and the last bin itself
    f[3, 0, 5] = hi          # replicate 3: bin 5 - within tol of bin 7
    f[1, 1, 0] = hi          # death (no true shift): every report is a false positive
    f[3, 1, 7] = hi
    f[3, 1, 6] = 0.0         # 2 ln BF = -inf: not reported
    kc = np.zeros((4, 2, 32), dtype=np.int64)
    kc[:, 0, 2] = 10         # birth: three rates, the truth, ...
    kc[3, 0, 2], kc[3, 0, 1] = 4, 6          # ... but replicate 3's mode is two (mean 2.4)
    kc[:, 1, 0] = 8
    kc[0, 1, 0], kc[0, 1, 1] = 5, 5          # death: a tie goes to the smaller K, the truth (mean 1.5)
    return truth, f, kc, pi


def test_power_false_positives_and_K_by_hand():
    truth, f, kc, pi = shifts_case()
    s = R.shifts(f, kc, truth, np.full(8, pi), bf=6.0, tol=2)
    b, d = s["birth"], s["death"]
    assert b["true_bins"] == [1, 7] and b["ratio"] == [4.0, 0.5] and d["true_bins"] == [] and d["power"] == []
    assert b["power"] == [0.5, 0.5], "bin 1: replicates 0 and 1; bin 7: replicates 2 and 3"
    assert b["false_positive"] == 0.25 and d["false_positive"] == 0.5
    assert (b["k_true"], d["k_true"]) == (3, 1) and b["k_mode_share"] == 0.75 and d["k_mode_share"] == 1.0
    assert b["k_mean"] == pytest.approx((3 + 3 + 3 + 2.4) / 4) and d["k_mean"] == pytest.approx((1.5 + 1 + 1 + 1) / 4)
    assert s["k_mode"].tolist() == [[3, 1], [3, 1], [3, 1], [2, 1]]
    # tol 0: only the last bin's own report counts; bins 0, 3, 4, 5 are all false positives
    s0 = R.shifts(f, kc, truth, np.full(8, pi), bf=6.0, tol=0)
    assert s0["birth"]["power"] == [0.0, 0.25] and s0["birth"]["false_positive"] == 1.0
    # a tol that reaches past both ends covers every bin: nothing is far from a true shift
    s9 = R.shifts(f, kc, truth, np.full(8, pi), bf=6.0, tol=9)
    assert s9["birth"]["power"] == [1.0, 1.0] and s9["birth"]["false_positive"] == 0.0 and s9["death"]["false_positive"] == 0.5
    # a higher threshold: nothing is reported
    s8 = R.shifts(f, kc, truth, np.full(8, pi), bf=8.0, tol=2)
    assert s8["birth"]["power"] == [0.0, 0.0] and s8["death"]["false_positive"] == 0.0
    # a prior vector: bin 4's own prior so high that replicate 2's frequency there is no evidence
    prior = np.full(8, pi)
    prior[4] = 0.5
    assert R.shifts(f, kc, truth, prior)["birth"]["false_positive"] == 0.0


def same_shifts(got, ref):
    for k, kind in enumerate(("birth", "death")):
        r = ref[kind]
        assert list(got["true_bins"][k]) == r["true_bins"] and list(got["ratio"][k]) == r["ratio"] and list(got["power"][k]) == r["power"]
        assert got["false_positive"][k] == r["false_positive"] and got["k_true"][k] == r["k_true"]
        assert got["k_mode_share"][k] == r["k_mode_share"] and got["k_mean"][k] == pytest.approx(r["k_mean"], rel=1e-14)
    assert np.array_equal(got["k_mode"], ref["k_mode"])


@pytest.mark.parametrize("tol,bf", [(2, 6.0), (0, 6.0), (9, 6.0), (2, 8.0), (1, 2.0)])
def test_the_modules_shift_arithmetic_is_the_restatements(tol, bf):
    truth, f, kc, pi = shifts_case()
    same_shifts(SS.shifts(f, kc, truth, pi, bf, tol), R.shifts(f, kc, truth, np.full(8, pi), bf, tol))
    flat = np.array([[0.3] * 8, [0.1] * 8])          # no shift of either kind: every report is a false positive
    got = SS.shifts(f, kc, flat, pi, bf, tol)
    same_shifts(got, R.shifts(f, kc, flat, np.full(8, pi), bf, tol))
    assert np.array_equal(got["reported"], R.reported(f, np.full(8, pi), bf))
    if (tol, bf) == (2, 6.0):
        assert got["false_positive"].tolist() == [1.0, 0.5] and got["k_true"].tolist() == [1, 1]


def test_the_tables_are_written_from_a_result(tmp_path):
    truth, f, kc, pi = shifts_case()
    res = SS.Result()
    res.scenario, res.settings, res.prior_s = truth, dict(seed=3, capacity=None), pi
    res.counts, res.totals = np.ones((5, 4, 8), dtype=np.int64), np.array([[50 + r, 20, 0, -1] for r in range(5)])
    res.totals[2, 2] = 1
    res.reason = SS.keep_replicates(res.counts, res.totals)
    res.kept, res.seeds = np.flatnonzero(res.reason == 0), 3 + np.arange(5)
    res.sp, res.ex, res.br = SS.statistics(res.counts[res.kept], 1)
    res.time = np.arange(8) + 0.5
    res.rates, res.shift_freq, res.k_counts = np.zeros((4, 3, 3, 8)), f, kc
    res.covered = R.covered(res.rates, truth)
    res.score, res.empirical = R.score(res.rates, truth)[0], SS.empirical_score(res.sp, res.ex, res.br, truth)
    res.shifts = SS.shifts(f, kc, truth, pi)
    files = SS.write_files(res, str(tmp_path / "st"))
    assert [os.path.basename(p) for p in files] == ["st_SIM_rates.tsv", "st_SIM_shifts.tsv", "st_SIM_replicates.tsv", "st_SIM.npz"]
    rates = open(files[0]).read().splitlines()
    assert rates[0].split("\t") == ["kind", "bin", "truth"] + SS.SCORE_HEAD + SS.EMP_HEAD and len(rates) == 1 + 3 * 8
    assert rates[1].split("\t")[:5] == ["birth", "0", "0.2", "4.0", "0.0"] and rates[17].split("\t")[:3] == ["net", "0", "0.1"]
    sh = open(files[1]).read().splitlines()
    assert sh[:3] == ["kind\tbin\tquantity\tvalue", "birth\t1\tratio\t4.0", "birth\t1\tpower\t0.5"] and "birth\t7\tratio\t0.5" in sh
    assert "death\tNA\tfalse_positive\t0.5" in sh and "birth\tNA\tk_true\t3.0" in sh and all(len(ln.split("\t")) == 4 for ln in sh), "one table"
    rp = open(files[2]).read().splitlines()
    assert rp[1] == "0\t3\t50\t20\tkept\t3\t1" and rp[3] == "2\t5\t52\t20\toverflow\tNA\tNA" and rp[5].endswith("kept\t2\t1")
    z = np.load(files[3])
    assert np.array_equal(z["shift_freq"], f) and z["birth_true_bins"].tolist() == [1, 7] and z["setting_capacity"] == -1
    assert np.array_equal(z["covered"], res.covered) and z["kept"].tolist() == [0, 1, 3, 4]


# ---- lr_rtt_score's refusals, before any launch -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from literate_amd import _hip
    return _hip.load()


BUF = (C.c_double * 64)()
P = C.c_void_p(C.addressof(BUF))          # a valid host address for every pointer: the calls below return before they use one


def problem(**kw):
    from literate_amd import _hip
    f = dict(trace=P, truth=P, rates=P, shift_freq=P, k_counts=P, covered=P, score=P, n_samples=100, n_chains=8, chains_per_group=2,
             reserved=0, start_age=0.0, end_age=12.5, burnin=0.2, stream=None)
    f.update(kw)
    return _hip.RttScoreProblem(**f)


def test_the_header_the_binding_and_the_build_agree():
    from literate_amd import _hip, build
    with open(os.path.join(ROOT, "include", "literate_hip_score.h")) as f:
        text = f.read()
    assert "#define LR_SCORE_MAX_SAMPLES 4096" in text and _hip.LR_SCORE_MAX_SAMPLES == 4096 and _hip.LR_SCORE_COLS == 6
    body = text[text.index("typedef struct lr_rtt_score_problem {"):text.index("} lr_rtt_score_problem;")]
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", body.split("{", 1)[1])          # every declarator of every field, in order
    assert names == [n for n, _ in _hip.RttScoreProblem._fields_], names
    assert _hip.SIGNATURES["lr_rtt_score"] == (C.c_int32, [C.POINTER(_hip.RttScoreProblem)])
    assert "workspace" not in re.sub(r"/\*.*?\*/", " ", text, flags=re.S) and "void* stream)" not in text
    assert "lr_score.hip" in build.SOURCES and "lr_rtt.h" in build.HEADERS and any(h.endswith("literate_hip_score.h") for h in build.HEADERS)
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        assert "lr_rtt_score" not in f.read()


def test_the_errors_before_a_launch_in_the_headers_order(lib):
    from literate_amd import _hip
    E = _hip
    call = lambda **kw: lib.lr_rtt_score(C.byref(problem(**kw)))
    assert lib.lr_rtt_score(None) == E.LR_ERR_NULL
    for field in ("trace", "rates", "shift_freq", "k_counts", "covered", "score"):
        assert call(**{field: None}) == E.LR_ERR_NULL, field
        assert call(**{field: None, "n_samples": 0}) == E.LR_ERR_NULL, "NULL comes before the sizes: " + field
    # sizes
    for kw in (dict(n_samples=0), dict(n_chains=0), dict(chains_per_group=0), dict(chains_per_group=-1), dict(chains_per_group=3),
               dict(n_chains=7), dict(burnin=1.0), dict(burnin=-0.1), dict(burnin=float("nan")),
               dict(end_age=12.0), dict(end_age=0.0), dict(end_age=0.5), dict(end_age=float("inf")), dict(start_age=float("nan")),
               dict(end_age=4096.5),                                     # beyond LR_MAX_BINS + 1
               dict(n_samples=1, chains_per_group=1),                    # n = 1: n_in = 1
               dict(n_samples=2, chains_per_group=1, burnin=0.5),        # n = 1 after the burn-in
               dict(n_samples=4097, chains_per_group=1, burnin=0.0),     # n = 4097
               dict(n_samples=2561, chains_per_group=2, burnin=0.2)):    # 2 x (2561 - 512) = 4098
        assert call(**kw) == E.LR_ERR_SIZE, kw
    # covered and score are not looked at without a truth - but the sizes still are
    assert call(truth=None, covered=None, score=None, n_chains=7) == E.LR_ERR_SIZE
    assert call(truth=None, covered=None, score=None, n_samples=4097, chains_per_group=1, burnin=0.0) == E.LR_ERR_SIZE
