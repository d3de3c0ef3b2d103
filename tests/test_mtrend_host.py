"""The joint covariate model without a GPU (literate_amd/multitrend.py, tests/helpers/mtrend_ref.py):

  1  the restatement's grouped likelihood - N log(base) + sum_j I_j coef_j SX_j - base E per side - equals the per-bin form of
     trend_rate.py:82 at rtol 1e-12 on random states
  2  every case of tests/test_hip_mtrend.py is held to the tie condition: no accept decision within 1e-6 of zero
  3  parsing and standardisation of the covariates, every refusal by its message, the window rule, the summary arithmetic on
     hand-made rows, the log's header and file name
"""
import argparse
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import mtrend_ref as mr          # noqa: E402


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins,P", [(1, 1), (40, 6), (65, 2), (129, 16), (512, 16)])
def test_1_grouped_equals_the_per_bin_form(n_bins, P):
    D = mr.synthetic(n_bins, P, 900 + n_bins)
    for k, I in enumerate(("zeros", "ones", "mixed", "mixed")):
        l0, m0, a, I_l, b, I_m = mr.random_params(D, 3, 50 + k, I)
        for c in range(3):
            for side, base, coef, ind in ((0, l0[c], a[c], I_l[c]), (1, m0[c], b[c], I_m[c])):
                want = mr.loglik_bins(D, side, base, coef, ind)
                got = mr.side_lik(D, side, base, coef, ind, mr.E_of(D, coef, ind))
                # rtol 1e-12 of the value, taken of the sum of the absolute terms where the value itself cancels
                mag = abs(D.N[side] * math.log(base)) + base * mr.E_of(D, coef, ind) + float(np.sum(np.abs(coef * ind * D.SX[side])))
                assert abs(got - want) <= 1e-12 * max(abs(want), mag), (side, I, got, want)


def test_1_a_nan_counts_as_minus_infinity_and_the_total_is_the_sum():
    assert mr.total(1.5, -2.0) == -0.5 and mr.total(np.inf, -np.inf) == -np.inf and mr.total(np.nan, 0.0) == -np.inf


def test_1_the_prior():
    D, st = mr.synthetic(5, 2, 1), mr.Settings(pI=0.2, slab_sd=2.0)
    a, b = np.array([0.3, -1.0]), np.array([0.0, 4.0])
    norm = lambda x: -0.5 * math.log(2 * math.pi) - math.log(2.0) - 0.5 * (x / 2.0) ** 2
    base = lambda x: -(x - .001) / 10.0 - math.log(10.0)
    want = base(0.2) + base(0.05) + sum(norm(x) for x in (0.3, -1.0, 0.0, 4.0)) + 1 * math.log(0.2) + 3 * math.log(0.8)
    assert abs(mr.log_prior(D, st, 0.2, 0.05, a, [1, 0], b, [0, 0]) - want) < 1e-13
    assert mr.log_prior(D, st, 0.0009, 0.05, a, [1, 0], b, [0, 0]) == -np.inf
    # a constant side has neither coefficients nor indicators in the prior
    want_b = base(0.2) + base(0.05) + norm(0.3) + norm(-1.0) + math.log(0.2) + math.log(0.8)
    for st_b in (mr.Settings(pI=0.2, slab_sd=2.0, m_death=1), mr.Settings(pI=0.2, slab_sd=2.0, no_death=1)):
        assert abs(mr.log_prior(D, st_b, 0.2, 0.05, a, [1, 0], b, [0, 0]) - want_b) < 1e-13


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_2_no_decision_of_a_case_is_within_1e_6_of_a_tie(case):
    D, st, rows, state, margin = mr.run_case(case)
    assert margin > mr.TIE, "%s: an accept decision within %g of a tie (margin %.3g): reseed it (RESEED)" % (case[0], mr.TIE, margin)
    assert rows.shape == ((case[3] + case[4] - 1) // case[4], mr.N_CHAINS, mr.ROW_W)
    prop = state[:, mr.S_PROPOSED:mr.S_PROPOSED + 4].sum(axis=1)
    assert (prop == case[3]).all(), "every iteration proposes one move"


def test_2_the_cases_cover_what_the_issue_lists():
    names = [c[0] for c in mr.CASES]
    assert len(set(names)) == len(names)
    for nb in mr.BIN_EDGES:
        for P in mr.P_EDGES:
            assert any(c[1][0] == nb and c[1][1] == P for c in mr.CASES)
    for mode, _ in mr.MODES:
        for sf in (1, 7):
            assert any(c[2] == mode and c[4] == sf for c in mr.CASES)
    # bvs_from inside the run and beyond its end
    assert mr.settings("bvs").bvs_from < mr.N_ITER < mr.settings("bvs_late").bvs_from
    # flips happen in the bvs cases and only there; included coefficients are moved in them
    for case in mr.CASES:
        state = mr.run_case(case)[3]
        flips, incl = state[:, mr.S_PROPOSED + 3].sum(), state[:, mr.S_PROPOSED + 4:mr.S_PROPOSED + 6].sum()
        if case[2] in ("bvs_late", "nobvs", "constBD"):
            assert flips == 0
        else:
            assert flips > 0 and state[:, mr.S_ACCEPTED + 3].sum() > 0 and incl > 0, case[0]


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
TABLE = np.array([[1.0, 10.0, 5.0], [2.0, 30.0, 5.0], [4.0, 20.0, 5.0], [8.0, 50.0, 5.0], [9.0, 99.0, 7.0]])
NAMES = ["market", "tech", "flat"]


def test_3_the_covariates_are_cut_and_standardised():
    from literate_amd import multitrend as mt
    X, names = mt.design_matrix(TABLE, NAMES, "0,1", 0, 4)
    assert names == ["market", "tech"] and X.shape == (2, 4)
    assert np.allclose(X.mean(axis=1), 0.0, atol=1e-15) and np.allclose(X.std(axis=1), 1.0, rtol=1e-15)
    want = (TABLE[:4, 0] - TABLE[:4, 0].mean()) / TABLE[:4, 0].std()
    assert np.array_equal(X[0], want), "the last row is dropped"
    X1, _ = mt.design_matrix(TABLE, NAMES, "1", 1, 3)
    assert np.array_equal(X1[0], mt.standardise(TABLE[1:4, 1])), "-rm_first_bin 1 drops the first row too"
    Xd, names_d = mt.design_matrix(TABLE, NAMES, "1", 0, 4, diversity=np.array([3.0, 4.0, 8.0, 1.0]))
    assert names_d == ["tech", "diversity"] and np.array_equal(Xd[1], mt.standardise([3.0, 4.0, 8.0, 1.0]))
    assert mt.parse_columns("all", 3) == [0, 1, 2] and mt.parse_columns("2,0", 3) == [2, 0]


def test_3_every_refusal_of_the_covariates_names_its_reason():
    from literate_amd import multitrend as mt
    with pytest.raises(ValueError, match=r"column 2 \(flat\) is constant"):
        mt.design_matrix(TABLE, NAMES, "all", 0, 4)
    bad = TABLE.copy()
    bad[1, 1] = np.inf
    with pytest.raises(ValueError, match=r"column 1 \(tech\) holds a value that is not finite"):
        mt.design_matrix(bad, NAMES, "1", 0, 4)
    bad[1, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        mt.design_matrix(bad, NAMES, "0,1", 0, 4)
    with pytest.raises(ValueError, match="column 3 lies outside the trend file"):
        mt.design_matrix(TABLE, NAMES, "0,3", 0, 4)
    with pytest.raises(ValueError, match="column -1 lies outside"):
        mt.design_matrix(TABLE, NAMES, "-1", 0, 4)
    with pytest.raises(ValueError, match="holds 5 rows, 4 in use: the data have 6 time bins"):
        mt.design_matrix(TABLE, NAMES, "0", 0, 6)
    with pytest.raises(ValueError, match="holds 5 rows, 3 in use: the data have 4 time bins"):
        mt.design_matrix(TABLE, NAMES, "0", 1, 4)
    with pytest.raises(ValueError, match="column diversity is constant"):
        mt.design_matrix(TABLE, NAMES, "0", 0, 4, diversity=np.ones(4))
    with pytest.raises(ValueError, match="--columns takes all or"):
        mt.design_matrix(TABLE, NAMES, "a,b", 0, 4)
    g = np.random.default_rng(0)
    wide = g.normal(size=(6, 17))
    with pytest.raises(ValueError, match="17 covariates: the joint model holds at most 16"):
        mt.design_matrix(wide, ["c%d" % i for i in range(17)], "all", 0, 5)
    X, _ = mt.design_matrix(wide, ["c%d" % i for i in range(17)], ",".join(str(i) for i in range(15)), 0, 5, diversity=g.normal(size=5))
    assert X.shape == (16, 5)
    with pytest.raises(ValueError, match="17 covariates"):
        mt.design_matrix(wide, ["c%d" % i for i in range(17)], ",".join(str(i) for i in range(16)), 0, 5, diversity=g.normal(size=5))
    long = g.normal(size=(514, 1))
    with pytest.raises(ValueError, match="513 time bins: the joint model holds at most 512"):
        mt.design_matrix(long, ["c"], "0", 0, 513)
    assert mt.design_matrix(long[:513], ["c"], "0", 0, 512)[0].shape == (1, 512)


def cli_args(*argv):
    sys.path.insert(0, ROOT)
    import MultiTrendRate
    return MultiTrendRate.build_parser().parse_args(["-d", "x.tsv", "-trend_data", "t.tsv"] + list(argv))


def test_3_every_refused_flag_names_its_reason():
    from literate_amd import multitrend as mt
    assert mt.arg_error(cli_args()) is None
    for argv, flag in ((["--replicates", "a*.tsv"], "replicates"), (["--mlik", "0.3"], "mlik"), (["--ppc", "0.2"], "ppc"),
                       (["--ppc_age", "0.2"], "ppc_age"), (["--ade", "0.2"], "ade"), (["--ade_joint", "0.2"], "ade_joint"),
                       (["--waic", "0.2"], "waic"), (["--loo", "0.2"], "loo"), (["--mc3", "4"], "mc3")):
        err = mt.arg_error(cli_args(*argv))
        assert err is not None and err.startswith("--%s: " % flag) and err == "--%s: %s" % (flag, mt.REFUSED[flag])
    assert len(set(mt.REFUSED.values())) >= 6, "the reasons differ"
    assert "several ranks" in mt.arg_error(cli_args(), world=2)
    assert "-pI" in mt.arg_error(cli_args("-pI", "1.0")) and "-slab_sd" in mt.arg_error(cli_args("-slab_sd", "0"))
    assert "--tune" in mt.arg_error(cli_args("--tune", "1.0")) and "-bvs" in mt.arg_error(cli_args("-bvs", "2"))
    assert "--summary" in mt.arg_error(cli_args("--summary", "1.5")) and "--chains" in mt.arg_error(cli_args("--chains", "0"))
    args = cli_args()
    args.trend_data = ""
    assert "-trend_data" in mt.arg_error(args)


def test_3_the_window_rule():
    from literate_amd import multitrend as mt
    from literate_amd import trend_mlik as tm
    assert mt.WIN0 == 0.1
    # win <- clip(win exp(4 (rate - 0.3) / sqrt(b)), 0.001, 20), per side; a side without a proposal keeps its window
    w = mt.tune_windows((0.1, 0.2), accepted=[60.0, 0.0], proposed=[100.0, 0.0], b=4)
    assert w[0] == pytest.approx(0.1 * math.exp(4.0 * (0.6 - 0.3) / 2.0), rel=1e-15) and w[1] == 0.2
    w = mt.tune_windows((0.1, 0.2), accepted=[30.0, 0.0], proposed=[100.0, 50.0], b=1)
    assert w[0] == pytest.approx(0.1, rel=1e-15) and w[1] == pytest.approx(0.2 * math.exp(-1.2), rel=1e-15)
    assert mt.tune_windows((19.0, 0.0011), [100.0, 0.0], [100.0, 100.0], 1) == (tm.WIN_MAX, tm.WIN_MIN)


def hand_rows():
    """five rows of P = 2: columns it .. m0, I_l, a, I_m, b"""
    rows = np.zeros((5, 16))
    rows[:, 6], rows[:, 7] = 0.2, 0.1
    rows[:, 8:10] = [[1, 0], [1, 0], [1, 1], [0, 0], [1, 0]]
    rows[:, 10:12] = [[0.5, 9.0], [0.7, 9.0], [0.6, -0.2], [3.0, 3.0], [0.4, 1.0]]
    rows[:, 12:14] = [[0, 0], [0, 1], [0, 0], [0, 0], [0, 0]]
    rows[:, 14:16] = [[1.0, 1.0], [1.0, 0.3], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0]]
    return rows


def test_3_the_summary_arithmetic_on_hand_made_rows():
    from literate_amd import multitrend as mt
    rows = hand_rows()
    X = np.array([[1.0, -1.0, 0.0], [0.5, 0.5, -1.0]])
    l, m = mt.bin_rates(rows, X)
    assert np.allclose(l[0], 0.2 * np.exp(0.5 * X[0]), rtol=1e-15) and np.allclose(l[2], 0.2 * np.exp(0.6 * X[0] - 0.2 * X[1]), rtol=1e-15)
    assert np.array_equal(l[3], [0.2] * 3) and np.allclose(m[1], 0.1 * np.exp(0.3 * X[1]), rtol=1e-15) and np.array_equal(m[0], [0.1] * 3)
    mean, lo, hi, n = mt.conditional_coef(rows[:, 8], rows[:, 10])
    assert n == 4 and mean == pytest.approx(0.55) and (lo, hi) == (0.4, 0.7)
    assert mt.conditional_coef(rows[:, 12], rows[:, 14])[3] == 0 and math.isnan(mt.conditional_coef(rows[:, 12], rows[:, 14])[0])
    table = mt.model_table(np.concatenate([rows[:, 8:10], rows[:, 12:14]], axis=1))
    assert [(t[1], t[2].tolist()) for t in table] == [(2, [1, 0, 0, 0]), (1, [0, 0, 0, 0]), (1, [1, 1, 0, 0]), (1, [1, 0, 0, 1])]
    assert table[0][0] == 0.4 and sum(t[0] for t in table) == pytest.approx(1.0)
    assert len(mt.model_table(np.random.default_rng(0).integers(0, 2, (4000, 6)))) == mt.N_MODELS
    # 2 ln BF against the prior odds, the frequency clipped to 1 / (2 n)
    assert mt.two_ln_bf(0.5, 0.1, 100) == pytest.approx(2 * math.log(9.0)) and mt.two_ln_bf(0.1, 0.1, 100) == pytest.approx(0.0, abs=1e-15)
    assert mt.two_ln_bf(1.0, 0.1, 100) == pytest.approx(2 * math.log(199.0 * 9.0)) and mt.two_ln_bf(0.0, 0.1, 100) == pytest.approx(-2 * math.log(199.0 / 9.0))
    cnt = np.zeros((2, 2, 6))
    cnt[:, 0] = [10, 20, 0, 8, 4, 0]
    cnt[:, 1] = [5, 20, 0, 2, 1, 0]
    acc = mt.acceptance(cnt)
    assert acc[[0, 1, 3, 4]].tolist() == [0.5, 1.0, 0.25, 0.25] and np.isnan(acc[[2, 5]]).all()


def test_3_the_files_of_the_summary(tmp_path):
    from literate_amd import multitrend as mt
    rows = hand_rows()
    I = [rows[:, 8:10], rows[:, 12:14]]
    cc = [[mt.conditional_coef(I[s][:, j], rows[:, (10, 14)[s] + j]) for j in range(2)] for s in (0, 1)]
    avg = [[(0.1, 50.0, 1.01)] * 2] * 2
    path = str(tmp_path / "x_joint_MT.tsv")
    mt.write_mt(path, ["market", "tech"], [0], [I[0].mean(axis=0), I[1].mean(axis=0)], cc, avg, np.array([0.5, 0.4, np.nan, 0.1, 0.3, np.nan]),
                (0.07, 0.1), 0.1, 5)
    head, lines = mt.read_tsv(path)
    assert head == mt.MT_HEAD and [(ln["side"], ln["covariate"]) for ln in lines] == [("birth", "market"), ("birth", "tech")]
    assert float(lines[0]["P_I"]) == 0.8 and float(lines[0]["2lnBF"]) == pytest.approx(2 * math.log(4.0 * 9.0)) and lines[0]["n_included"] == "4"
    assert float(lines[0]["coef_minHPD"]) == 0.4 and float(lines[0]["window"]) == 0.07 and float(lines[1]["accept_flip"]) == 0.1
    mt.write_models(str(tmp_path / "m.tsv"), mt.model_table(np.concatenate(I, axis=1)), 2)
    head, lines = mt.read_tsv(str(tmp_path / "m.tsv"))
    assert head == mt.MODELS_HEAD and (lines[0]["birth"], lines[0]["death"], lines[0]["frequency"]) == ("10", "00", "0.4") and lines[3]["death"] == "01"
    three = lambda v: (np.full(3, v), np.full(3, v - 1), np.full(3, v + 1))
    mt.write_rates(str(tmp_path / "r.tsv"), three(0.2), three(0.1), (np.arange(3.0), np.arange(3.0) / 2))
    head, lines = mt.read_tsv(str(tmp_path / "r.tsv"))
    assert head == mt.RATES_HEAD and len(lines) == 3 and float(lines[2]["l_empirical"]) == 2.0 and float(lines[1]["m_maxHPD"]) == 1.1


def test_3_the_header_and_the_names():
    from literate_amd import multitrend as mt
    head = mt.header(["market", "tech"], 3)
    assert head == ["it", "posterior", "likelihood", "likelihood_birth", "likelihood_death", "prior", "l0", "m0", "I_l_market", "I_l_tech",
                    "a_market", "a_tech", "I_m_market", "I_m_tech", "b_market", "b_tech", "l_0", "l_1", "l_2", "m_0", "m_1", "m_2"]
    assert mt.log_name("/d/cars.tsv", 7, False, False, False) == "/d/cars_7_EXPB_EXPD_joint.multitrend.log"
    assert mt.log_name("/d/cars.tsv", 7, True, True, True, 3) == "/d/cars_7_CONB_ND_joint_c3.multitrend.log"
    assert mt.log_name("cars.tsv", 7, False, True, False, 0) == "cars_7_EXPB_COND_joint_c0.multitrend.log"
    assert mt.summary_stem("/d/cars.tsv") == "/d/cars_joint_MT"


def test_3_the_layouts_of_ops_and_the_restatement_agree():
    from literate_amd import _hip, ops
    assert (_hip.LR_MTREND_STATE_W, _hip.LR_MTREND_ROW_W, _hip.LR_MTREND_MOVES) == (mr.STATE_W, mr.ROW_W, mr.MOVES)
    assert (_hip.LR_MTREND_MAX_BINS, _hip.LR_MTREND_MAX_COVS) == (mr.MAX_BINS, mr.MAX_COVS)
    S = ops.MTREND_STATE
    assert [S[k] for k in ("l0", "m0", "lik_b", "lik_d", "prior", "E_b", "E_d", "proposed", "accepted", "I_l", "a", "I_m", "b")] == \
        [mr.S_L0, mr.S_M0, mr.S_LIK_B, mr.S_LIK_D, mr.S_PRIOR, mr.S_E_B, mr.S_E_D, mr.S_PROPOSED, mr.S_ACCEPTED, mr.S_IL, mr.S_A, mr.S_IM, mr.S_B]
    cols = ops.mtrend_row_columns(16)
    assert cols["b"].stop == cols["width"] == mr.ROW_W and len(ops.MTREND_MOVES) == mr.MOVES
    with open(os.path.join(ROOT, "include", "literate_hip_mtrend.h")) as f:
        text = f.read()
    for name, v in (("STATE_W", mr.STATE_W), ("ROW_W", mr.ROW_W), ("S_PROPOSED", mr.S_PROPOSED), ("S_ACCEPTED", mr.S_ACCEPTED), ("S_IL", mr.S_IL),
                    ("S_A", mr.S_A), ("S_IM", mr.S_IM), ("S_B", mr.S_B)):
        assert "#define LR_MTREND_%s %d " % (name, v) in text, name
    for name, v in (("MOVE", mr.P_MOVE), ("NORM", mr.P_NORM), ("ACCEPT", mr.P_ACCEPT), ("INIT", mr.P_INIT)):
        assert "#define LR_P_MTREND_%s %d " % (name, v) in text, name
