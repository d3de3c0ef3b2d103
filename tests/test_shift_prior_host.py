"""The host side of the Bayes factors for rate shifts (no GPU): the numpy restatement of lr_shift_prior against the closed
form of its K distribution and against the reference's own get_prior_shift (tests/golden/shift_prior_reference.json, written
by tests/golden/make_shift_prior_golden.py), literate_amd.shift_bf against the reference's thresholds and at its edge
values, the three tables of logs.write_rtt_bf_tables, the ABI surface and the command line's argument errors."""
import json
import os

import numpy as np
import pytest

from helpers import shift_prior_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture_runs():
    with open(os.path.join(ROOT, "tests", "golden", "shift_prior_reference.json")) as f:
        return json.load(f)


def zeta_minus_1(s, N=1000):
    """zeta(s) - 1 = sum_{n >= 2} n^-s: the terms below N, then Euler-Maclaurin's integral, half term and first correction
    (the next one is of order s^3 N^(-s-3) / 720 < 1e-15 for s >= 3)"""
    n = np.arange(2, N, dtype=np.float64)
    return float(np.sum(n ** -s) + N ** (1.0 - s) / (s - 1.0) + 0.5 * N ** -s + s * N ** (-s - 1.0) / 12.0)


def test_surface_declares_and_binds_the_entry_point():
    from literate_amd import _hip, build
    header = open(os.path.join(ROOT, "include", "literate_hip.h")).read()
    assert "int lr_shift_prior(" in header and "#define LR_SHIFT_PRIOR_KCAP 64" in header
    assert "lr_prior.hip" in build.SOURCES
    res, args = _hip.SIGNATURES["lr_shift_prior"]
    assert res is _hip.c_i32 and len(args) == 12
    assert _hip.LR_SHIFT_PRIOR_KCAP == ref.KCAP == 64
    assert ("#define LR_SHIFT_PRIOR_BLOCKS %d" % _hip.LR_SHIFT_PRIOR_BLOCKS) in header
    src = open(os.path.join(ROOT, "literate_amd", "csrc", "lr_prior.hip")).read()
    assert ("#define LR_P_SHIFT_PRIOR %d" % ref.P_SHIFT_PRIOR) in src


def test_k_follows_the_gamma_mixture_of_truncated_poissons():
    """P(K = k) = (k + 1) (zeta(k + 2) - 1): the Gamma(2, 1) mixture of zero-truncated Poissons,
    int l e^-l  e^-l l^k / (k! (1 - e^-l)) dl = (k + 1) sum_{n >= 2} n^-(k+2).  Each k <= 8 of 2^20 replicates within five
    binomial standard errors."""
    n = 1 << 20
    K, capped = ref.draw_k(ref.replicates(0, n), seed=12345)
    assert not capped.any() and K.min() >= 1
    total = 0.0
    for k in range(1, 9):
        p = (k + 1) * zeta_minus_1(k + 2)
        total += p
        got = np.mean(K == k)
        se = np.sqrt(p * (1 - p) / n)
        print("k %d: %.5f against %.5f, %.2f standard errors" % (k, got, p, (got - p) / se))
        assert abs(got - p) < 5 * se, (k, got, p)
    assert abs(zeta_minus_1(3) - 0.2020569031595943) < 1e-14 and 0.98 < total < 1.0


def test_fixed_lambda_k_is_the_truncated_poisson():
    n = 1 << 16
    lam = 0.5
    K, capped = ref.draw_k(ref.replicates(7, n), seed=3, poi_lambda=lam)
    assert not capped.any()
    p, fact = [], 1.0
    for k in range(1, 5):
        fact *= k
        p.append(np.exp(-lam) * lam ** k / fact / (1 - np.exp(-lam)))
    for k, pk in enumerate(p, 1):
        assert abs(np.mean(K == k) - pk) < 5 * np.sqrt(pk * (1 - pk) / n), k


@pytest.fixture(scope="module")
def helper_runs(fixture_runs):
    """the restatement at 2^18 replicates on the fixture's two spans (computed once)"""
    return [ref.shift_prior_ref(c["a"], c["b"], 0, 1 << 18, 2020) for c in fixture_runs["cases"]]


@pytest.mark.parametrize("case", [0, 1])
def test_prior_s_agrees_with_the_reference_loop(fixture_runs, helper_runs, case):
    """prior_s of the restatement against the mean of the reference's 16 runs.  The standard error of the difference comes
    from the reference's own run-to-run spread s (16 runs of 100 000 replicates): s^2 / 16 for their mean plus
    s^2 * 100 000 / n for a run of n replicates here; the bound is five of those."""
    from literate_amd import shift_bf
    c, h = fixture_runs["cases"][case], helper_runs[case]
    runs = np.array(c["runs"])
    assert runs.shape == (16, 3) and fixture_runs["reps"] == 100000
    n = int(h.k_drawn.sum())
    s2 = runs[:, 0].var(ddof=1)
    se = np.sqrt(s2 / 16 + s2 * fixture_runs["reps"] / n)
    got = shift_bf.prior_s(h.shift_hist, h.totals[0])
    print("span (%s, %s): prior_s %.6f against %.6f +- %.6f (%.2f standard errors), acceptance %.4f"
          % (c["a"], c["b"], got, runs[:, 0].mean(), se, (got - runs[:, 0].mean()) / se, h.totals[0] / n))
    assert abs(got - runs[:, 0].mean()) < 5 * se
    # the bookkeeping of the restatement itself
    assert h.totals[0] == h.accept.sum() == h.k_accepted.sum() and h.totals[2] == 0
    assert h.totals[3] == (h.K[h.accept] - 1).sum() and h.totals[1] == h.shift_hist.sum() <= h.totals[3]
    assert len(h.shift_hist) == int(c["b"] - c["a"])


def test_thresholds_are_the_reference_expression(fixture_runs):
    from literate_amd import shift_bf
    for c in fixture_runs["cases"]:
        for ps, bf2, bf6 in c["runs"]:
            g2, g6 = shift_bf.thresholds(ps)
            assert abs(g2 - bf2) <= 1e-15 * bf2 and abs(g6 - bf6) <= 1e-15 * bf6
            assert shift_bf.calc_bf(2, ps) == g2 and shift_bf.calc_bf(6, ps) == g6
            # calcBF inverts two_ln_bf
            assert abs(shift_bf.two_ln_bf(g2, ps) - 2) < 1e-12 and abs(shift_bf.two_ln_bf(g6, ps) - 6) < 1e-12


def test_prior_s_is_the_mean_of_the_bin_frequencies():
    from literate_amd import shift_bf
    hist = np.array([3, 0, 5, 12], dtype=np.int64)
    assert shift_bf.prior_s(hist, 40) == np.mean(hist / 40.0)
    assert shift_bf.prior_s(hist, 0) == 0.0 and shift_bf.prior_s(np.zeros(3), 10) == 0.0
    assert shift_bf.thresholds(0.0) == (0.0, 0.0)


def test_edge_values_of_two_ln_bf_and_flags():
    from literate_amd import shift_bf
    pi = 0.02
    bf2, bf6 = shift_bf.thresholds(pi)
    f = np.array([0.0, 1.0, bf2, bf6, np.nextafter(bf2, 0), np.nextafter(bf6, 0), pi, 0.5])
    v = shift_bf.two_ln_bf(f, pi)
    assert v[0] == -np.inf and v[1] == np.inf and v[6] == 0.0
    assert abs(v[2] - 2) < 1e-12 and abs(v[3] - 6) < 1e-12
    assert np.all(np.isnan(shift_bf.two_ln_bf(f, 0.0))) and np.isnan(shift_bf.two_ln_bf(0.3, 0.0))
    assert isinstance(shift_bf.two_ln_bf(0.3, pi), float)
    rate = np.arange(1.0, 9.0)
    b2, b6 = shift_bf.flags(f, rate, bf2, bf6)
    #                 f = 0    1     bf2   bf6   <bf2   <bf6   pi    .5
    assert np.array_equal(np.isnan(b2), [True, True, False, True, True, False, True, True])
    assert np.array_equal(np.isnan(b6), [True, False, True, False, True, True, True, False])
    assert b2[2] == 3.0 and b2[5] == 6.0 and b6[1] == 2.0 and b6[3] == 4.0 and b6[7] == 8.0
    # an empty prior: thresholds 0, Bayes factors NaN, nothing raises
    z2, z6 = shift_bf.thresholds(shift_bf.prior_s(np.zeros(2), 0))
    assert (z2, z6) == (0.0, 0.0)
    e2, e6 = shift_bf.flags(np.array([0.0, 0.1]), np.array([1.0, 2.0]), z2, z6)
    assert np.all(np.isnan(e2)) and np.array_equal(e6, [1.0, 2.0])


def test_k_bayes_factor():
    from literate_amd import shift_bf
    post = np.zeros(32, dtype=np.int64)
    post[:3] = [600, 300, 100]
    pri = np.zeros(64, dtype=np.int64)
    pri[:4] = [500, 300, 150, 50]
    assert abs(shift_bf.k_bayes_factor(post, pri) - 2 * np.log((400 / 600) / (500 / 500))) < 1e-15
    only_one = np.zeros(32, dtype=np.int64)
    only_one[0] = 10
    assert shift_bf.k_bayes_factor(only_one, pri) == -np.inf
    never_one = np.zeros(32, dtype=np.int64)
    never_one[1] = 10
    assert shift_bf.k_bayes_factor(never_one, pri) == np.inf
    assert np.isnan(shift_bf.k_bayes_factor(np.zeros(32), pri))
    assert np.isnan(shift_bf.k_bayes_factor(post, np.zeros(64))) and np.isnan(shift_bf.k_bayes_factor(post, only_one))


def test_tables_headers_and_round_trip(tmp_path, helper_runs):
    from literate_amd import logs, ops, shift_bf
    h = helper_runs[1]                                    # (0, 12.5): 12 bins
    nb = len(h.shift_hist)
    time = ops.rtt_time(0.0, 12.5)
    rng = np.random.default_rng(4)
    rates = rng.uniform(0.1, 0.9, (3, 3, nb))
    freq = rng.uniform(0.0, 0.3, (2, nb))
    freq[0, 0], freq[1, 3], freq[0, 5] = 0.0, 1.0, 0.6
    kc = np.zeros((2, 32), dtype=np.int64)
    kc[0, :3], kc[1, :2] = [700, 250, 50], [900, 100]
    stem = str(tmp_path / "run")
    ps, bf2, bf6 = logs.write_rtt_bf_tables(stem, time, rates, freq, kc, h.totals, h.shift_hist, h.k_accepted, 1 << 18)
    assert ps == shift_bf.prior_s(h.shift_hist, h.totals[0]) and (bf2, bf6) == shift_bf.thresholds(ps)
    lines = open(stem + "_RTT_BF.tsv").read().split("\n")
    assert lines[0].split("\t") == logs.RTT_BF_HEAD and len(lines) == nb + 2 and lines[-1] == ""
    tab = np.loadtxt(stem + "_RTT_BF.tsv", skiprows=1)
    assert np.array_equal(tab[:, 0], time) and np.array_equal(tab[:, 1], freq[0]) and np.array_equal(tab[:, 2], freq[1])
    assert np.array_equal(tab[:, 3], h.shift_hist / float(h.totals[0]))
    for col, want in ((4, shift_bf.two_ln_bf(freq[0], ps)), (5, shift_bf.two_ln_bf(freq[1], ps)),
                      (6, shift_bf.flags(freq[0], rates[0, 0], bf2, bf6)[0]), (7, shift_bf.flags(freq[0], rates[0, 0], bf2, bf6)[1]),
                      (8, shift_bf.flags(freq[1], rates[1, 0], bf2, bf6)[0]), (9, shift_bf.flags(freq[1], rates[1, 0], bf2, bf6)[1])):
        assert np.array_equal(tab[:, col], want, equal_nan=True), col
    assert tab[0, 4] == -np.inf and tab[3, 5] == np.inf and tab[5, 7] == rates[0, 0, 5] and np.isnan(tab[5, 6])
    assert lines[1].split("\t")[4] == "-inf" and lines[1].split("\t")[0] == str(float(time[0]))
    pl = open(stem + "_RTT_BF_prior.tsv").read().split("\n")
    assert pl[0].split("\t") == logs.RTT_BF_PRIOR_HEAD and len(pl) == 3
    row = pl[1].split("\t")
    assert row[:3] == [str(1 << 18), str(int(h.totals[0])), "0"] and row[3] == "0.0"
    assert [float(x) for x in row[4:7]] == [ps, bf2, bf6] and row[5] == str(bf2)
    assert float(row[7]) == shift_bf.k_bayes_factor(kc[0], h.k_accepted)
    assert float(row[8]) == shift_bf.k_bayes_factor(kc[1], h.k_accepted)
    kl = open(stem + "_RTT_BF_K.tsv").read().split("\n")
    assert kl[0].split("\t") == logs.RTT_BF_K_HEAD and len(kl) == 64 + 2
    K = np.loadtxt(stem + "_RTT_BF_K.tsv", skiprows=1)
    assert K[:, 0].tolist() == list(range(1, 65))
    assert np.array_equal(K[:, 1], h.k_accepted / float(h.totals[0]))
    assert np.array_equal(K[:32, 2], kc[0] / 1000.0) and np.array_equal(K[:32, 3], kc[1] / 1000.0) and not K[32:, 2:].any()
    # an empty prior (a span that accepts no shift) writes zeros and NaN, and does not raise
    empty = np.zeros(1, dtype=np.int64)
    ps0, z2, z6 = logs.write_rtt_bf_tables(stem + "_e", time[:1], rates[:, :, :1], freq[:, :1], kc, np.zeros(4, dtype=np.int64),
                                           empty, np.zeros(64, dtype=np.int64), 100, 0.5)
    assert (ps0, z2, z6) == (0.0, 0.0, 0.0)
    e = open(stem + "_e_RTT_BF.tsv").read().split("\n")[1].split("\t")
    assert e[3] == "0.0" and e[4] == "nan" and e[5] == "nan"
    assert open(stem + "_e_RTT_BF_prior.tsv").read().split("\n")[1].split("\t")[3] == "0.5"


def test_cli_refuses_bad_rtt_bf_before_touching_a_device(monkeypatch):
    import importlib
    import torch
    from literate_amd import _hip

    def no_device(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(_hip, "require_gpu", no_device)
    mod = importlib.import_module("LiteRateForward")
    args = mod.build_parser().parse_args(["-d", "x.tsv"])
    assert args.rtt_bf == 0 and args.rtt_bf_lambda == 0.0                      # off by default
    with pytest.raises(SystemExit, match="needs --rtt BURNIN"):
        mod.main(["-d", "x.tsv", "--rtt_bf", "1000"])
    with pytest.raises(SystemExit, match="between 1 and 2\\^40"):
        mod.main(["-d", "x.tsv", "--rtt", "0.2", "--rtt_bf", "-5"])
    with pytest.raises(SystemExit, match="between 1 and 2\\^40"):
        mod.main(["-d", "x.tsv", "--rtt", "0.2", "--rtt_bf", str((1 << 40) + 1)])
    with pytest.raises(SystemExit, match="needs --rtt_bf"):
        mod.main(["-d", "x.tsv", "--rtt", "0.2", "--rtt_bf_lambda", "2"])
    for bad in ("-1", "701", "nan"):
        with pytest.raises(SystemExit, match="rtt_bf_lambda takes"):
            mod.main(["-d", "x.tsv", "--rtt", "0.2", "--rtt_bf", "1000", "--rtt_bf_lambda", bad])
    from literate_amd.logs import rtt_bf_arg_error
    assert rtt_bf_arg_error(0, 0.0, -1.0) is None and rtt_bf_arg_error(1000, 0.0, 0.2) is None
    assert rtt_bf_arg_error(1 << 40, 700.0, 0.0) is None


def test_shift_prior_has_no_cpu_path(monkeypatch):
    import torch
    from literate_amd import _hip, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.HipLibraryError):
        ops.shift_prior(0.0, 12.5, n_reps=100)
