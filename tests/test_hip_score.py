"""The grouped summary and its score on the device (include/literate_hip_score.h, csrc/lr_score.hip, literate_amd/simstudy.py):
  1. bit parity with lr_rtt_summary(pooled) on every group's slice, on an engine's trace and on rows written here, at the
     sizes where the kernel takes another path (the block width, the cap, the padding, bins, groups beyond 65 535);
  2. covered and score against tests/helpers/score_ref.py, truths on the ends of a band included;
  3. independence: of the other groups, of what the buffers held, of a truth being given;
  4. the stream contract on a busy side stream;  5. refusals that leave every byte;
  6. the whole study, deterministic, against the restatement;  7. that a wrong truth and a real shift show."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import score_ref as R          # noqa: E402

pytestmark = pytest.mark.gpu

KMAX, HEAD = 32, 13
W = HEAD + 2 * (2 * KMAX - 1)
COL_L, COL_TL, COL_M, COL_TM = HEAD, HEAD + KMAX, HEAD + 2 * KMAX - 1, HEAD + 3 * KMAX - 1
EPS = 2.0 ** -52


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def make_rows(S, Cn, a, nb, seed):
    """[S, Cn, W] trace rows written here: K_l, K_m 1 .. LR_KMAX (both ends forced), half the rows with their shift times in
    descending order, times outside the edges, exactly on the first, the last and inner edges, rates on a grid of eighths in
    half the rows (ties, and equal birth and death rates: exact zeros in the net column), and the last two samples of chain 0
    - kept behind any burn-in, both in group 0 - with all rates equal"""
    rng = np.random.default_rng(seed)
    n = S * Cn
    rows = np.zeros((n, W))
    rows[:, 0] = np.arange(n)
    K = rng.integers(1, KMAX + 1, size=(n, 2))
    K[rng.random((n, 2)) < 0.3] = 1
    K[rng.random((n, 2)) < 0.1] = 2
    K[0], K[n - 1] = (KMAX, 1), (1, KMAX)
    rows[:, 6:8] = K
    rows[:, 8], rows[:, 9] = a, a + nb + 0.5
    for col_r, col_t in ((COL_L, COL_TL), (COL_M, COL_TM)):
        rates = rng.gamma(2.0, 0.2, size=(n, KMAX)) + 1e-3
        grid = rng.random(n) < 0.5
        rates[grid] = np.ceil(rates[grid] * 8.0) / 8.0
        rows[:, col_r:col_r + KMAX] = rates
        t = rng.uniform(a - 1.0, a + nb + 1.5, size=(n, KMAX - 1))
        on_edge = rng.random((n, KMAX - 1)) < 0.15
        t[on_edge] = a + rng.integers(0, nb + 1, size=int(on_edge.sum()))
        t = np.sort(t, axis=1)
        desc = rng.random(n) < 0.5
        t[desc] = t[desc, ::-1]
        mixed = rng.random(n) < 0.25
        t[mixed] = rng.permuted(t[mixed], axis=1)
        rows[:, col_t:col_t + KMAX - 1] = t
    same = [(S - 1) * Cn, (S - 2) * Cn]
    rows[same, COL_L:COL_L + KMAX] = 0.375
    rows[same, COL_M:COL_M + KMAX] = 0.375
    return rows.reshape(S, Cn, W)


def parity(torch, ops, trace, S, cpg, a, b, burnin, groups=None, truth=None):
    res = ops.rtt_score(trace, S, cpg, a, b, truth=truth, burnin=burnin)
    G = trace.shape[1] // cpg
    assert tuple(res.rates.shape) == (G, 3, 3, res.time.size) and res.n_samples == cpg * (S - int(burnin * S))
    for g in (range(G) if groups is None else groups):
        ref = ops.rtt_summary(trace[:, g * cpg:(g + 1) * cpg].contiguous(), S, a, b, burnin, pooled=True)
        assert ref.n_samples == res.n_samples and np.array_equal(ref.time, res.time)
        for name in ("rates", "shift_freq", "k_counts"):
            got, want = getattr(res, name)[g], getattr(ref, name)[0]
            assert got.dtype == want.dtype and torch.equal(got, want), "group %d of %d: %s differs (n = %d)" % (g, G, name, res.n_samples)
    return res


# ---- 1. bit parity --------------------------------------------------------------------------------------------------------------
# (S, chains per group, groups, bins, burn-in): n = chains per group x (S - int(burnin S)) samples per group
SHAPES = [(2, 1, 3, 5, 0.0),            # n = 2: the smallest with n_in = 2
          (3, 1, 2, 5, 0.0), (37, 1, 3, 12, 0.0),
          (255, 1, 2, 12, 0.0), (256, 1, 2, 12, 0.0), (257, 1, 2, 12, 0.0),          # the block width
          (4095, 1, 2, 3, 0.0), (4096, 1, 1, 12, 0.0), (2048, 2, 2, 2, 0.0),        # the padding and the cap (one group; two chains)
          (50, 1, 3, 12, 0.2), (50, 2, 3, 12, 0.2), (50, 3, 2, 12, 0.3),            # the pooled row mapping behind a burn-in
          (40, 1, 2, 1, 0.1), (40, 2, 2, 2, 0.1), (40, 1, 3, 65, 0.1), (64, 2, 2, 512, 0.25)]          # bins


@pytest.mark.parametrize("S,cpg,G,nb,burnin", SHAPES, ids=["S%d-c%d-G%d-b%d-burn%g" % s for s in SHAPES])
def test_1_bit_parity_on_rows_written_here(S, cpg, G, nb, burnin):
    import torch
    from literate_amd import ops
    a = 3.25
    trace = torch.as_tensor(make_rows(S, G * cpg, a, nb, 100 + S + nb), device="cuda")
    res = parity(torch, ops, trace, S, cpg, a, a + nb + 0.5, burnin)
    assert res.time.size == nb and res.covered is None and res.score is None
    rates = res.rates.cpu().numpy()
    assert np.isfinite(rates).all() and (res.k_counts.sum(dim=2) == res.n_samples).all() and (rates[:, :, 1] <= rates[:, :, 2]).all()


def test_1_bit_parity_on_an_engines_trace():
    import torch
    from literate_amd import ops
    from literate_amd.replicates import ReplicateEngine, Replicates
    rng = np.random.default_rng(5)
    Rn, nb, cpr, S = 4, 12, 2, 120
    br = 15.0 + 10.0 * rng.random((Rn, nb))
    lam = np.where(np.arange(nb) < 6, 0.15, 0.6)
    reps = Replicates.from_counts(rng.poisson(lam * br), rng.poisson(0.1 * br), br, 0.0, nb + 0.5)
    eng = ReplicateEngine(reps, Rn * cpr, model=0, seed=3, s_freq=5, n_trace_slots=S)
    eng.init()
    eng.steps(S * 5)
    eng.check_status()
    res = parity(torch, ops, eng.trace, S, cpr, 0.0, nb + 0.5, 0.2)
    assert res.n_samples == 2 * 96 and float(res.shift_freq.sum()) > 0.0
    parity(torch, ops, eng.trace, S, 1, 0.0, nb + 0.5, 0.1)
    eng.close()


def test_1_more_groups_than_grid_y_holds():
    import torch
    from literate_amd import ops
    G, nb, a = 65537, 3, 0.0
    rng = np.random.default_rng(9)
    base = make_rows(2, 4096, a, nb, 77)
    pick = rng.integers(0, 4096, size=G)
    trace = torch.as_tensor(np.ascontiguousarray(base[:, pick]), device="cuda")
    groups = sorted(set(np.linspace(0, G - 1, 62).astype(int).tolist() + [65534, 65535, 65536]))[:64]
    assert len(groups) == 64 and groups[-1] == G - 1 and 65535 in groups
    res = parity(torch, ops, trace, 2, 1, a, a + nb + 0.5, 0.0, groups=groups)
    # every group, against the groups that read the same two rows
    first = {}
    for g, p in enumerate(pick.tolist()):
        first.setdefault(p, g)
    src = torch.as_tensor(np.array([first[p] for p in pick.tolist()]), device="cuda")
    assert torch.equal(res.rates, res.rates[src]) and torch.equal(res.k_counts, res.k_counts[src]) and torch.equal(res.shift_freq, res.shift_freq[src])


# ---- 2. scoring -----------------------------------------------------------------------------------------------------------------
def check_score(score, rates, truth, label=""):
    """columns 0 and 1 exact; the four sums within G 2^-52 (sum |terms| / G), the bound of a reordered sum - the root of
    column 4 compared as its square.  (The device's own roundings - the terms' products, at most ceil(G / 256) serial adds
    and the eight levels of the tree, the division and the root - are about 11 x 2^-53 of the same magnitude: well inside.)"""
    want, mag = R.score(rates, truth)
    G = rates.shape[0]
    assert np.array_equal(score[:, :, 0], want[:, :, 0]) and np.array_equal(score[:, :, 1], want[:, :, 1]), label
    for col, m in ((2, 0), (3, 1), (4, 2), (5, 3)):
        got, ref = (score[:, :, col] ** 2, want[:, :, col] ** 2) if col == 4 else (score[:, :, col], want[:, :, col])
        bound = G * EPS * mag[:, :, m]
        err = np.abs(got - ref)
        print("%s column %d: largest error %.3g of bound %.3g" % (label, col, float((err / np.maximum(bound, 1e-300)).max()), 1.0))
        assert (err <= bound).all(), (label, col, float(err.max()))


def test_2_covered_and_score_are_the_restatements():
    import torch
    from literate_amd import ops
    S, cpg, G, nb, a = 20, 2, 300, 7, 1.5          # 300 groups: a thread of the table kernel adds two of them
    trace = torch.as_tensor(make_rows(S, G * cpg, a, nb, 21), device="cuda")
    plain = ops.rtt_score(trace, S, cpg, a, a + nb + 0.5, burnin=0.1)
    rates = plain.rates.cpu().numpy()
    rng = np.random.default_rng(4)
    truth = rates[:, :2, 0] * rng.uniform(0.3, 1.7, size=(G, 2, nb))          # around the means: in and out of the band
    truth[0::7] = rates[0::7, :2, 1]          # ... on the low end of the band
    truth[3::7] = rates[3::7, :2, 2]          # ... on the high end
    truth[5::7] = np.nextafter(rates[5::7, :2, 2], np.inf)          # ... and just outside
    res = ops.rtt_score(trace, S, cpg, a, a + nb + 0.5, truth=truth, burnin=0.1)
    assert torch.equal(res.rates, plain.rates) and torch.equal(res.shift_freq, plain.shift_freq) and torch.equal(res.k_counts, plain.k_counts)
    cov = res.covered.cpu().numpy()
    assert cov.dtype == np.int32 and np.array_equal(cov, R.covered(rates, truth))
    assert cov[0::7, :2].all() and cov[3::7, :2].all() and not cov[5::7, :2].any() and 0 < cov.mean() < 1
    check_score(res.score.cpu().numpy(), rates, truth, "per-group truth")
    # one truth for every group, [2, n_bins]
    one = np.stack([np.full(nb, 0.4), np.full(nb, 0.375)])
    res1 = ops.rtt_score(trace, S, cpg, a, a + nb + 0.5, truth=one, burnin=0.1)
    assert np.array_equal(res1.covered.cpu().numpy(), R.covered(rates, one))
    check_score(res1.score.cpu().numpy(), rates, one, "shared truth")


# ---- 3. independence ------------------------------------------------------------------------------------------------------------
def test_3_permuting_the_groups_permutes_their_outputs():
    import torch
    from literate_amd import ops
    S, cpg, G, nb, a = 30, 3, 11, 9, 0.0
    rows = make_rows(S, G * cpg, a, nb, 31)
    rng = np.random.default_rng(2)
    truth = rng.uniform(0.1, 0.8, size=(G, 2, nb))
    perm = rng.permutation(G)
    chains = (perm[:, None] * cpg + np.arange(cpg)[None]).ravel()
    one = ops.rtt_score(torch.as_tensor(rows, device="cuda"), S, cpg, a, a + nb + 0.5, truth=truth, burnin=0.2)
    two = ops.rtt_score(torch.as_tensor(np.ascontiguousarray(rows[:, chains]), device="cuda"), S, cpg, a, a + nb + 0.5, truth=truth[perm], burnin=0.2)
    p = torch.as_tensor(perm, device="cuda")
    for name in ("rates", "shift_freq", "k_counts", "covered"):
        assert torch.equal(getattr(two, name), getattr(one, name)[p]), name
    assert torch.equal(two.score[:, :, :2], one.score[:, :, :2]), "the count and the coverage do not depend on the order"
    assert np.array_equal(two.covered.cpu().numpy(), R.covered(two.rates.cpu().numpy(), truth[perm]))
    # a group alone gives what it gives among the others
    g = 4
    alone = ops.rtt_score(torch.as_tensor(np.ascontiguousarray(rows[:, g * cpg:(g + 1) * cpg]), device="cuda"), S, cpg, a, a + nb + 0.5, truth=truth[g:g + 1], burnin=0.2)
    assert torch.equal(alone.rates[0], one.rates[g]) and torch.equal(alone.covered[0], one.covered[g]) and torch.equal(alone.k_counts[0], one.k_counts[g])


@pytest.mark.parametrize("with_truth", [True, False])
def test_3_the_outputs_do_not_depend_on_what_the_buffers_held(with_truth):
    """exact-size buffers between guards, filled with 0xFF (NaN bytes) and with zeros: the same bits, every payload byte
    written, a second call on the dirty buffers the same again"""
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    S, cpg, G, nb, a = 25, 2, 5, 6, 0.0
    trace = torch.as_tensor(make_rows(S, G * cpg, a, nb, 41), device="cuda")
    truth = torch.as_tensor(np.random.default_rng(1).uniform(0.1, 0.8, size=(G, 2, nb)), device="cuda") if with_truth else None
    out = contract(ops, torch, lambda: ops.rtt_score(trace, S, cpg, a, a + nb + 0.5, truth=truth, burnin=0.2), label="rtt_score")
    assert (out.covered is None) == (not with_truth) and (out.score is None) == (not with_truth)


def test_3_without_a_truth_nothing_else_is_written():
    import torch
    from literate_amd import _hip, ops
    S, cpg, G, nb, a = 25, 2, 5, 6, 0.0
    trace = torch.as_tensor(make_rows(S, G * cpg, a, nb, 41), device="cuda")
    want = ops.rtt_score(trace, S, cpg, a, a + nb + 0.5, burnin=0.2)
    rates, freq, kc = torch.empty_like(want.rates), torch.empty_like(want.shift_freq), torch.empty_like(want.k_counts)
    covered = torch.full((G, 3, nb), -7, dtype=torch.int32, device="cuda")
    score = torch.full((3, nb, 6), -7.0, dtype=torch.float64, device="cuda")
    prob = _hip.RttScoreProblem(_hip.ptr(trace), None, _hip.ptr(rates), _hip.ptr(freq), _hip.ptr(kc), _hip.ptr(covered), _hip.ptr(score),
                                S, G * cpg, cpg, 0, a, a + nb + 0.5, 0.2, None)
    assert _hip.launch_problem(_hip.load().lr_rtt_score, trace.device, prob) == 0
    torch.cuda.synchronize()
    assert torch.equal(rates, want.rates) and torch.equal(freq, want.shift_freq) and torch.equal(kc, want.k_counts)
    assert bool((covered == -7).all()) and bool((score == -7.0).all())


# ---- 4. the stream --------------------------------------------------------------------------------------------------------------
def test_4_the_stream_contract_on_a_busy_side_stream():
    """lr_rtt_score takes the stream in its descriptor, so it is not among the functions helpers/stream_cases finds by their
    last parameter: the library handed to TorchRuntime is an adapter with the stream last, which puts it into the descriptor
    and calls the entry point.  The trace and the truth are the inputs copied behind the delay."""
    import torch
    from helpers import stream_cases as S
    from literate_amd import _hip, ops
    lib = _hip.load()
    Sn, cpg, G, nb, a = 40, 2, 6, 8, 0.0

    def score(prob, stream):
        prob.stream = stream
        return lib.lr_rtt_score(C.byref(prob))
    adapters = types.SimpleNamespace(lr_rtt_score=score)
    rt = S.TorchRuntime(library=(adapters, ["lr_rtt_score"]))

    def make(seed):
        return make_rows(Sn, G * cpg, a, nb, seed), np.random.default_rng(seed).uniform(0.1, 0.8, size=(G, 2, nb))

    def call(trace, truth):
        out = dict(rates=ops.alloc_output((G, 3, 3, nb), torch.float64, "cuda"), shift_freq=ops.alloc_output((G, 2, nb), torch.float64, "cuda"),
                   k_counts=ops.alloc_output((G, 2, KMAX), torch.int64, "cuda"), covered=ops.alloc_output((G, 3, nb), torch.int32, "cuda"),
                   score=ops.alloc_output((3, nb, 6), torch.float64, "cuda"))
        prob = _hip.RttScoreProblem(_hip.ptr(trace), _hip.ptr(truth), _hip.ptr(out["rates"]), _hip.ptr(out["shift_freq"]), _hip.ptr(out["k_counts"]),
                                    _hip.ptr(out["covered"]), _hip.ptr(out["score"]), Sn, G * cpg, cpg, 0, a, a + nb + 0.5, 0.2, None)
        assert adapters.lr_rtt_score(prob, rt.current_stream_arg()) == 0
        return out
    a_in, b_in = [S.dev(torch, x) for x in make(50)], [S.dev(torch, x) for x in make(51)]
    bufs = [torch.empty_like(x) for x in a_in]
    want, table = S.ordered(rt, lambda: call(*bufs), a_in, b_in, bufs, "rtt_score")
    assert table["lr_rtt_score"]["calls"] == 1
    ref = ops.rtt_score(a_in[0], Sn, cpg, a, a + nb + 0.5, truth=a_in[1], burnin=0.2)
    assert np.array_equal(np.frombuffer(want["rates"]).reshape(G, 3, 3, nb), ref.rates.cpu().numpy())
    assert np.array_equal(np.frombuffer(want["score"]).reshape(3, nb, 6), ref.score.cpu().numpy())


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_5_refusals_leave_every_output_byte_as_it_was():
    import torch
    from helpers.abi_cases import refuses
    from literate_amd import ops
    nb, a = 6, 0.0
    small = torch.as_tensor(make_rows(10, 6, a, nb, 3), device="cuda")
    long = torch.zeros((4097, 1, W), dtype=torch.float64, device="cuda")
    truth = torch.full((2, nb), 0.25, dtype=torch.float64, device="cuda")
    for what, call in (
            ("n = 4097", lambda: ops.rtt_score(long, 4097, 1, a, a + nb + 0.5, truth=truth, burnin=0.0)),
            ("6 chains in groups of 4", lambda: ops.rtt_score(small, 10, 4, a, a + nb + 0.5, burnin=0.2)),
            ("an integer span", lambda: ops.rtt_score(small, 10, 2, a, a + nb + 1.0, burnin=0.2)),
            ("burn-in 1.0", lambda: ops.rtt_score(small, 10, 2, a, a + nb + 0.5, truth=truth, burnin=1.0)),
            ("n_in = 1", lambda: ops.rtt_score(small, 1, 1, a, a + nb + 0.5, burnin=0.0))):
        refuses(ops, torch, call, "LR_ERR_SIZE", label=what, entry="lr_rtt_score")
    with pytest.raises(ValueError, match=r"lr_rtt_score: LR_ERR_SIZE \(6 chains are not a multiple of chains_per_group = 4\)"):
        ops.rtt_score(small, 10, 4, a, a + nb + 0.5, burnin=0.2)
    for cpg in (0, -2):
        with pytest.raises(ValueError, match="chains_per_group must be at least 1"):
            ops.rtt_score(small, 10, cpg, a, a + nb + 0.5, burnin=0.2)
    ok = ops.rtt_score(long[:4096], 4096, 1, a, a + nb + 0.5, burnin=0.0)          # the cap itself is served (rows of zeros: K clamped to 1)
    assert ok.n_samples == 4096 and bool((ok.rates == 0.0).all()) and int(ok.k_counts[0, 0, 0]) == 4096


# ---- 6. the whole study ---------------------------------------------------------------------------------------------------------
NB = 12
CONSTANT = np.stack([np.full(NB, 0.3), np.full(NB, 0.1)])
STEP = np.stack([np.where(np.arange(NB) < 6, 0.15, 0.6), np.full(NB, 0.1)])
STUDY = dict(n_reps=64, chains_per_rep=1, n_iter=20000, s_freq=20, seed=7, n_start=200)


@pytest.fixture(scope="module")
def constant_run():
    from literate_amd import simstudy
    return simstudy.run(CONSTANT, keep_trace=True, **STUDY)


def check_tables(res, sc):
    from literate_amd import simstudy
    G = res.kept.size
    assert G >= 2 and res.rates.shape == (G, 3, 3, NB) and res.n_samples == 800
    assert np.array_equal(res.covered, R.covered(res.rates, sc))
    check_score(res.score, res.rates, sc, "study")
    sp, ex, br = res.counts[res.kept, 0].astype(float), res.counts[res.kept, 1].astype(float), res.counts[res.kept, 3] / 100.0
    assert np.array_equal(sp, res.sp) and np.array_equal(ex, res.ex) and np.array_equal(br, res.br)
    assert np.allclose(res.empirical, R.empirical(sp, ex, br, sc), rtol=1e-13, atol=0, equal_nan=True)
    ref = R.shifts(res.shift_freq, res.k_counts, sc, np.full(NB, res.prior_s), bf=6.0, tol=2)
    for k, kind in enumerate(("birth", "death")):
        r = ref[kind]
        assert list(res.shifts["true_bins"][k]) == r["true_bins"] and list(res.shifts["power"][k]) == r["power"]
        assert res.shifts["false_positive"][k] == r["false_positive"] and res.shifts["k_mode_share"][k] == r["k_mode_share"]
        assert res.shifts["k_mean"][k] == pytest.approx(r["k_mean"], rel=1e-13)
    assert np.array_equal(res.shifts["k_mode"], ref["k_mode"])
    lines = simstudy.rates_table(res).splitlines()
    assert len(lines) == 1 + 3 * NB and lines[1].split("\t")[:3] == ["birth", "0", str(float(sc[0, 0]))]
    assert [float(v) for v in lines[1].split("\t")[3:9]] == res.score[0, 0].tolist()


def test_6_the_tables_are_the_restatements(constant_run):
    import torch
    from literate_amd import ops, shift_bf
    res = constant_run
    check_tables(res, CONSTANT)
    assert (res.reason == 0).sum() == res.kept.size and res.totals.shape == (64, 4) and res.seeds.tolist() == list(range(7, 71))
    # the rates are the summary's on the engine's trace, the prior the one --rtt_bf computes
    for g in range(res.kept.size):
        ref = ops.rtt_summary(res.trace[:, g:g + 1].contiguous(), 1000, 0.0, NB + 0.5, 0.2, pooled=True)
        assert np.array_equal(ref.rates[0].cpu().numpy(), res.rates[g]) and np.array_equal(ref.shift_freq[0].cpu().numpy(), res.shift_freq[g]), g
        assert np.array_equal(ref.k_counts[0].cpu().numpy(), res.k_counts[g]), g
    prior = ops.shift_prior(0.0, NB + 0.5, n_reps=1 << 20, seed=7)
    assert res.prior_s == shift_bf.prior_s(prior.shift_hist.cpu().numpy(), int(prior.totals[0].item())) and 0 < res.prior_s < 1
    print("constant scenario, %d replicates: coverage birth %s death %s; false positives %s; K mode share %s" %
          (res.kept.size, res.score[0, :, 1].round(3).tolist(), res.score[1, :, 1].round(3).tolist(), res.shifts["false_positive"].tolist(),
           res.shifts["k_mode_share"].tolist()))
    assert set(res.seconds) == {"simulate", "sample", "score", "shifts"}


def test_6_a_second_run_gives_the_same_bytes(constant_run):
    from literate_amd import simstudy
    again = simstudy.run(CONSTANT, **STUDY)
    a, b = constant_run.arrays(), again.arrays()
    assert set(a) == set(b) and again.trace is None
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for table in (simstudy.rates_table, simstudy.shifts_table, simstudy.replicates_table):
        assert table(constant_run) == table(again)


def test_6_two_chains_per_replicate(constant_run):
    import torch
    from literate_amd import ops, simstudy
    res = simstudy.run(CONSTANT, keep_trace=True, **dict(STUDY, chains_per_rep=2))
    assert res.n_samples == 1600 and tuple(res.trace.shape) == (1000, 2 * res.kept.size, W)
    assert np.array_equal(res.kept, constant_run.kept) and np.array_equal(res.counts, constant_run.counts), "the same simulated data"
    ref = ops.rtt_summary(res.trace[:, 0:2].contiguous(), 1000, 0.0, NB + 0.5, 0.2, pooled=True)
    assert np.array_equal(ref.rates[0].cpu().numpy(), res.rates[0]) and np.array_equal(ref.shift_freq[0].cpu().numpy(), res.shift_freq[0])
    assert np.array_equal(ref.k_counts[0].cpu().numpy(), res.k_counts[0])
    assert np.array_equal(res.covered, R.covered(res.rates, CONSTANT))


# ---- 7. teeth -------------------------------------------------------------------------------------------------------------------
def test_7_a_wrong_truth_is_covered_less_often(constant_run):
    import torch
    from literate_amd import ops
    res = constant_run
    tripled = ops.rtt_score(res.trace, 1000, 1, 0.0, NB + 0.5, truth=3.0 * CONSTANT, burnin=0.2)
    assert np.array_equal(tripled.rates.cpu().numpy(), res.rates)
    wrong, right = tripled.score[0, :, 1].cpu().numpy(), res.score[0, :, 1]
    print("birth coverage per bin: true scenario %s, every rate tripled %s" % (right.round(3).tolist(), wrong.round(3).tolist()))
    assert (wrong < right).all()
    assert (np.abs(tripled.score[0, :, 2].cpu().numpy()) > np.abs(res.score[0, :, 2])).all(), "and the bias is larger"


def test_7_a_real_shift_is_reported_at_least_as_often_as_none(constant_run):
    from literate_amd import simstudy
    res = simstudy.run(STEP, **dict(STUDY, n_start=500))
    check_tables(res, STEP)
    assert list(res.shifts["true_bins"][0]) == [6] and res.shifts["ratio"][0].tolist() == [4.0] and res.shifts["k_true"].tolist() == [2, 1]
    near = np.abs(np.arange(NB) - 6) <= 2
    there = constant_run.shifts["reported"][:, 0, near].any(axis=1).mean()
    power = float(res.shifts["power"][0][0])
    print("birth shift within 2 bins of bin 6: step scenario %.3f of %d replicates, constant scenario %.3f of %d; step: coverage birth %s, "
          "false positives %s, K mode share %s" % (power, res.kept.size, there, constant_run.kept.size, res.score[0, :, 1].round(3).tolist(),
                                                     res.shifts["false_positive"].tolist(), res.shifts["k_mode_share"].tolist()))
    assert power >= there
