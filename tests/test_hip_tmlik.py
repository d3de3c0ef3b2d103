"""Marginal likelihoods of the trend_rate.py models on the device (include/literate_hip_tmlik.h, literate_amd/trend_mlik.py):

   1. the chains against the numpy restatement tests/helpers/tmlik_ref.py iteration by iteration, rtol 1e-9 / atol 1e-9 (the
      device evaluates t ** d as exp(d log t)): every flags value, 1, 2, 63, 64, 65 and 512 bins, ladders of 2, 9 and 15 chains per
      model (a last workgroup partly empty), 1, 3 and 64 models with two sharing a column and one column unused, windows 0.001
      and a table of distinct ones, covariates that hold the 1e-15 floor and an exact 1.0 - every case's seed such that no
      accept decision of the restatement is closer than 1e-6 to its threshold (asserted: a flipped decision cannot pass as
      rounding);
   2. the hottest chain of an EXPB_EXPD model at window 0.001 against oracle.trend_mcmc_oracle.run_trend_mcmc, the same way;
   3. a run cut into launches, into groups of replicates or into groups of models, bit for bit;
   4. exact-size, dirty, guarded buffers, and a launch at slot0 > 0 that leaves every other slot alone;
   5. every argument error in the header's order, the buffers untouched;
   6. trend_mlik.run on the shared problem of tests/test_tmlik_host.py (b): the same bound against the quadrature for all
      three models, the reported standard errors within a factor 2 of REF_SD / sqrt(R);
   7. the tuned windows and the null model's;
   8. lr_mlik_estimate on rows[m] of a 3-model run against the restatement's estimator at rtol 1e-12;
   9. both entry points on a busy side stream (tests/helpers/stream_cases.ordered);
  10. trend_rate.py --mlik end to end on a 3-column trend file, and the compare tool."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from helpers import mlik_ref
from helpers import tmlik_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IT = 300
MARGIN = 1e-6


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def synthetic(n_bins, n_cols, seed):
    """seeded statistics of n_bins bins and n_cols covariates, each normalised: its minimum at the 1e-15 floor, its maximum
    exactly 1 (one bin: a value inside)"""
    rng = np.random.default_rng(seed)
    DT = np.abs(20.0 + np.cumsum(rng.normal(size=n_bins) * 3.0)) + 1.0 + rng.random(n_bins)
    n_spec, n_exti = rng.poisson(0.3 * DT), rng.poisson(0.2 * DT)
    raw = np.cumsum(rng.normal(size=(n_cols, n_bins)), axis=1) + rng.random((n_cols, n_bins))
    trends = np.array([ref.normalise(x) for x in raw]) if n_bins > 1 else 0.2 + 0.6 * rng.random((n_cols, 1))
    if n_bins > 1:
        assert (trends.min(axis=1) == 1e-15).all() and (trends.max(axis=1) == 1.0).all()
    return ref.Problem(n_spec, n_exti, DT, trends)


def ladder(T):
    betas = ref.temperatures(T, 0.3)
    return betas, ref.window_scales(betas, 8.0)


def win_table(M, T):
    """distinct windows per (model, temperature), 0.002 .. a few"""
    return 0.002 * 1.35 ** (np.arange(M * T).reshape(M, T) % 23) + 1e-4 * np.arange(M * T).reshape(M, T)


# (n_bins, (T, R), col, flags, n_cols, table of windows?, seed, key0 of model 0)
CASES = [
    (1, (2, 1), [0], [0], 1, False, 11, 0),
    (2, (3, 3), [0], [1], 1, True, 12, 4),
    (63, (5, 3), [0], [2], 1, False, 13, 0),
    (64, (2, 1), [0], [3], 1, True, 14, 7),
    (65, (3, 3), [1, 1, 0], [0, 3, 2], 3, True, 15, 0),          # two models share column 1, column 2 is not used
    (512, (5, 3), [0, 2, 2], [1, 0, 3], 3, False, 16, 2),
    (5, (2, 1), [i % 2 for i in range(64)], [i % 4 for i in range(64)], 3, True, 17, 0),
]


@functools.lru_cache(maxsize=None)
def reference(i):
    """the restatement's run of case i, computed once -> (problem, grid arguments, wins, rows, state, margin)"""
    n_bins, (T, R), col, flags, n_cols, table, seed, k0 = CASES[i]
    P = synthetic(n_bins, n_cols, 100 + n_bins)
    betas, scales = ladder(T)
    M = len(col)
    key0 = [k0 + m * R for m in range(M)]
    wins = win_table(M, T) if table else np.full((M, T), 0.001)
    rows, state, margin = ref.run(P, col, flags, key0, betas, scales, wins, R, N_IT, 1, seed)
    return P, (col, flags, key0, betas, scales, R), wins, rows, state, margin


def dev_data(P):
    from literate_amd import ops
    return ops.TmlikData(P.n_spec, P.n_exti, P.DT, P.trends)


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    same_inf = np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(got)], want[np.isinf(want)])
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / (1e-9 + 1e-9 * np.abs(want[fin]))
    worst = float(err.max()) if err.size else 0.0
    print("%s: largest error %.3g of the tolerance" % (what, worst))
    if not (same_inf and worst <= 1.0 and np.isfinite(got[fin]).all()):
        at = np.argwhere(~np.isclose(got, want, rtol=1e-9, atol=1e-9))[:3]
        raise AssertionError("%s: differs first at %s: %s against %s" % (what, at.tolist(), got[tuple(at[0])], want[tuple(at[0])]))


def bits(ts):
    return [np.ascontiguousarray(t.cpu().numpy()).tobytes() for t in ts]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=["bins%d_T%dxR%d_M%d" % (c[0], c[1][0], c[1][1], len(c[2])) for c in CASES])
def test_1_the_chains_follow_the_restatement_iteration_by_iteration(i):
    import torch
    from literate_amd import ops
    P, grid_args, wins, want_rows, want_state, margin = reference(i)
    seed = CASES[i][6]
    print("smallest margin of an accept decision: %.3g" % margin)
    assert margin >= MARGIN, "choose another seed: a decision of the restatement is within rounding of its threshold"
    grid = ops.TmlikGrid(*grid_args)
    rows, state = ops.tmlik_run(dev_data(P), grid, torch.as_tensor(wins, device="cuda"), N_IT, 1, seed)
    rows, state = rows.cpu().numpy(), state.cpu().numpy()
    assert rows.shape == (grid.M, N_IT, grid.R, grid.T, ref.ROW_W) and state.shape == (grid.M, grid.R, grid.T, ref.STATE_W)
    close(rows, want_rows, "rows")
    close(state, want_state, "state")
    assert np.array_equal(state[..., ref.S_PROPOSED:ref.S_BETA], want_state[..., ref.S_PROPOSED:ref.S_BETA])            # proposals made and accepted
    assert np.array_equal(rows[..., ref.R_BETA], np.broadcast_to(grid.betas, rows.shape[:-1]))
    assert np.array_equal(rows[..., ref.R_WIN], np.broadcast_to(wins[:, None, None, :], rows.shape[:-1]))
    assert np.array_equal(rows[..., ref.R_MODEL], np.broadcast_to(np.arange(grid.M)[:, None, None, None], rows.shape[:-1]))
    assert np.array_equal(state[..., ref.S_WIN], np.broadcast_to(wins[:, None, :], state.shape[:-1]))
    acc = want_state[..., ref.S_ACCEPTED:ref.S_ACCEPTED + 2].sum()
    assert acc > 0.2 * N_IT * grid.M * grid.R * grid.T, "the restatement's chains hardly move: the case tests little"


def test_1_the_cases_cover_what_they_should():
    assert {c[0] for c in CASES} >= {1, 2, 63, 64, 65, 512} and {c[1] for c in CASES} == {(2, 1), (3, 3), (5, 3)}
    assert {len(c[2]) for c in CASES} == {1, 3, 64} and {f for c in CASES for f in c[3]} == {0, 1, 2, 3}
    assert {c[5] for c in CASES} == {False, True}
    shared = [c for c in CASES if len(c[2]) == 3 and len(set(c[2])) == 2 and c[4] == 3]
    assert shared, "two models share a column and one column is not used"
    t = np.unique(win_table(64, 2))
    assert t.size == 128 and t.min() >= 0.002


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
def test_2_the_hottest_chain_is_trend_rate_pys_own():
    from literate_amd import ops
    from oracle.trend_mcmc_oracle import PhiloxDraws, run_trend_mcmc
    z = np.load(os.path.join(ROOT, "tests", "golden", "ratemaps.npz"))
    P = ref.Problem(z["N_SPEC"], z["N_EXTI"], z["DT"], z["TREND"])
    T, R, seed, k0 = 3, 2, 23, 5
    betas, scales = ladder(T)
    assert betas[-1] == 1.0 and scales[-1] == 1.0
    grid = ops.TmlikGrid([0], [0], [k0], betas, scales, R)
    rows, _ = ops.tmlik_run(dev_data(P), grid, 0.001, N_IT, 1, seed)
    rows = rows.cpu().numpy()
    for r in range(R):
        draws = PhiloxDraws(seed, (k0 + r) * T + T - 1)
        with np.errstate(all="ignore"):
            o = np.array([w[:12] for w in run_trend_mcmc(P.n_spec, P.n_exti, P.DT, P.trends[0], draws, N_IT, 1)])
        ch = ref.Chain(P, 0, 0, 1.0, 1.0, 0.001)
        ref.run_chain(ch, PhiloxDraws(seed, (k0 + r) * T + T - 1), N_IT, 1)
        assert ch.margin >= MARGIN
        close(np.column_stack([rows[0, :, r, T - 1, 2:4], rows[0, :, r, T - 1, 4:10]]), np.column_stack([o[:, 2], o[:, 5], o[:, 6:12]]),
              "replicate %d at beta 1 against run_trend_mcmc" % r)
        assert len(set(o[:, 2])) > 50


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
def test_3_a_run_cut_into_launches_replicates_or_models_is_the_same_run():
    import torch
    from literate_amd import ops
    P = synthetic(65, 3, 9)
    data = dev_data(P)
    betas, scales = ladder(3)
    R, s, seed = 5, 7, 21                                  # s divides none of the cuts 100, 101
    grid = ops.TmlikGrid([0, 1, 1, 2, 0], [0, 1, 2, 3, 0], [3 + m * R for m in range(5)], betas, scales, R)
    wins = torch.as_tensor(win_table(5, 3), device="cuda")
    rows, state = ops.tmlik_run(data, grid, wins, N_IT, s, seed)
    assert rows.shape[1] == 43
    # launches: it0 and slot0
    st = ops.tmlik_init(data, grid, wins, seed)
    buf = torch.full_like(rows, -3.0)
    slot = 0
    for a, b in ((0, 100), (100, 101), (101, N_IT)):
        ops.tmlik_steps(data, grid, wins, st, a, b - a, s, seed, rows=buf, slot0=slot)
        slot += ops.rows_due(a, b - a, s)
    assert slot == 43 and bits([buf, st]) == bits([rows, state])
    # replicates: two groups by key0
    parts = [ops.tmlik_run(data, grid.part(reps=ab), wins, N_IT, s, seed) for ab in ((0, 2), (2, 5))]
    assert bits([torch.cat([p[0] for p in parts], dim=2), torch.cat([p[1] for p in parts], dim=1)]) == bits([rows, state])
    # models: 5 in one call against 2 + 3 (column 11 of a row and slot 15 of the state hold the model's index IN ITS CALL)
    parts = [ops.tmlik_run(data, grid.part(models=ab), wins[ab[0]:ab[1]].contiguous(), N_IT, s, seed) for ab in ((0, 2), (2, 5))]
    got_rows, got_state = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    assert bits([got_rows[..., :ref.R_MODEL], got_state[..., :ref.S_MODEL]]) == bits([rows[..., :ref.R_MODEL], state[..., :ref.S_MODEL]])
    assert got_rows[2:, ..., ref.R_MODEL].unique().tolist() == [0.0, 1.0, 2.0]
    none = ops.tmlik_steps(data, grid, wins, st, N_IT, 0, s, seed)
    assert none.shape[1] == 0


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins,shape,M", [(1, (2, 1), 1), (64, (3, 3), 3), (512, (5, 3), 2)])
def test_4_the_buffer_contract_on_exact_size_guarded_buffers(n_bins, shape, M):
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    T, R = shape
    P = synthetic(n_bins, 2, 5)
    data = dev_data(P)
    betas, scales = ladder(T)
    grid = ops.TmlikGrid([m % 2 for m in range(M)], [m % 3 for m in range(M)], [m * R for m in range(M)], betas, scales, R)
    wins = torch.as_tensor(win_table(M, T), device="cuda")

    def whole():
        state = ops.tmlik_init(data, grid, wins, 9)
        first = ops.tmlik_steps(data, grid, wins, state, 0, 25, 3, 9)               # rows_cap exactly the 9 rows written
        rows = ops.alloc_output((M, 13, R, T, ref.ROW_W), torch.float64, "cuda")
        ops.tmlik_steps(data, grid, wins, state, 25, 15, 3, 9, rows=rows)           # iterations 27 .. 39: slots 0 .. 4
        ops.tmlik_steps(data, grid, wins, state, 40, 24, 3, 9, rows=rows, slot0=5)  # 42 .. 63: slots 5 .. 12, exactly to the end
        est = ops.mlik_estimate(rows[M - 1], betas, row0=2)
        return (first, rows, state) + tuple(est)

    out = contract(ops, torch, whole, label="tmlik bins %d" % n_bins)
    assert out[0].shape[1] == 9 and out[1][0, 0, 0, 0, 0] == 27 and out[1][M - 1, -1, 0, 0, 0] == 63 and out[1][0, 5, 0, 0, 0] == 42
    # slot0 > 0 leaves the slots before it, and those behind the launch's rows, as they were
    state = ops.tmlik_init(data, grid, wins, 9)
    rows = torch.full((M, 12, R, T, ref.ROW_W), 7.0, dtype=torch.float64, device="cuda")
    ops.tmlik_steps(data, grid, wins, state, 0, 12, 3, 9, rows=rows, slot0=4)       # iterations 0, 3, 6, 9: slots 4 .. 7
    assert bool((rows[:, :4] == 7.0).all()) and bool((rows[:, 8:] == 7.0).all())
    assert rows[:, 4:8, ..., 0].unique().tolist() == [0.0, 3.0, 6.0, 9.0] and not bool((rows[:, 4:8] == 7.0).any())


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def test_5_argument_errors_in_the_headers_order_leave_the_buffers_untouched():
    import torch
    from helpers.abi_cases import refuses
    from literate_amd import _hip, ops
    lib = _hip.load()
    P = synthetic(8, 2, 5)
    data, big = dev_data(P), dev_data(synthetic(513, 2, 5))
    betas, scales = ladder(3)
    bad0, desc, one = np.array([0.1, 0.5, 1.0]), np.array([0.0, 0.7, 0.6, 1.0]), np.array([1.0])
    inf_s, neg_s = np.array([1.0, np.inf, 1.0]), np.array([1.0, 0.0, 1.0])
    G = lambda col=(0, 1), flags=(0, 1), key0=(0, 2), b=betas, s=scales, R=2: ops.TmlikGrid(col, flags, key0, b, s, R)
    far = (2 ** 31 - 1) // 3 - 1                                     # (far + 2) * 3 = 2^31 - 1 + 2
    for what, call, code in (
            ("513 bins", lambda: ops.tmlik_init(big, G(), 0.001, 1), "LR_ERR_SIZE"),
            ("513 bins before the betas", lambda: ops.tmlik_init(big, G(b=bad0), 0.001, 1), "LR_ERR_SIZE"),
            ("T = 1", lambda: ops.tmlik_init(data, G(b=one, s=one), 0.001, 1), "LR_ERR_SIZE"),
            ("T = 1 before the model", lambda: ops.tmlik_init(data, G(col=(0, 2), b=one, s=one), 0.001, 1), "LR_ERR_SIZE"),
            ("65 models", lambda: ops.tmlik_init(data, G(col=[0] * 65, flags=[0] * 65, key0=[0] * 65), 0.001, 1), "LR_ERR_SIZE"),
            ("a column out of range", lambda: ops.tmlik_init(data, G(col=(0, 2)), 0.001, 1), "LR_ERR_MODEL"),
            ("a column < 0", lambda: ops.tmlik_init(data, G(col=(-1, 1)), 0.001, 1), "LR_ERR_MODEL"),
            ("flags 4", lambda: ops.tmlik_init(data, G(flags=(0, 4)), 0.001, 1), "LR_ERR_MODEL"),
            ("key0 < 0", lambda: ops.tmlik_init(data, G(key0=(0, -1)), 0.001, 1), "LR_ERR_MODEL"),
            ("the key beyond 2^31 - 1", lambda: ops.tmlik_init(data, G(key0=(0, far)), 0.001, 1), "LR_ERR_MODEL"),
            ("key0 beyond int32", lambda: ops.tmlik_init(data, G(key0=(0, 2 ** 40)), 0.001, 1), "LR_ERR_MODEL"),
            ("betas[0] != 0", lambda: ops.tmlik_init(data, G(b=bad0), 0.001, 1), "LR_ERR_MODEL"),
            ("descending betas", lambda: ops.tmlik_init(data, G(b=desc, s=np.ones(4)), 0.001, 1), "LR_ERR_MODEL"),
            ("a scale not finite", lambda: ops.tmlik_init(data, G(s=inf_s), 0.001, 1), "LR_ERR_MODEL"),
            ("a scale of 0", lambda: ops.tmlik_init(data, G(s=neg_s), 0.001, 1), "LR_ERR_MODEL")):
        refuses(ops, torch, call, code, label=what, entry="lr_tmlik_init")
    assert (far - 1 + 2) * 3 <= 2 ** 31 - 1 < (far + 2) * 3
    ops.tmlik_init(data, G(key0=(0, far - 1)), 0.001, 1)             # the largest key is allowed
    grid = G()
    wins = torch.full((2, 3), 0.001, dtype=torch.float64, device="cuda")
    state = ops.tmlik_init(data, grid, wins, 1)
    for what, g, code in (("steps: descending betas", G(b=desc[:3]), "LR_ERR_MODEL"), ("steps: a scale not finite", G(s=inf_s), "LR_ERR_MODEL"),
                          ("steps: flags 4", G(flags=(4, 0)), "LR_ERR_MODEL")):
        before = state.clone()
        refuses(ops, torch, lambda: ops.tmlik_steps(data, g, wins, state, 0, 10, 1, 1), code, label=what, entry="lr_tmlik_steps")
        assert torch.equal(before, state)
    # the step arguments, and the order NULL < SIZE < MODEL < the step arguments: straight at the library, on buffers of a known fill
    rows = torch.full((2, 9, 2, 3, ref.ROW_W), 7.0, dtype=torch.float64, device="cuda")
    before = state.clone()

    def steps(d=data, g=grid, st=state, w=wins, cap=10, rows_=rows, it0=0, n_it=10, s=1, slot0=0, null=None):
        prob = ops.tmlik_problem(d, g, w, st, 1)
        if null:
            setattr(prob, null, None)
        return _hip.launch_problem(lib.lr_tmlik_steps, d.device, prob, it0, n_it, s, _hip.ptr(rows_), cap, slot0)

    assert steps(cap=9) == _hip.LR_ERR_SIZE and steps(cap=10, slot0=1) == _hip.LR_ERR_SIZE and steps(cap=-1) == _hip.LR_ERR_SIZE
    assert steps(g=G(b=bad0), cap=9) == _hip.LR_ERR_MODEL and steps(g=G(col=(0, 2)), cap=9) == _hip.LR_ERR_MODEL
    assert steps(g=G(R=0)) == steps(g=G(R=0, b=bad0)) == _hip.LR_ERR_SIZE          # no replicate (with a state that is not NULL)
    assert steps(s=0) == steps(it0=-1) == steps(n_it=-1) == steps(slot0=-1) == _hip.LR_ERR_SIZE and steps(g=G(b=bad0), s=0) == _hip.LR_ERR_MODEL
    # ... also without rows: NULL is the answer only where the step arguments are valid and a row is due
    assert steps(rows_=None, s=0) == steps(rows_=None, it0=-1) == steps(rows_=None, n_it=-1) == _hip.LR_ERR_SIZE
    for what, call in (("s_freq 0", lambda: ops.tmlik_steps(data, grid, wins, state, 0, 10, 0, 1)), ("it0 < 0", lambda: ops.tmlik_steps(data, grid, wins, state, -1, 10, 1, 1)),
                       ("n_iters < 0", lambda: ops.tmlik_steps(data, grid, wins, state, 0, -1, 1, 1))):
        with pytest.raises(ValueError, match="lr_tmlik_steps: LR_ERR_SIZE"):
            call()
    assert steps(d=big, g=G(b=bad0)) == _hip.LR_ERR_SIZE and steps(d=big, st=None) == _hip.LR_ERR_NULL and steps(rows_=None) == _hip.LR_ERR_NULL
    for field in ("n_spec", "n_exti", "DT", "trends", "wins", "state", "betas", "scales", "col", "flags", "key0"):
        assert steps(d=big, null=field) == _hip.LR_ERR_NULL, field
    assert lib.lr_tmlik_steps(None, 0, 10, 1, _hip.ptr(rows), 10, 0) == _hip.LR_ERR_NULL and lib.lr_tmlik_init(None) == _hip.LR_ERR_NULL
    torch.cuda.synchronize()
    assert torch.equal(before, state) and bool((rows == 7.0).all())
    # where no row is due rows may be NULL; n_iters = 0 launches nothing
    assert steps(rows_=None, it0=1, n_it=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, state)
    assert steps(rows_=None, it0=1, n_it=2, s=5) == 0 and steps(cap=9, n_it=9) == 0
    torch.cuda.synchronize()
    assert not torch.equal(before, state) and rows[:, :9, ..., 0].unique().tolist() == [float(i) for i in range(9)]


# ---- 6, 7 -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shared_run():
    from literate_amd import trend_mlik
    P = ref.shared_problem()
    return trend_mlik.run(P.n_spec, P.n_exti, P.DT, P.trends, ref.MODELS, ref.T, ref.R, ref.N_IT, ref.S_FREQ, ref.SEED, ref.BURN, ref.ALPHA,
                          ref.WIDEN)


def test_6_the_marginal_likelihoods_of_the_shared_problem_on_the_device(shared_run):
    truth, _ = ref.shared_truth(161)
    assert [(r.col, r.const_b, r.const_d) for r in shared_run.models] == ref.MODELS
    for r, want, sd in zip(shared_run.models, truth, ref.REF_SD):
        f = r.fit
        print("%s: log Z %.4f +- %.4f against %.4f (REF_SD / sqrt(R) %.4f), ti %.4f, smallest ESS %.0f"
              % (r.name, f["logZ_ss"], f["logZ_ss_se"], want, sd / math.sqrt(ref.R), f["logZ_ti"], f["min_lik_ess"]))
        assert abs(f["logZ_ss"] - want) <= 4 * sd / math.sqrt(ref.R) + 1e-3
        assert sd / math.sqrt(ref.R) / 2 <= f["logZ_ss_se"] <= 2 * sd / math.sqrt(ref.R)
        assert r.ss.shape == (ref.R,) and f["logZ_ss"] == r.pooled and f["min_lik_ess"] > 0
    null = shared_run.models[0]
    assert null.fit["two_ln_bf"] == 0.0 and null.fit["two_ln_bf_se"] == 0.0
    for r in shared_run.models[1:]:
        assert r.fit["two_ln_bf"] == 2.0 * (r.fit["logZ_ss"] - null.fit["logZ_ss"])
        assert r.fit["two_ln_bf_se"] == 2.0 * math.sqrt(r.fit["logZ_ss_se"] ** 2 + null.fit["logZ_ss_se"] ** 2)
    assert shared_run.settings["samples_kept"] == 1400


def test_7_the_tuned_windows_and_the_null_model(shared_run):
    """the null model is never tuned (it makes no counted additive proposal); the two others end in the open interval
    (0.001, 20), fall from the prior's end of the ladder to the posterior's, and hold the additive move's acceptance in
    [0.2, 0.5] at every temperature"""
    null, others = shared_run.models[0], shared_run.models[1:]
    assert np.all(null.wins == 0.001) and all(t[3] == 0.001 for t in null.temps)
    assert all(math.isnan(t[8]) for t in null.temps) and math.isnan(null.fit["accept_add_min"])
    for r in others:
        add = np.array([t[8] for t in r.temps])
        print(r.name, "windows", np.round(r.wins, 4), "additive acceptance", np.round(add, 3))
        assert np.all(r.wins > 0.001) and np.all(r.wins < 20.0)
        assert np.all(add >= 0.2) and np.all(add <= 0.5)
        assert r.fit["accept_add_min"] == add.min() and r.fit["accept_add_max"] == add.max()
        assert [t[3] for t in r.temps] == list(r.wins) and r.wins[-1] < r.wins[0]


def test_7_the_grouping_never_shows(shared_run):
    """one model per device call (a workspace of one model's rows) gives the same numbers"""
    from literate_amd import trend_mlik
    P = ref.shared_problem()
    n, burn = 300, 0.3
    a = trend_mlik.run(P.n_spec, P.n_exti, P.DT, P.trends, ref.MODELS, 4, 3, n * 10, 10, 5, burn, 0.3, 8.0)
    b = trend_mlik.run(P.n_spec, P.n_exti, P.DT, P.trends, ref.MODELS, 4, 3, n * 10, 10, 5, burn, 0.3, 8.0, workspace_bytes=n * 3 * 4 * 96)
    assert trend_mlik.group_size(n, 3, 4, n * 3 * 4 * 96) == 1
    for x, y in zip(a.models, b.models):
        assert np.array_equal(x.ss, y.ss) and np.array_equal(x.wins, y.wins) and x.temps[-1][:4] == y.temps[-1][:4]
        np.testing.assert_equal(x.fit, y.fit)


def test_7_a_run_whose_own_model_is_the_null():
    """-const_B -const_D: the selection is the null alone, no column is read, one model comes back"""
    from literate_amd import trend_mlik
    P = ref.shared_problem()
    res = trend_mlik.run(P.n_spec, P.n_exti, P.DT, np.ones((2, 5)), [(1, True, True)], 4, 3, 3000, 10, 5, 0.3, 0.3, 8.0)
    assert len(res.models) == 1 and res.models[0].name == "_CONB_COND" and res.models[0].fit["two_ln_bf"] == 0.0
    assert math.isfinite(res.models[0].fit["logZ_ss"]) and np.all(res.models[0].wins == 0.001)
    both = trend_mlik.run(P.n_spec, P.n_exti, P.DT, P.trends, ref.MODELS, 4, 3, 3000, 10, 5, 0.3, 0.3, 8.0)
    assert np.array_equal(both.models[0].ss, res.models[0].ss), "the null model's chains do not depend on what runs beside them"


# ---- 8 ----------------------------------------------------------------------------------------------------------------------
def test_8_the_estimator_reads_a_models_rows():
    import torch
    from literate_amd import ops
    P, grid_args, wins, want_rows, _, _ = reference(4)                               # 65 bins, three models, T = 3, R = 3
    grid = ops.TmlikGrid(*grid_args)
    rows, _ = ops.tmlik_run(dev_data(P), grid, torch.as_tensor(wins, device="cuda"), N_IT, 1, CASES[4][6])
    host = rows.cpu().numpy()
    assert not np.array_equal(host[0, ..., 2], host[1, ..., 2]) and not np.array_equal(host[1, ..., 2], host[2, ..., 2])
    est = ops.mlik_estimate(rows[1], grid.betas, row0=40)
    want = mlik_ref.estimate(host[1], grid.betas, 40)
    for k in ("stone", "ss", "lik_mean", "lik_var", "ti", "pooled"):
        got, w = getattr(est, k).cpu().numpy(), want[k]
        assert got.shape == w.shape and np.isfinite(w).all(), k
        np.testing.assert_allclose(got, w, rtol=1e-12, atol=0, err_msg=k)
    other = mlik_ref.estimate(host[0], grid.betas, 40)
    assert not np.allclose(other["ss"], want["ss"], rtol=1e-6)


# ---- 9 ----------------------------------------------------------------------------------------------------------------------
def test_9_the_stream_contract_on_a_busy_side_stream():
    """lr_tmlik_init and lr_tmlik_steps take the stream in their descriptor, so they are not among the functions
    helpers/stream_cases finds by their last parameter: the library handed to TorchRuntime here is a pair of adapters with the
    stream last, which put it into the descriptor and call the entry point.  8 bins, T = 3, R = 2, M = 2, 60 iterations in two
    launches; the statistics, the covariates and the windows are the inputs copied behind the delay."""
    import torch
    from helpers import stream_cases as S
    from literate_amd import _hip, ops
    lib = _hip.load()
    nb, T, R, M = 8, 3, 2, 2
    betas, scales = ladder(T)
    grid = ops.TmlikGrid([0, 1], [0, 2], [0, R], betas, scales, R)

    def init(prob, stream):
        prob.stream = stream
        return lib.lr_tmlik_init(C.byref(prob))

    def steps(prob, it0, n, s, rows, cap, slot0, stream):
        prob.stream = stream
        return lib.lr_tmlik_steps(C.byref(prob), it0, n, s, rows, cap, slot0)
    adapters = types.SimpleNamespace(lr_tmlik_init=init, lr_tmlik_steps=steps)
    rt = S.TorchRuntime(library=(adapters, ["lr_tmlik_init", "lr_tmlik_steps"]))

    def make(seed):
        P = synthetic(nb, 2, 40 + seed)
        return P.n_spec, P.n_exti, P.DT, P.trends, win_table(M, T) * (1.0 + seed)

    def call(n_spec, n_exti, DT, trends, wins):
        data = ops.TmlikData(n_spec, n_exti, DT, trends)
        assert data.trends.data_ptr() == trends.data_ptr() and data.DT.data_ptr() == DT.data_ptr()          # used as they are: no copy
        state = ops.alloc_output((M, R, T, ref.STATE_W), torch.float64, "cuda")
        rows = ops.alloc_output((M, 20, R, T, ref.ROW_W), torch.float64, "cuda")
        prob = ops.tmlik_problem(data, grid, wins, state, 9)
        here = rt.current_stream_arg
        assert adapters.lr_tmlik_init(prob, here()) == 0
        assert adapters.lr_tmlik_steps(prob, 0, 25, 3, _hip.ptr(rows), 20, 0, here()) == 0          # rows of iterations 0 .. 24: slots 0 .. 8
        assert adapters.lr_tmlik_steps(prob, 25, 35, 3, _hip.ptr(rows), 20, 9, here()) == 0         # 27 .. 57: slots 9 .. 19
        return dict(state=state, rows=rows)
    a, b = [S.dev(torch, x) for x in make(0)], [S.dev(torch, x) for x in make(1)]
    bufs = [torch.empty_like(x) for x in a]
    want, table = S.ordered(rt, lambda: call(*bufs), a, b, bufs, "tmlik")
    assert table["lr_tmlik_init"]["calls"] == 1 and table["lr_tmlik_steps"]["calls"] == 2
    rows = np.frombuffer(want["rows"]).reshape(M, 20, R, T, ref.ROW_W)
    assert rows[0, -1, 0, 0, 0] == 57.0 and rows[1, 9, 1, 2, 0] == 27.0


# ---- 10 ---------------------------------------------------------------------------------------------------------------------
def test_10_the_command_line_end_to_end(tmp_path):
    from helpers import waic_cases as W
    from literate_amd import mlik, trend_mlik
    from literate_amd.trendrate import model_suffix
    data = W._data(str(tmp_path))
    ts, te, origin, n_bins, DT = W._dd_setup(data)
    t = np.arange(n_bins + 1)
    cols = {"year": t.astype(float), "gdp": 3.0 + np.sin(t / 4.0) + t / 10.0, "sales": np.cos(t / 3.0) ** 2 + 0.01 * t}
    trend_file = os.path.join(str(tmp_path), "trend.tsv")
    with open(trend_file, "w") as f:
        f.write("\t".join(cols) + "\n")
        for i in t:
            f.write("\t".join(repr(float(cols[k][i])) for k in cols) + "\n")
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "trend_rate.py"), "-d", data, "-TBP", "-n", "3000", "-s", "10", "-p", "1000", "-seed", "31",
           "--chains", "2", "-trend_data", trend_file, "-trend_index", "1", "--mlik", "0.3", "--mlik_columns", "all", "--mlik_models", "all",
           "--mlik_temps", "5", "--mlik_reps", "3"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("MLIK:")]
    assert len(line) == 1 and "_MLIK.tsv" in line[0] and "10 models" in line[0]
    stem = os.path.join(str(tmp_path), "example_31" + model_suffix(False, False) + "_1")
    assert all(os.path.exists(stem + k) for k in ("_MLIK.tsv", "_MLIK_temps.tsv", "_MLIK.npz"))
    fit = trend_mlik.read_fit(stem)
    print(open(stem + "_MLIK.tsv").read())
    assert len(fit) == 10 and list(fit[0]) == trend_mlik.FIT_HEAD
    z = [r["logZ_ss"] for r in fit]
    assert z == sorted(z, reverse=True) and all(math.isfinite(v) for v in z) and all(r["logZ_ss_se"] > 0 for r in fit)
    assert sorted((r["model"], r["column"]) for r in fit) == sorted([("_CONB_COND", 0)] + [(m, c) for c in range(3) for m in ("_EXPB_EXPD", "_EXPB_COND", "_CONB_EXPD")])
    null = [r for r in fit if r["model"] == "_CONB_COND"]
    assert len(null) == 1 and null[0]["two_ln_bf"] == 0.0 and null[0]["two_ln_bf_se"] == 0.0 and null[0]["column_name"] == "-"
    assert {r["column_name"] for r in fit if r["column"] == 2} == {"sales"}
    for r in fit:
        assert r["two_ln_bf"] == 2.0 * (r["logZ_ss"] - null[0]["logZ_ss"])
    with open(stem + "_MLIK_temps.tsv") as f:
        temps = [l.rstrip("\n").split("\t") for l in f]
    assert temps[0] == trend_mlik.TEMPS_HEAD and len(temps) == 1 + 10 * 5 and [t[0] for t in temps[1::5]] == [r["model"] for r in fit]
    assert float(temps[1][3]) == 0.0 and float(temps[5][3]) == 1.0
    with np.load(stem + "_MLIK.npz") as f:
        assert f["ss"].shape == (10, 3) and f["names"].shape == (10,) and list(f["logZ_ss"]) == z and f["fingerprint"][0] == len(ts)
    # the same numbers from the module, on the statistics the run saw
    from literate_amd.literate_library import create_bins, parse_ts_te
    TS, TE, PRESENT, ORIGIN = parse_ts_te(data, True, -1, -1, .5)
    _, _, n_spec, n_exti, DT, _, _ = create_bins(ORIGIN, PRESENT, np.asarray(TS, float), np.asarray(TE, float), 0)
    trends, names = trend_mlik.read_trends(trend_file, 0)
    res = trend_mlik.run(n_spec, n_exti, DT, trends, trend_mlik.select_models("all", "all", 1, False, False, 3), 5, 3, 3000, 10, 31, 0.3, 0.3, 8.0)
    assert names == list(cols) and sorted(r.fit["logZ_ss"] for r in res.models) == sorted(z)
    # the compare tool: one row per model; a file of other data is refused
    npz = stem + "_MLIK.npz"
    out = subprocess.run([sys.executable, "-m", "literate_amd.mlik", npz], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    table = [l.split("\t") for l in out.stdout.strip().splitlines()]
    assert table[0] == mlik.COMPARE_HEAD and len(table) == 11 and float(table[1][4]) == 0.0 and float(table[1][2]) == z[0]
    other = os.path.join(str(tmp_path), "other_MLIK.npz")
    with np.load(npz) as f:
        np.savez(other, **dict({k: f[k] for k in f.files}, fingerprint=f["fingerprint"] + np.array([1., 0, 0, 0, 0, 0])))
    out = subprocess.run([sys.executable, "-m", "literate_amd.mlik", npz, other], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert out.returncode != 0 and "different data" in out.stderr
