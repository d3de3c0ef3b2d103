"""Trait-dependent rates on the GPU (include/literate_hip_trait.h, csrc/lr_trait.hip) against the numpy restatement
tests/helpers/trait_ref.py.

   1. lr_trait_weights against the per-lineage, per-bin loop: n in {1, 63, 64, 65, 4097, one tile +- 1}, n_bins in {1, 2, 64, 65,
      512}, C in {1, Cb - 1, Cb, Cb + 1}; sorted and shuffled, year-resolution and continuous times; lineages born and dead in
      one bin, born before t0, alive past the window, with ts or te on an edge; kappa (x - x0) = +-800, x0 at both range edges.
      Tolerance on W_b, derived: (lineages overlapping bin b) 2^-(F + 1) for the one rounding of every term to 2^-F, plus 1e-12
      relative for the device exponential (the project's rtol for br_length in tests/test_hip_parity.py).  Slog: rtol 1e-12,
      atol 1e-9, as lr_bd_loglik_batch's tests.
   2. at kappa = 0 on year-resolution input 2 W is lr_bin_unit_events' br_length bit for bit.
   3. the same bits per state whatever the other states of the call (chains reversed).
   4. exact-size dirty guarded buffers; the error codes in the header's order with the outputs untouched.
   5. the sampler's baseline half against lr_rjbin_steps (model 3 on sp, ex, WL, WM): bit for bit.  The row's likelihood, prior
      and posterior hold Slog and the kappas' prior: they are compared after subtracting those, to 4 ulp of the larger operand.
   6. one trait move of 256 chains against the restatement fed with the device's own W' and Slog'.
   7. a run cut into calls; 8. a busy side stream; 9. end to end against the restatement's sampler; 10. the command line.
"""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import trait_ref as tr           # noqa: E402
from oracle import mcmc_oracle as mo          # noqa: E402
from oracle import philox                     # noqa: E402

pytestmark = pytest.mark.gpu

KMAX, HEAD = 32, 13
TW = HEAD + 2 * (2 * KMAX - 1)
RW = TW + 8
T0 = 5.0
TILE = 2048


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def make_lineages(n, n_bins, seed, year, shuffled):
    """n lineages around the window [T0, T0 + n_bins]; from 12 lineages on, the first ones are the special cases"""
    rng = np.random.default_rng(seed)
    lo, hi = T0 - 3.0, T0 + n_bins + 3.0
    ts = rng.uniform(lo, hi - 1.0, n)
    te = np.minimum(ts + rng.exponential(max(n_bins / 3.0, 1.5), n), hi + 2.0)
    if year:
        ts, te = np.floor(ts), np.floor(te) + rng.integers(0, 2, n)
    special = [(T0 + 0.25, T0 + 0.75), (T0 + n_bins - 0.5, T0 + n_bins - 0.125),      # born and dead in one bin
               (T0 - 2.5, T0 + 0.5), (T0 - 2.0, T0 + n_bins + 2.0),                   # born before t0 (the second spans the window)
               (T0 + 0.5, T0 + n_bins + 1.5),                                         # alive past the window
               (T0, T0 + 1.0), (T0 + n_bins - 1.0, T0 + n_bins),                      # ts and te exactly on edges
               (T0 + n_bins, T0 + n_bins + 1.0), (T0 - 2.0, T0),                      # just outside, touching the edges
               (T0 + 0.5, T0 + 0.5), (T0 + 1.0, T0 - 1.0),                            # no lineage-time
               (T0 - 3.0, T0 - 1.0)]                                                  # wholly before
    if year:
        special = [(math.floor(a), math.floor(b) + (1.0 if b > a and math.floor(b) == math.floor(a) else 0.0)) for a, b in special]
    if n >= len(special):
        for i, (a, b) in enumerate(special):
            ts[i], te[i] = a, b
    x = rng.normal(size=n)
    if n >= 2:
        x[-1], x[-2] = 2.5, -2.5
    order = np.argsort(ts, kind="stable")
    if shuffled:
        order = rng.permutation(n)
    return ts[order], te[order], x[order]


def make_params(Cn, x, seed, k):
    """Cn states: rotating through the edge cases, then random ones"""
    rng = np.random.default_rng(seed)
    xmax = float(np.max(np.abs(x))) or 1.0
    edge = [(float(x.min()), 1.3), (float(x.max()), -0.7), (0.0, 800.0 / xmax), (0.0, -800.0 / xmax), (0.3, 0.0)]
    P = [edge[(k + i) % len(edge)] for i in range(min(Cn, len(edge)))]
    P += [(rng.uniform(-2, 2), rng.normal() * 2.0) for _ in range(Cn - len(P))]
    return np.array(P, dtype=float).reshape(Cn, 2)


def plan_tiles(n):
    """the header's tiling, a function of n alone: at most 1024 tiles of at least TILE lineages, a multiple of 256 each"""
    t = max(1, min(1024, -(-n // TILE)))
    chunk = -(-(-(-n // t)) // 256) * 256
    return -(-n // chunk)


def check_weights(ops, ts, te, x, n_bins, P, label):
    W, sb, sd = [t.cpu().numpy() for t in ops.trait_weights(ts, te, x, T0, n_bins, P)]
    rW, rsb, rsd, cnt = tr.weights(ts, te, x, T0, n_bins, P)
    bound = cnt[None, :] * 2.0 ** -(tr.F + 1) + 1e-12 * np.abs(rW)
    err = np.abs(W - rW)
    print("%s: max |W - ref| / bound = %.3g" % (label, float(np.max(err / np.maximum(bound, 1e-300))) if err.any() else 0.0))
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(sb)) and np.all(np.isfinite(sd)), label
    assert np.all(err <= bound), (label, float(err.max()))
    np.testing.assert_allclose(sb, rsb, rtol=1e-12, atol=1e-9, err_msg=label)
    np.testing.assert_allclose(sd, rsd, rtol=1e-12, atol=1e-9, err_msg=label)
    return W, sb, sd


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 2, 64, 65, 512])
def test_1_weights_against_the_loop(n_bins):
    from literate_amd import _hip, ops
    cb = ops.trait_weights_plan(100, n_bins, 1)["cb"]
    assert cb == _hip.LR_TRAIT_CB
    for k, n in enumerate([1, 63, 64, 65, 4097, TILE - 1, TILE, TILE + 1]):
        Cn = [1, cb - 1, cb, cb + 1][(k + n_bins) % 4]
        year, shuffled = bool(k & 1), bool((k >> 1) & 1) ^ bool(n_bins & 1)
        ts, te, x = make_lineages(n, n_bins, 100 * n_bins + k, year, shuffled)
        plan = ops.trait_weights_plan(n, n_bins, Cn)
        assert plan["passes"] == -(-Cn // cb) and plan["tiles"] == plan_tiles(n)
        check_weights(ops, ts, te, x, n_bins, make_params(Cn, x, k, k), "n %d bins %d C %d year %d shuffled %d" % (n, n_bins, Cn, year, shuffled))


def test_1_the_loop_and_its_vectorised_form_agree_on_the_device_too():
    from literate_amd import ops
    ts, te, x = make_lineages(65, 7, 3, False, True)
    P = make_params(9, x, 1, 0)
    W, sb, sd = check_weights(ops, ts, te, x, 7, P, "loop")
    for c in range(9):
        lW, lsb, lsd, cnt = tr.weights_loop(ts, te, x, T0, 7, P[c, 0], P[c, 1])
        assert np.all(np.abs(W[c] - lW) <= cnt * 2.0 ** -(tr.F + 1) + 1e-12 * np.abs(lW))
        np.testing.assert_allclose([sb[c], sd[c]], [lsb, lsd], rtol=1e-12, atol=1e-9)


def test_1_more_state_groups_than_a_grids_second_dimension_holds():
    """C up to 2^20 is 2^17 groups of 8: past 65 535"""
    from literate_amd import ops
    ts, te, x = make_lineages(13, 2, 9, False, False)
    Cn = (1 << 19) + 9
    rng = np.random.default_rng(3)
    P = np.column_stack([rng.uniform(-2, 2, Cn), rng.normal(size=Cn) * 2.0])
    assert ops.trait_weights_plan(13, 2, Cn)["passes"] == (1 << 16) + 2
    check_weights(ops, ts, te, x, 2, P, "C 2^19 + 9")


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_bins", [(65, 1), (4097, 64), (TILE + 1, 65), (4097, 512)])
def test_2_at_kappa_0_twice_W_is_br_length_bit_for_bit(n, n_bins):
    import torch
    from literate_amd import ops
    ts, te, x = make_lineages(n, n_bins, 7 + n_bins, True, n_bins == 65)
    sp, ex, br = ops.bin_unit_events(ts, te, T0, n_bins)
    W, sb, sd = ops.trait_weights(ts, te, x, T0, n_bins, [[0.4, 0.0], [-7.0, 0.0]])
    assert torch.equal(2.0 * W[0], br) and torch.equal(W[1], W[0])
    # Slog at s = 1/2: log(1/2) per counted event
    np.testing.assert_allclose(sb.cpu().numpy(), float(sp.sum()) * math.log(0.5), rtol=1e-12)
    np.testing.assert_allclose(sd.cpu().numpy(), float(ex.sum()) * math.log(0.5), rtol=1e-12)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
def test_3_a_states_bits_do_not_depend_on_the_other_states():
    import torch
    from literate_amd import ops
    ts, te, x = make_lineages(4097, 65, 11, False, True)
    P = make_params(9, x, 5, 0)
    a = ops.trait_weights(ts, te, x, T0, 65, P)
    b = ops.trait_weights(ts, te, x, T0, 65, P)
    r = ops.trait_weights(ts, te, x, T0, 65, P[::-1].copy())
    one = ops.trait_weights(ts, te, x, T0, 65, P[3:4])
    for u, v, w in zip(a, b, r):
        assert torch.equal(u, v) and torch.equal(u, torch.flip(w, dims=[0]))
    assert all(torch.equal(u[3:4], v) for u, v in zip(a, one))


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_bins,Cn", [(65, 2, 1), (4097, 65, 9), (TILE, 512, 8)])
def test_4_the_buffer_contract_on_exact_size_guarded_buffers(n, n_bins, Cn):
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    ts, te, x = make_lineages(n, n_bins, 13, False, False)
    P = make_params(Cn, x, 2, 1)
    dev = [torch.as_tensor(v, device="cuda") for v in (ts, te, x, P)]
    contract(ops, torch, lambda: ops.trait_weights(dev[0], dev[1], dev[2], T0, n_bins, dev[3]), label="trait_weights bins %d" % n_bins)


def test_4_sampler_buffer_contract():
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    ts, te, x = make_lineages(300, 65, 17, False, False)
    st = ops.TraitSettings(trait_every=4, x0_lo=-3.0, x0_hi=3.0)

    def whole():
        data = ops.TraitData(ts, te, x, T0, 65)
        state = ops.trait_init(data, 5, 9, st)
        first = ops.trait_steps(data, state, 0, 25, 3, 9, st)                           # exactly the 9 rows written
        rows = ops.alloc_output((13, 5, RW), torch.float64, "cuda")
        ops.trait_steps(data, state, 25, 15, 3, 9, st, rows=rows)                       # 27 .. 39: slots 0 .. 4
        ops.trait_steps(data, state, 40, 24, 3, 9, st, rows=rows, slot0=5)              # 42 .. 63: slots 5 .. 12
        return first, rows, state
    out = contract(ops, torch, whole, label="trait sampler")
    assert out[0].shape[0] == 9 and out[1][0, 0, 0] == 27 and out[1][-1, 4, 0] == 63 and out[1][5, 0, 0] == 42


def test_4_argument_errors_in_the_headers_order_leave_the_buffers_untouched():
    import torch
    from literate_amd import _hip, ops
    lib = _hip.load()
    E = _hip
    ts, te, x = [torch.as_tensor(v, device="cuda") for v in make_lineages(65, 8, 1, False, False)]
    P = torch.zeros(3, 2, dtype=torch.float64, device="cuda")
    W = torch.full((3, 8), 7.0, dtype=torch.float64, device="cuda")
    sb, sd = torch.full((3,), 7.0, dtype=torch.float64, device="cuda"), torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    need = lib.lr_trait_weights_workspace_bytes(65, 8, 3)
    assert need > 0
    ws = torch.full((need,), 7, dtype=torch.uint8, device="cuda")

    def call(null=None, **kw):
        prob = _hip.TraitWeightsProblem(_hip.ptr(ts), _hip.ptr(te), _hip.ptr(x), _hip.ptr(P), _hip.ptr(W), _hip.ptr(sb), _hip.ptr(sd),
                                        _hip.ptr(ws), need, 65, T0, 8, 3, None)
        if null:
            setattr(prob, null, None)
        for k, v in kw.items():
            setattr(prob, k, v)
        return _hip.launch_problem(lib.lr_trait_weights, ts.device, prob)
    assert lib.lr_trait_weights(None) == E.LR_ERR_NULL
    bad = dict(n=0, t0=0.5, workspace_bytes=need - 1)              # wrong in every later way
    for field in ("ts", "te", "x", "params", "W", "Slog_birth", "Slog_death", "workspace"):
        assert call(null=field, **bad) == E.LR_ERR_NULL, field
    assert call(**bad) == E.LR_ERR_SIZE
    for kw in (dict(n=0), dict(n=E.LR_TRAIT_MAX_N + 1), dict(n_bins=0), dict(n_bins=E.LR_RJBIN_MAX_BINS + 1), dict(C=0), dict(C=(1 << 20) + 1)):
        assert call(t0=0.5, workspace_bytes=0, **kw) == E.LR_ERR_SIZE, kw
    assert call(t0=0.5, workspace_bytes=need - 1) == call(t0=2e9, workspace_bytes=0) == call(t0=float("nan")) == E.LR_ERR_T0
    assert call(workspace_bytes=need - 1) == call(workspace_bytes=0) == E.LR_ERR_WORKSPACE
    assert lib.lr_trait_weights_workspace_bytes(E.LR_TRAIT_MAX_N + 1, 8, 3) == E.LR_ERR_SIZE
    assert lib.lr_trait_weights_workspace_bytes(65, 513, 3) == lib.lr_trait_workspace_bytes(65, 8, 0) == E.LR_ERR_SIZE
    out4 = (C.c_int32 * 4)()
    assert lib.lr_trait_weights_plan(65, 8, 3, None) == E.LR_ERR_NULL and lib.lr_trait_weights_plan(0, 8, 3, out4) == E.LR_ERR_SIZE
    torch.cuda.synchronize()
    assert bool((W == 7.0).all()) and bool((sb == 7.0).all()) and bool((sd == 7.0).all()) and bool((ws == 7).all())
    assert call() == 0
    # the sampler: NULL < SIZE < T0 < MODEL < WORKSPACE < the step arguments
    data = ops.TraitData(ts, te, x, T0, 8)
    state = ops.trait_init(data, 4, 1)
    before = state.clone()
    rows = torch.full((10, 4, RW), 7.0, dtype=torch.float64, device="cuda")
    wneed = lib.lr_trait_workspace_bytes(65, 8, 4)
    sws = torch.full((wneed,), 7, dtype=torch.uint8, device="cuda")
    S = ops.TraitSettings

    def steps(s=S(), cap=10, rows_=rows, it0=0, n_it=10, sf=1, slot0=0, null=None, **kw):
        prob = ops.trait_problem(data, state, sws, 4, 1, s)
        if null:
            setattr(prob, null, None)
        for k, v in kw.items():
            setattr(prob, k, v)
        return _hip.launch_problem(lib.lr_trait_steps, data.device, prob, it0, n_it, sf, _hip.ptr(rows_), cap, slot0)
    assert lib.lr_trait_steps(None, 0, 10, 1, _hip.ptr(rows), 10, 0) == lib.lr_trait_init(None, None) == E.LR_ERR_NULL
    for field in ("ts", "te", "x", "sp", "ex", "state", "warn", "workspace"):
        assert steps(null=field, n=0, t0=0.5, s=S(update_fraction=2.0), workspace_bytes=0, sf=0) == E.LR_ERR_NULL, field
    assert steps(rows_=None) == E.LR_ERR_NULL and steps(rows_=None, sf=0) == steps(rows_=None, n_it=-1) == E.LR_ERR_SIZE
    for kw in (dict(n=0), dict(n_bins=513), dict(C=0), dict(trait_every=-1)):
        assert steps(t0=0.5, s=S(update_fraction=2.0), workspace_bytes=0, **kw) == E.LR_ERR_SIZE, kw
    assert steps(t0=0.5, s=S(update_fraction=2.0), workspace_bytes=0) == E.LR_ERR_T0
    for s in (S(update_fraction=2.0), S(poisson_HP=-1.0), S(win_x0=(-1.0, 0.5)), S(win_kappa=(0.1, float("nan"))), S(x0_lo=1.0, x0_hi=0.0)):
        assert steps(s=s, workspace_bytes=0, sf=0) == E.LR_ERR_MODEL, s
    assert steps(start_time=9.0, end_time=9.0, workspace_bytes=0) == E.LR_ERR_MODEL
    assert steps(workspace_bytes=wneed - 1, sf=0) == E.LR_ERR_WORKSPACE
    assert steps(sf=0) == steps(it0=-1) == steps(n_it=-1) == steps(slot0=-1) == steps(cap=9) == steps(slot0=1) == E.LR_ERR_SIZE
    torch.cuda.synchronize()
    assert torch.equal(before, state) and bool((rows == 7.0).all()) and bool((sws == 7).all()) and data.warnings() == 0
    assert steps(rows_=None, it0=1, n_it=0) == 0 and steps(rows_=None, it0=1, n_it=2, sf=5) == 0 and steps(cap=9, it0=3, n_it=9) == 0
    torch.cuda.synchronize()
    assert rows[:9, :, 0].unique().tolist() == [float(i) for i in range(3, 12)] and bool((rows[9] == 7.0).all())


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def near(a, b, scale):
    return np.all(np.abs(a - b) <= 4 * np.finfo(float).eps * scale)


@pytest.mark.parametrize("n_bins,Cn", [(1, 1), (64, 5), (65, 5), (65, 1)])
def test_5_the_baseline_half_is_lr_rjbin_steps_bit_for_bit(n_bins, Cn):
    import torch
    from literate_amd import _hip, ops
    ts, te, x = make_lineages(300, n_bins, 21 + n_bins, False, False)
    rng = np.random.default_rng(n_bins)
    p0 = np.column_stack([rng.uniform(-1, 1, Cn), rng.normal(size=Cn), rng.uniform(-1, 1, Cn), rng.normal(size=Cn)])
    st = ops.TraitSettings(trait_every=0)
    data = ops.TraitData(ts, te, x, T0, n_bins)
    state = ops.trait_init(data, Cn, 31, st, chain0=3, params0=p0)
    state0 = state.clone()
    rows = ops.trait_steps(data, state, 0, 300, 1, 31, st, chain0=3)
    WL, sL, _ = ops.trait_weights(ts, te, x, T0, n_bins, p0[:, 0:2])
    WM, _, sM = ops.trait_weights(ts, te, x, T0, n_bins, p0[:, 2:4])
    sc = state[:, _hip.LR_TRAIT_ROW_SCALARS:_hip.LR_TRAIT_ROW_SCALARS + 10].cpu().numpy()
    assert np.array_equal(sc[:, :4], p0) and np.array_equal(sc[:, 4], sL.cpu().numpy()) and np.array_equal(sc[:, 5], sM.cpu().numpy())
    assert not sc[:, 6:].any()
    assert torch.equal(state[:, _hip.LR_TRAIT_ROW_WL:_hip.LR_TRAIT_ROW_WL + n_bins], WL)
    assert torch.equal(state[:, _hip.LR_TRAIT_ROW_WM:_hip.LR_TRAIT_ROW_WM + n_bins], WM)
    assert not state[:, _hip.LR_TRAIT_ROW_WL + n_bins:_hip.LR_TRAIT_ROW_WM].any() and not state[:, _hip.LR_TRAIT_ROW_WM + n_bins:].any()
    tile = lambda v: v.reshape(1, -1).repeat(Cn, 1).contiguous()
    rj = ops.RjbinData(tile(data.sp), tile(data.ex), WL, [data.start_time] * Cn, [data.end_time] * Cn, 1, ex_dead=tile(data.ex), br_dead=WM)
    rst = ops.RjbinSettings(model=3)
    rstate = ops.rjbin_init(rj, 31, rst, chain0=3)
    assert torch.equal(rstate, state0[:, :_hip.LR_RJBIN_STATE_W])
    rrows = ops.rjbin_steps(rj, rstate, 0, 300, 1, 31, rst, chain0=3)
    assert torch.equal(rstate, state[:, :_hip.LR_RJBIN_STATE_W])
    a, b = rows.cpu().numpy(), rrows.cpu().numpy()
    keep = [c for c in range(TW) if c not in (1, 2, 3)]
    assert np.array_equal(a[:, :, keep], b[:, :, keep], equal_nan=True)
    slog = (sL + sM).cpu().numpy()[None, :]
    tp = np.array([tr.trait_prior(p[1], p[3]) for p in p0])[None, :]
    assert near(a[:, :, 2] - slog, b[:, :, 2], np.abs(a[:, :, 2]) + np.abs(slog))
    assert near(a[:, :, 3] - tp, b[:, :, 3], np.abs(a[:, :, 3]) + np.abs(tp))
    assert near(a[:, :, 1] - slog - tp, b[:, :, 1], np.abs(a[:, :, 1]) + np.abs(slog) + np.abs(tp) + np.abs(a[:, :, 2]) + np.abs(a[:, :, 3]))
    tail = a[:, :, TW:]
    assert np.array_equal(tail[:, :, :4], np.broadcast_to(p0, tail[:, :, :4].shape)) and not tail[:, :, 6:].any()
    assert data.warnings() == rj.warnings()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
MOVE = dict(n=400, n_bins=30, C=256, seed=4, chain0=2, it=9, win_x0=(0.5, 0.8), win_kappa=(0.3, 0.2), x0_range=(-1.0, 1.0))


def move_case():
    """the given state of test 6: the initial state at per-chain parameters, a third of them within a window of a range edge"""
    m = MOVE
    ts, te, x = make_lineages(m["n"], m["n_bins"], 33, False, False)
    rng = np.random.default_rng(6)
    p0 = np.column_stack([rng.uniform(-1, 1, m["C"]), rng.normal(size=m["C"]), rng.uniform(-1, 1, m["C"]), rng.normal(size=m["C"])])
    p0[::3, 0], p0[1::3, 2] = 0.95, -0.95
    return ts, te, x, p0


def move_restatement(ts, te, x, p0, W0=None, S0=None, LM=None, likA=None, prop_stats=None):
    """every chain's move of iteration MOVE['it'] from the initial state; the device's values where given, numpy's otherwise"""
    m = MOVE
    nb = m["n_bins"]
    e = tr.overlaps(ts, te, T0, nb)
    sp = np.array([np.count_nonzero((ts >= T0 + b) & (ts < T0 + b + 1)) for b in range(nb)], dtype=float)
    ex = np.array([np.count_nonzero((te > T0 + b) & (te <= T0 + b + 1)) for b in range(nb)], dtype=float)
    if W0 is None:
        wl, sl, _, _ = tr.weights(ts, te, x, T0, nb, p0[:, 0:2], e)
        wm, _, sm, _ = tr.weights(ts, te, x, T0, nb, p0[:, 2:4], e)
        W0, S0 = np.stack([wl, wm], 1), np.stack([sl, sm], 1)
    out = []
    for c in range(m["C"]):
        stream = philox.Stream(m["seed"], m["chain0"] + c)
        if LM is None:
            l0, m0 = mo.PhiloxDraws(m["seed"], m["chain0"] + c).init_rates()
            L, M = float(np.ravel(l0)[0]), float(np.ravel(m0)[0])
        else:
            L, M = LM[c]
        lam, mu = np.full(nb, L), np.full(nb, M)
        lik0 = tr.baseline_lik(lam, mu, sp, ex, W0[c, 0], W0[c, 1]) if likA is None else likA[c]
        side, x0p, kp = tr.propose(stream, m["it"], [p0[c, 0], p0[c, 2]], [p0[c, 1], p0[c, 3]], m["win_x0"], m["win_kappa"])
        if prop_stats is None:
            wp, sb, sd, _ = tr.weights(ts, te, x, T0, nb, [[x0p, kp]], e)
            Wp, sp_ = wp[0], (sb[0] if side == 0 else sd[0])
        else:
            Wp, sp_ = prop_stats[0][c], prop_stats[1][c, side]
        ok, delta, log_u, lik = tr.settle(stream, m["it"], lam, mu, sp, ex, W0[c], S0[c], [p0[c, 1], p0[c, 3]], lik0, side, x0p, kp, Wp, sp_,
                                          m["x0_range"])
        out.append(dict(side=side, x0p=x0p, kp=kp, ok=ok, delta=delta, log_u=log_u, lik=lik, Wp=Wp, slog_p=sp_,
                        in_range=m["x0_range"][0] <= x0p <= m["x0_range"][1]))
    return out


def test_6_one_trait_move_of_256_chains():
    import torch
    from literate_amd import _hip, ops
    m = MOVE
    ts, te, x, p0 = move_case()
    Cn, nb = m["C"], m["n_bins"]
    st = ops.TraitSettings(trait_every=10, win_x0=m["win_x0"], win_kappa=m["win_kappa"], x0_lo=m["x0_range"][0], x0_hi=m["x0_range"][1])
    data = ops.TraitData(ts, te, x, T0, nb)
    state = ops.trait_init(data, Cn, m["seed"], st, chain0=m["chain0"], params0=p0)
    s0 = state.cpu().numpy()
    rows = ops.trait_steps(data, state, m["it"], 1, 1, m["seed"], st, chain0=m["chain0"]).cpu().numpy()
    s1 = state.cpu().numpy()
    SC, WLo, WMo = _hip.LR_TRAIT_ROW_SCALARS, _hip.LR_TRAIT_ROW_WL, _hip.LR_TRAIT_ROW_WM
    W0 = np.stack([s0[:, WLo:WLo + nb], s0[:, WMo:WMo + nb]], 1)
    S0 = s0[:, SC + 4:SC + 6]
    LM = s0[:, [0, 64]]                                   # K = 1: lane 0 of the two rate rows
    assert np.all(s0[:, 6 * 64 + 6:6 * 64 + 8] == 1.0)
    likA = s0[:, 6 * 64]
    # the restatement on numpy alone keeps every chain clear of a tie (what the seed was chosen for) ...
    host = move_restatement(ts, te, x, p0)
    margin = min(abs(h["delta"] - h["log_u"]) for h in host if h["in_range"])
    print("least |delta - log u| on the host: %.3g" % margin)
    assert margin > 1e-6
    # ... and, fed with the device's own W', Slog', state, leaves out none
    props = np.array([[h["x0p"], h["kp"]] for h in host])
    Wp, sb, sd = [t.cpu().numpy() for t in ops.trait_weights(ts, te, x, T0, nb, props)]
    ref = move_restatement(ts, te, x, p0, W0, S0, LM, likA, (Wp, np.stack([sb, sd], 1)))
    left_out = [c for c, r in enumerate(ref) if r["in_range"] and abs(r["delta"] - r["log_u"]) < 1e-9]
    assert len(left_out) == 0
    n_out = n_ok = 0
    for c, r in enumerate(ref):
        side = r["side"]
        sc0, sc1 = s0[c, SC:SC + 10], s1[c, SC:SC + 10]
        assert sc1[6 + 2 * side] == sc0[6 + 2 * side] + 1 and sc1[6 + 2 * (1 - side)] == 0, c          # the same side
        same = np.delete(np.arange(_hip.LR_TRAIT_STATE_W), SC + 6 + 2 * side)
        if not r["in_range"]:
            n_out += 1
        if r["ok"]:
            n_ok += 1
            assert np.array_equal(sc1[[2 * side, 2 * side + 1]], [r["x0p"], r["kp"]])          # product and sum rounded apart, as numpy
            assert sc1[4 + side] == r["slog_p"] and sc1[7 + 2 * side] == 1.0
            off = WLo if side == 0 else WMo
            assert np.array_equal(s1[c, off:off + nb], r["Wp"])
            np.testing.assert_allclose(s1[c, 6 * 64], r["lik"], rtol=1e-12)
            other = WMo if side == 0 else WLo
            assert np.array_equal(s1[c, other:other + 512], s0[c, other:other + 512])
            assert np.array_equal(sc1[[2 - 2 * side, 3 - 2 * side, 5 - side]], sc0[[2 - 2 * side, 3 - 2 * side, 5 - side]])
            keep = [j for j in range(_hip.LR_RJBIN_STATE_W) if j != 6 * 64]
            assert np.array_equal(s1[c, keep], s0[c, keep])
        else:
            assert np.array_equal(s1[c, same], s0[c, same]), c                                          # untouched
        row = rows[0, c]
        assert row[0] == m["it"] and np.array_equal(row[TW:TW + 6], s1[c, SC:SC + 6]) and np.array_equal(row[TW + 6:], sc1[[7, 9]])
        np.testing.assert_allclose(row[2], s1[c, 6 * 64] + sc1[4] + sc1[5], rtol=1e-14)
    print("accepted %d of %d, %d proposed outside the range" % (n_ok, Cn, n_out))
    assert n_out >= 10 and 10 <= n_ok <= Cn - 10


# ---- 7 ----------------------------------------------------------------------------------------------------------------------
def test_7_a_run_cut_into_calls_is_the_same_run():
    import torch
    from literate_amd import ops
    ts, te, x = make_lineages(300, 65, 41, False, True)
    st = ops.TraitSettings(trait_every=10, win_kappa=(0.5, 0.5), x0_lo=-3.0, x0_hi=3.0)
    data = ops.TraitData(ts, te, x, T0, 65)
    a = ops.trait_init(data, 5, 7, st)
    b = a.clone()
    rows_a = ops.trait_steps(data, a, 0, 45, 3, 7, st)
    assert rows_a.shape[0] == 15
    rows_b = torch.full((17, 5, RW), -7.0, dtype=torch.float64, device="cuda")
    slot = 1
    for it0, n in ((0, 7), (7, 13), (20, 25)):
        ops.trait_steps(data, b, it0, n, 3, 7, st, rows=rows_b, slot0=slot)
        slot += ops.rows_due(it0, n, 3)
    assert slot == 16 and torch.equal(a, b) and torch.equal(rows_a.view(torch.int64), rows_b[1:16].view(torch.int64))          # (bits: the rows pad with NaN)
    assert bool((rows_b[0] == -7.0).all()) and bool((rows_b[16] == -7.0).all())
    assert rows_a[:, 0, 0].tolist() == [float(i) for i in range(0, 45, 3)]
    prop = a[:, 448 + 6] + a[:, 448 + 8]
    assert prop.tolist() == [4.0] * 5                                                    # iterations 9, 19, 29, 39


# ---- 8 ----------------------------------------------------------------------------------------------------------------------
def test_8_the_stream_contract_on_a_busy_side_stream():
    import torch
    from helpers import stream_cases as S
    from literate_amd import _hip, ops
    lib = _hip.load()
    nb, Cn, n = 8, 4, 300

    def weights(prob, stream):
        prob.stream = stream
        return lib.lr_trait_weights(C.byref(prob))

    def init(prob, p0, stream):
        prob.stream = stream
        return lib.lr_trait_init(C.byref(prob), p0)

    def steps(prob, it0, n_it, s, rows, cap, slot0, stream):
        prob.stream = stream
        return lib.lr_trait_steps(C.byref(prob), it0, n_it, s, rows, cap, slot0)
    adapters = types.SimpleNamespace(lr_trait_weights=weights, lr_trait_init=init, lr_trait_steps=steps)
    rt = S.TorchRuntime(library=(adapters, ["lr_trait_weights", "lr_trait_init", "lr_trait_steps"]))

    def make(seed):
        ts, te, x = make_lineages(n, nb, 50 + seed, False, False)
        sp = np.array([np.count_nonzero((ts >= T0 + b) & (ts < T0 + b + 1)) for b in range(nb)], dtype=float)
        ex = np.array([np.count_nonzero((te > T0 + b) & (te <= T0 + b + 1)) for b in range(nb)], dtype=float)
        return ts, te, x, sp, ex, make_params(Cn, x, seed, seed)

    def call(ts, te, x, sp, ex, P):
        data = types.SimpleNamespace(ts=ts, te=te, x=x, sp=sp, ex=ex, n=n, t0=T0, n_bins=nb, start_time=float(T0 - 3.0),
                                     end_time=float(T0 + nb + 5.0), warn=torch.zeros(1, dtype=torch.int32, device="cuda"), device=ts.device)
        here = rt.current_stream_arg
        W, sb, sd = [ops.alloc_output(s, torch.float64, "cuda") for s in ((Cn, nb), (Cn,), (Cn,))]
        ws = ops.alloc_workspace(lib.lr_trait_weights_workspace_bytes(n, nb, Cn), "cuda")
        wp = _hip.TraitWeightsProblem(_hip.ptr(ts), _hip.ptr(te), _hip.ptr(x), _hip.ptr(P), _hip.ptr(W), _hip.ptr(sb), _hip.ptr(sd), _hip.ptr(ws),
                                      ws.numel(), n, T0, nb, Cn, None)
        assert adapters.lr_trait_weights(wp, here()) == 0
        state = ops.alloc_output((Cn, _hip.LR_TRAIT_STATE_W), torch.float64, "cuda")
        rows = ops.alloc_output((20, Cn, RW), torch.float64, "cuda")
        sws = ops.alloc_workspace(lib.lr_trait_workspace_bytes(n, nb, Cn), "cuda")
        prob = ops.trait_problem(data, state, sws, Cn, 9, ops.TraitSettings(trait_every=5, x0_lo=-3.0, x0_hi=3.0))
        assert adapters.lr_trait_init(prob, None, here()) == 0
        assert adapters.lr_trait_steps(prob, 0, 25, 3, _hip.ptr(rows), 20, 0, here()) == 0
        assert adapters.lr_trait_steps(prob, 25, 35, 3, _hip.ptr(rows), 20, 9, here()) == 0
        return dict(W=W, sb=sb, sd=sd, state=state, rows=rows)
    a, b = [S.dev(torch, v) for v in make(0)], [S.dev(torch, v) for v in make(1)]
    bufs = [torch.empty_like(v) for v in a]
    want, table = S.ordered(rt, lambda: call(*bufs), a, b, bufs, "trait")
    assert table["lr_trait_weights"]["calls"] == 1 and table["lr_trait_init"]["calls"] == 1 and table["lr_trait_steps"]["calls"] == 2
    rows = np.frombuffer(want["rows"]).reshape(20, Cn, RW)
    assert rows[-1, 0, 0] == 57.0 and rows[9, 3, 0] == 27.0


# ---- 9 ----------------------------------------------------------------------------------------------------------------------
def pooled_mean_se(chains):
    """chains [C, S] -> (pooled mean, its Monte Carlo standard error, the chains' ESS): the variance of every chain's mean is its
    variance over its own ESS, with Tracer's estimator (helpers/ess_ref.series: se2 = V / n)"""
    from helpers import ess_ref
    res = [ess_ref.series(np.asarray(c, dtype=float)) for c in chains]
    se = math.sqrt(sum(r["se2"] for r in res)) / len(res)
    return float(np.mean([r["mean"] for r in res])), se, np.array([r["ess"] for r in res])


def test_9_end_to_end_against_the_restatements_sampler():
    """2000 lineages over 30 bins, true kappa_M = 1.5, kappa_L = 0, constant baseline rates on both sides: 64 chains on the
    device, 4 of the numpy restatement; the pooled posterior means of both kappas within 4 Monte Carlo standard errors."""
    from literate_amd import ops
    n_iter, s_freq, every = 80000, 40, 2
    ts, te, x = tr.simulate(2000, 30, 0.0, 1.5, 12345)
    span = x.max() - x.min()
    rng_x0 = (float(x.min() - 0.1 * span), float(x.max() + 0.1 * span))
    win_x0, win_k = (0.5, 0.5), (0.4, 0.4)
    st = ops.TraitSettings(const_rates=1, trait_every=every, win_x0=win_x0, win_kappa=win_k, x0_lo=rng_x0[0], x0_hi=rng_x0[1])
    eng = ops.TraitEngine(ts, te, x, 64, t0=0.0, n_bins=30, seed=5, settings=st, s_freq=s_freq, n_trace_slots=n_iter // s_freq)
    eng.init()
    eng.steps(n_iter)
    dev = eng.trace_rows()[n_iter // s_freq // 2:, :, TW:TW + 4]                  # [S / 2, 64, 4]
    assert eng.warnings() == 0
    host = np.stack([tr.run_sampler(ts, te, x, 0.0, 30, n_iter, s_freq, every, win_x0, win_k, rng_x0, 100 + c)[n_iter // s_freq // 2:]
                     for c in range(4)], axis=1)                                  # [S / 2, 4, 4]
    for name, col in (("kappa_l", 1), ("kappa_m", 3)):
        md, sed, essd = pooled_mean_se(dev[:, :, col].T)
        mh, seh, essh = pooled_mean_se(host[:, :, col].T)
        print("%s: device %.4f +- %.4f (ESS %.0f), restatement %.4f +- %.4f (ESS %.0f)" % (name, md, sed, essd.sum(), mh, seh, essh.sum()))
        assert abs(md - mh) <= 4.0 * math.hypot(sed, seh), name
    assert (dev[:, :, 3] > 0).mean() > 0.99 and (host[:, :, 3] > 0).mean() > 0.99


# ---- 10 ---------------------------------------------------------------------------------------------------------------------
def test_10_the_command_line_end_to_end(tmp_path, golden_dir, capsys):
    import LiteTraitRate as cli
    from literate_amd import traitrate as T
    G = np.load(os.path.join(golden_dir, "binning_lik.npz"))
    ts, te = G["example_TBP/ts"], G["example_TBP/te"] - 0.5
    rng = np.random.default_rng(10)
    data, traits = tmp_path / "example.tsv", tmp_path / "traits.tsv"
    with open(data, "w") as f, open(traits, "w") as g:
        f.write("id\tts\tte\n"), g.write("id\tsize\n")
        for i, (a, b) in enumerate(zip(ts, te)):
            f.write("sp%d\t%g\t%g\n" % (i, 1990.0 + a, 1990.0 + b))
            g.write("sp%d\t%r\n" % (i, float(3.0 + 2.0 * rng.normal() + 0.1 * (b - a))))
        g.write("not_in_the_data\t1.0\n")
    cli.main(["-d", str(data), "-trait_data", str(traits), "-n", "3000", "-s", "10", "-p", "1000", "-seed", "3", "--chains", "4",
              "--trait_tune", "0.2", "--rtt", "0.2", "--ess", "0.2", "--block", "1000"])
    out = capsys.readouterr().out
    assert "trait effect:" in out and "multiplier s = 1" in out and "convergence:" in out
    out_dir, _, stem = T.log_paths(str(data))
    for c in range(4):
        p = T.log_paths(str(data), "", c)[1]
        lines = open(p["mcmc"]).read().splitlines()
        assert lines[0].startswith("# trait: %d lineages, standardised; mean " % len(ts)) and lines[1].split("\t") == T.TRAIT_MCMC_HEAD
        mc = np.array([l.split("\t") for l in lines[2:]], dtype=float)
        assert mc.shape == (300, 16) and mc[:, 0].tolist() == [10.0 * i for i in range(300)]
        np.testing.assert_allclose(mc[:, 1], mc[:, 2] + mc[:, 3], rtol=1e-12)
        assert len(open(p["sp_rates"]).read().splitlines()) == len(open(p["ex_rates"]).read().splitlines()) == 300
        assert len(np.unique(mc[:, 9])) > 3 and len(np.unique(mc[:, 11])) > 3                     # the kappas move
    eff = [l.split("\t") for l in open(stem + "_trait_effect.tsv").read().splitlines()]
    assert eff[0] == T.EFFECT_HEAD and [r[0] for r in eff[1:]] == list(T.PARAMS)
    vals = np.array([[float(v) for v in r[1:]] for r in eff[1:]])
    assert np.all(vals[:, 1] <= vals[:, 0]) and np.all(vals[:, 0] <= vals[:, 2]) and np.all(np.isfinite(vals[:, [0, 1, 2, 7, 8]]))
    assert np.isnan(vals[0, 6]) and 0.0 <= vals[1, 6] <= 1.0 and np.all((vals[:, 7] > 0) & (vals[:, 7] < 1))
    assert vals[0, 8] != 0.5 and vals[1, 8] != 0.1                                                   # the windows were tuned
    cur = np.array([l.split("\t") for l in open(stem + "_trait_curves.tsv").read().splitlines()[1:]], dtype=float)
    assert cur.shape == (101, 8) and np.all((cur[:, 3] <= cur[:, 2]) & (cur[:, 2] <= cur[:, 4])) and np.all((cur[:, 2:] >= 0) & (cur[:, 2:] <= 1))
    for name in ("_trait_RTT.tsv", "_trait_RTT_K.tsv", "_trait_ESS.tsv", "_trait_ESS_chains.tsv"):
        assert os.path.getsize(stem + name) > 0
    # a lineage without a value is refused by name, before any device work
    with open(traits, "w") as g:
        g.write("id\tsize\nsp0\t1.0\n")
    with pytest.raises(SystemExit, match="no trait value for lineage 'sp1'"):
        cli.main(["-d", str(data), "-trait_data", str(traits), "-n", "100", "-seed", "3"])
