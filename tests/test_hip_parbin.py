"""The parametric samplers on per-chain binned statistics (include/literate_hip_parbin.h, csrc/lr_parbin.hip,
literate_amd/replicates_par.py) on the GPU:

  1  against the numpy restatement (tests/helpers/parbin_ref.py): rows and final state at 1e-9 under every DDRate model and all
     four trend models, 3 replicates x 2 chains, chain0 = 5
  2  the bins-per-lane and lane edges, both samplers, 1 and 3 chains per replicate
  3  the chain-count edges of the four-wave workgroup
  4  a chain's bits depend on its own arguments alone
  5  a run cut into launches - in iterations, or into groups of replicates - is the same run bit for bit
  6  bit for bit the beta = 1 chain of lr_mlik_steps / lr_tmlik_steps at R = 1 (they share the iteration, csrc/lr_par_iter.h)
  7  ParametricReplicateEngine against DDRateEngine / TrendRateEngine from lineages
  8  the buffer and stream contract
  9  the posterior mean of l_max under constant rates, in closed form
 10  the command lines

The bound on trajectory rows is the project's standing one: 1e-9 relative (absolute where the value is 0); it decides nothing
about an accept decision because the restatement's smallest margin is held above 1e-6 in every case (the tie condition,
asserted here and - without a GPU - in tests/test_parbin_host.py).
"""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import parbin_ref as pr          # noqa: E402

pytestmark = pytest.mark.gpu
W = pr.TRACE_W


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def dev_data(ops, D, cpr, sampler):
    return ops.ParbinData(D.n_spec, D.n_exti, D.DT, D.origin, D.present, cpr, D.trend if sampler == 2 else None)


def device_run(D, sampler, mb, md, cpr, n_it, s_freq, seed, chain0, cuts=None):
    """the whole run in one launch, or cut into launches of `cuts` iterations -> (rows, state) on the device"""
    import torch
    from literate_amd import ops
    data, st = dev_data(ops, D, cpr, sampler), ops.ParbinSettings(sampler, mb, md, 0.1)
    state = ops.parbin_init(data, seed, st, chain0)
    if cuts is None:
        return ops.parbin_steps(data, state, 0, n_it, s_freq, seed, st, chain0), state
    n = (n_it + s_freq - 1) // s_freq
    rows = torch.full((n, data.n_chains, W), float("nan"), dtype=torch.float64, device="cuda")
    it = 0
    while it < n_it:
        k = min(cuts, n_it - it)
        ops.parbin_steps(data, state, it, k, s_freq, seed, st, chain0, rows=rows, slot0=(it + s_freq - 1) // s_freq)
        it += k
    return rows, state


def close(got, want, what):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    err = np.where(same, 0.0, err)
    assert not np.isnan(err).any() and err.max() <= 1e-9, "%s: largest error %.3g at %s" % (
        what, np.nanmax(err), np.unravel_index(np.nanargmax(err), err.shape))


def against_restatement(case):
    name, key, sampler, mb, md, cpr, n_it, s_freq, seed, chain0 = case
    D, want_rows, want_state, margin = pr.run_case(case)
    print("%s: smallest margin %.3g" % (name, margin))
    assert margin > pr.TIE, "%s: an accept decision within %g of a tie" % (name, pr.TIE)
    rows, state = device_run(D, sampler, mb, md, cpr, n_it, s_freq, seed, chain0)
    close(rows.cpu().numpy(), want_rows, name + " rows")
    close(state.cpu().numpy(), want_state, name + " state")


def bits(*ts):
    return [t.cpu().numpy().tobytes() for t in ts]


# ---- 1, 2, 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.CASES_MODELS, ids=[c[0] for c in pr.CASES_MODELS])
def test_1_every_model_against_the_restatement(case):
    assert case[1][0] * case[5] == 6 and case[6] == 600 and case[7] == 7 and case[9] == 5
    against_restatement(case)


def test_1_the_case_table_holds_every_model():
    got = sorted((c[2], c[3], c[4]) for c in pr.CASES_MODELS)
    assert got == sorted([(1, mb, md) for mb in (0, 1, 2) for md in (-2, -1, 0, 1, 2)] + [(2, b, d) for b in (0, 1) for d in (0, 1)])
    assert sorted({c[1][1] for c in pr.CASES_BINS}) == [1, 2, 63, 64, 65, 128, 129, 256, 257, 511, 512]
    assert sorted({c[1][0] * c[5] for c in pr.CASES_CHAINS}) == [1, 3, 4, 5, 8, 9]


@pytest.mark.parametrize("case", pr.CASES_BINS, ids=[c[0] for c in pr.CASES_BINS])
def test_2_bins_per_lane_and_lane_edges(case):
    against_restatement(case)


@pytest.mark.parametrize("case", pr.CASES_CHAINS, ids=[c[0] for c in pr.CASES_CHAINS])
def test_3_chain_count_edges(case):
    against_restatement(case)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [1, 2])
def test_4_a_chains_bits_depend_on_its_own_arguments_alone(sampler):
    X, YZ = pr.synthetic(1, 70, 1), pr.synthetic(2, 70, 2)
    B = pr.Data(np.concatenate([YZ.n_spec, X.n_spec]), np.concatenate([YZ.n_exti, X.n_exti]), np.concatenate([YZ.DT, X.DT]),
                np.concatenate([YZ.origin, X.origin]), np.concatenate([YZ.present, X.present]), X.trend)
    mb, md, k = (2, 2, 7) if sampler == 1 else (0, 0, 7)
    rows_a, state_a = device_run(X, sampler, mb, md, 1, 150, 3, 11, k)
    rows_b, state_b = device_run(B, sampler, mb, md, 1, 150, 3, 11, k - 2)
    assert bits(rows_a[:, 0], state_a[0]) == bits(rows_b[:, 2], state_b[2])
    assert bits(rows_a[:, 0]) != bits(rows_b[:, 1]), "another replicate's chain runs on other data"


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [1, 2])
@pytest.mark.parametrize("s_freq", [1, 7])
def test_5_a_run_cut_into_launches_is_the_same_run(sampler, s_freq):
    D = pr.synthetic(2, 40, 3)
    mb, md = (2, 2) if sampler == 1 else (0, 0)
    want = bits(*device_run(D, sampler, mb, md, 2, 193, s_freq, 21, 4))
    for cuts in (1, 6, 100):
        assert bits(*device_run(D, sampler, mb, md, 2, 193, s_freq, 21, 4, cuts=cuts)) == want, "cuts of %d iterations" % cuts


@pytest.mark.parametrize("sampler", [1, 2])
def test_5_disjoint_replicate_groups_with_chain0_advanced(sampler):
    import torch
    D = pr.synthetic(4, 40, 4)
    mb, md = (2, 2) if sampler == 1 else (0, 0)
    rows, state = device_run(D, sampler, mb, md, 2, 193, 7, 22, 3)
    r0, s0 = device_run(D.take([0, 1]), sampler, mb, md, 2, 193, 7, 22, 3)
    r1, s1 = device_run(D.take([2, 3]), sampler, mb, md, 2, 193, 7, 22, 3 + 4)
    assert bits(torch.cat([r0, r1], dim=1), torch.cat([s0, s1], dim=0)) == bits(rows, state)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [12, 130])
def test_6_sampler_1_is_the_cold_chain_of_lr_mlik_steps(n_bins):
    """T = 2, betas (0, 1), scales (1, 1): the beta = 1 chain of replicate rep0 + r has key (rep0 + r) 2 + 1; the iteration is
    shared (csrc/lr_par_iter.h), so likelihood, prior and parameters agree bit for bit"""
    from literate_amd import ops
    D = pr.synthetic(1, n_bins, 6)
    rep0, n_reps, n_it, s_freq, seed = 3, 3, 300, 3, 31
    for mb, md in ((2, 2), (1, -1), (0, 0)):
        data = ops.MlikData(D.n_spec[0], D.n_exti[0], D.DT[0], D.origin[0], D.present[0], mb, md, 0.1)
        mrows, mstate = ops.mlik_run(data, [0.0, 1.0], [1.0, 1.0], n_reps, n_it, s_freq, seed, rep0)
        for r in range(n_reps):
            rows, state = device_run(D, 1, mb, md, 1, n_it, s_freq, seed, (rep0 + r) * 2 + 1)
            assert bits(rows[:, 0, 2:12]) == bits(mrows[:, r, 1, 2:12]), (mb, md, r)
            assert bits(state[0, :14]) == bits(mstate[r, 1, :14]), (mb, md, r)


@pytest.mark.parametrize("n_bins", [12, 130])
def test_6_sampler_2_is_the_cold_chain_of_lr_tmlik_steps(n_bins):
    from literate_amd import ops
    D = pr.synthetic(1, n_bins, 7)
    key0, n_reps, n_it, s_freq, seed = 2, 2, 300, 3, 32
    data = ops.TmlikData(D.n_spec[0], D.n_exti[0], D.DT[0], D.trend)
    flags = [0, 1, 2, 3]
    grid = ops.TmlikGrid([0] * 4, flags, [key0] * 4, [0.0, 1.0], [1.0, 1.0], n_reps)
    trows, tstate = ops.tmlik_run(data, grid, 0.001, n_it, s_freq, seed)
    for m, f in enumerate(flags):
        for r in range(n_reps):
            rows, state = device_run(D, 2, f & 1, (f >> 1) & 1, 1, n_it, s_freq, seed, (key0 + r) * 2 + 1)
            assert bits(rows[:, 0, 2:10]) == bits(trows[m, :, r, 1, 2:10]), (f, r)
            assert bits(state[0, :6], state[0, 8:14]) == bits(tstate[m, r, 1, :6], tstate[m, r, 1, 6:12]), (f, r)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [1, 2])
def test_7_against_the_lineage_engines(sampler):
    from literate_amd import replicates_par as rp
    from literate_amd.ddrate import DDRateEngine
    from literate_amd.trendrate import TrendRateEngine
    lins = pr.lineage_replicates()
    D, want_rows, want_state, margin = pr.run_lineage_case(sampler)
    assert margin > pr.TIE
    seed, n_it, cpr = pr.LINEAGE_SEEDS[sampler], pr.LINEAGE_ITERS, pr.LINEAGE_CPR
    args = types.SimpleNamespace(rm_first_bin=0)
    reps = rp.load_binned_replicates(["r0", "r1"], args, parse=lambda path, a: lins[int(path[1:])], trend=D.trend if sampler == 2 else None)
    np.testing.assert_array_equal(reps.DT, D.DT), np.testing.assert_array_equal(reps.n_spec, D.n_spec)
    assert reps.n_bins == 12 and not np.array_equal(reps.n_exti[0], reps.n_exti[1])
    mb, md = (2, 2) if sampler == 1 else (0, 0)
    eng = rp.ParametricReplicateEngine(reps, 2 * cpr, sampler=sampler, m_birth=mb, m_death=md, seed=seed, s_freq=1, n_trace_slots=n_it)
    eng.init()
    eng.steps(n_it)
    got = eng.trace_rows()
    table, cols, head = eng.ess_rows(eng.trace[:n_it])
    table = table.cpu().numpy()
    close(got, want_rows, "the engine against the restatement")
    for r, (ts, te, present, origin) in enumerate(lins):
        if sampler == 1:
            one = DDRateEngine(ts, te, origin, present, cpr, m_birth=mb, m_death=md, seed=seed, s_freq=1, n_trace_slots=n_it, chain_offset=r * cpr)
        else:
            one = TrendRateEngine(ts, te, origin, present, D.trend, cpr, seed=seed, s_freq=1, n_trace_slots=n_it, chain_offset=r * cpr)
        one.init()
        one.steps(n_it)
        want = one.trace_rows()
        wtable = one.ess_rows(one.trace[:n_it])[0].cpu().numpy()
        one.close()
        close(got[:, eng.chains_of(r), :4 + eng.npar], want[:, :, :4 + eng.npar], "replicate %d against its lineage engine" % r)
        close(table[:, eng.chains_of(r)][..., cols], wtable[..., cols], "replicate %d: the ESS table, as the log holds it" % r)
        assert np.all(got[:, eng.chains_of(r), 4 + eng.npar:] == 0.0)
    eng.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins,R,cpr,sampler", [(1, 1, 1, 1), (65, 3, 2, 2), (512, 2, 3, 1), (257, 1, 5, 2)])
def test_8_the_buffer_contract_on_exact_size_guarded_buffers(n_bins, R, cpr, sampler):
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    D = pr.synthetic(R, n_bins, 5)
    st = ops.ParbinSettings(sampler, 2 if sampler == 1 else 0, 2 if sampler == 1 else 0, 0.1)
    Cn = R * cpr

    def whole():
        data = dev_data(ops, D, cpr, sampler)
        state = ops.parbin_init(data, 9, st)
        first = ops.parbin_steps(data, state, 0, 25, 3, 9, st)                           # rows_cap exactly the 9 rows written
        rows = ops.alloc_output((13, Cn, W), torch.float64, "cuda")
        ops.parbin_steps(data, state, 25, 15, 3, 9, st, rows=rows)                       # iterations 27 .. 39: slots 0 .. 4
        ops.parbin_steps(data, state, 40, 24, 3, 9, st, rows=rows, slot0=5)              # 42 .. 63: slots 5 .. 12, exactly to the end
        return first, rows, state

    out = contract(ops, torch, whole, label="parbin bins %d" % n_bins)
    assert out[0].shape[0] == 9 and out[1][0, 0, 0] == 27 and out[1][-1, Cn - 1, 0] == 63 and out[1][5, 0, 0] == 42


def test_8_slots_outside_the_launch_are_untouched():
    import torch
    from literate_amd import ops
    D = pr.synthetic(2, 9, 5)
    data, st = dev_data(ops, D, 2, 1), ops.ParbinSettings()
    state = ops.parbin_init(data, 9, st)
    rows = torch.full((12, 4, W), float("nan"), dtype=torch.float64, device="cuda")
    ops.parbin_steps(data, state, 0, 10, 3, 9, st, rows=rows, slot0=3)          # iterations 0, 3, 6, 9: slots 3 .. 6
    h = rows.cpu().numpy()
    assert np.isnan(h[:3]).all() and np.isnan(h[7:]).all() and not np.isnan(h[3:7]).any()
    assert h[3:7, :, 0].T.tolist() == [[0.0, 3.0, 6.0, 9.0]] * 4 and np.all(h[3:7, :, 12:] == 0.0)


def test_8_argument_errors_in_the_headers_order_leave_the_buffers_untouched():
    import torch
    from helpers.abi_cases import refuses
    from literate_amd import _hip, ops
    lib = _hip.load()
    small, big = pr.synthetic(2, 8, 5), pr.synthetic(2, 513, 5)
    D = lambda d=small, cpr=2, sampler=1: dev_data(ops, d, cpr, sampler)
    S = ops.ParbinSettings
    for what, call, code in (
            ("513 bins", lambda: ops.parbin_init(D(big), 1), "LR_ERR_SIZE"),
            ("513 bins before the model", lambda: ops.parbin_init(D(big), 1, S(sampler=3)), "LR_ERR_SIZE"),
            ("sampler 2 without the trend, before 513 bins", lambda: ops.parbin_init(D(big), 1, S(sampler=2, m_birth=0, m_death=0)), "LR_ERR_NULL"),
            ("sampler 0", lambda: ops.parbin_init(D(), 1, S(sampler=0)), "LR_ERR_MODEL"),
            ("sampler 3", lambda: ops.parbin_init(D(), 1, S(sampler=3)), "LR_ERR_MODEL"),
            ("m_birth 3", lambda: ops.parbin_init(D(), 1, S(m_birth=3)), "LR_ERR_MODEL"),
            ("m_birth -1", lambda: ops.parbin_init(D(), 1, S(m_birth=-1)), "LR_ERR_MODEL"),
            ("m_death -3", lambda: ops.parbin_init(D(), 1, S(m_death=-3)), "LR_ERR_MODEL"),
            ("m_death 3", lambda: ops.parbin_init(D(), 1, S(m_death=3)), "LR_ERR_MODEL"),
            ("init_death nan", lambda: ops.parbin_init(D(), 1, S(init_death=float("nan"))), "LR_ERR_MODEL"),
            ("const_B 2", lambda: ops.parbin_init(D(sampler=2), 1, S(sampler=2, m_birth=2, m_death=0)), "LR_ERR_MODEL"),
            ("const_D -1", lambda: ops.parbin_init(D(sampler=2), 1, S(sampler=2, m_birth=0, m_death=-1)), "LR_ERR_MODEL")):
        refuses(ops, torch, call, code, label=what, entry="lr_parbin_init")
    # the step arguments, and the order NULL < SIZE < MODEL < the step arguments: straight at the library, on buffers of a known fill
    data, bigd = D(), D(big)
    state = ops.parbin_init(data, 1)
    before = state.clone()
    rows = torch.full((9, 4, W), 7.0, dtype=torch.float64, device="cuda")

    def steps(d=data, st=state, s=S(), cap=10, rows_=rows, it0=0, n_it=10, sf=1, slot0=0, null=None, R=None, cpr=None):
        prob = ops.parbin_problem(d, st, 1, s)
        if null:
            setattr(prob, null, None)
        if R is not None:
            prob.R = R
        if cpr is not None:
            prob.chains_per_rep = cpr
        return _hip.launch_problem(lib.lr_parbin_steps, d.device, prob, it0, n_it, sf, _hip.ptr(rows_), cap, slot0)

    E = _hip
    assert steps(cap=9) == E.LR_ERR_SIZE and steps(cap=10, slot0=1) == E.LR_ERR_SIZE and steps(cap=-1) == E.LR_ERR_SIZE
    assert steps(s=S(sampler=4), cap=9) == E.LR_ERR_MODEL and steps(s=S(m_birth=5), sf=0) == E.LR_ERR_MODEL
    assert steps(sf=0) == steps(it0=-1) == steps(n_it=-1) == steps(slot0=-1) == E.LR_ERR_SIZE
    assert steps(R=0) == steps(R=0, s=S(sampler=4)) == steps(cpr=0) == steps(R=2 ** 30, cpr=2) == E.LR_ERR_SIZE
    # ... also without rows: NULL is the answer only where the step arguments are valid and a row is due
    assert steps(rows_=None, sf=0) == steps(rows_=None, it0=-1) == steps(rows_=None, n_it=-1) == E.LR_ERR_SIZE
    assert steps(rows_=None) == E.LR_ERR_NULL and steps(d=bigd, s=S(sampler=4)) == E.LR_ERR_SIZE
    for field in ("n_spec", "n_exti", "DT", "origin", "present", "state"):
        assert steps(d=bigd, s=S(sampler=4), null=field) == E.LR_ERR_NULL, field
    assert steps(d=bigd, s=S(sampler=2, m_birth=0, m_death=0)) == E.LR_ERR_NULL, "sampler 2 without the trend"
    assert steps(null="trend", cap=9, n_it=0) == 0, "the trend is required for sampler 2 only"
    assert lib.lr_parbin_steps(None, 0, 10, 1, _hip.ptr(rows), 10, 0) == E.LR_ERR_NULL and lib.lr_parbin_init(None) == E.LR_ERR_NULL
    torch.cuda.synchronize()
    assert torch.equal(before, state) and bool((rows == 7.0).all())
    for what, call in (("s_freq 0", lambda: ops.parbin_steps(data, state, 0, 10, 0, 1)), ("it0 < 0", lambda: ops.parbin_steps(data, state, -1, 10, 1, 1)),
                       ("n_iters < 0", lambda: ops.parbin_steps(data, state, 0, -1, 1, 1))):
        with pytest.raises(ValueError, match="lr_parbin_steps: LR_ERR_SIZE"):
            call()
    # where no row is due rows may be NULL; n_iters = 0 launches nothing
    assert steps(rows_=None, it0=1, n_it=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, state)
    assert steps(rows_=None, it0=1, n_it=2, sf=5) == 0 and steps(cap=9, it0=3, n_it=9) == 0
    torch.cuda.synchronize()
    assert not torch.equal(before, state) and rows[:, :, 0].unique().tolist() == [float(i) for i in range(3, 12)]


@pytest.mark.parametrize("sampler", [1, 2])
def test_8_the_stream_contract_on_a_busy_side_stream(sampler):
    """lr_parbin_init and lr_parbin_steps take the stream in their descriptor, so they are not among the functions
    helpers/stream_cases finds by their last parameter: the library handed to TorchRuntime here is a pair of adapters with the
    stream last, which put it into the descriptor and call the entry point.  8 bins, 2 replicates x 2 chains, 60 iterations in
    two launches; the statistics, the windows and the covariate are the inputs copied behind the delay."""
    import torch
    from helpers import stream_cases as S
    from literate_amd import _hip, ops
    lib = _hip.load()
    nb, R, cpr = 8, 2, 2
    st = ops.ParbinSettings(sampler, 2 if sampler == 1 else 0, 2 if sampler == 1 else 0, 0.1)

    def init(prob, stream):
        prob.stream = stream
        return lib.lr_parbin_init(C.byref(prob))

    def steps(prob, it0, n, s, rows, cap, slot0, stream):
        prob.stream = stream
        return lib.lr_parbin_steps(C.byref(prob), it0, n, s, rows, cap, slot0)
    adapters = types.SimpleNamespace(lr_parbin_init=init, lr_parbin_steps=steps)
    rt = S.TorchRuntime(library=(adapters, ["lr_parbin_init", "lr_parbin_steps"]))

    def make(seed):
        D = pr.synthetic(R, nb, 40 + seed)
        return D.n_spec, D.n_exti, D.DT, D.origin, D.present, D.trend

    def call(n_spec, n_exti, DT, origin, present, trend):
        data = ops.ParbinData(n_spec, n_exti, DT, origin, present, cpr, trend if sampler == 2 else None)
        assert data.n_spec.data_ptr() == n_spec.data_ptr() and data.present.data_ptr() == present.data_ptr()          # used as they are: no copy
        assert sampler == 1 or data.trend.data_ptr() == trend.data_ptr()
        state = ops.alloc_output((R * cpr, _hip.LR_PARBIN_STATE_W), torch.float64, "cuda")
        rows = ops.alloc_output((20, R * cpr, W), torch.float64, "cuda")
        prob = ops.parbin_problem(data, state, 9, st)
        here = rt.current_stream_arg
        assert adapters.lr_parbin_init(prob, here()) == 0
        assert adapters.lr_parbin_steps(prob, 0, 25, 3, _hip.ptr(rows), 20, 0, here()) == 0          # rows of iterations 0 .. 24: slots 0 .. 8
        assert adapters.lr_parbin_steps(prob, 25, 35, 3, _hip.ptr(rows), 20, 9, here()) == 0         # 27 .. 57: slots 9 .. 19
        return dict(state=state, rows=rows)
    a, b = [S.dev(torch, x) for x in make(0)], [S.dev(torch, x) for x in make(1)]
    bufs = [torch.empty_like(x) for x in a]
    want, table = S.ordered(rt, lambda: call(*bufs), a, b, bufs, "parbin sampler %d" % sampler)
    assert table["lr_parbin_init"]["calls"] == 1 and table["lr_parbin_steps"]["calls"] == 2
    rows = np.frombuffer(want["rows"]).reshape(20, R * cpr, W)
    assert rows[-1, 0, 0] == 57.0 and rows[9, 3, 0] == 27.0


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_9_the_posterior_mean_of_l_max_under_constant_rates():
    """DDRate model (0, 0): lam_b = l_max in every bin, so the likelihood of l_max is l^N exp(-l T) with N = sum n_spec and
    T = sum DT.  dd_calc_prior (DD:110-122) puts Gamma(shape 1, scale 10) on l_max, density ~ exp(-l / 10), independent of
    every other parameter, and no other term of the posterior involves l_max; the multiplier move with its Hastings ratio
    log m leaves the posterior invariant on l > 0.  Hence l_max | data ~ Gamma(N + 1, rate T + 0.1) with mean
    (N + 1) / (T + 0.1) (pr.constant_rate_posterior_mean).  64 chains per replicate, 6000 iterations sampled every 10, the
    first 100 samples dropped: the mean of the chain means lies within 4 between-chain standard errors (sd of the chain means /
    sqrt(64)) of that mean - the margin of tests/test_hip_mc3.py - for a replicate and, in the same launch, for a second one
    with doubled counts, which lands on its own value and not the first's."""
    X = pr.synthetic(1, 12, 9)
    D = pr.Data(np.concatenate([X.n_spec, 2 * X.n_spec]), np.concatenate([X.n_exti, 2 * X.n_exti]), np.concatenate([X.DT, X.DT]),
                np.concatenate([X.origin, X.origin + 2.0]), np.concatenate([X.present, X.present + 2.0]))
    rows, _ = device_run(D, 1, 0, 0, 64, 6000, 10, 77, 0)
    l_max = rows[100:, :, 4].cpu().numpy()
    means = l_max.mean(axis=0).reshape(2, 64)
    want = [pr.constant_rate_posterior_mean(D.n_spec[r].sum(), D.DT[r].sum()) for r in range(2)]
    for r in range(2):
        m, se = means[r].mean(), means[r].std(ddof=1) / np.sqrt(64)
        print("replicate %d: mean of chain means %.6g, derived %.6g, se %.3g (%.2f se)" % (r, m, want[r], se, (m - want[r]) / se))
        assert abs(m - want[r]) <= 4 * se
        assert abs(m - want[1 - r]) > 4 * se, "replicate %d lands on the other replicate's value" % r


# ---- 10 -----------------------------------------------------------------------------------------------------------------------
def write_tsv(path, ts, te):
    with open(path, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, b) in enumerate(zip(ts, te)):
            f.write("%d\t%d\t%d\n" % (i, a, b))


def cli(prog, args, cwd, **env):
    env = dict(os.environ, PYTHONPATH=ROOT, **env)
    return subprocess.run([sys.executable, os.path.join(ROOT, prog)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


def make_files(tmp_path, R=3, n=200):
    rng = np.random.default_rng(8)
    ts = np.sort(rng.integers(1950, 1985, n))
    ts[0], files = 1950, []
    for r in range(R):
        te = np.minimum(ts + rng.integers(0, 25, n), 1990)
        te[-1] = 1990
        d = tmp_path / ("rep%d" % r)
        d.mkdir()
        files.append(str(d / ("bands_%d.tsv" % r)))
        write_tsv(files[-1], ts, te)
    trend = str(tmp_path / "trend.tsv")
    with open(trend, "w") as f:
        f.write("year\tcov\n")
        for i, v in enumerate(rng.uniform(1.0, 9.0, 41)):          # one value per window of create_bins: the last is dropped
            f.write("%d\t%r\n" % (1950 + i, float(v)))
    return files, trend


def read_log(path):
    with open(path, newline="") as f:
        text = f.read()
    lines = text.split("\r\n")
    assert lines[-1] == "" and "\n" not in text.replace("\r\n", ""), "%s: csv.writer's line ends" % path
    return lines[0].split("\t"), np.array([[float(x) for x in ln.split("\t")] for ln in lines[1:-1]])


@pytest.mark.parametrize("prog", ["DDRate.py", "trend_rate.py"])
def test_10_the_command_line_end_to_end(tmp_path, prog):
    files, trend = make_files(tmp_path)
    dd = prog == "DDRate.py"
    model = [] if dd else ["-trend_data", trend, "-trend_index", "1"]
    suffix, tail, ptail = ("_LDDN_MDDN", ".log", "") if dd else ("_EXPB_EXPD", "_1.trendrate.log", "_1")
    run = ["--chains", "6", "-n", "400", "-s", "10", "-seed", "3", "--ess", "0.1", "--summary", "0.2"] + model
    res = cli(prog, ["--replicates", str(tmp_path / "rep*" / "bands_*.tsv")] + run, str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    nb, npar = 40, 8 if dd else 6
    n_cols = (14 + 4 * nb + 3) if dd else (12 + 2 * nb + 3)
    logs = {}
    for r, path in enumerate(files):
        for k in range(2):
            p = "%s_3%s_c%d%s" % (os.path.splitext(path)[0], suffix, k, tail)
            head, tab = read_log(p)
            assert head[:2] == ["it", "posterior"] and head[-3:] == ["corr_coeff", "rsquared", "gelman_r2"] and len(head) == n_cols
            assert tab.shape == (40, n_cols) and tab[:, 0].tolist() == [10.0 * i for i in range(40)]
            logs[r, k] = tab
    assert not np.allclose(logs[0, 0][:, 2], logs[1, 0][:, 2]), "replicates differ in their data"
    base = os.path.join(os.path.dirname(files[0]), "replicates3")
    stem = "%s_3%s%s" % (base, suffix, ptail)
    kinds = 5 if dd else 3
    with open(stem + "_summary.tsv") as f:
        lines = f.read().splitlines()
    assert lines[0].split("\t")[:4] == ["time", "net_diversity", "emp_birth", "emp_death"] and len(lines[0].split("\t")) == 4 + 3 * kinds
    assert len(lines) == 1 + nb
    with open(stem + "_summary_params.tsv") as f:
        lines = f.read().splitlines()
    assert lines[0] == "parameter\tmean\tminHPD\tmaxHPD" and len(lines) == 1 + 3 + npar
    with open(stem + "_replicates.tsv") as f:
        lines = f.read().splitlines()
    from literate_amd import replicates_par as rp
    assert lines[0].split("\t") == rp.REPLICATES_HEAD and len(lines) == 1 + 3 * (3 + npar)
    assert lines[1].split("\t")[:3] == ["0", "bands_0.tsv", "posterior"]
    with open(stem + "_ESS.tsv") as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("#") and "between-imputation variance" in lines[0] and len(lines) == 2 + 3 + npar
    with open(stem + "_ESS_chains.tsv") as f:
        assert len(f.read().splitlines()) == 1 + 6 * (3 + npar)
    div = np.loadtxt(base + "_div_replicates.tsv", skiprows=1)
    assert div.shape == (nb, 10)
    # replicate 0 alone, by the plain command line: chain k has the same Philox key
    res = cli(prog, ["-d", files[0], "--chains", "2", "-n", "400", "-s", "10", "-seed", "3"] + model, str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    for k in range(2):
        head, tab = read_log("%s_3%s_c%d%s" % (os.path.splitext(files[0])[0], suffix, k, tail))
        assert len(head) == n_cols
        close(logs[0, k], tab, "the log of replicate 0 chain %d against %s -d" % (k, prog))


@pytest.mark.parametrize("prog", ["DDRate.py", "trend_rate.py"])
def test_10_every_refused_flag_exits_with_its_sentence(tmp_path, prog):
    from literate_amd import replicates_par as rp
    files, trend = make_files(tmp_path, R=2, n=50)
    model = [] if prog == "DDRate.py" else ["-trend_data", trend, "-trend_index", "1"]
    one = ["--replicates", files[0], "-n", "200", "-s", "100"] + model
    sentences = dict((n, why) for n, _, why in rp.REFUSED)
    assert sorted(sentences) == ["ade", "ade_joint", "loo", "mlik", "ppc", "ppc_age", "waic"]
    # (every one of these exits on its arguments, before the GPU is opened: they run side by side)
    jobs = [(one + ["--%s" % name, "0.2"], {}, want) for name, want in sorted(sentences.items())]
    jobs += [(one + ["-d", files[0]], {}, "leave -d empty"), (one, dict(WORLD_SIZE="2"), "runs on one GPU (WORLD_SIZE is 2)"),
             (["--replicates", ",".join(files), "--chains", "3", "-n", "200", "-s", "100"] + model, {}, "must be a multiple of the 2 files")]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(5) as pool:
        done = list(pool.map(lambda j: cli(prog, j[0], str(tmp_path), **j[1]), jobs))
    for (args, env, want), res in zip(jobs, done):
        assert res.returncode != 0 and want in res.stderr, (args, env, res.stderr[-500:])
        assert "Traceback" not in res.stderr, (args, res.stderr[-500:])
