"""The multi-trait extinction sampler (include/literate_hip_mte.h, csrc/lr_mte.hip, literate_amd/mte.py) on the GPU:

  1  ops.mte_loglik against the per-lineage likelihood (MTEmodel.py:336-354, tests/helpers/mte_ref.py) at rtol 1e-9: every
     instantiation and its edges, T = 1 and 16, I all 0 / all 1 / mixed, empty combinations, m = 1e-6 and 1e3; the example file
  2  the sampler against the numpy restatement: rows and final state at 1e-9, the counters exactly
  3  a run cut into launches - in iterations, or into groups of problems - is the same run bit for bit; a chain's bits depend
     on its own arguments alone
  4  the buffer and stream contract, every error code in the header's order
  5  with constant = 1 the posterior of m is Gamma(E_tot + 1, rate B_tot + 1)
  6  a trait that drives extinction is selected before one that does not, and its multipliers are ordered as the truth
  7  the command line end to end on the fixture

The bound on trajectory rows is the project's standing one: 1e-9 relative (absolute where the value is 0); it decides nothing
about an accept decision because the restatement's smallest margin is held above 1e-6 in every case (the tie condition,
asserted here and - without a GPU - in tests/test_mte_host.py).
"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import mte_ref as mr          # noqa: E402

pytestmark = pytest.mark.gpu
W = mr.ROW_W


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def dev_data(ops, D, cpp):
    return ops.MteData(D.code, D.n_states, D.n, D.E, D.B, cpp)


def settings_of(ops, st):
    return ops.MteSettings(*st)


def device_run(D, st, cpp, n_it, s_freq, seed, chain0, cuts=None):
    """the whole run in one launch, or cut into launches of `cuts` iterations -> (rows, state) on the device"""
    import torch
    from literate_amd import ops
    data, S = dev_data(ops, D, cpp), settings_of(ops, st)
    state = ops.mte_init(data, seed, S, chain0)
    if cuts is None:
        return ops.mte_steps(data, state, 0, n_it, s_freq, seed, S, chain0), state
    n = (n_it + s_freq - 1) // s_freq
    rows = torch.full((n, data.n_chains, W), float("nan"), dtype=torch.float64, device="cuda")
    it = 0
    for k in cuts:
        ops.mte_steps(data, state, it, k, s_freq, seed, S, chain0, rows=rows, slot0=(it + s_freq - 1) // s_freq)
        it += k
    assert it == n_it
    return rows, state


def close(got, want, what, rtol=1e-9):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    err = np.where(same, 0.0, err)
    assert not np.isnan(err).any() and err.max() <= rtol, "%s: largest error %.3g at %s" % (
        what, np.nanmax(err), np.unravel_index(np.nanargmax(err), err.shape))


def bits(*ts):
    return [t.cpu().numpy().tobytes() for t in ts]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def loglik_case(D, lineages, label):
    """P problems x 5 chains: I all 0, all 1, mixed, then m = 1e-6 and m = 1e3 (mixed I); sd and beta_hp random"""
    from literate_amd import ops
    combo, bl, ex, tr, keep = lineages
    cpp, C = 5, 5 * D.P
    g = np.random.default_rng(12)
    m, Y, I = mr.random_params(D, C, 13, "mixed")
    for p in range(D.P):
        I[p * cpp], I[p * cpp + 1] = 0, 1
        m[p * cpp + 3], m[p * cpp + 4] = 1e-6, 1e3
    sd, beta = g.uniform(0.3, 3.0, (C, D.T)), g.uniform(0.2, 5.0, C)
    lik, prior = ops.mte_loglik(dev_data(ops, D, cpp), m, Y, I, sd, beta)
    lik, prior = lik.cpu().numpy(), prior.cpu().numpy()
    for c in range(C):
        p = c // cpp
        want, _ = mr.loglik_lineages(bl[keep[p]], ex[keep[p]], tr[keep[p]], D.n_states, m[c], Y[c], I[c])
        close(lik[c], want, "%s: the likelihood of chain %d" % (label, c))
        close(prior[c], mr.log_prior(D, m[c], Y[c], I[c], sd[c], beta[c], 0.05), "%s: the prior of chain %d" % (label, c))


@pytest.mark.parametrize("G", mr.G_EDGES + [mr.G_MID8])
@pytest.mark.parametrize("n_states", [mr.T1, mr.T16], ids=["T1", "T16"])
def test_1_loglik_against_the_per_lineage_likelihood(G, n_states):
    D, lineages = mr.synthetic(2, G, n_states, 500 + G, n_lin=max(2 * G, 150))
    assert G == 1 or (D.n[1] == 0).any(), "the second problem leaves combinations empty"
    loglik_case(D, lineages, "G %d T %d" % (G, len(n_states)))


def test_1_loglik_on_the_example_file():
    from literate_amd import ops
    ts, te, traits, _ = mr.read_example()
    tab = ops.mte_tables(ts, te, traits, mr.EXAMPLE_SLICES)
    D = mr.Data(tab["code"], tab["n_states"], tab["n"], tab["E"], tab["B"])
    keep = [ops.mte_slice(ts, te, t0, t1) for t0, t1 in mr.EXAMPLE_SLICES]
    # per slice its own bl and ex: the lineages are laid out slice after slice
    bl, ex = np.concatenate([k[1] for k in keep]), np.concatenate([k[2] for k in keep])
    tr = np.concatenate([tab["code"][tab["combo"][k[0]]].astype(np.int64) for k in keep])
    edges = np.cumsum([0] + [int(k[0].sum()) for k in keep])
    masks = [(np.arange(len(bl)) >= a) & (np.arange(len(bl)) < b) for a, b in zip(edges[:-1], edges[1:])]
    loglik_case(D, (None, bl, ex, tr, masks), "the example")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_2_the_sampler_against_the_restatement(case):
    name, key, st, cpp, n_it, s_freq, seed, chain0 = case
    D, want_rows, want_state, margin = mr.run_case(case)
    print("%s: smallest margin %.3g" % (name, margin))
    assert margin > mr.TIE, "%s: an accept decision within %g of a tie" % (name, mr.TIE)
    rows, state = device_run(D, st, cpp, n_it, s_freq, seed, chain0)
    rows, state = rows.cpu().numpy(), state.cpu().numpy()
    cnt = slice(mr.S_PROPOSED, mr.S_PROPOSED + 6)
    assert np.array_equal(state[:, cnt], want_state[:, cnt]), "%s: the counters" % name
    close(rows, want_rows, name + " rows")
    close(state, want_state, name + " state")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_freq", [1, 7])
@pytest.mark.parametrize("G,n_states", [(65, mr.T3), (300, mr.T16)], ids=["G65", "G300"])
def test_3_a_run_cut_into_launches_is_the_same_run(G, n_states, s_freq):
    D = mr.synthetic(2, G, n_states, 3)[0]
    want = bits(*device_run(D, mr.BVS, 3, 300, s_freq, 21, 4))
    for cuts in ((100, 200), (1, 6, 293)):
        assert bits(*device_run(D, mr.BVS, 3, 300, s_freq, 21, 4, cuts=cuts)) == want, "cuts %s" % (cuts,)


def test_3_disjoint_problem_groups_with_chain0_advanced():
    import torch
    D = mr.synthetic(4, 129, mr.T3, 4)[0]
    rows, state = device_run(D, mr.BVS, 3, 300, 7, 22, 3)
    r0, s0 = device_run(D.take([0, 1]), mr.BVS, 3, 300, 7, 22, 3)
    r1, s1 = device_run(D.take([2, 3]), mr.BVS, 3, 300, 7, 22, 3 + 6)
    assert bits(torch.cat([r0, r1], dim=1), torch.cat([s0, s1], dim=0)) == bits(rows, state)


def test_3_a_chains_bits_depend_on_its_own_arguments_alone():
    X, YZ = mr.synthetic(1, 70, mr.T3, 1)[0], mr.synthetic(2, 70, mr.T3, 2)[0]
    # the same table of combinations under other problems' statistics: X's problem last, behind two others
    B = mr.Data(X.code, X.n_states, np.concatenate([YZ.n, X.n]), np.concatenate([YZ.E, X.E]), np.concatenate([YZ.B, X.B]))
    rows_a, state_a = device_run(X, mr.BVS, 1, 300, 3, 11, 7)
    rows_b, state_b = device_run(B, mr.BVS, 1, 300, 3, 11, 5)
    assert bits(rows_a[:, 0], state_a[0]) == bits(rows_b[:, 2], state_b[2])
    assert bits(rows_a[:, 0]) != bits(rows_b[:, 1]), "another problem's chain runs on other data"
    # ... and with more chains per problem: chain 7 of problem 0 is chain 7
    rows_c, state_c = device_run(X, mr.BVS, 6, 300, 3, 11, 2)
    assert bits(rows_a[:, 0], state_a[0]) == bits(rows_c[:, 5], state_c[5])


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,n_states,P,cpp", [(1, mr.T1, 1, 1), (65, mr.T3, 3, 2), (1024, mr.T16, 2, 3), (300, mr.T16, 1, 5)])
def test_4_the_buffer_contract_on_exact_size_guarded_buffers(G, n_states, P, cpp):
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    D = mr.synthetic(P, G, n_states, 5)[0]
    st = settings_of(ops, mr.BVS)
    Cn = P * cpp

    def whole():
        data = dev_data(ops, D, cpp)
        state = ops.mte_init(data, 9, st)
        first = ops.mte_steps(data, state, 0, 25, 3, 9, st)                           # rows_cap exactly the 9 rows written
        rows = ops.alloc_output((13, Cn, W), torch.float64, "cuda")
        ops.mte_steps(data, state, 25, 15, 3, 9, st, rows=rows)                       # iterations 27 .. 39: slots 0 .. 4
        ops.mte_steps(data, state, 40, 24, 3, 9, st, rows=rows, slot0=5)              # 42 .. 63: slots 5 .. 12, exactly to the end
        given = ops.mte_init(data, 9, st, given=state.clone())
        return first, rows, state, given

    out = contract(ops, torch, whole, label="mte G %d" % G)
    assert out[0].shape[0] == 9 and out[1][0, 0, 0] == 27 and out[1][-1, Cn - 1, 0] == 63 and out[1][5, 0, 0] == 42
    o = ops.MTE_STATE
    assert torch.equal(out[3][:, o["lik"]:o["prior"] + 1], out[2][:, o["lik"]:o["prior"] + 1]), "given = 1 recomputes the same likelihood and prior"
    assert bool((out[3][:, o["proposed"]:o["I"]] == 0).all())


def test_4_slots_outside_the_launch_are_untouched():
    import torch
    from literate_amd import ops
    D = mr.synthetic(2, 9, mr.T3, 5)[0]
    data, st = dev_data(ops, D, 2), ops.MteSettings()
    state = ops.mte_init(data, 9, st)
    rows = torch.full((12, 4, W), float("nan"), dtype=torch.float64, device="cuda")
    ops.mte_steps(data, state, 0, 10, 3, 9, st, rows=rows, slot0=3)          # iterations 0, 3, 6, 9: slots 3 .. 6
    h = rows.cpu().numpy()
    used = ops.mte_row_columns(D.n_states)["width"]
    assert np.isnan(h[:3]).all() and np.isnan(h[7:]).all() and not np.isnan(h[3:7]).any()
    assert h[3:7, :, 0].T.tolist() == [[0.0, 3.0, 6.0, 9.0]] * 4 and np.all(h[3:7, :, used:] == 0.0)


def test_4_argument_errors_in_the_headers_order_leave_the_buffers_untouched():
    import torch
    from helpers.abi_cases import refuses
    from literate_amd import _hip, ops
    lib = _hip.load()
    E = _hip
    D = mr.synthetic(2, 8, mr.T3, 5)[0]
    S = ops.MteSettings
    for what, call, code in (
            ("bvs 2", lambda: ops.mte_init(dev_data(ops, D, 2), 1, S(bvs=2)), "LR_ERR_MODEL"),
            ("constant -1", lambda: ops.mte_init(dev_data(ops, D, 2), 1, S(constant=-1)), "LR_ERR_MODEL"),
            ("pI 0", lambda: ops.mte_init(dev_data(ops, D, 2), 1, S(pI=0.0)), "LR_ERR_MODEL"),
            ("pI 1", lambda: ops.mte_init(dev_data(ops, D, 2), 1, S(pI=1.0)), "LR_ERR_MODEL"),
            ("pI nan", lambda: ops.mte_init(dev_data(ops, D, 2), 1, S(pI=float("nan"))), "LR_ERR_MODEL"),
            ("bvs_from -1", lambda: ops.mte_init(dev_data(ops, D, 2), 1, S(bvs_from=-1)), "LR_ERR_MODEL")):
        refuses(ops, torch, call, code, label=what, entry="lr_mte_init")
    with pytest.raises(ValueError, match="a code lies outside"):
        ops.MteData(np.array([[0, 0, 5]]), D.n_states, D.n[:, :1], D.E[:, :1], D.B[:, :1])
    # the step arguments, and the order NULL < SIZE < MODEL < the step arguments: straight at the library, on buffers of a known fill
    data = dev_data(ops, D, 2)
    state = ops.mte_init(data, 1)
    before = state.clone()
    rows = torch.full((9, 4, W), 7.0, dtype=torch.float64, device="cuda")
    keep = []

    def steps(s=S(), cap=10, rows_=rows, it0=0, n_it=10, sf=1, slot0=0, null=None, host=None, init=None, **fields):
        prob = ops.mte_problem(data, state, 1, s)
        if null:
            setattr(prob, null, None)
        if host is not None:
            keep.append(np.ascontiguousarray(host, dtype=np.int32))
            prob.n_states_host = keep[-1].ctypes.data_as(_hip.c_vp)
        for k, v in fields.items():
            setattr(prob, k, v)
        if init is not None:
            return _hip.launch_problem(lib.lr_mte_init, data.device, prob, init)
        return _hip.launch_problem(lib.lr_mte_steps, data.device, prob, it0, n_it, sf, _hip.ptr(rows_), cap, slot0)

    bad = S(bvs=3)
    assert steps(cap=9) == E.LR_ERR_SIZE and steps(cap=10, slot0=1) == E.LR_ERR_SIZE and steps(cap=-1) == E.LR_ERR_SIZE
    assert steps(s=bad, cap=9) == E.LR_ERR_MODEL and steps(s=S(pI=2.0), sf=0) == E.LR_ERR_MODEL
    assert steps(sf=0) == steps(it0=-1) == steps(n_it=-1) == steps(slot0=-1) == E.LR_ERR_SIZE
    for fields in (dict(G=0), dict(T=0), dict(P=0), dict(chains_per_problem=0), dict(G=1025), dict(T=17), dict(P=2 ** 30, chains_per_problem=2)):
        assert steps(s=bad, **fields) == E.LR_ERR_SIZE, fields
    for host in ([3, 0, 5], [3, 17, 5], [3, 1, -1]):
        assert steps(s=bad, host=host) == E.LR_ERR_SIZE, host
    assert steps(s=bad, host=[16] * 9, T=9) == E.LR_ERR_SIZE, "144 categories"
    assert steps(init=2) == steps(init=-1) == E.LR_ERR_SIZE and steps(s=bad, init=2) == E.LR_ERR_SIZE and steps(s=bad, init=1) == E.LR_ERR_MODEL
    # ... also without rows: NULL is the answer only where the step arguments are valid and a row is due
    assert steps(rows_=None, sf=0) == steps(rows_=None, it0=-1) == steps(rows_=None, n_it=-1) == E.LR_ERR_SIZE
    assert steps(rows_=None) == E.LR_ERR_NULL
    for field in ("code", "n_states", "n_states_host", "n", "E", "B", "state"):
        assert steps(s=bad, G=0, null=field) == E.LR_ERR_NULL, field
        assert steps(s=bad, G=0, null=field, init=0) == E.LR_ERR_NULL, field
    assert lib.lr_mte_steps(None, 0, 10, 1, _hip.ptr(rows), 10, 0) == E.LR_ERR_NULL and lib.lr_mte_init(None, 0) == E.LR_ERR_NULL
    torch.cuda.synchronize()
    assert torch.equal(before, state) and bool((rows == 7.0).all())
    for what, call in (("s_freq 0", lambda: ops.mte_steps(data, state, 0, 10, 0, 1)), ("it0 < 0", lambda: ops.mte_steps(data, state, -1, 10, 1, 1)),
                       ("n_iters < 0", lambda: ops.mte_steps(data, state, 0, -1, 1, 1))):
        with pytest.raises(ValueError, match="lr_mte_steps: LR_ERR_SIZE"):
            call()
    # where no row is due rows may be NULL; n_iters = 0 launches nothing
    assert steps(rows_=None, it0=1, n_it=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, state)
    assert steps(rows_=None, it0=1, n_it=2, sf=5) == 0 and steps(cap=9, it0=3, n_it=9) == 0
    torch.cuda.synchronize()
    assert not torch.equal(before, state) and rows[:, :, 0].unique().tolist() == [float(i) for i in range(3, 12)]


@pytest.mark.parametrize("st", [mr.BVS, mr.CONSTANT], ids=["bvs", "const"])
def test_4_the_stream_contract_on_a_busy_side_stream(st):
    """lr_mte_init and lr_mte_steps take the stream in their descriptor, so they are not among the functions
    helpers/stream_cases finds by their last parameter: the library handed to TorchRuntime here is a pair of adapters with the
    stream last, which put it into the descriptor and call the entry point.  65 combinations, 2 problems x 2 chains, 60
    iterations in two launches; the table of codes, the numbers of states and the statistics are the inputs copied behind the
    delay."""
    import torch
    from helpers import stream_cases as S
    from literate_amd import _hip, ops
    lib = _hip.load()
    G, P, cpp = 65, 2, 2
    sett = settings_of(ops, st)

    def init(prob, given, stream):
        prob.stream = stream
        return lib.lr_mte_init(C.byref(prob), given)

    def steps(prob, it0, n, s, rows, cap, slot0, stream):
        prob.stream = stream
        return lib.lr_mte_steps(C.byref(prob), it0, n, s, rows, cap, slot0)
    adapters = types.SimpleNamespace(lr_mte_init=init, lr_mte_steps=steps)
    rt = S.TorchRuntime(library=(adapters, ["lr_mte_init", "lr_mte_steps"]))
    host_states = np.asarray(mr.T3, dtype=np.int32)

    def make(seed):
        D = mr.synthetic(P, G, mr.T3, 40 + seed)[0]
        return D.code.astype(np.uint8), host_states, D.n, D.E, D.B

    def call(code, n_states, n, E, B):
        data = ops.MteData(code, n_states, n, E, B, cpp, n_states_host=host_states)
        assert data.code.data_ptr() == code.data_ptr() and data.n.data_ptr() == n.data_ptr() and data.B.data_ptr() == B.data_ptr()   # no copy
        state = ops.alloc_output((P * cpp, _hip.LR_MTE_STATE_W), torch.float64, "cuda")
        rows = ops.alloc_output((20, P * cpp, W), torch.float64, "cuda")
        prob = ops.mte_problem(data, state, 9, sett)
        here = rt.current_stream_arg
        assert adapters.lr_mte_init(prob, 0, here()) == 0
        assert adapters.lr_mte_steps(prob, 0, 25, 3, _hip.ptr(rows), 20, 0, here()) == 0          # rows of iterations 0 .. 24: slots 0 .. 8
        assert adapters.lr_mte_steps(prob, 25, 35, 3, _hip.ptr(rows), 20, 9, here()) == 0         # 27 .. 57: slots 9 .. 19
        return dict(state=state, rows=rows)
    a, b = [S.dev(torch, x) for x in make(0)], [S.dev(torch, x) for x in make(1)]
    bufs = [torch.empty_like(x) for x in a]
    want, table = S.ordered(rt, lambda: call(*bufs), a, b, bufs, "mte %s" % (st,))
    assert table["lr_mte_init"]["calls"] == 1 and table["lr_mte_steps"]["calls"] == 2
    rows = np.frombuffer(want["rows"]).reshape(20, P * cpp, W)
    assert rows[-1, 0, 0] == 57.0 and rows[9, 3, 0] == 27.0


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_5_the_posterior_of_m_under_the_constant_model():
    """mr.constant_posterior: m | data ~ Gamma(E_tot + 1, rate B_tot + 1).  64 chains x 20 000 iterations sampled every 10, the
    first tenth dropped.  The pooled mean lies within 5 standard errors - the spread of the 64 chain means / sqrt(64) - of
    (E_tot + 1) / (B_tot + 1); the pooled variance (the mean of the chains' mean squared deviation from the pooled mean) within 5
    standard errors, taken likewise from the spread of the 64 chains' values, of (E_tot + 1) / (B_tot + 1)^2.  Two problems in
    one launch: each lands on its own value."""
    D = mr.synthetic(2, 65, mr.T3, 9)[0]
    rows, _ = device_run(D, mr.CONSTANT, 64, 20000, 10, 77, 0)
    m = rows[200:, :, 4].cpu().numpy().reshape(-1, 2, 64)
    for p in range(2):
        mean_want, var_want = mr.constant_posterior(D.E[p].sum(), D.B[p].sum())
        x = m[:, p]
        means = x.mean(axis=0)
        pooled = means.mean()
        se = means.std(ddof=1) / 8.0
        v = ((x - pooled) ** 2).mean(axis=0)
        var, se_v = v.mean(), v.std(ddof=1) / 8.0
        print("problem %d: mean %.6g, derived %.6g, se %.3g (%.2f se); variance %.6g, derived %.6g, se %.3g (%.2f se)" %
              (p, pooled, mean_want, se, (pooled - mean_want) / se, var, var_want, se_v, (var - var_want) / se_v))
        assert abs(pooled - mean_want) <= 5 * se
        assert abs(var - var_want) <= 5 * se_v
    assert abs(mr.constant_posterior(D.E[0].sum(), D.B[0].sum())[0] - mr.constant_posterior(D.E[1].sum(), D.B[1].sum())[0]) > 1e-3


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_6_the_trait_that_drives_extinction_is_the_one_selected():
    """mr.relation_lineages: 3000 lineages, trait A's states die at rates 1 : 2 : 4, trait B is assigned at random.  Pooled over 64
    chains x 20 000 iterations (sampled every 10, the first tenth dropped): P(I_A = 1) > P(I_B = 1), and the mean multipliers of
    A order its states as the truth does."""
    from literate_amd import ops
    ts, te, traits = mr.relation_lineages()
    data = ops.MteData.from_lineages(ts, te, traits, [(np.inf, 0.0)], chains_per_problem=64, names=["A", "B"])
    assert data.G == 9 and data.n_states_host.tolist() == [3, 3]
    rows, _ = ops.mte_run(data, 20000, 10, 5, ops.MteSettings())
    x = rows[200:].cpu().numpy().reshape(-1, W)
    cols = ops.mte_row_columns(data.n_states_host)
    P_A, P_B = x[:, cols["I"]].mean(axis=0)
    qA = x[:, cols["q"]][:, :3].mean(axis=0)
    print("P(I_A) %.4f P(I_B) %.4f mean q_A %s" % (P_A, P_B, qA))
    assert P_A > P_B
    assert qA[0] < qA[1] < qA[2]


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def read_log(path):
    with open(path, newline="") as f:
        text = f.read()
    lines = text.split("\r\n")
    assert lines[-1] == "" and "\n" not in text.replace("\r\n", ""), "%s: csv.writer's line ends" % path
    return lines[0].split("\t"), np.array([[float(x) for x in ln.split("\t")] for ln in lines[1:-1]])


def test_7_the_command_line_end_to_end(tmp_path):
    from literate_amd import mte, ops
    src = str(tmp_path / "example.txt")
    shutil.copy(mr.FIXTURE, src)
    args = ["-d", src, "--slices", "23-8,8-0", "--chains", "2", "-n", "2000", "-s", "100", "-seed", "5", "--bvs_from", "200",
            "--summary", "0.2", "--ess", "0.2", "-mu_species", "1", "--block", "700"]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "MTEmodel.py")] + args, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT),
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    ts, te, traits, names = mr.read_example()
    slices = [(23.0, 8.0), (8.0, 0.0)]
    data = ops.MteData.from_lineages(ts, te, traits, slices, chains_per_problem=2, names=names)
    rows, _ = ops.mte_run(data, 2000, 100, 5, ops.MteSettings(1, 0, 200, 0.05))
    rows = rows.cpu().numpy()
    cols = ops.mte_row_columns(data.n_states_host)
    for p, (t0, t1) in enumerate(slices):
        combos = mte.combo_names(data.tables, p)[0]
        for k in range(2):
            path = str(tmp_path / ("example%s-%s_c%d.log" % (t0, t1, k)))
            head, tab = read_log(path)
            assert head == mte.header(names, data.n_states_host, combos) and head[5] == "I_trait1" and head[-1].startswith("m")
            assert tab.shape == (20, cols["width"] + len(combos)) and tab[:, 0].tolist() == [100.0 * i for i in range(20)]
            close(tab[:, :cols["width"]], rows[:, 2 * p + k, :cols["width"]], "the log of slice %d chain %d against ops.mte_run" % (p, k))
            assert (tab[:, cols["width"]:] > 0).all()
    summ = mte.read_summary(str(tmp_path / "example_MTE.tsv"))
    assert len(summ) == 2 * (cols["width"] - 4 + 3)
    for t0, t1 in slices:
        for name in names:
            e = summ[t0, t1, "I_" + name]
            assert 0.0 <= e["P_I"] <= 1.0 and np.isfinite(e["2lnBF"])
        assert summ[t0, t1, "mean_r"]["minHPD"] <= summ[t0, t1, "mean_r"]["mean"] <= summ[t0, t1, "mean_r"]["maxHPD"]
        assert 0.0 <= summ[t0, t1, "accept_m"]["mean"] <= 1.0
        assert os.path.exists(str(tmp_path / ("example_%s-%s_ESS.tsv" % (t0, t1))))
