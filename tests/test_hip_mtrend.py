"""The joint covariate sampler (include/literate_hip_mtrend.h, csrc/lr_mtrend.hip, literate_amd/multitrend.py) on the GPU:

  1  ops.mtrend_loglik against the per-bin likelihood (trend_rate.py:82, tests/helpers/mtrend_ref.py) at 1e-9: every
     instantiation and its edges, P = 1, 2 and 16, I all 0 / all 1 / mixed, one side constant, no_death
  2  the sampler against the numpy restatement: rows and final state at 1e-9, the counters and the indicators exactly
  3  a run cut into launches - in iterations, or into groups of chains, also with a window changed at the cut - is the same
     run bit for bit; a chain's bits depend on its own arguments alone
  4  the buffer and stream contract, every error code in the header's order
  5  with both sides constant the posterior of l0 is Gamma(N_spec + 1, rate sum DT + 0.1)
  6  the covariate that drives the births is selected, its correlated proxy and every other one is not
  7  the command line end to end

The bound on trajectory rows is the project's standing one: 1e-9 relative (absolute where the value is 0); it decides nothing
about an accept decision because the restatement's smallest margin is held above 1e-6 in every case (the tie condition,
asserted here and - without a GPU - in tests/test_mtrend_host.py).
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

from helpers import mtrend_ref as mr          # noqa: E402

pytestmark = pytest.mark.gpu
W = mr.ROW_W


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def dev_data(ops, D, C):
    return ops.MtrendData(D.n[0], D.n[1], D.DT, D.X, C)


def settings_of(ops, st, win=None):
    t = st.astuple()
    return ops.MtrendSettings(*(t[:-1] + (tuple(win if win is not None else t[-1]),)))


def device_run(D, st, C, n_it, s_freq, seed, chain0, cuts=None, win_at=None):
    """the whole run in one launch, or cut into launches of `cuts` iterations -> (rows, state) on the device.  win_at = (it,
    win): the launches from iteration `it` on (a cut must fall there) take the windows `win`"""
    import torch
    from literate_amd import ops
    data = dev_data(ops, D, C)
    state = ops.mtrend_init(data, seed, settings_of(ops, st), chain0)
    n = (n_it + s_freq - 1) // s_freq
    rows = torch.full((n, C, W), float("nan"), dtype=torch.float64, device="cuda")
    it = 0
    for k in (cuts if cuts is not None else (n_it,)):
        S = settings_of(ops, st, win_at[1] if win_at is not None and it >= win_at[0] else None)
        assert win_at is None or not (it < win_at[0] < it + k), "a cut falls where the windows change"
        ops.mtrend_steps(data, state, it, k, s_freq, seed, S, chain0, rows=rows, slot0=(it + s_freq - 1) // s_freq)
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
@pytest.mark.parametrize("n_bins", mr.BIN_EDGES)
@pytest.mark.parametrize("P", mr.P_EDGES)
def test_1_loglik_against_the_per_bin_form(n_bins, P):
    """six chains: I all 0, all 1, then mixed; under the free model, each side constant, and no_death"""
    from literate_amd import ops
    D = mr.synthetic(n_bins, P, 500 + n_bins)
    Cn = 6
    l0, m0, a, I_l, b, I_m = mr.random_params(D, Cn, 13, "mixed")
    I_l[0], I_m[0], I_l[1], I_m[1] = 0, 0, 1, 1
    data = dev_data(ops, D, Cn)
    zero = np.zeros(P)
    for label, kw in (("free", {}), ("constB", dict(m_birth=1)), ("constD", dict(m_death=1)), ("nodeath", dict(no_death=1))):
        st = mr.Settings(pI=0.2, slab_sd=1.5, **kw)
        lik, lik_b, lik_d, prior = [t.cpu().numpy() for t in ops.mtrend_loglik(data, l0, m0, a, I_l, b, I_m, settings_of(ops, st))]
        for c in range(Cn):
            ab, Ib = (zero, zero) if kw.get("m_birth") else (a[c], I_l[c])
            ad, Id = (zero, zero) if (kw.get("m_death") or kw.get("no_death")) else (b[c], I_m[c])
            want_b = mr.loglik_bins(D, 0, l0[c], ab, Ib)
            want_d = 0.0 if kw.get("no_death") else mr.loglik_bins(D, 1, m0[c], ad, Id)
            what = "%d bins P %d %s chain %d" % (n_bins, P, label, c)
            close(lik_b[c], want_b, what + ": birth")
            close(lik_d[c], want_d, what + ": death")
            close(lik[c], want_b + want_d, what + ": the sum")
            close(prior[c], mr.log_prior(D, st, l0[c], m0[c], ab, Ib, ad, Id), what + ": the prior")
        if kw.get("no_death"):
            assert (lik_d == 0.0).all()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_2_the_sampler_against_the_restatement(case):
    name, key, mode, n_it, s_freq, seed, chain0 = case
    D, st, want_rows, want_state, margin = mr.run_case(case)
    print("%s: smallest margin %.3g" % (name, margin))
    assert margin > mr.TIE, "%s: an accept decision within %g of a tie" % (name, mr.TIE)
    rows, state = device_run(D, st, mr.N_CHAINS, n_it, s_freq, seed, chain0)
    rows, state = rows.cpu().numpy(), state.cpu().numpy()
    cnt = slice(mr.S_PROPOSED, mr.S_IL)
    assert np.array_equal(state[:, cnt], want_state[:, cnt]), "%s: the counters" % name
    P = D.P
    for lo in (mr.S_IL, mr.S_IM):
        assert np.array_equal(state[:, lo:lo + 16], want_state[:, lo:lo + 16]), "%s: the indicators of the state" % name
    for lo in (8, 8 + 2 * P):
        assert np.array_equal(rows[:, :, lo:lo + P], want_rows[:, :, lo:lo + P]), "%s: the indicators of the rows" % name
    close(rows, want_rows, name + " rows")
    close(state, want_state, name + " state")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_freq", [1, 7])
@pytest.mark.parametrize("n_bins,P", [(65, 2), (300, 16)], ids=["b65", "b300"])
def test_3_a_run_cut_into_launches_is_the_same_run(n_bins, P, s_freq):
    D, st = mr.synthetic(n_bins, P, 3), mr.settings("bvs")
    want = bits(*device_run(D, st, 3, 400, s_freq, 21, 4))
    for cuts in ((100, 300), (1, 6, 393), (5, 0, 395)):          # cuts at iterations 100; 1 and 7; 5 (twice): with s_freq 7 all but one fall between two rows
        assert bits(*device_run(D, st, 3, 400, s_freq, 21, 4, cuts=cuts)) == want, "cuts %s" % (cuts,)


def test_3_disjoint_chain_groups_with_chain0_advanced():
    import torch
    D, st = mr.synthetic(129, 3, 4), mr.settings("bvs")
    rows, state = device_run(D, st, 11, 400, 7, 22, 3)
    parts = [device_run(D, st, n, 400, 7, 22, 3 + c0) for c0, n in ((0, 2), (2, 5), (7, 4))]
    assert bits(torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=0)) == bits(rows, state)


def test_3_a_chains_bits_depend_on_its_own_arguments_alone():
    D, st = mr.synthetic(70, 3, 1), mr.settings("bvs")
    rows_a, state_a = device_run(D, st, 1, 400, 3, 11, 7)
    for Cn, c0 in ((6, 2), (9, 0)):          # chain 7 among five neighbours, and as the last of nine
        rows_b, state_b = device_run(D, st, Cn, 400, 3, 11, c0)
        assert bits(rows_a[:, 0], state_a[0]) == bits(rows_b[:, 7 - c0], state_b[7 - c0]), (Cn, c0)
        assert bits(rows_a[:, 0]) != bits(rows_b[:, 0]), "another chain draws from another stream"


def test_3_a_window_changed_at_the_cut():
    """the windows of a launch are its own: (0.1, 0.07) until iteration 150, (0.03, 0.2) from there - one cut, or several, give
    the same bits, and the run is the restatement's with the windows changed at that iteration"""
    D, st = mr.synthetic(65, 2, 6), mr.settings("nobvs")
    win_at = (150, (0.03, 0.2))
    rows, state = device_run(D, st, 3, 400, 7, 31, 1, cuts=(150, 250), win_at=win_at)
    assert bits(*device_run(D, st, 3, 400, 7, 31, 1, cuts=(50, 100, 3, 247), win_at=win_at)) == bits(rows, state)
    assert bits(*device_run(D, st, 3, 400, 7, 31, 1)) != bits(rows, state), "the windows matter"
    want_rows, want_state, margin = mr.run(D, st, 3, 400, 7, 31, 1, win_at=win_at)
    assert margin > mr.TIE
    cnt = slice(mr.S_PROPOSED, mr.S_IL)
    assert np.array_equal(state.cpu().numpy()[:, cnt], want_state[:, cnt])
    close(rows.cpu().numpy(), want_rows, "rows with the windows changed")
    close(state.cpu().numpy(), want_state, "state with the windows changed")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins,P,Cn", [(1, 1, 1), (65, 2, 6), (512, 16, 3), (300, 16, 5)])
def test_4_the_buffer_contract_on_exact_size_guarded_buffers(n_bins, P, Cn):
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    D = mr.synthetic(n_bins, P, 5)
    st = settings_of(ops, mr.settings("bvs"))

    def whole():
        data = dev_data(ops, D, Cn)
        state = ops.mtrend_init(data, 9, st)
        first = ops.mtrend_steps(data, state, 0, 25, 3, 9, st)                           # rows_cap exactly the 9 rows written
        rows = ops.alloc_output((13, Cn, W), torch.float64, "cuda")
        ops.mtrend_steps(data, state, 25, 15, 3, 9, st, rows=rows)                       # iterations 27 .. 39: slots 0 .. 4
        ops.mtrend_steps(data, state, 40, 24, 3, 9, st, rows=rows, slot0=5)              # 42 .. 63: slots 5 .. 12, exactly to the end
        given = ops.mtrend_init(data, 9, st, given=state.clone())
        return first, rows, state, given

    out = contract(ops, torch, whole, label="mtrend %d bins" % n_bins)
    assert out[0].shape[0] == 9 and out[1][0, 0, 0] == 27 and out[1][-1, Cn - 1, 0] == 63 and out[1][5, 0, 0] == 42
    o = ops.MTREND_STATE
    assert torch.equal(out[3][:, :o["proposed"]], out[2][:, :o["proposed"]]), "given = 1 recomputes the same E, likelihoods and prior"
    assert torch.equal(out[3][:, o["I_l"]:], out[2][:, o["I_l"]:]) and bool((out[3][:, o["proposed"]:o["I_l"]] == 0).all())


def test_4_slots_outside_the_launch_are_untouched():
    import torch
    from literate_amd import ops
    D = mr.synthetic(9, 3, 5)
    data, st = dev_data(ops, D, 4), ops.MtrendSettings()
    state = ops.mtrend_init(data, 9, st)
    rows = torch.full((12, 4, W), float("nan"), dtype=torch.float64, device="cuda")
    ops.mtrend_steps(data, state, 0, 10, 3, 9, st, rows=rows, slot0=3)          # iterations 0, 3, 6, 9: slots 3 .. 6
    h = rows.cpu().numpy()
    used = ops.mtrend_row_columns(3)["width"]
    assert np.isnan(h[:3]).all() and np.isnan(h[7:]).all() and not np.isnan(h[3:7]).any()
    assert h[3:7, :, 0].T.tolist() == [[0.0, 3.0, 6.0, 9.0]] * 4 and np.all(h[3:7, :, used:] == 0.0)


def test_4_argument_errors_in_the_headers_order_leave_the_buffers_untouched():
    import torch
    from helpers.abi_cases import refuses
    from literate_amd import _hip, ops
    lib = _hip.load()
    E = _hip
    D = mr.synthetic(8, 3, 5)
    S = ops.MtrendSettings
    nan, inf = float("nan"), float("inf")
    for what, st in (("m_birth 2", S(m_birth=2)), ("m_death -1", S(m_death=-1)), ("no_death 2", S(no_death=2)), ("bvs 2", S(bvs=2)),
                     ("pI 0", S(pI=0.0)), ("pI 1", S(pI=1.0)), ("pI nan", S(pI=nan)), ("slab_sd 0", S(slab_sd=0.0)), ("slab_sd inf", S(slab_sd=inf)),
                     ("slab_sd nan", S(slab_sd=nan)), ("win -1", S(win=(-1.0, 0.1))), ("win nan", S(win=(0.1, nan))), ("win inf", S(win=(inf, 0.1))),
                     ("bvs_from -1", S(bvs_from=-1))):
        refuses(ops, torch, lambda st=st: ops.mtrend_init(dev_data(ops, D, 4), 1, st), "LR_ERR_MODEL", label=what, entry="lr_mtrend_init")
    # the step arguments, and the order NULL < SIZE < MODEL < the step arguments: straight at the library, on buffers of a known fill
    data = dev_data(ops, D, 4)
    state = ops.mtrend_init(data, 1)
    before = state.clone()
    rows = torch.full((9, 4, W), 7.0, dtype=torch.float64, device="cuda")

    def steps(s=S(), cap=10, rows_=rows, it0=0, n_it=10, sf=1, slot0=0, null=None, init=None, **fields):
        prob = ops.mtrend_problem(data, state, 1, s)
        if null:
            setattr(prob, null, None)
        for k, v in fields.items():
            setattr(prob, k, v)
        if init is not None:
            return _hip.launch_problem(lib.lr_mtrend_init, data.device, prob, init)
        return _hip.launch_problem(lib.lr_mtrend_steps, data.device, prob, it0, n_it, sf, _hip.ptr(rows_), cap, slot0)

    bad = S(bvs=3)
    assert steps(cap=9) == E.LR_ERR_SIZE and steps(cap=10, slot0=1) == E.LR_ERR_SIZE and steps(cap=-1) == E.LR_ERR_SIZE
    assert steps(s=bad, cap=9) == E.LR_ERR_MODEL and steps(s=S(pI=2.0), sf=0) == E.LR_ERR_MODEL
    assert steps(sf=0) == steps(it0=-1) == steps(n_it=-1) == steps(slot0=-1) == E.LR_ERR_SIZE
    for fields in (dict(n_bins=0), dict(n_bins=513), dict(P=0), dict(P=17), dict(C=0), dict(C=-3)):
        assert steps(s=bad, **fields) == E.LR_ERR_SIZE, fields
    assert steps(init=2) == steps(init=-1) == E.LR_ERR_SIZE and steps(s=bad, init=2) == E.LR_ERR_SIZE and steps(s=bad, init=1) == E.LR_ERR_MODEL
    # ... also without rows: NULL is the answer only where the step arguments are valid and a row is due
    assert steps(rows_=None, sf=0) == steps(rows_=None, it0=-1) == steps(rows_=None, n_it=-1) == E.LR_ERR_SIZE
    assert steps(rows_=None) == E.LR_ERR_NULL
    for field in ("n_spec", "n_exti", "DT", "X", "sx_spec", "sx_exti", "state"):
        assert steps(s=bad, n_bins=0, null=field) == E.LR_ERR_NULL, field
        assert steps(s=bad, n_bins=0, null=field, init=0) == E.LR_ERR_NULL, field
    assert lib.lr_mtrend_steps(None, 0, 10, 1, _hip.ptr(rows), 10, 0) == E.LR_ERR_NULL and lib.lr_mtrend_init(None, 0) == E.LR_ERR_NULL
    torch.cuda.synchronize()
    assert torch.equal(before, state) and bool((rows == 7.0).all())
    for what, call in (("s_freq 0", lambda: ops.mtrend_steps(data, state, 0, 10, 0, 1)), ("it0 < 0", lambda: ops.mtrend_steps(data, state, -1, 10, 1, 1)),
                       ("n_iters < 0", lambda: ops.mtrend_steps(data, state, 0, -1, 1, 1))):
        with pytest.raises(ValueError, match="lr_mtrend_steps: LR_ERR_SIZE"):
            call()
    # where no row is due rows may be NULL; n_iters = 0 launches nothing
    assert steps(rows_=None, it0=1, n_it=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, state)
    assert steps(rows_=None, it0=1, n_it=2, sf=5) == 0 and steps(cap=9, it0=3, n_it=9) == 0
    torch.cuda.synchronize()
    assert not torch.equal(before, state) and rows[:, :, 0].unique().tolist() == [float(i) for i in range(3, 12)]


@pytest.mark.parametrize("mode", ["bvs", "constBD"])
def test_4_the_stream_contract_on_a_busy_side_stream(mode):
    """lr_mtrend_init and lr_mtrend_steps take the stream in their descriptor, so they are not among the functions
    helpers/stream_cases finds by their last parameter: the library handed to TorchRuntime here is a pair of adapters with the
    stream last, which put it into the descriptor and call the entry point.  65 bins, 3 covariates, 5 chains, 60 iterations in
    two launches; the statistics and the covariates are the inputs copied behind the delay (SX rides on the host)."""
    import torch
    from helpers import stream_cases as S
    from literate_amd import _hip, ops
    lib = _hip.load()
    nb, P, Cn = 65, 3, 5
    sett = settings_of(ops, mr.settings(mode))

    def init(prob, given, stream):
        prob.stream = stream
        return lib.lr_mtrend_init(C.byref(prob), given)

    def steps(prob, it0, n, s, rows, cap, slot0, stream):
        prob.stream = stream
        return lib.lr_mtrend_steps(C.byref(prob), it0, n, s, rows, cap, slot0)
    adapters = types.SimpleNamespace(lr_mtrend_init=init, lr_mtrend_steps=steps)
    rt = S.TorchRuntime(library=(adapters, ["lr_mtrend_init", "lr_mtrend_steps"]))
    D0 = mr.synthetic(nb, P, 40)
    sx = (D0.SX[0], D0.SX[1])

    def make(seed):
        D = mr.synthetic(nb, P, 40 + seed)
        return D.n[0], D.n[1], D.DT, D.X

    def call(n_spec, n_exti, DT, X):
        data = ops.MtrendData(n_spec, n_exti, DT, X, Cn, sx=sx)
        assert data.n_spec.data_ptr() == n_spec.data_ptr() and data.X.data_ptr() == X.data_ptr() and data.DT.data_ptr() == DT.data_ptr()   # no copy
        state = ops.alloc_output((Cn, _hip.LR_MTREND_STATE_W), torch.float64, "cuda")
        rows = ops.alloc_output((20, Cn, W), torch.float64, "cuda")
        prob = ops.mtrend_problem(data, state, 9, sett)
        here = rt.current_stream_arg
        assert adapters.lr_mtrend_init(prob, 0, here()) == 0
        assert adapters.lr_mtrend_steps(prob, 0, 25, 3, _hip.ptr(rows), 20, 0, here()) == 0          # rows of iterations 0 .. 24: slots 0 .. 8
        assert adapters.lr_mtrend_steps(prob, 25, 35, 3, _hip.ptr(rows), 20, 9, here()) == 0         # 27 .. 57: slots 9 .. 19
        return dict(state=state, rows=rows)
    a, b = [S.dev(torch, x) for x in make(0)], [S.dev(torch, x) for x in make(1)]
    bufs = [torch.empty_like(x) for x in a]
    want, table = S.ordered(rt, lambda: call(*bufs), a, b, bufs, "mtrend %s" % mode)
    assert table["lr_mtrend_init"]["calls"] == 1 and table["lr_mtrend_steps"]["calls"] == 2
    rows = np.frombuffer(want["rows"]).reshape(20, Cn, W)
    assert rows[-1, 0, 0] == 57.0 and rows[9, 3, 0] == 27.0


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_5_the_posterior_of_l0_under_the_constant_model():
    """mr.constant_posterior: l0 | data ~ Gamma(N_spec + 1, rate sum DT + 0.1); 65 bins with about 270 births, so the mean is near
    0.15, its sd near 0.009 and the truncation at 0.001 sixteen sd away.  64 chains x 20 000 iterations sampled every 10, the
    first tenth dropped.  The pooled mean lies within 5 Monte-Carlo standard errors - the pooled sd over the square root of the
    pooled ESS that ops.ess_summary measures - of (N_spec + 1) / (sum DT + 0.1)."""
    from literate_amd import ops
    D, st = mr.synthetic(65, 2, 9), mr.settings("constBD")
    rows, state = device_run(D, st, 64, 20000, 10, 77, 0)
    assert bool((state[:, mr.S_PROPOSED + 1:mr.S_PROPOSED + 6] == 0).all()) and bool((state[:, mr.S_IL:] == 0).all())
    ess = ops.ess_summary(rows, 2000, [6], burnin=0.1)
    x = rows[200:, :, 6].cpu().numpy()
    mean_want, var_want = mr.constant_posterior(D.N[0], D.DT.sum())
    n_eff = float(ess.pooled_ess[0])
    se = x.std() / np.sqrt(n_eff)
    print("N_spec %d, sum DT %.1f: mean %.6g, derived %.6g, ESS %.0f of %d, se %.3g (%.2f se); variance %.4g, derived %.4g" %
          (D.N[0], D.DT.sum(), x.mean(), mean_want, n_eff, x.size, se, (x.mean() - mean_want) / se, x.var(), var_want))
    assert (mean_want - 0.001) / np.sqrt(var_want) > 10, "the truncation is negligible"
    assert 100 < n_eff <= x.size
    assert float(ess.pooled_mean[0]) == pytest.approx(x.mean(), rel=1e-12)
    assert abs(x.mean() - mean_want) <= 5 * se


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_6_the_driver_is_selected_and_its_proxy_is_not():
    """mr.selection_data (data seed 4): 40 bins, births Poisson(0.2 exp(0.6 x_2) DT_b), six columns, x_3 correlated with x_2 at 0.80.
    64 chains x 20 000 iterations (pI 0.1, slab_sd 1, windows 0.05, flips from iteration 0), sampled every 10, the first quarter
    dropped, pooled.  P(I = 1) of (birth, x_2) is above 0.9, every other (side, column) below 0.3, and the 95 % HPD of a_2
    given inclusion holds 0.6.

    The numpy restatement on the CPU, chains 0 .. 3 of this run (seed 11): P(I = 1) birth [0.002 0.003 1.000 0.002 0.003 0.001],
    death [0.006 0.005 0.001 0.006 0.043 0.007]; the HPD of a_2 given inclusion (0.523, 0.639); every chain includes x_2 within
    its first 100 iterations.  (Data seeds 1, 2, 3, 5 and 6 give the same picture: (birth, x_2) at 1.000, the largest other
    frequency 0.116.)"""
    from literate_amd import ops
    D = mr.selection_data()
    assert D.n_bins == 40 and D.P == 6 and 0.75 < np.corrcoef(D.X[2], D.X[3])[0, 1] < 0.85
    st = mr.Settings(**mr.SELECTION_SETTINGS)
    rows, _ = ops.mtrend_run(dev_data(ops, D, 64), 20000, 10, 11, settings_of(ops, st))
    x = rows[500:].cpu().numpy().reshape(-1, W)
    P_I, (lo, hi) = mr.selection_outcome(x)
    print("P(I = 1) birth %s death %s; a_2 given inclusion in (%.4f, %.4f)" % (np.round(P_I[0], 4), np.round(P_I[1], 4), lo, hi))
    assert P_I[0, 2] > 0.9
    others = np.delete(P_I.reshape(-1), 2)
    assert others.max() < 0.3, others
    assert lo < 0.6 < hi


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def read_log(path):
    with open(path, newline="") as f:
        text = f.read()
    lines = text.split("\r\n")
    assert lines[-1] == "" and "\n" not in text.replace("\r\n", ""), "%s: csv.writer's line ends" % path
    return lines[0].split("\t"), np.array([[float(x) for x in ln.split("\t")] for ln in lines[1:-1]])


def make_files(tmp_path, n=300):
    rng = np.random.default_rng(8)
    ts = np.sort(rng.integers(1950, 1985, n))
    ts[0] = 1950
    te = np.minimum(ts + rng.integers(0, 25, n), 1990)
    te[-1] = 1990
    data = str(tmp_path / "bands.tsv")
    with open(data, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, b) in enumerate(zip(ts, te)):
            f.write("%d\t%d\t%d\n" % (i, a, b))
    trend = str(tmp_path / "trend.tsv")
    cov = rng.uniform(1.0, 9.0, (41, 3))          # one row per window of create_bins: the last is dropped
    with open(trend, "w") as f:
        f.write("year\tmarket\ttech\tprice\n")
        for i, v in enumerate(cov):
            f.write("%d\t%r\t%r\t%r\n" % (1950 + i, float(v[0]), float(v[1]), float(v[2])))
    return data, trend, cov


def cli(args, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, "MultiTrendRate.py")] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT),
                          capture_output=True, text=True, timeout=600)


def test_7_the_command_line_end_to_end(tmp_path):
    from literate_amd import multitrend as mt
    data, trend, cov = make_files(tmp_path)
    res = cli(["-d", data, "-trend_data", trend, "--columns", "1,3", "--with_diversity", "--chains", "2", "-n", "2000", "-s", "100", "-seed", "5",
               "--tune", "0", "--bvs_from", "200", "-pI", "0.5", "--summary", "0.2", "--ess", "0.2", "--block", "700"], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    names, nb = ["market", "price", "diversity"], 40
    head0 = mt.header(names, nb)
    logs = []
    for k in range(2):
        head, tab = read_log(str(tmp_path / ("bands_5_EXPB_EXPD_joint_c%d.multitrend.log" % k)))
        assert head == head0 and head[8] == "I_l_market" and head[-1] == "m_39"
        assert tab.shape == (20, 8 + 12 + 2 * nb) and tab[:, 0].tolist() == [100.0 * i for i in range(20)]
        logs.append(tab)
    # the first chain's log is the restatement's rows: without tuning the windows stay at 0.1, and the indicators, all 1 at the
    # start, flip from iteration 200 on
    from literate_amd.literate_library import create_bins, parse_ts_te
    TS, TE, PRESENT, ORIGIN = parse_ts_te(data, False, -1, -1, .5)
    _, _, n_spec, n_exti, Dt, n_bins, _ = create_bins(ORIGIN, PRESENT, np.asarray(TS, dtype=float), np.asarray(TE, dtype=float), 0)
    assert n_bins == nb
    X, got_names = mt.design_matrix(np.concatenate([np.arange(41.0)[:, None], cov], axis=1), ["year", "market", "tech", "price"], "1,3", 0, nb, Dt)
    assert got_names == names
    D = mr.Data(n_spec, n_exti, Dt, X)
    st = mr.Settings(bvs=1, bvs_from=200, pI=0.5, slab_sd=1.0, win=(0.1, 0.1))
    want, _, margin = mr.run(D, st, 1, 2000, 100, 5, 0, full_start=True)          # the command starts from the full model
    assert margin > mr.TIE
    close(logs[0][:, :20], want[:, 0, :20], "the log of chain 0 against the restatement")
    l, m = mt.bin_rates(want[:, 0], X)
    close(logs[0][:, 20:20 + nb], l, "l_b of the log")
    close(logs[0][:, 20 + nb:], m, "m_b of the log")
    assert np.array_equal(logs[0][:, 8:11], want[:, 0, 8:11]) and logs[0][:, 8:11].max() == 1.0
    stem = str(tmp_path / "bands_joint_MT")
    head, lines = mt.read_tsv(stem + ".tsv")
    assert head == mt.MT_HEAD and [(ln["side"], ln["covariate"]) for ln in lines] == [(s, n) for s in ("birth", "death") for n in names]
    for ln in lines:
        assert 0.0 <= float(ln["P_I"]) <= 1.0 and np.isfinite(float(ln["2lnBF"])) and float(ln["window"]) == 0.1
        assert 0.0 <= float(ln["accept_flip"]) <= 1.0          # (ESS and R-hat are NaN where a chain never included the covariate)
    Ia = np.concatenate([t[4:, 8:11] * t[4:, 11:14] for t in logs]).mean(axis=0)          # the model-averaged effect: I x coef
    assert [float(ln["avg_mean"]) for ln in lines[:3]] == pytest.approx(Ia.tolist(), rel=1e-9, abs=1e-15)
    P_birth = np.concatenate([t[4:, 8:11] for t in logs]).mean(axis=0)          # 20 rows a chain, the first 4 dropped
    assert [float(ln["P_I"]) for ln in lines[:3]] == pytest.approx(P_birth.tolist(), rel=1e-12)
    head, lines = mt.read_tsv(stem + "_models.tsv")
    assert head == mt.MODELS_HEAD and 1 <= len(lines) <= 20 and sum(float(ln["frequency"]) for ln in lines) <= 1.0 + 1e-12
    assert len(lines[0]["birth"]) == 3 and sum(int(ln["n"]) for ln in lines) <= 32
    head, lines = mt.read_tsv(stem + "_rates.tsv")
    assert head == mt.RATES_HEAD and len(lines) == nb
    l_all = np.concatenate([t[4:, 20:20 + nb] for t in logs])
    assert [float(ln["l_mean"]) for ln in lines] == pytest.approx(l_all.mean(axis=0).tolist(), rel=1e-9)
    assert all(float(ln["l_minHPD"]) <= float(ln["l_mean"]) <= float(ln["l_maxHPD"]) for ln in lines)
    assert float(lines[3]["l_empirical"]) == pytest.approx(n_spec[3] / Dt[3]) and os.path.exists(stem + "_ESS.tsv")


def test_7_tuning_moves_the_windows_and_a_refused_flag_exits_with_its_reason(tmp_path):
    from literate_amd import multitrend as mt
    data, trend, _ = make_files(tmp_path)
    res = cli(["-d", data, "-trend_data", trend, "--columns", "all", "--chains", "2", "-n", "100", "-s", "10", "--mlik", "0.3"], str(tmp_path))
    assert res.returncode != 0 and mt.REFUSED["mlik"] in res.stderr and not os.path.exists(str(tmp_path / "bands_joint_MT.tsv"))
    res = cli(["-d", data, "-trend_data", trend, "--columns", "1,7", "--chains", "2", "-n", "100", "-s", "10", "-seed", "5"], str(tmp_path))
    assert res.returncode != 0 and "column 7 lies outside the trend file" in res.stderr
    res = cli(["-d", data, "-trend_data", trend, "--columns", "1,2", "-bvs", "0", "--chains", "8", "-n", "4000", "-s", "100", "-seed", "5",
               "--tune", "0.5", "--summary", "0.5", "-no_death", "1"], str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert os.path.exists(str(tmp_path / "bands_5_EXPB_ND_joint_c7.multitrend.log"))
    head, lines = mt.read_tsv(str(tmp_path / "bands_joint_MT.tsv"))
    assert [ln["side"] for ln in lines] == ["birth", "birth"] and all(float(ln["P_I"]) == 1.0 for ln in lines)
    # 300 births over two coefficients: a step of sd 0.1 is accepted well above 30 % of the time, so the window has grown
    assert float(lines[0]["window"]) > 0.1 and 0.1 < float(lines[0]["accept_coef_included"]) < 0.9
