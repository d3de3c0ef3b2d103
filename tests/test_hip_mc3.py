"""The Metropolis-coupled RJ sampler (include/literate_hip_rjmc3.h, csrc/lr_rjmc3.hip, literate_amd/mc3.py) on the GPU, against
lr_rjbin_* at one temperature, against the numpy restatement of the ladder (tests/helpers/rjmc3_ref.py: run_mcmc's loop body
per replica, PhiloxDraws(seed, chain0 + g T + w), the swap rounds) and against a closed form.

   1. T = 1 is lr_rjbin, bit for bit;
   2. every replica of every ladder against the restatement: T = 2, 3, 4, 5, 8 x swap_every 1, 7 x models 0 .. 3;
   3. the bin edges 1, 64, 65, 256, 257, 512 at T = 4 and at T = 8 (257, 512 refused there), the cap on the rates at T = 2;
   4. a run cut into launches, and into groups of ladders, is the same run bit for bit;
   5. exact-size guarded buffers, the error codes in the header's order, a busy side stream;
   6. the closed-form posterior of constant rates, at every temperature;
   7. the RJ sampler's cold chains against plain chains;
   8. the command line end to end.

The tolerance against the restatement is rtol = atol = 1e-9, as in test_hip_replicates.py; replica indices and swap counts are
exact.  The seeds were run through the restatement alone: no acceptance or swap decision of any case is closer to its
threshold than 1e-6 (asserted in ladder_case), so the device's last bits decide none.
"""
import ctypes as C
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import rjmc3_ref as ref          # noqa: E402
from test_hip_replicates import (HEAD, KMAX, W, bits, cli, close, dev_data, dev_settings, full_init, make_stats, settings,          # noqa: E402
                                 want_rows, write_tsv)

pytestmark = pytest.mark.gpu

MARGIN = 1e-6


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


@functools.lru_cache(maxsize=None)
def ladder_case(R, n_bins, data_seed, cpr, seed, chain0, T, dt, every, n_it, s_freq, kw=(), init_kind=None):
    """the restatement's run of every ladder, once per case -> (reps, [out per ladder]); no decision within MARGIN of a tie"""
    kw = dict(kw)
    reps = make_stats(R, n_bins, data_seed, dead=kw.get("model", 2) == 3)
    betas = ref.ladder_betas(T, dt)
    outs = []
    for g in range(R * cpr):
        st, start, end = reps[g // cpr]
        inits = [full_init(g * T + w, start, end, n_bins) for w in range(T)] if init_kind == "full" else None
        outs.append(ref.run_ladder(st, start, end, settings(**kw), seed, chain0 + g * T, betas, every, n_it, s_freq, k_max=KMAX, inits=inits))
        assert np.isfinite(np.array(outs[-1]["mcmc"])).all(), "ladder %d: the restatement's own rows hold nan / inf" % g
    worst = min(o["margin"] for o in outs)
    print("smallest margin of a decision: %.3g" % worst)
    assert worst >= MARGIN, "a decision of the restatement is within %g of a tie (%g): choose another seed" % (MARGIN, worst)
    return reps, outs


def device_ladders(reps, cpr, seed, chain0, betas, every, n_it, s_freq, kw=(), init=None):
    from literate_amd import ops
    kw = dict(kw)
    data = dev_data(ops, reps, cpr, dead=kw.get("model", 2) == 3)
    st = dev_settings(ops, **kw)
    state, swaps = ops.rjmc3_init(data, seed, betas, st, chain0, init=init)
    rows, ladder = ops.rjmc3_steps(data, state, swaps, 0, n_it, s_freq, seed, betas, every, st, chain0)
    return rows.cpu().numpy(), ladder.cpu().numpy(), swaps.cpu().numpy(), state.cpu().numpy(), data.warnings()


def near(got, want, what):
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9, err_msg=what)


def check_against(outs, T, rows, ladder, swaps, state, what):
    """cold rows, the ladder buffer (replica indices exact), the swap counts (exact), the final state of every replica"""
    from literate_amd.ops import RJBIN_ROWS as RW, RJBIN_SCALARS as X
    G = len(outs)
    close(rows, want_rows(outs), what + ": cold rows")
    want_l = np.stack([o["ladder"] for o in outs], axis=1)
    assert ladder.shape == want_l.shape == (rows.shape[0], G, T, 4)
    assert np.array_equal(ladder[..., 0], want_l[..., 0]), what + ": the replica at every position"
    assert np.array_equal(ladder[..., 2:], want_l[..., 2:]), what + ": K_l, K_m at every position"
    near(ladder[..., 1], want_l[..., 1], what + ": likA at every position")
    assert np.array_equal(swaps, np.stack([o["swaps"] for o in outs])), (what, swaps.tolist())
    S = state.reshape(G, T, -1, 64)
    for g, o in enumerate(outs):
        for w, s in enumerate(o["states"]):
            kl, km = len(s["L"]), len(s["M"])
            sc = S[g, w, RW["scalars"]]
            assert (sc[X["K_l"]], sc[X["K_m"]], sc[X["accepted"]], sc[9]) == (kl, km, s["accepted"], o["pos"][w]), (what, g, w)
            near(S[g, w, RW["L"], :kl], s["L"], what), near(S[g, w, RW["M"], :km], s["M"], what)
            near(S[g, w, RW["tL"], :kl + 1], s["tL"], what), near(S[g, w, RW["tM"], :km + 1], s["tM"], what)
            assert not S[g, w, RW["L"], kl:].any() and not S[g, w, RW["tM"], km + 1:].any() and not sc[10:].any()
            near([sc[X[k]] for k in ("likA", "priorA", "priorPoiA", "Gamma_rate_l", "Gamma_rate_m", "Poi_lambda")],
                 [s["likA"], s["priorA"], s["priorPoiA"], s["Gamma_rate"][0], s["Gamma_rate"][1], s["Poi"]], what)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def test_1_one_temperature_is_lr_rjbin_bit_for_bit():
    """R = 3 x 2 chains, 40 bins, 300 iterations, s_freq 1, swap rounds on: state and rows of ops.rjbin_* with the seed and chain0"""
    from literate_amd import ops
    reps = make_stats(3, 40, 7)
    data = dev_data(ops, reps, 2)
    seed, chain0 = 11, 5
    want_state = ops.rjbin_init(data, seed, chain0=chain0)
    want0 = want_state.clone()
    want_rows_ = ops.rjbin_steps(data, want_state, 0, 300, 1, seed, chain0=chain0)
    state, swaps = ops.rjmc3_init(data, seed, [1.0], chain0=chain0)
    assert tuple(swaps.shape) == (6, 0, 2) and bits([state]) == bits([want0])
    rows, ladder = ops.rjmc3_steps(data, state, swaps, 0, 300, 1, seed, [1.0], 3, chain0=chain0)
    assert bits([rows, state]) == bits([want_rows_, want_state])
    lad = ladder.cpu().numpy()
    assert lad.shape == (300, 6, 1, 4) and (lad[..., 0] == 0).all()
    assert np.array_equal(lad[:, :, 0, 1:], rows.cpu().numpy()[:, :, [2, 6, 7]]) and data.warnings() == 0


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2, 3])
@pytest.mark.parametrize("every", [1, 7])
@pytest.mark.parametrize("T", [2, 3, 4, 5, 8])
def test_2_every_replica_against_the_restatement(T, every, model):
    """2 replicates x 1 ladder, 40 bins, 200 iterations, s_freq 1, betas 1 / (1 + 0.5 j): swap_every 1 makes every iteration a
    swap iteration - both parities, and at odd T the position that sits a round out"""
    kw = (("model", model),)
    reps, outs = ladder_case(2, 40, 7, 1, 23, 4, T, 0.5, every, 200, 1, kw)
    got = device_ladders(reps, 1, 23, 4, ref.ladder_betas(T, 0.5), every, 200, 1, kw)
    check_against(outs, T, *got[:4], "T %d, swap_every %d, model %d" % (T, every, model))
    assert got[2][:, :, 0].min() >= 200 // every // 2 and got[2][:, :, 1].sum() > 0, "swaps were proposed and some accepted"
    assert (got[1][..., 0] != np.arange(T)).any(), "replicas left their first position"


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 8])
@pytest.mark.parametrize("n_bins", [1, 64, 65, 256, 257, 512])
def test_3_bin_edges_and_block_shapes(n_bins, T):
    import torch
    from literate_amd import _hip, ops
    n_it = 100 if n_bins <= 65 else 40
    betas = ref.ladder_betas(T, 0.5)
    if T > 4 and n_bins > _hip.LR_RJMC3_WIDE_MAX_BINS:
        lib = _hip.load()
        data = dev_data(ops, make_stats(1, n_bins, 30 + n_bins), 2)
        state = torch.full((2 * T, _hip.LR_RJBIN_STATE_W), 7.0, dtype=torch.float64, device="cuda")
        swaps = torch.full((2, T - 1, 2), 7, dtype=torch.int64, device="cuda")
        rows = torch.full((4, 2, W), 7.0, dtype=torch.float64, device="cuda")
        ladder = torch.full((4, 2, T, 4), 7.0, dtype=torch.float64, device="cuda")
        prob = ops.rjmc3_problem(data, state, swaps, 1, betas, 3)
        assert _hip.launch_problem(lib.lr_rjmc3_init, data.device, prob, None, None, None, None, None, None) == _hip.LR_ERR_SIZE
        assert _hip.launch_problem(lib.lr_rjmc3_steps, data.device, prob, 0, 4, 1, _hip.ptr(rows), _hip.ptr(ladder), 4, 0) == _hip.LR_ERR_SIZE
        with pytest.raises(ValueError, match="lr_rjmc3_init: LR_ERR_SIZE"):
            ops.rjmc3_init(data, 1, betas)
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in (state, swaps, rows, ladder)) and data.warnings() == 0
        return
    reps, outs = ladder_case(1, n_bins, 30 + n_bins, 2, 5, 0, T, 0.5, 3, n_it, 1)
    got = device_ladders(reps, 2, 5, 0, betas, 3, n_it, 1)
    check_against(outs, T, *got[:4], "%d bins, T %d" % (n_bins, T))


@pytest.mark.parametrize("seed", [3, 4])
def test_3_the_cap_on_the_number_of_rates(seed):
    """K_l = K_m = LR_KMAX for both replicas of 2 ladders at 128 bins: LR_WARN_KCAP is set exactly when the restatement met the cap"""
    from literate_amd import _hip
    reps, outs = ladder_case(2, 128, 9, 1, seed, 0, 2, 0.5, 5, 150, 1, (), "full")
    inits = [full_init(c, reps[c // 2][1], reps[c // 2][2], 128) for c in range(4)]
    init = (np.array([i[0] for i in inits]), np.array([i[1] for i in inits]), np.array([i[2] for i in inits]),
            np.array([i[3] for i in inits]), np.full(4, KMAX), np.full(4, KMAX))
    got = device_ladders(reps, 1, seed, 0, ref.ladder_betas(2, 0.5), 5, 150, 1, (), init=init)
    check_against(outs, 2, *got[:4], "from K = 32")
    overflows = sum(o["overflows"] for o in outs)
    print("overflows the restatement met: %d, warning word %d" % (overflows, got[4]))
    assert bool(got[4] & _hip.LR_WARN_KCAP) == (overflows > 0)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 5])
def test_4_a_run_cut_into_launches_or_groups_of_ladders_is_the_same_run(T):
    """swap iterations 4, 9, 14, ... (swap_every 5), row iterations 0, 7, 14, ...: launches that start just before, on and just
    behind a swap iteration (3, 4, 5), a row iteration (6, 7, 8) and one that is both (13, 14, 15); an empty launch"""
    import torch
    from literate_amd import ops
    reps = make_stats(2, 40, 7)
    data = dev_data(ops, reps, 2)
    betas, seed, s, every, n_it, chain0 = ref.ladder_betas(T, 0.5), 17, 7, 5, 120, 6
    due = ops.rows_due(0, n_it, s)
    cap, first = due + 4, 2
    fill = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    one_r, one_l = fill(cap, 4, W), fill(cap, 4, T, 4)
    st1, sw1 = ops.rjmc3_init(data, seed, betas, chain0=chain0)
    ops.rjmc3_steps(data, st1, sw1, 0, n_it, s, seed, betas, every, chain0=chain0, rows=one_r, ladder=one_l, slot0=first)
    cut_r, cut_l = fill(cap, 4, W), fill(cap, 4, T, 4)
    st2, sw2 = ops.rjmc3_init(data, seed, betas, chain0=chain0)
    it, slot = 0, first
    for nxt in (3, 4, 5, 5, 6, 7, 8, 13, 14, 15, 20, 21, 22, 50, n_it):
        ops.rjmc3_steps(data, st2, sw2, it, nxt - it, s, seed, betas, every, chain0=chain0, rows=cut_r, ladder=cut_l, slot0=slot)
        slot += ops.rows_due(it, nxt - it, s)
        it = nxt
    assert slot == first + due
    assert bits([one_r, one_l, st1, sw1]) == bits([cut_r, cut_l, st2, sw2])
    host = one_r.cpu().numpy()
    assert (host[:first] == -7.0).all() and (host[first + due:] == -7.0).all() and not (host[first:first + due, :, :HEAD] == -7.0).any()
    assert int(sw1[:, 0, 0].min()) == n_it // every // 2 and int(sw1[:, :, 1].sum()) > 0
    # groups of ladders: replicate 0's two ladders, then replicate 1's at chain0 + 2 T
    parts = []
    for r in range(2):
        d = dev_data(ops, reps[r:r + 1], 2)
        c0 = chain0 + 2 * T * r
        st, sw = ops.rjmc3_init(d, seed, betas, chain0=c0)
        rows, lad = ops.rjmc3_steps(d, st, sw, 0, n_it, s, seed, betas, every, chain0=c0)
        parts.append((rows, lad, st, sw))
    cat = [torch.cat([parts[0][i], parts[1][i]], dim=d) for i, d in ((0, 1), (1, 1), (2, 0), (3, 0))]
    assert bits(cat) == bits([one_r[first:first + due], one_l[first:first + due], st1, sw1])
    # and the run is the restatement's
    _, outs = ladder_case(2, 40, 7, 2, seed, chain0, T, 0.5, every, n_it, s)
    check_against(outs, T, host[first:first + due], one_l.cpu().numpy()[first:first + due], sw1.cpu().numpy(), st1.cpu().numpy(), "cut")


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins,R,cpr,model,T", [(1, 1, 1, 2, 1), (65, 3, 2, 0, 3), (512, 2, 1, 3, 4), (256, 1, 2, 2, 8)])
def test_5_the_buffer_contract_on_exact_size_guarded_buffers(n_bins, R, cpr, model, T):
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    reps = make_stats(R, n_bins, 5, dead=model == 3)
    st = ops.RjbinSettings(model=model)
    G, betas = R * cpr, ref.ladder_betas(T, 0.5)

    def whole():
        data = dev_data(ops, reps, cpr, dead=model == 3)
        state, swaps = ops.rjmc3_init(data, 9, betas, st)
        first, first_l = ops.rjmc3_steps(data, state, swaps, 0, 25, 3, 9, betas, 4, st)          # caps exactly the 9 rows written
        rows = ops.alloc_output((13, G, W), torch.float64, "cuda")
        lad = ops.alloc_output((13, G, T, 4), torch.float64, "cuda")
        ops.rjmc3_steps(data, state, swaps, 25, 15, 3, 9, betas, 4, st, rows=rows, ladder=lad)              # 27 .. 39: slots 0 .. 4
        ops.rjmc3_steps(data, state, swaps, 40, 24, 3, 9, betas, 4, st, rows=rows, ladder=lad, slot0=5)     # 42 .. 63: slots 5 .. 12
        bare, none = ops.rjmc3_steps(data, state, swaps, 64, 6, 3, 9, betas, 4, st, with_ladder=False)      # ladder NULL: 66, 69
        assert none is None
        return first, first_l, rows, lad, bare, state, swaps

    out = contract(ops, torch, whole, label="rjmc3 bins %d T %d" % (n_bins, T))
    assert out[0].shape[0] == 9 and out[2][0, 0, 0] == 27 and out[2][-1, G - 1, 0] == 63 and out[2][5, 0, 0] == 42
    assert out[4].shape[0] == 2 and out[4][1, 0, 0] == 69
    who = out[3][..., 0].cpu().numpy()
    assert (np.sort(who, axis=-1) == np.arange(T)).all()
    if T > 1:
        assert out[6][:, :, 0].cpu().numpy().tolist() == [[9 if j % 2 else 8 for j in range(T - 1)]] * G          # rounds 1 .. 17


def test_5_argument_errors_in_the_headers_order_leave_the_buffers_untouched():
    import torch
    from helpers.abi_cases import refuses
    from literate_amd import _hip, ops
    lib = _hip.load()
    E = _hip
    reps, big, wide = make_stats(2, 8, 5, dead=True), make_stats(2, 513, 5, dead=True), make_stats(2, 257, 5, dead=True)
    D = lambda r=reps, cpr=2, dead=True: dev_data(ops, r, cpr, dead=dead)
    St = ops.RjbinSettings
    b3 = ref.ladder_betas(3, 0.5)
    for what, call, code in (
            ("513 bins", lambda: ops.rjmc3_init(D(big), 1, b3), "LR_ERR_SIZE"),
            ("model 4", lambda: ops.rjmc3_init(D(), 1, b3, St(model=4)), "LR_ERR_MODEL"),
            ("nine temperatures", lambda: ops.rjmc3_init(D(), 1, ref.ladder_betas(9, 0.1)), "LR_ERR_SIZE"),
            ("betas[0] != 1", lambda: ops.rjmc3_init(D(), 1, [0.9, 0.5]), "LR_ERR_MODEL"),
            ("betas rise", lambda: ops.rjmc3_init(D(), 1, [1.0, 0.5, 0.5]), "LR_ERR_MODEL"),
            ("a beta of 0", lambda: ops.rjmc3_init(D(), 1, [1.0, 0.0]), "LR_ERR_MODEL"),
            ("a beta that is no number", lambda: ops.rjmc3_init(D(), 1, [1.0, float("nan")]), "LR_ERR_MODEL"),
            ("257 bins at T = 5", lambda: ops.rjmc3_init(D(wide), 1, ref.ladder_betas(5, 0.5)), "LR_ERR_SIZE")):
        refuses(ops, torch, call, code, label=what, entry="lr_rjmc3_init")
    data, T = D(), 3
    state, swaps = ops.rjmc3_init(data, 1, b3)
    before, before_sw = state.clone(), swaps.clone()
    rows = torch.full((9, 4, W), 7.0, dtype=torch.float64, device="cuda")
    lad = torch.full((9, 4, T, 4), 7.0, dtype=torch.float64, device="cuda")

    def steps(d=data, s=St(), betas=b3, every=2, cap=10, rows_=rows, lad_=lad, it0=0, n_it=10, sf=1, slot0=0, null=None, R=None, Tn=None):
        prob = ops.rjmc3_problem(d, state, swaps, 1, betas, every, s)
        if null:
            setattr(prob, null, None)
        if R is not None:
            prob.R = R
        if Tn is not None:
            prob.T = Tn
        return _hip.launch_problem(lib.lr_rjmc3_steps, d.device, prob, it0, n_it, sf, _hip.ptr(rows_), _hip.ptr(lad_), cap, slot0)

    # lr_rjbin's own first, in their order
    assert steps(cap=9) == steps(sf=0) == steps(it0=-1) == steps(slot0=-1) == E.LR_ERR_SIZE
    assert steps(s=St(model=4), cap=9) == steps(s=St(model=4), Tn=9) == steps(s=St(update_fraction=2.0), betas=[0.5]) == E.LR_ERR_MODEL
    assert steps(rows_=None) == steps(rows_=None, Tn=9) == steps(null="state", Tn=0) == steps(null="sp", s=St(model=4)) == E.LR_ERR_NULL
    assert steps(cap=9, Tn=9) == steps(cap=9, null="betas") == steps(cap=9, betas=[0.9, 0.5, 0.1]) == E.LR_ERR_SIZE
    # then T, then NULL, then MODEL, then the sizes of the ladders
    assert steps(Tn=0) == steps(Tn=9) == steps(Tn=-1) == steps(Tn=9, null="betas") == steps(Tn=0, null="swaps", every=-1) == E.LR_ERR_SIZE
    assert steps(null="betas") == steps(null="swaps") == steps(null="swaps", betas=[0.9, 0.5, 0.1]) == steps(null="betas", every=-1) == E.LR_ERR_NULL
    assert steps(betas=[0.9, 0.5, 0.1]) == steps(betas=[1.0, 0.5, 0.5]) == steps(betas=[1.0, 0.5, 0.6]) == steps(betas=[1.0, 0.5, 0.0]) \
        == steps(betas=[1.0, 0.5, -0.1]) == steps(betas=[1.0, float("nan"), 0.1]) == steps(betas=[1.0, 1.0, 0.5]) == steps(every=-1) == E.LR_ERR_MODEL
    assert steps(R=2 ** 29, Tn=2) == E.LR_ERR_SIZE and steps(R=2 ** 29, betas=[0.9, 0.5, 0.1]) == E.LR_ERR_MODEL          # 2^30 ladders x 2, x 3
    assert steps(d=D(wide), betas=ref.ladder_betas(5, 0.5)) == E.LR_ERR_SIZE and steps(d=D(wide), betas=[1.0, 0.5, 0.7, 0.2, 0.1]) == E.LR_ERR_MODEL
    assert lib.lr_rjmc3_steps(None, 0, 10, 1, _hip.ptr(rows), None, 10, 0) == E.LR_ERR_NULL
    assert lib.lr_rjmc3_init(None, None, None, None, None, None, None) == E.LR_ERR_NULL
    prob = ops.rjmc3_problem(data, state, swaps, 1, b3)
    assert _hip.launch_problem(lib.lr_rjmc3_init, data.device, prob, _hip.ptr(rows), None, None, None, None, None) == E.LR_ERR_NULL
    torch.cuda.synchronize()
    assert torch.equal(before, state) and torch.equal(before_sw, swaps) and bool((rows == 7.0).all()) and bool((lad == 7.0).all())
    assert data.warnings() == 0
    for what, call in (("s_freq 0", lambda: ops.rjmc3_steps(data, state, swaps, 0, 10, 0, 1, b3, 2)),
                       ("n_iters < 0", lambda: ops.rjmc3_steps(data, state, swaps, 0, -1, 1, 1, b3, 2))):
        with pytest.raises(ValueError, match="lr_rjmc3_steps: LR_ERR_SIZE"):
            call()
    # n_iters = 0 launches nothing; rows and ladder may be NULL where no row is due; swaps may be NULL at T = 1
    assert steps(rows_=None, lad_=None, it0=1, n_it=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, state)
    assert steps(rows_=None, lad_=None, it0=1, n_it=2, sf=5) == 0 and steps(cap=9, it0=3, n_it=9, lad_=None) == 0
    torch.cuda.synchronize()
    assert not torch.equal(before, state) and rows[:, :, 0].unique().tolist() == [float(i) for i in range(3, 12)] and bool((lad == 7.0).all())
    assert int(swaps[:, :, 0].sum()) > 0
    one = ops.rjmc3_init(D(), 1, [1.0])[0]
    prob = ops.rjmc3_problem(D(), one, None, 1, [1.0], 2)
    assert prob.swaps is None and _hip.launch_problem(lib.lr_rjmc3_steps, data.device, prob, 0, 4, 1, _hip.ptr(rows), None, 9, 0) == 0
    torch.cuda.synchronize()


def test_5_the_stream_contract_on_a_busy_side_stream():
    """lr_rjmc3_init and lr_rjmc3_steps take the stream in their descriptor: the library handed to TorchRuntime is a pair of
    adapters with the stream last, which put it into the descriptor and call the entry point.  8 bins, 2 replicates x 2 ladders
    of 3 temperatures, 60 iterations in two launches with swap rounds every 4; the statistics and the times are the inputs
    copied behind the delay."""
    import torch
    from helpers import stream_cases as S
    from literate_amd import _hip, ops
    lib = _hip.load()
    nb, R, cpr, T = 8, 2, 2, 3
    betas = ref.ladder_betas(T, 0.5)

    def init(prob, stream):
        prob.stream = stream
        return lib.lr_rjmc3_init(C.byref(prob), None, None, None, None, None, None)

    def steps(prob, it0, n, s, rows, ladder, cap, slot0, stream):
        prob.stream = stream
        return lib.lr_rjmc3_steps(C.byref(prob), it0, n, s, rows, ladder, cap, slot0)
    adapters = types.SimpleNamespace(lr_rjmc3_init=init, lr_rjmc3_steps=steps)
    rt = S.TorchRuntime(library=(adapters, ["lr_rjmc3_init", "lr_rjmc3_steps"]))

    def make(seed):
        reps = make_stats(R, nb, 40 + seed)
        arr = lambda k: np.array([st[k] for st, _, _ in reps])
        return arr("sp"), arr("ex"), arr("br"), np.array([s for _, s, _ in reps]), np.array([e for _, _, e in reps])

    def call(sp, ex, br, start, end):
        data = ops.RjbinData(sp, ex, br, start, end, cpr)
        assert data.sp.data_ptr() == sp.data_ptr() and data.end_time.data_ptr() == end.data_ptr()          # used as they are: no copy
        state = ops.alloc_output((R * cpr * T, _hip.LR_RJBIN_STATE_W), torch.float64, "cuda")
        swaps = ops.alloc_output((R * cpr, T - 1, 2), torch.int64, "cuda")
        rows = ops.alloc_output((20, R * cpr, W), torch.float64, "cuda")
        ladder = ops.alloc_output((20, R * cpr, T, 4), torch.float64, "cuda")
        prob = ops.rjmc3_problem(data, state, swaps, 9, betas, 4)
        here = rt.current_stream_arg
        assert adapters.lr_rjmc3_init(prob, here()) == 0
        assert adapters.lr_rjmc3_steps(prob, 0, 25, 3, _hip.ptr(rows), _hip.ptr(ladder), 20, 0, here()) == 0          # slots 0 .. 8
        assert adapters.lr_rjmc3_steps(prob, 25, 35, 3, _hip.ptr(rows), _hip.ptr(ladder), 20, 9, here()) == 0         # 27 .. 57: slots 9 .. 19
        return dict(state=state, swaps=swaps, rows=rows, ladder=ladder)
    a, b = [S.dev(torch, x) for x in make(0)], [S.dev(torch, x) for x in make(1)]
    bufs = [torch.empty_like(x) for x in a]
    want, table = S.ordered(rt, lambda: call(*bufs), a, b, bufs, "rjmc3")
    assert table["lr_rjmc3_init"]["calls"] == 1 and table["lr_rjmc3_steps"]["calls"] == 2
    rows = np.frombuffer(want["rows"]).reshape(20, R * cpr, W)
    assert rows[-1, 0, 0] == 57.0 and rows[9, 3, 0] == 27.0
    assert np.frombuffer(want["swaps"], dtype=np.int64).reshape(R * cpr, T - 1, 2)[:, :, 0].tolist() == [[7, 8]] * 4          # rounds 1 .. 15


# ---- 6, 7 -------------------------------------------------------------------------------------------------------------------
def between(x):
    """(mean, standard error) over the chains of their own means: x [samples, chains]"""
    m = x.mean(axis=0)
    return float(m.mean()), float(m.std(ddof=1) / np.sqrt(m.size))


def test_6_the_closed_form_posterior_of_constant_rates():
    """const_rates = 1, use_rate_HP = 0, model 2, 40 bins: the one birth rate has the posterior Gamma(2 + sum sp, 1 + sum br) (the
    Gamma(2, 1) prior times lam^sp exp(-lam br)), the death rate likewise on sum ex; at position j, Gamma(2 + beta_j sum sp, 1 +
    beta_j sum br).  64 ladders x T = 4, betas (1, .5, .2, .05), swap_every 10, 20000 iterations, s_freq 10, the first tenth
    dropped: the cold chains' mean rates within 4 between-ladder standard errors of the closed form - and first the plain
    lr_rjbin chains', so that a failure of the data or the seed is not blamed on the swaps."""
    from literate_amd import ops
    (st, start, end), = make_stats(1, 40, 61)
    data = ops.RjbinData(st["sp"], st["ex"], st["br"], [start], [end], 64)
    sett = ops.RjbinSettings(model=2, const_rates=1, use_rate_HP=0)
    n_it, s, seed = 20000, 10, 77
    burn = n_it // s // 10
    truth = ((2 + st["sp"].sum()) / (1 + st["br"].sum()), (2 + st["ex"].sum()) / (1 + st["br"].sum()))
    plain_state = ops.rjbin_init(data, seed, sett)
    plain = ops.rjbin_steps(data, plain_state, 0, n_it, s, seed, sett).cpu().numpy()[burn:]
    for col, name, want in ((4, "birth", truth[0]), (5, "death", truth[1])):
        m, se = between(plain[:, :, col])
        print("plain chains: mean %s rate %.6f, closed form %.6f, %.2f standard errors (%.2g)" % (name, m, want, (m - want) / se, se))
        assert abs(m - want) <= 4 * se, name
    betas = [1.0, 0.5, 0.2, 0.05]
    state, swaps = ops.rjmc3_init(data, seed, betas, sett, chain0=1000)
    rows, ladder = ops.rjmc3_steps(data, state, swaps, 0, n_it, s, seed, betas, 10, sett, chain0=1000)
    rows, ladder, swaps = rows.cpu().numpy()[burn:], ladder.cpu().numpy()[burn:], swaps.cpu().numpy()
    assert (rows[:, :, 6:8] == 1).all() and (rows[:, :, 10:12] == 1).all()
    for col, name, want in ((4, "birth", truth[0]), (5, "death", truth[1])):
        m, se = between(rows[:, :, col])
        print("cold chains: mean %s rate %.6f, closed form %.6f, %.2f standard errors (%.2g)" % (name, m, want, (m - want) / se, se))
        assert abs(m - want) <= 4 * se, name
    # the test has power: the hottest position samples another distribution, and the states do travel
    cold, se_cold = between(ladder[:, :, 0, 1])
    hot, se_hot = between(ladder[:, :, 3, 1])
    print("mean likelihood at position 0: %.3f, at position 3: %.3f (standard error %.3g)" % (cold, hot, se_hot))
    assert cold - hot > 10 * se_hot
    rate = swaps[:, :, 1].sum(axis=0) / swaps[:, :, 0].sum(axis=0)
    print("swap rates per pair:", rate)
    assert ((rate > 0) & (rate < 1)).all() and (swaps[:, :, 0] == [[1000, 1000, 1000]]).all()


def test_7_the_cold_chains_of_the_rj_sampler_against_plain_chains():
    """default settings, 40 bins: 64 lr_rjbin chains against the cold chains of 64 ladders x T = 4 (betas 1 / (1 + 0.3 j), swap_every
    20), 30000 iterations, s_freq 10, the first fifth dropped: the means of K_l, K_m and the likelihood agree within 4
    sqrt(se_a^2 + se_b^2), the standard errors taken between chains"""
    from literate_amd import mc3, ops
    (st, start, end), = make_stats(1, 40, 62)
    data = ops.RjbinData(st["sp"], st["ex"], st["br"], [start], [end], 64)
    n_it, s, seed = 30000, 10, 78
    burn = n_it // s // 5
    plain_state = ops.rjbin_init(data, seed)
    plain = ops.rjbin_steps(data, plain_state, 0, n_it, s, seed).cpu().numpy()[burn:]
    betas = mc3.ladder_betas(4, 0.3)
    state, swaps = ops.rjmc3_init(data, seed, betas, chain0=1000)
    rows, _ = ops.rjmc3_steps(data, state, swaps, 0, n_it, s, seed, betas, 20, chain0=1000, with_ladder=False)
    cold = rows.cpu().numpy()[burn:]
    assert data.warnings() == 0
    for col, name in ((6, "K_l"), (7, "K_m"), (2, "likelihood")):
        (a, sa), (b, sb) = between(plain[:, :, col]), between(cold[:, :, col])
        se = np.sqrt(sa * sa + sb * sb)
        print("%s: plain %.4f (%.2g), cold %.4f (%.2g): %.2f standard errors apart" % (name, a, sa, b, sb, (a - b) / se))
        assert abs(a - b) <= 4 * se, name
    assert plain[:, :, 6:8].max() > 1 and cold[:, :, 6:8].max() > 1, "the RJ moves ran"
    assert int(swaps[:, :, 1].sum()) > 0


# ---- 8 ----------------------------------------------------------------------------------------------------------------------
def small_files(tmp_path, n, last=1990):
    rng = np.random.default_rng(8)
    ts = np.sort(rng.integers(1950, 1985, 200))
    ts[0], files = 1950, []
    for r in range(n):
        te = np.minimum(ts + rng.integers(0, 25, 200), last)
        te[-1] = last
        d = tmp_path / ("rep%d" % r)
        d.mkdir()
        files.append(str(d / ("bands_%d.tsv" % r)))
        write_tsv(files[-1], ts, te)
    return files


def test_8_the_command_line_end_to_end(tmp_path):
    from literate_amd import logs
    files = small_files(tmp_path, 2)
    head = "\t".join(logs.MCMC_HEAD + logs.ADEQUACY_HEAD) + "\n"
    flags = ["--mc3", "4", "--chains", "4", "-n", "2000", "-s", "100", "-seed", "3", "--rtt", "0.2", "--ess", "0.2"]
    res = cli(["-d", files[0]] + flags, str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out_dir = os.path.join(os.path.dirname(files[0]), "literate_mcmc_logs")
    for k in range(4):
        p = logs.log_paths(files[0], 0, "", k)[1]
        assert os.path.basename(p["mcmc"]) == "bands_0_BD_c%d_mcmc.log" % k and os.path.dirname(p["mcmc"]) == out_dir
        with open(p["mcmc"]) as f:
            lines = f.readlines()
        assert lines[0] == head and len(lines) == 21 and [float(l.split("\t")[0]) for l in lines[1:]] == [100.0 * i for i in range(20)]
        for kind in ("sp_rates", "ex_rates"):
            with open(p[kind]) as f:
                assert len(f.readlines()) == 20
    assert os.path.exists(logs.log_paths(files[0], 0, "")[1]["div"])
    stem = os.path.join(out_dir, "bands_0_BD")
    for tail in ("_RTT.tsv", "_RTT_K.tsv", "_ESS.tsv", "_ESS_chains.tsv", "_MC3.tsv"):
        assert os.path.exists(stem + tail), tail
    with open(stem + "_MC3.tsv") as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("# 4 ladders of 4 temperatures, a swap round every 100 iterations")
    pairs = [l.split("\t") for l in lines[2:5]]
    assert [p[0] for p in pairs] == ["0", "1", "2"] and [int(p[3]) for p in pairs] == [4 * 10] * 3          # rounds 1 .. 20, 4 ladders
    assert [float(p[1]) for p in pairs] == [1.0, 1 / 1.1, 1 / 1.2] and all(0 <= int(p[4]) <= 40 for p in pairs)
    assert lines[6] == "ladder\tround_trips" and [l.split("\t")[0] for l in lines[7:]] == ["0", "1", "2", "3"]
    assert "--mc3: 4 temperatures" in res.stdout and "swap rates per pair" in res.stdout
    # on replicates: two files, two cold chains each
    res = cli(["--replicates", ",".join(files), "--mc3", "2", "--mc3_every", "10", "--chains", "4", "-n", "1000", "-s", "100", "--combine", "0.2"],
              str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    for r, path in enumerate(files):
        for k in range(2):
            with open(logs.log_paths(path, 0, "", k)[1]["mcmc"]) as f:
                assert len(f.readlines()) == 11
    stem = os.path.join(out_dir, "replicates2")
    assert os.path.exists(stem + "_MC3.tsv") and os.path.exists(stem + "_COMBINED_mcmc.log") and os.path.exists(stem + "_div_replicates.tsv")


def test_8_every_refused_flag_combination_exits_with_its_sentence(tmp_path):
    from literate_amd import mc3
    files = small_files(tmp_path, 1)
    one = ["-d", files[0], "--mc3", "4", "-n", "200", "-s", "100"]
    sentences = dict((n, why) for n, _, why in mc3.NOT_WITH_MC3)
    for flag in ("ppc", "ppc_age", "ade", "ade_joint", "waic", "loo"):
        res = cli(one + ["--" + flag, "0.2"], str(tmp_path))
        assert res.returncode != 0 and sentences[flag] in res.stderr and "--mc3" in sentences[flag], (flag, res.stderr[-500:])
    for extra, want in ((["--checkpoint", "ck"], "--checkpoint saves one engine's workspace"), (["--init_shifts", "2"], "--init_shifts builds the start"),
                        (["-rm_first_bin", "1"], "-rm_first_bin 1 makes the reference's own sampler fail"),
                        (["--replicates", files[0]], "not on both"), (["--mc3", "9"], "1 to 8 temperatures")):
        res = cli(one + extra, str(tmp_path))
        assert res.returncode != 0 and want in res.stderr and "--mc3" in res.stderr, (extra, res.stderr[-500:])
    env = dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE="2")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "LiteRateForward.py")] + one, cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode != 0 and "--mc3 runs on one GPU (WORLD_SIZE is 2)" in res.stderr
    # the replicate path's own limits: more than 512 unit bins; more than 256 with more than 4 temperatures
    long = str(tmp_path / "long.tsv")
    write_tsv(long, [1000, 1200], [1100, 1513])
    res = cli(["-d", long, "--mc3", "4", "-n", "200", "-s", "100"], str(tmp_path))
    assert res.returncode != 0 and "513 time bins; the replicate sampler holds at most 512" in res.stderr
    write_tsv(long, [1000, 1200], [1100, 1257])
    res = cli(["-d", long, "--mc3", "5", "-n", "200", "-s", "100"], str(tmp_path))
    assert res.returncode != 0 and "257 time bins: a ladder of more than 4 temperatures holds at most 256" in res.stderr
