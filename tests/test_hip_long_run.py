"""Every sampler across iterations 2^31 and 2^32, and the Philox key across 2^32 (the cases, the references and why they are the
references: tests/helpers/long_run.py; the seeds' margins and the power of the cases: tests/test_long_run_host.py).

Each run is started 24 iterations short of a boundary - N = 2^31 - 24 and 2^32 - 24 - and taken 60 iterations on, once in one
launch and once in the launches of 20 + 4 + 1 + 35, which end 4 short of the boundary, exactly on it and one past it: the
counter is stored and loaded on both sides of the LO -> HI carry, as a low word with the sign bit set, and as (0, 1).

   2. the stepping samplers at it0 = N - lr_rjbin_steps (40 bins, models 0 and 2; 512 bins; s_freq 8 at slot0 = 2 between
      sentinel slots), lr_rjmc3_steps (T = 4 and 5, swap rounds every 1, 5 and 3 iterations, with the ladder buffer and the swap
      counts), lr_tmlik_steps, lr_mlik_steps, lr_adej_steps (the shapes of their own "cut into launches" cases): the cut run
      and the single launch bit for bit, every row of every chain against the restatement started at it0 = N at rtol = atol =
      1e-9 (iteration column, K columns, replica indices, proposal and swap counts exact), column 0 counting N .. N + 59;
   3. the chain engines, N written into the state that lr_mcmc_init left and lr_mcmc_restore after it: every kernel family on
      the configurations of tests/helpers/chain_edges.py at 6 chains, rows against the oracle loop on the remapped draws
      (E.check_rj_rows / E.check_param_rows), every chain at iteration N + 60, the final likA re-scored by the oracle and on the
      device, the cut run and the single launch bit for bit; the last test of the section holds the set of cases and the kernels
      they ran;
   4. the key wraps: chain0 / chain_offset = 2^32 - 2 and seed = 2^32 + 5 are the keys taken modulo 2^32.

The tolerance is the project's rtol = atol = 1e-9 (tests/test_hip_replicates.py); no case is skipped.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import chain_edges as CE          # noqa: E402
from helpers import edges as E          # noqa: E402
from helpers import long_run as LR          # noqa: E402

pytestmark = pytest.mark.gpu

OFFSETS, CUTS, N_IT = LR.OFFSETS, LR.CUTS, LR.N_IT
OFFSET_IDS = ["2p31", "2p32"]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def bits(ts):
    return [np.ascontiguousarray(t.cpu().numpy()).tobytes() for t in ts]


def launches(N):
    """(it0, iterations) of the cut run"""
    out, it = [], N
    for n in CUTS:
        out.append((it, n))
        it += n
    assert it == N + N_IT and [a + n for a, n in out[:3]] == [LR.boundary(N) - 4, LR.boundary(N), LR.boundary(N) + 1]
    return out


def counts(col0, N, s=1):
    """the iteration column [rows, ...] of every chain runs N, N + s, ... exactly"""
    col0, want = np.asarray(col0, dtype=np.float64), np.arange(N, N + N_IT, s, dtype=np.float64)
    assert col0.shape[0] == len(want) and (col0.reshape(len(want), -1) == want[:, None]).all(), col0.reshape(col0.shape[0], -1)[:, 0]


# ---- 2: the stepping samplers -----------------------------------------------------------------------------------------------
def check_rjbin_state(state, outs, what):
    """the final state of every chain against the restatement's (tests/test_hip_mc3.py's check_against, one temperature)"""
    from literate_amd.ops import RJBIN_ROWS as RW, RJBIN_SCALARS as X
    from test_hip_mc3 import near
    S = state.reshape(len(outs), -1, 64)
    for c, o in enumerate(outs):
        s = o["state"]
        kl, km = len(s["L"]), len(s["M"])
        sc = S[c, RW["scalars"]]
        assert (sc[X["K_l"]], sc[X["K_m"]], sc[X["accepted"]]) == (kl, km, s["accepted"]), (what, c)
        near(S[c, RW["L"], :kl], s["L"], what), near(S[c, RW["M"], :km], s["M"], what)
        near(S[c, RW["tL"], :kl + 1], s["tL"], what), near(S[c, RW["tM"], :km + 1], s["tM"], what)
        near([sc[X[k]] for k in ("likA", "priorA", "priorPoiA", "Gamma_rate_l", "Gamma_rate_m", "Poi_lambda")],
             [s["likA"], s["priorA"], s["priorPoiA"], s["Gamma_rate"][0], s["Gamma_rate"][1], s["Poi"]], what)


@pytest.mark.parametrize("N", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("case", sorted(LR.RJBIN_CASES))
def test_2_rjbin_across_the_boundary(case, N):
    import torch
    from literate_amd import ops
    from test_hip_replicates import W, close, dev_data, dev_settings, want_rows
    n_bins, model, s = LR.RJBIN_CASES[case]
    seed, chain0 = LR.RJBIN_SEED, LR.RJBIN_CHAIN0
    reps, outs, margin = LR.rjbin_reference(case, N)
    assert margin >= LR.MARGIN, margin
    data, st = dev_data(ops, reps, 2), dev_settings(ops, model=model)
    due = ops.rows_due(N, N_IT, s)
    first = 2 if s > 1 else 0                                    # s_freq 8: slots 0, 1 stay as they are, the cap is exactly reached
    fill = lambda: torch.full((first + due, 4, W), -7.0, dtype=torch.float64, device="cuda")
    one, st1 = fill(), ops.rjbin_init(data, seed, st, chain0)
    ops.rjbin_steps(data, st1, N, N_IT, s, seed, st, chain0, rows=one, slot0=first)
    cut, st2, slot = fill(), ops.rjbin_init(data, seed, st, chain0), first
    for it, n in launches(N):
        ops.rjbin_steps(data, st2, it, n, s, seed, st, chain0, rows=cut, slot0=slot)
        slot += ops.rows_due(it, n, s)
    assert slot == first + due and due == len(range(0, N_IT, s))
    assert bits([one, st1]) == bits([cut, st2])
    host, want = one.cpu().numpy(), want_rows(outs)
    assert (host[:first] == -7.0).all() and not (host[first:, :, :13] == -7.0).any()
    close(host[first:], want, "%s at %d" % (case, N))
    assert np.array_equal(host[first:, :, [0, 6, 7]], want[:, :, [0, 6, 7]])
    counts(host[first:, :, 0], N, s)
    check_rjbin_state(st1.cpu().numpy(), outs, case)
    assert data.warnings() == 0


@pytest.mark.parametrize("N", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("T,every", LR.RJMC3_CASES)
def test_2_rjmc3_across_the_boundary(T, every, N):
    import torch
    from helpers import rjmc3_ref as ref
    from literate_amd import ops
    from test_hip_mc3 import check_against
    from test_hip_replicates import W, dev_data
    seed, chain0 = LR.RJMC3_SEED, LR.RJMC3_CHAIN0
    reps, outs, margin = LR.rjmc3_reference(T, every, N)
    assert margin >= LR.MARGIN, margin
    # the parity lr_rjmc3 starts its rounds on: from (N + until_swap + 1) // swap_every - even only at swap_every 3, 2^32 - 24
    first = LR.first_round(N, every)
    assert first == (N + (every - 1 - N % every) + 1) // every and (first & 1) == (0 if (every, N) == (3, OFFSETS[1]) else 1)
    data, betas = dev_data(ops, reps, 1), ref.ladder_betas(T, 0.5)
    st1, sw1 = ops.rjmc3_init(data, seed, betas, chain0=chain0)
    one_r, one_l = ops.rjmc3_steps(data, st1, sw1, N, N_IT, 1, seed, betas, every, chain0=chain0)
    fill = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    cut_r, cut_l = fill(N_IT, 2, W), fill(N_IT, 2, T, 4)
    st2, sw2 = ops.rjmc3_init(data, seed, betas, chain0=chain0)
    for it, n in launches(N):
        ops.rjmc3_steps(data, st2, sw2, it, n, 1, seed, betas, every, chain0=chain0, rows=cut_r, ladder=cut_l, slot0=it - N)
    assert bits([one_r, one_l, st1, sw1]) == bits([cut_r, cut_l, st2, sw2])
    rows, swaps = one_r.cpu().numpy(), sw1.cpu().numpy()
    check_against(outs, T, rows, one_l.cpu().numpy(), swaps, st1.cpu().numpy(), "T %d, swap_every %d at %d" % (T, every, N))
    counts(rows[:, :, 0], N)
    # the rounds of the run, counted here: pair j is proposed in the rounds of its parity
    rounds = [(it + 1) // every for it in range(N, N + N_IT) if (it + 1) % every == 0]
    assert rounds[0] == first and swaps[:, :, 0].tolist() == [[sum(1 for n in rounds if n % 2 == j % 2) for j in range(T - 1)]] * 2
    assert swaps[:, :, 1].sum() > 0 and data.warnings() == 0


@pytest.mark.parametrize("N", OFFSETS, ids=OFFSET_IDS)
def test_2_tmlik_across_the_boundary(N):
    import torch
    import test_hip_tmlik as t
    from helpers import tmlik_ref as ref
    from literate_amd import ops
    P, grid_args, wins = LR.tmlik_problem()
    want_rows, want_state, margin = LR.tmlik_reference(N)
    assert margin >= LR.MARGIN, margin
    data, grid, seed, s = t.dev_data(P), ops.TmlikGrid(*grid_args), LR.TMLIK["seed"], LR.TMLIK["s"]
    wins_d = torch.as_tensor(wins, device="cuda")
    st1 = ops.tmlik_init(data, grid, wins_d, seed)
    one = ops.tmlik_steps(data, grid, wins_d, st1, N, N_IT, s, seed)
    st2, cut = ops.tmlik_init(data, grid, wins_d, seed), torch.full_like(one, -3.0)
    for it, n in launches(N):
        ops.tmlik_steps(data, grid, wins_d, st2, it, n, s, seed, rows=cut, slot0=it - N)
    assert bits([one, st1]) == bits([cut, st2])
    rows, state = one.cpu().numpy(), st1.cpu().numpy()
    assert rows.shape == want_rows.shape == (grid.M, N_IT, grid.R, grid.T, ref.ROW_W)
    t.close(rows, want_rows, "rows at %d" % N)
    t.close(state, want_state, "state at %d" % N)
    assert np.array_equal(state[..., ref.S_PROPOSED:ref.S_BETA], want_state[..., ref.S_PROPOSED:ref.S_BETA])
    assert want_state[..., ref.S_ACCEPTED:ref.S_ACCEPTED + 2].sum() > 0.2 * N_IT * grid.M * grid.R * grid.T
    counts(rows[..., ref.R_IT].transpose(1, 0, 2, 3), N)


@pytest.mark.parametrize("N", OFFSETS, ids=OFFSET_IDS)
def test_2_mlik_across_the_boundary(N):
    import torch
    import test_hip_mlik as t
    from literate_amd import ops
    M, betas, scales = LR.mlik_problem()
    want_rows, want_state = LR.mlik_reference(N)          # (the restatement reports no margins: as tests/test_hip_mlik.py)
    data, R, seed, s = t.dev_data(M), LR.MLIK["R"], LR.MLIK["seed"], LR.MLIK["s"]
    st1 = ops.mlik_init(data, betas, scales, R, seed)
    one = ops.mlik_steps(data, betas, scales, st1, N, N_IT, s, seed)
    st2 = ops.mlik_init(data, betas, scales, R, seed)
    parts = [ops.mlik_steps(data, betas, scales, st2, it, n, s, seed) for it, n in launches(N)]
    assert [int(p.shape[0]) for p in parts] == list(CUTS) and bits([one, st1]) == bits([torch.cat(parts), st2])
    rows, state = one.cpu().numpy(), st1.cpu().numpy()
    t.close(rows, want_rows, "rows at %d" % N)
    t.close(state, want_state, "state at %d" % N)
    assert np.array_equal(state[:, :, 10:14], want_state[:, :, 10:14])            # proposals made and accepted
    assert want_state[:, :, 12:14].sum() > 0.2 * N_IT * R * len(betas)
    counts(rows[..., 0], N)


@pytest.mark.parametrize("N", OFFSETS, ids=OFFSET_IDS)
def test_2_adej_across_the_boundary(N):
    import torch
    from helpers import adej_cases as cases
    from literate_amd import ops
    c = LR.ADEJ
    runs, margin = LR.adej_reference(N)
    assert margin >= cases.MARGIN_FLOOR == LR.MARGIN, margin
    data, st = cases.dev_data(*cases.table(c["table"])), cases.settings()
    st1 = ops.adej_init(data, 0.0, c["chains"], c["seed"], st)
    one = ops.adej_steps(data, 0.0, st1, N, N_IT, c["s"], c["seed"], st)
    st2 = ops.adej_init(data, 0.0, c["chains"], c["seed"], st)
    parts = [ops.adej_steps(data, 0.0, st2, it, n, c["s"], c["seed"], st) for it, n in launches(N)]
    assert bits([one, st1]) == bits([torch.cat(parts), st2])
    rows = one.cpu().numpy()
    cases.compare_run("adej at %d" % N, rows, st1.cpu().numpy(), runs, c["compared"])
    counts(rows[:, :, 0], N)


# ---- 3: the chain engines ---------------------------------------------------------------------------------------------------
ENGINE_CASES = LR.engine_cases()
RAN = {}                                     # case id at an offset -> the kernel lr_mcmc_describe named


def leavings(eng):
    import torch
    torch.cuda.synchronize()
    return dict(S=eng.state_f64.cpu().numpy().copy(), I=eng.state_i32.cpu().numpy().copy(), rows=eng.trace_rows().copy())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_family(case, eng, cid):
    """the engine runs as the family the case names (the layout and lr_mcmc_describe's kernel name)"""
    lay, name = eng.layout, eng.kernel_name()
    want = {"persistent4": (2, "lr_persist4_kernel<"), "persistent2": (1, "lr_persist_kernel<"), "spec": (3, "lr_spec_kernel<")}.get(case.engine)
    if want:
        assert lay.persistent == want[0] and name.startswith(want[1]), (cid, lay.persistent, name)
    elif case.engine == "packed":
        assert lay.persistent == 0 and lay.packed_scan == 1 and name.startswith("lr_packscan_kernel<"), (cid, name)
    elif case.engine == "stream":
        assert lay.persistent == 0 and lay.streaming == 1 and name.startswith("lr_stream_kernel<"), (cid, name)
    else:
        assert lay.persistent == 0 and lay.packed_scan == 0 and lay.streaming == 0, (cid, name)
        if case.chains == LR.PIPELINED_CHAINS:
            assert lay.pipelined == 1 and name.startswith("lr_fused_iter_kernel<"), (cid, lay.pipelined, name)
    return name


def check_engine_run(case, eng, N, cid, chain_offset=0):
    """what a run of 60 iterations from N leaves, against the reference of tests/helpers/long_run.py"""
    cfg, C, s = CE.CONFIGS[case.config], case.chains, case.s_freq
    tr, snap = eng.trace_rows(), eng.snapshot()
    n_rows = len(range(0, N_IT, s))
    assert tr.shape[:2] == (n_rows, C)
    assert np.array_equal(tr[:, :, 0], np.broadcast_to(np.arange(N, N + N_IT, s, dtype=float)[:, None], (n_rows, C))), tr[:, :, 0]
    assert np.all(snap["it"] == N + N_IT) and snap["it"].dtype == np.int64, snap["it"]
    from literate_amd import _hip as H
    I = eng.state_i32.cpu().numpy()[:, H.IROW_SCALARS]
    assert all(LR.join64(I[c, H.I_IT_LO], I[c, H.I_IT_HI]) == N + N_IT and I[c, H.I_SLOT] == n_rows
               and LR.join64(I[c, H.I_NEXT_LO], I[c, H.I_NEXT_HI]) == N + n_rows * s for c in range(C)), I[:, H.I_IT_LO:H.I_SLOT + 1]
    CE.check_distinct_states(snap)
    if cfg.sampler == 0:
        ts, te = CE.data(case.config)
        refs = {c: LR.engine_rows(case, c, N, chain_offset=chain_offset) for c in LR.followed(case)}
        E.check_rj_rows(tr, refs, n_rows, cid)
        lam, mu = E.check_rj_states(snap, ts, te, cfg.model, cfg.n_bins, CE.rj_stats(case.config), N + N_IT, cid,
                                    CE.lineage_bins(case.config))
        E.rescore_rj_on_device(eng, snap, lam, mu, cfg.model, CE.rj_stats(case.config), cid)
    else:
        ts, te, bins, trend = CE.param_data(case.config)
        for c in LR.followed(case):
            got = eng.log_rows_from(tr[:, c], emp=CE.param_emp(case.config))
            E.check_param_rows(got, LR.engine_rows(case, c, N, chain_offset=chain_offset), n_rows, cid, c)
        assert np.all(np.isfinite(snap["likA"]))
        E.rescore_param_on_device(eng, CE.KIND[cfg.sampler], snap, ts, te, bins, trend, cid)


@pytest.mark.parametrize("N", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("case", ENGINE_CASES, ids=[LR.engine_case_id(c) for c in ENGINE_CASES])
def test_3_engine_across_the_boundary(case, N, monkeypatch):
    cid = "%s at %d" % (LR.engine_case_id(case), N)
    if case.generic:
        monkeypatch.setenv("LR_P4_GENERIC", "1")
    else:
        monkeypatch.delenv("LR_P4_GENERIC", raising=False)
    eng = LR.make_engine(case)
    try:
        name = check_family(case, eng, cid)
        LR.start_engine_at(eng, N)
        if case.engine == "persistent4" and case.config == "A":
            # the specialised word (models 0 / 1) with the lean draw duty, and the generic instantiation of the same kernel
            assert eng.p4_config() == (0 if case.generic else 1), (cid, eng.p4_config())
            assert case.generic or eng.p4_draws() == "lean", (cid, eng.p4_draws())
        for n in CUTS:
            eng.steps(n)
        assert eng.iterations == N_IT
        check_engine_run(case, eng, N, cid)
        cut = leavings(eng)
    finally:
        eng.close()
    eng = LR.make_engine(case)
    try:
        LR.start_engine_at(eng, N)
        eng.steps(N_IT)
        one = leavings(eng)
    finally:
        eng.close()
    assert all(same_bits(cut[k], one[k]) for k in ("rows", "S", "I")), (cid, [k for k in cut if not same_bits(cut[k], one[k])])
    RAN[(LR.engine_case_id(case), N)] = name


def test_3_every_case_ran_and_every_kernel_family_was_among_them():
    """(Runs after the cases of this section: run the whole file.)  Twice N_ENGINE_CASES cases, none skipped, and the kernels
    lr_mcmc_describe named over them include every family's; the pairs without a case are LR.EXCLUDED, by name."""
    assert len(ENGINE_CASES) == LR.N_ENGINE_CASES and len(RAN) == 2 * LR.N_ENGINE_CASES, (len(ENGINE_CASES), len(RAN))
    kernels = {name.split("<")[0] for name in RAN.values()}
    missing = [k for k in LR.KERNELS if k not in kernels]
    assert not missing, (missing, sorted(kernels))
    assert LR.EXCLUDED == (("B", "persistent2"), ("F", "persistent2")) and not {(c.config, c.engine) for c in ENGINE_CASES} & set(LR.EXCLUDED)
    print("%d cases ran the kernels %s" % (len(RAN), sorted(kernels)))


# ---- 4: the key wraps at 2^32 -----------------------------------------------------------------------------------------------
def test_4_rjbin_keys_wrap():
    """chain0 = 2^32 - 2, four chains on one replicate: chains 2 and 3 are chains 0 and 1 of the run at chain0 = 0, all four are
    the restatement's on PhiloxDraws(seed, (chain0 + c) % 2^32); seed 2^32 + 5 is seed 5"""
    from literate_amd import ops
    from test_hip_replicates import close, dev_data, dev_settings, want_rows
    case, seed = "bins40-m2", LR.RJBIN_SEED
    reps, outs, margin = LR.rjbin_reference(case, 0, seed, LR.WRAP_CHAIN0, None, 4)
    assert margin >= LR.MARGIN and len(reps) == 1
    data, st = dev_data(ops, reps, 4), dev_settings(ops, model=2)

    def run(seed_, chain0):
        state = ops.rjbin_init(data, seed_, st, chain0)
        return ops.rjbin_steps(data, state, 0, N_IT, 1, seed_, st, chain0), state
    hi_r, hi_s = run(seed, LR.WRAP_CHAIN0)
    lo_r, lo_s = run(seed, 0)
    assert bits([hi_r[:, 2:], hi_s[2:]]) == bits([lo_r[:, :2], lo_s[:2]])
    assert bits([hi_r[:, :2]]) != bits([lo_r[:, 2:]])
    close(hi_r.cpu().numpy(), want_rows(outs), "chain0 = 2^32 - 2")
    check_rjbin_state(hi_s.cpu().numpy(), outs, "chain0 = 2^32 - 2")
    assert bits(run(2 ** 32 + 5, 3)) == bits(run(5, 3)) != bits(run(6, 3))


def test_4_rjmc3_keys_wrap_inside_a_ladder():
    """T = 4, chain0 = 2^32 - 2: ladder 0 draws from the keys 2^32 - 2, 2^32 - 1, 0, 1 and its swap uniforms from 2^32 - 2, ladder 1
    from 2 .. 5 and 2"""
    from helpers import rjmc3_ref as ref
    from literate_amd import ops
    from test_hip_mc3 import check_against
    from test_hip_replicates import dev_data
    T, every, seed = 4, 5, LR.RJMC3_SEED
    reps, outs, margin = LR.rjmc3_reference(T, every, 0, seed, LR.WRAP_CHAIN0)
    assert margin >= LR.MARGIN
    data, betas = dev_data(ops, reps, 1), ref.ladder_betas(T, 0.5)
    state, swaps = ops.rjmc3_init(data, seed, betas, chain0=LR.WRAP_CHAIN0)
    rows, ladder = ops.rjmc3_steps(data, state, swaps, 0, N_IT, 1, seed, betas, every, chain0=LR.WRAP_CHAIN0)
    check_against(outs, T, rows.cpu().numpy(), ladder.cpu().numpy(), swaps.cpu().numpy(), state.cpu().numpy(), "chain0 = 2^32 - 2")
    # ladder 1 of this run is ladder 0 of the run at chain0 = 2 on the second replicate's data
    d1 = dev_data(ops, reps[1:], 1)
    s1, w1 = ops.rjmc3_init(d1, seed, betas, chain0=2)
    r1, l1 = ops.rjmc3_steps(d1, s1, w1, 0, N_IT, 1, seed, betas, every, chain0=2)
    assert bits([rows[:, 1:], ladder[:, 1:], state[T:], swaps[1:]]) == bits([r1, l1, s1, w1])


@pytest.mark.parametrize("engine", ["launch", "persistent4"])
def test_4_engine_keys_wrap(engine, monkeypatch):
    """chain_offset = 2^32 - 2, 6 chains, from iteration 0: every chain against the oracle on the key (chain_offset + c) % 2^32;
    chains 2 .. 5 are the keys 0 .. 3"""
    monkeypatch.delenv("LR_P4_GENERIC", raising=False)
    case = LR.EngineCase("A", engine, LR.N_CHAINS, 1, False)
    cid = "A-%s-off2p32m2" % engine
    eng = LR.make_engine(case, chain_offset=LR.WRAP_CHAIN0)
    try:
        check_family(case, eng, cid)
        eng.init()
        eng.steps(25)
        eng.steps(N_IT - 25)
        tr, snap = eng.trace_rows(), eng.snapshot()
        refs = {c: LR.rj_engine_rows("A", (LR.WRAP_CHAIN0 + c) % 2 ** 32, 0, 1) for c in range(case.chains)}
        assert refs[2] is LR.rj_engine_rows("A", 0, 0, 1)
        E.check_rj_rows(tr, refs, N_IT, cid)
        CE.check_rj_case(tr, snap, "A", LR.WRAP_CHAIN0, cid)          # (CE.rj_trajectory: PhiloxDraws reduces the key itself)
    finally:
        eng.close()
