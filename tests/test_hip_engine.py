"""GPU parity of the fused RJMCMC engine (lr_mcmc_*): device chains against the oracle's
restatement of runMCMC (pinned to the reference's own trajectories in test_oracle_golden.py)
fed the SAME Philox draws, step by step."""
import os

import numpy as np
import pytest

from helpers.edges import accepted_rates as _accepted_rates

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden_dir):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: no ROCm device visible")
    return np.load(os.path.join(golden_dir, "binning_lik.npz"))


def _oracle_run(G, name, model, seed, chain, n_it, **kw):
    from oracle import mcmc_oracle as mo
    stats = dict(sp=G[name + "/sp"], ex=G[name + "/ex"], br=G[name + "/br"],
                 ex_dead=G[name + "/ex_dead"], br_dead=G[name + "/br_dead"])
    start, end = G[name + "/start_end"]
    st = mo.Settings(model_BDI=model, **kw)
    with np.errstate(all="ignore"):
        return mo.run_mcmc(stats, start, end, st, mo.PhiloxDraws(seed, chain), n_it, 1, k_max=32)


@pytest.mark.parametrize("model,kw", [(0, {}), (2, {}), (1, {}), (3, {}),
                                       (0, dict(const_rates=1)), (0, dict(const_death_rate=1)),
                                       (2, dict(use_rate_HP=0, Poisson_HP=2.5)),
                                       (0, dict(unit_resolution=False)), (1, dict(unit_resolution=False)),
                                       (0, dict(engine="launch")), (2, dict(engine="launch")),
                                       (1, dict(engine="persistent")), (0, dict(engine="persistent4")),
                                       (2, dict(engine="persistent4")), (1, dict(engine="persistent2")),
                                       (0, dict(engine="spec")), (2, dict(engine="spec", team=2)),
                                       (0, dict(engine="spec", team=4)), (1, dict(engine="spec", team=8)),
                                       (0, dict(engine="spec", team=1, cpt=1)), (2, dict(engine="spec", team=2, cpt=1)),
                                       (1, dict(engine="spec", team=4, cpt=1)), (0, dict(engine="spec", team=1, cpt=2)),
                                       (3, dict(engine="spec", team=8, cpt=1)), (0, dict(engine="spec", cpt=1, unit_resolution=False)),
                                       (3, dict(engine="launch")), (3, dict(engine="spec", team=2)),
                                       (3, dict(engine="persistent4")), (3, dict(engine="persistent2")),
                                       (3, dict(engine="spec", unit_resolution=False)),
                                       # (a chain on its own CU with the pair planes by the helper waves - the kernel mode of
                                       # long scans - forced on this short one)
                                       (0, dict(engine="spec", team=1, cpt=1, planes_by_scanners=0)),
                                       # (the four-chain kernel's form without helper waves: fourteen scanner waves)
                                       (0, dict(engine="persistent4", p4_help=0)), (3, dict(engine="persistent4", p4_help=0)),
                                       # (the resident streaming kernel - the planner's choice for few chains x very many
                                       # lineages - forced on this short input: lr_stream.hip)
                                       (1, dict(engine="stream", unit_resolution=False)), (2, dict(engine="stream", use_rate_HP=0, Poisson_HP=2.5)),
                                       # (a chain on its own CU with the pair planes by the helper waves, on general times)
                                       (1, dict(engine="spec", team=1, cpt=1, planes_by_scanners=0, unit_resolution=False)),
                                       # (the launch-based engine scanning the PACKED lineages - the planner's choice for very
                                       # many lineages at unit resolution - forced on this short input: lr_packscan.hip)
                                       (0, dict(engine="packed")), (2, dict(engine="packed", const_rates=1)), (1, dict(engine="packed")),
                                       (3, dict(engine="packed")), (3, dict(engine="packed", unit_resolution=False)),
                                       (0, dict(engine="stream")), (2, dict(engine="stream", const_rates=1))])
def test_engine_follows_oracle_trajectory(G, model, kw, monkeypatch):
    from literate_amd.engine import ChainEngine, split_trace_row
    name, seed, n_it, C, off = "example_TBP", 2024, 1500, 6, 40
    kw = dict(kw)
    if "planes_by_scanners" in kw:
        monkeypatch.setenv("LR_SPEC_PLANES_BY_SCANNERS", str(kw.pop("planes_by_scanners")))
    if "p4_help" in kw:
        monkeypatch.setenv("LR_P4_HELP", str(kw.pop("p4_help")))
    ekw = dict(const_rates=kw.get("const_rates", 0), const_death_rate=kw.get("const_death_rate", 0),
               use_rate_HP=kw.get("use_rate_HP", 1), poisson_HP=kw.get("Poisson_HP", 0.0),
               unit_resolution=kw.pop("unit_resolution", None), engine=kw.pop("engine", "auto"), team=kw.pop("team", 0),
               chains_per_team=kw.pop("cpt", 0))
    eng = ChainEngine(G[name + "/ts"], G[name + "/te"], C, model=model, seed=seed, s_freq=1,
                      n_trace_slots=n_it, chain_offset=off, **ekw)
    if ekw["engine"] == "spec":
        assert eng.layout.persistent == 3 and eng.layout.team_blocks == (ekw["team"] or eng.layout.team_blocks)
        assert eng.layout.spec_chains_per_team == (ekw["chains_per_team"] or eng.layout.spec_chains_per_team)
        if "LR_SPEC_PLANES_BY_SCANNERS" in os.environ:
            assert eng.kernel_name().endswith(", 3>")
    if ekw["engine"] == "persistent2":
        assert eng.layout.persistent == 1
    if ekw["engine"] == "stream":
        assert eng.layout.persistent == 0 and eng.layout.streaming == 1 and eng.kernel_name().startswith("lr_stream_kernel<")
    if ekw["engine"] == "packed":
        assert eng.layout.persistent == 0 and eng.layout.packed_scan == 1 and eng.kernel_name().startswith("lr_packscan_kernel<4,")
        assert eng.kernel_name().endswith("true>" if ekw["unit_resolution"] is False else "false>")
    if ekw["engine"] == "persistent4" and ekw["unit_resolution"] is not False:
        # <H, general, parametric, helper waves>
        assert eng.kernel_name().endswith("false, false, false>" if "LR_P4_HELP" in os.environ else "false, false, true>")
    # binning done by the engine's own kernel must equal the reference's
    assert np.array_equal(eng.sp_events.cpu().numpy(), G[name + "/sp"])
    assert np.array_equal(eng.br_length.cpu().numpy(), G[name + "/br"])
    eng.init()
    eng.steps(n_it)
    tr = eng.trace_rows()
    assert tr.shape[0] == n_it
    n_moves = 0
    for c in range(C):
        ref = _oracle_run(G, name, model, seed, off + c, n_it, **kw)
        for i in range(n_it):
            head, sp, ex = split_trace_row(tr[i, c])
            r = ref["mcmc"][i]
            assert head[0] == r[0] and head[6] == r[6] and head[7] == r[7], (c, i, head[:8], r[:8])
            assert np.allclose(head[1:13], r[1:13], rtol=1e-9, atol=1e-9), (c, i, head, r)
            assert np.allclose(sp, ref["sp"][i], rtol=1e-10) and np.allclose(ex, ref["ex"][i], rtol=1e-10)
        n_moves += len(set(np.round(np.array(ref["mcmc"])[:, 2], 6)))
    assert n_moves > C * 50          # the chains actually moved
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it)
    eng.close()


@pytest.mark.parametrize("unit", [True, False])
def test_pipelined_partitioned_engine_follows_oracle(G, unit):
    _pipelined_case(G, unit, "launch")


def test_persistent_engine_follows_oracle(G):
    _pipelined_case(G, True, "auto")


def _pipelined_case(G, unit, engine):
    """64 chains: two stream partitions, each software-pipelined in two halves (fused scan|step launches,
    hipGraph replays).  Chains from every half of every partition are compared with the oracle loop, and the
    engine layout is checked to really be the pipelined one.  unit=True: unit-resolution tables (8-byte
    entries, 16 chains per block), False: the general-times kernels on the same data."""
    from literate_amd.engine import ChainEngine, split_trace_row
    name, seed, n_it, C = "metal_bands", 404, 400, 64
    eng = ChainEngine(G[name + "/ts"], G[name + "/te"], C, model=2, seed=seed, s_freq=1, n_trace_slots=n_it,
                      unit_resolution=unit, engine=engine)
    assert eng.unit_resolution == unit and eng.layout.chains_per_block == (16 if unit else 8)
    assert eng.layout.n_parts == 2 and eng.layout.pipelined == 1
    assert (eng.layout.persistent > 0) == (engine != "launch")
    eng.init()
    eng.steps(150); eng.steps(1); eng.steps(249)        # graph replays + prologue/epilogue launches, three calls
    tr = eng.trace_rows()
    for c in (0, 15, 16, 31, 32, 47, 48, 63):
        ref = _oracle_run(G, name, 2, seed, c, n_it)
        for i in range(n_it):
            head, sp, ex = split_trace_row(tr[i, c])
            r = ref["mcmc"][i]
            assert head[0] == r[0] and head[6] == r[6] and head[7] == r[7], (c, i, head[:8], r[:8])
            assert np.allclose(head[1:13], r[1:13], rtol=1e-9, atol=1e-9), (c, i, head, r)
            assert np.allclose(sp, ref["sp"][i], rtol=1e-10) and np.allclose(ex, ref["ex"][i], rtol=1e-10)
    assert np.all(eng.snapshot()["it"] == n_it)
    eng.close()


@pytest.mark.parametrize("engine,kw", [("launch", {}), ("launch", dict(C=12)), ("auto", {}), ("spec", dict(team=1)), ("spec", dict(team=4)),
                                       ("persistent4", {})])
def test_engine_continuous_times_general_path(G, engine, kw):
    """Lineage times that are NOT unit-resolution (uniform jitter added): the engine must pick the general-times
    kernels by itself and still follow the oracle loop run on statistics binned from the same jittered data.
    "launch" = the launch-based engine (fp64 in-bin fractions from ts / te); the persistent engines (speculative team
    kernel, four-chain kernel) carry the fractions as 32-bit fixed point in the pair-general table layout.  The jitter
    sits on the 2^-32 grid, so that packing is exact and every engine must reproduce the oracle's decisions."""
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    from oracle import mcmc_oracle as mo
    rng = np.random.default_rng(4)
    grid = lambda x: np.round(x * 2.0 ** 32) / 2.0 ** 32
    ts = G["metal_bands/ts"][:6000] + grid(rng.uniform(0, 0.999, 6000))
    te = np.maximum(G["metal_bands/te"][:6000] + grid(rng.uniform(0, 0.4, 6000)), ts + 0.0078125)
    te[G["metal_bands/te"][:6000] >= 2000.5] = 2000.5
    kw = dict(kw)
    n_it, seed, C = 300, 21, kw.pop("C", 40)
    eng = ChainEngine(ts, te, C, model=2, seed=seed, s_freq=1, n_trace_slots=n_it, engine=engine, **kw)
    assert not eng.unit_resolution
    if engine == "launch" and C == 12:
        # 9 to 16 chains: one pass of the sixteen-chain scan per iteration instead of two pipelined halves of eight
        assert eng.layout.persistent == 0 and eng.layout.chains_per_block == 16 and eng.layout.pipelined == 0
        assert eng.layout.table_mode == 0 and eng.kernel_name().startswith("lr_scan_wide_kernel<")
    elif engine == "launch":
        assert eng.layout.persistent == 0 and eng.layout.chains_per_block == 8 and eng.layout.pipelined == 1
        assert eng.layout.table_mode == 0
    else:
        assert eng.layout.persistent == (2 if engine == "persistent4" else 3) and eng.layout.table_mode == 2
        if "team" in kw:
            assert eng.layout.team_blocks == kw["team"]
    with pytest.raises(ValueError):
        ChainEngine(ts, te, C, model=2, unit_resolution=True)
    eng.init(); eng.steps(n_it)
    tr = eng.trace_rows()
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    assert np.array_equal(eng.sp_events.cpu().numpy(), sp) and np.allclose(eng.br_length.cpu().numpy(), br, rtol=1e-12)
    for c in sorted({0, C // 2 - 1, C // 2, C - 1}):
        with np.errstate(all="ignore"):
            ref = mo.run_mcmc(dict(sp=sp, ex=ex, br=br), ts.min(), te.max(), mo.Settings(model_BDI=2),
                              mo.PhiloxDraws(seed, c), n_it, 1, k_max=32)
        for i in range(n_it):
            head, s_row, e_row = split_trace_row(tr[i, c])
            assert np.allclose(head[:13], ref["mcmc"][i][:13], rtol=1e-9, atol=1e-9), (c, i, head, ref["mcmc"][i])
    eng.close()


def test_general_times_fraction_packing_stays_within_tolerance():
    """Arbitrary fp64 times (not on the 2^-32 grid): the persistent engines round the in-bin fractions to 32-bit fixed
    point.  Their log-likelihoods must agree with the launch-based engine (exact fp64 fractions) to the 1e-9 relative
    tolerance of the north star on every sampled state of a short run - decisions included."""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    rng = np.random.default_rng(5)
    ts, te, _ = synth.make_lineages(20000, 128, 20, 0)
    ts = ts + rng.uniform(0, 1, len(ts)) * 0.999
    te = np.maximum(np.ceil(te) - 1.0 + rng.uniform(1e-3, 0.999, len(te)), ts + 1e-3)
    ref = None
    for engine, team in (("launch", 0), ("spec", 1), ("spec", 4), ("persistent4", 0)):
        eng = ChainEngine(ts, te, 8, model=0, seed=3, s_freq=1, n_trace_slots=100, engine=engine, team=team)
        eng.init(); eng.steps(100)
        tr = eng.trace_rows()[:, :, :13]
        eng.close()
        if ref is None:
            ref = tr
        assert np.allclose(tr, ref, rtol=1e-9, atol=1e-9), engine


def test_engine_given_initial_state_and_graph_replay(G):
    """runMCMC called with a multi-rate initial state (SURVEY 'config-1 note'); > 32 iterations so the
    captured hipGraph path runs, compared with single-launch stepping bit for bit."""
    from literate_amd.engine import ChainEngine
    name = "example_TBP"
    C = 3
    L = [np.array([.6, .2, .3])] * C
    M = [np.array([.15, .19])] * C
    tL = [np.array([0, 4.55, 12.2, 24.5])] * C
    tM = [np.array([0, 16.682, 24.5])] * C
    outs = []
    for chunks in ([100], [1] * 100, [33, 67]):
        eng = ChainEngine(G[name + "/ts"], G[name + "/te"], C, model=2, seed=5, s_freq=10, n_trace_slots=10)
        eng.init(L, M, tL, tM)
        for n in chunks:
            eng.steps(n)
        outs.append((eng.trace_rows().copy(), eng.state_f64.cpu().numpy().copy()))
        eng.close()
    for tr, st in outs[1:]:
        assert np.array_equal(tr, outs[0][0], equal_nan=True)
        assert np.array_equal(st, outs[0][1], equal_nan=True)
    # oracle with the same init
    from oracle import mcmc_oracle as mo
    stats = dict(sp=G[name + "/sp"], ex=G[name + "/ex"], br=G[name + "/br"])
    start, end = G[name + "/start_end"]
    with np.errstate(all="ignore"):
        ref = mo.run_mcmc(stats, start, end, mo.Settings(model_BDI=2), mo.PhiloxDraws(5, 1), 100, 10,
                          init=(L[0], M[0], tL[0], tM[0]), k_max=32)
    got = outs[0][0][:, 1, :13]
    assert np.allclose(got, np.array(ref["mcmc"])[:, :13], rtol=1e-9)


def test_engine_chain_streams_do_not_depend_on_sharding(G):
    """Chain g gives the same trajectory whether it is local chain g of one engine or local chain 0
    of an engine with chain_offset=g (how ranks shard chains)."""
    from literate_amd.engine import ChainEngine
    name = "example_TBP"
    a = ChainEngine(G[name + "/ts"], G[name + "/te"], 8, model=0, seed=9, s_freq=5, n_trace_slots=40)
    a.init(); a.steps(200)
    b = ChainEngine(G[name + "/ts"], G[name + "/te"], 3, model=0, seed=9, s_freq=5, n_trace_slots=40, chain_offset=4)
    b.init(); b.steps(200)
    ta, tb = a.trace_rows(), b.trace_rows()
    assert np.allclose(ta[:, 4:7], tb, rtol=1e-12, equal_nan=True)
    a.close(); b.close()


@pytest.mark.parametrize("name,model,C,n_it,s,k_tol", [("example_TBP", 0, 256, 400_000, 400, 0.25),
                                                       ("metal_bands", 2, 128, 600_000, 600, 0.8)])
def test_engine_posterior_matches_reference_chains(G, golden_dir, name, model, C, n_it, s, k_tol):
    """Posterior rate marginals within Monte-Carlo error of long runs of the reference CLI
    (tests/golden/make_chains.py: 32 chains x 2M iterations for example_TBP, 16 for metal_bands, so that the reference side
    no longer dominates the standard error): per-bin marginal means at |z| < 4 and 8 % relative, mean K.  (With 16
    example_TBP chains the reference's own grand mean of the recent death rates sat 0.5 % = 2.7 of its standard errors
    below that of the next 16 - scratch/posterior_check.py; the device agrees with all 32 at |z| < 2.)
    metal_bands / 128 chains / RJ prior is BASELINE.json configs[1]."""
    path = os.path.join(golden_dir, "posterior_%s_m%d.npz" % (name, model))
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    R = np.load(path)
    n_ref = int(R["meta"][3])
    assert n_ref >= 16
    eng = ChainEngine(G[name + "/ts"], G[name + "/te"], C, model=model, seed=77, s_freq=s, n_trace_slots=n_it // s)
    eng.init(); eng.steps(n_it)
    tr = eng.trace_rows()
    eng.close()
    start, end = G[name + "/start_end"]
    burn = tr.shape[0] // 5
    per_chain_sp, per_chain_ex, kl = [], [], []
    for c in range(C):
        rows = [split_trace_row(tr[i, c]) for i in range(tr.shape[0])]
        per_chain_sp.append(lo.marginal_rates_from_rows([r[1] for r in rows], end, start)[0])
        per_chain_ex.append(lo.marginal_rates_from_rows([r[2] for r in rows], end, start)[0])
        kl.append(np.mean([r[0][6] for r in rows[burn:]]))
    sp = np.array(per_chain_sp); ex = np.array(per_chain_ex)
    ref_sp = np.array([R["c%d/sp_mean" % c] for c in range(n_ref)])
    ref_ex = np.array([R["c%d/ex_mean" % c] for c in range(n_ref)])
    # z-score of the difference of grand means, using between-chain spread on both sides
    for mine, ref in ((sp, ref_sp), (ex, ref_ex)):
        se = np.sqrt(mine.var(0, ddof=1) / len(mine) + ref.var(0, ddof=1) / len(ref))
        z = (mine.mean(0) - ref.mean(0)) / se
        assert np.max(np.abs(z)) < 4.0, z
        assert np.allclose(mine.mean(0), ref.mean(0), rtol=0.08), np.max(np.abs(mine.mean(0) / ref.mean(0) - 1.0))
    ref_kl = [np.dot(R["c%d/K_l_hist" % c], np.arange(40)) / R["c%d/K_l_hist" % c].sum() for c in range(n_ref)]
    assert abs(np.mean(kl) - np.mean(ref_kl)) < k_tol
    if name == "metal_bands":
        # the posterior the reference SHIPS for this dataset (100 chains, each on its own imputation replicate of the
        # death times - so only a loose check): per-year mean birth rate, death rate on its two plateaus, inside the
        # shipped 95 % HPD nearly everywhere, and the same most frequent number of birth-rate shifts
        S = np.load(os.path.join(golden_dir, "shipped_metal_bands_100chains.npz"))
        mine_b, mine_d = sp.mean(0)[::-1], ex.mean(0)[::-1]            # marginal rates come most recent first
        assert np.allclose(mine_b, S["birth_rate"], rtol=0.12)
        assert np.allclose(mine_d[:10], S["death_rate"][:10], rtol=0.15) and np.allclose(mine_d[-10:], S["death_rate"][-10:], rtol=0.2)
        inside = (mine_b >= S["birth_minHPD"]) & (mine_b <= S["birth_maxHPD"])
        assert inside.mean() > 0.9
        k_hist = np.bincount(np.concatenate([[int(split_trace_row(tr[i, c])[0][6]) - 1 for i in range(burn, tr.shape[0])] for c in range(0, C, 8)]))
        assert abs(int(np.argmax(k_hist)) - int(S["unique"][np.argmax(S["counts"])])) <= 1


def test_cfg3_synthetic_10k_lineages_256_chains(G):
    """BASELINE.json configs[2]: synthetic 10k lineages, 20 true shifts, 256 chains, RJ prior.  A few chains are
    followed against the oracle loop (binned statistics from the oracle's own binning of the same data)."""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    from oracle import mcmc_oracle as mo
    ts, te, _ = synth.make_lineages(10_000, n_bins=128, n_shifts=20, seed=3)
    n_it, seed = 300, 12
    eng = ChainEngine(ts, te, 256, model=0, seed=seed, s_freq=1, n_trace_slots=n_it)
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    assert np.array_equal(eng.sp_events.cpu().numpy(), sp) and np.array_equal(eng.br_length.cpu().numpy(), br)
    eng.init(); eng.steps(n_it)
    tr = eng.trace_rows()
    stats = dict(sp=sp, ex=ex, br=br)
    for c in (0, 100, 255):
        with np.errstate(all="ignore"):
            ref = mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=0), mo.PhiloxDraws(seed, c), n_it, 1, k_max=32)
        for i in range(n_it):
            head, s_row, e_row = split_trace_row(tr[i, c])
            assert np.allclose(head[:13], ref["mcmc"][i][:13], rtol=1e-9, atol=1e-9), (c, i)
    eng.close()


@pytest.mark.parametrize("engine,C,kw", [("spec", 12, {}), ("spec", 128, {}), ("spec", 128, dict(team=1, cpt=1)),
                                          ("persistent2", 24, {}), ("persistent4", 24, {}),
                                          ("spec", 6, dict(general=True)), ("persistent4", 24, dict(general=True))])
def test_long_inputs_and_few_chain_shards_keep_parity(engine, C, kw):
    """1.3 million lineages (the advisor's out-of-bounds case of round 1: more than 136 trips per scanner wave) and the
    128-chain shard of BASELINE.json configs[3] (1024 chains over 8 GPUs) under every persistent kernel: the accepted
    log-likelihood every chain carries after a run must equal an independent evaluation of its accepted state - by
    lr_bd_loglik_batch (another kernel) for all chains and by the oracle's binned form for a sample; one chain also
    walks the oracle loop's trajectory."""
    from literate_amd import ops, synth
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    from oracle import mcmc_oracle as mo
    general = kw.get("general", False)
    n_lin = 100_000 if C == 128 else 1_300_000
    ts, te, _ = synth.make_lineages(n_lin, n_bins=128, n_shifts=20, seed=4)
    if general:
        rng = np.random.default_rng(9)
        grid = lambda x: np.round(x * 2.0 ** 32) / 2.0 ** 32
        ts = ts + grid(rng.uniform(0, 0.999, n_lin))
        te = np.maximum(np.ceil(te) - 1.0 + grid(rng.uniform(1e-3, 0.999, n_lin)), ts + 0.0078125)
    n_it, seed = 40, 77
    eng = ChainEngine(ts, te, C, model=0, seed=seed, s_freq=1, n_trace_slots=n_it, engine=engine, team=kw.get("team", 0),
                      chains_per_team=kw.get("cpt", 0))
    assert eng.layout.persistent == {"spec": 3, "persistent2": 1, "persistent4": 2}[engine]
    if engine == "spec" and "team" in kw:
        # a chain per CU on a long scan: the kernel mode without the exchange between blocks
        assert (eng.layout.team_blocks, eng.layout.spec_chains_per_team) == (1, 1)
    elif engine == "spec":
        # the 128-chain shard: a team of 2 CUs per chain (a team of 4 per pair on general times); few chains: teams of 8
        assert (eng.layout.team_blocks, eng.layout.spec_chains_per_team) == (((4, 2) if general else (2, 1)) if C == 128 else (8, 1))
    assert eng.layout.table_mode == (2 if general else 1)
    eng.init(); eng.steps(25); eng.steps(n_it - 25)
    if engine == "spec" and "team" in kw:
        assert eng.kernel_name().endswith(", 3>")        # (the mode follows the packed lineages: known once init() has run)
    tr = eng.trace_rows()
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it) and np.all(np.isfinite(snap["likA"]))
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    n_bins = eng.n_bins
    lam = np.stack([snap["L"][c][lo.get_rate_index(np.floor(snap["tL"][c]), n_bins)] for c in range(C)])
    mu = np.stack([snap["M"][c][lo.get_rate_index(np.floor(snap["tM"][c]), n_bins)] for c in range(C)])
    lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, 0, br_length=br).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9)
    stats = dict(sp=sp, ex=ex, br=br)
    for c in range(0, C, max(1, C // 5)):
        assert lo.calc_likelihood(0, lam[c], mu[c], stats) == pytest.approx(snap["likA"][c], rel=1e-9)
    c = C - 1
    with np.errstate(all="ignore"):
        ref = mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=0), mo.PhiloxDraws(seed, c), n_it, 1, k_max=32)
    for i in range(n_it):
        head, s_row, e_row = split_trace_row(tr[i, c])
        assert np.allclose(head[:13], ref["mcmc"][i][:13], rtol=1e-9, atol=1e-9), (c, i)
    eng.close()


@pytest.mark.parametrize("engine,model,general", [("spec", 0, False), ("persistent4", 0, False), ("persistent2", 2, False),
                                                  ("spec", 3, False), ("persistent4", 3, False), ("spec", 0, True),
                                                  ("persistent4", 0, True), ("spec", 3, True),
                                                  ("persistent4", 1, True), ("persistent4", 2, True),
                                                  ("persistent4", 3, True), ("spec", 1, True)])
def test_packing_of_unsorted_sparse_and_extant_lineages(engine, model, general):
    """The pair-slot packing (csrc/lr_pack.hip) on input it was not designed for: lineages in RANDOM order (runs of one or
    two lineages of a birth bin, death bins far apart or decreasing: singles, short stretches, groups of one slot), many
    extant lineages (model 3 sends them through the extant block), a window of few bins.  The accepted log-likelihoods
    after a run must equal an independent evaluation of the accepted states by lr_bd_loglik_batch on the raw times."""
    from literate_amd import ops, synth
    from literate_amd.engine import ChainEngine
    from oracle import literate_oracle as lo
    rng = np.random.default_rng(31)
    n_lin, C, n_it = 3000, 10, 60
    ts, te, _ = synth.make_lineages(n_lin, n_bins=40, n_shifts=4, seed=12)
    if general:
        grid = lambda x: np.round(x * 2.0 ** 32) / 2.0 ** 32
        ts = ts + grid(rng.uniform(0, 0.999, n_lin))
        te = np.maximum(np.ceil(te) - 1.0 + grid(rng.uniform(1e-3, 0.999, n_lin)), ts + 0.0078125)
    order = rng.permutation(n_lin)
    order[:600] = np.sort(order[:600])          # a sorted stretch inside the shuffle: pairs beside singles
    ts, te = ts[order], te[order]
    eng = ChainEngine(ts, te, C, model=model, seed=3, s_freq=10, n_trace_slots=8, engine=engine, sort_lineages=False)
    assert eng.layout.persistent == {"spec": 3, "persistent2": 1, "persistent4": 2}[engine]
    assert eng.layout.table_mode == (2 if general else 1)
    eng.init(); eng.steps(n_it)
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it) and np.all(np.isfinite(snap["likA"]))
    n_bins = eng.n_bins
    lam = np.stack([snap["L"][c][lo.get_rate_index(np.floor(snap["tL"][c]), n_bins)] for c in range(C)])
    mu = np.stack([snap["M"][c][lo.get_rate_index(np.floor(snap["tM"][c]), n_bins)] for c in range(C)])
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, model, br_length=br, end_time=eng.end_time).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9), (lik, snap["likA"])
    eng.close()


def test_cfg4_full_size_1024_chains_100k_lineages():
    """BASELINE.json configs[3] at FULL size on one GPU (the bench workload: 1024 chains x 100k lineages, the
    four-chain persistent kernel).  (i) chains from the first / a middle / the last block walk the oracle loop's
    trajectory row by row; (ii) size-independent property over ALL chains: the accepted log-likelihood the engine
    carries equals an independent evaluation of the accepted state by lr_bd_loglik_batch (another kernel, per-bin
    rates expanded on the host with the oracle's get_rate_index); (iii) every chain has moved."""
    from literate_amd import ops, synth
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    from oracle import mcmc_oracle as mo
    ts, te, _ = synth.make_lineages(100_000, n_bins=128, n_shifts=20, seed=0)
    n_it, seed, C = 150, 2026, 1024
    eng = ChainEngine(ts, te, C, model=0, seed=seed, s_freq=1, n_trace_slots=n_it)
    assert eng.layout.persistent == 2 and eng.unit_resolution
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    assert np.array_equal(eng.sp_events.cpu().numpy(), sp) and np.array_equal(eng.ex_events.cpu().numpy(), ex)
    assert np.array_equal(eng.br_length.cpu().numpy(), br)
    eng.init(); eng.steps(100); eng.steps(n_it - 100)
    tr = eng.trace_rows()
    stats = dict(sp=sp, ex=ex, br=br)
    for c in (0, 1, 2, 3, 513, 1022, 1023):
        with np.errstate(all="ignore"):
            ref = mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=0), mo.PhiloxDraws(seed, c), n_it, 1, k_max=32)
        for i in range(n_it):
            head, s_row, e_row = split_trace_row(tr[i, c])
            assert np.allclose(head[:13], ref["mcmc"][i][:13], rtol=1e-9, atol=1e-9), (c, i)
            assert np.allclose(s_row, ref["sp"][i], rtol=1e-10) and np.allclose(e_row, ref["ex"][i], rtol=1e-10)
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it) and np.all(snap["accepted"] > 0) and np.all(np.isfinite(snap["likA"]))
    n_bins = eng.n_bins
    lam = np.stack([snap["L"][c][lo.get_rate_index(np.floor(snap["tL"][c]), n_bins)] for c in range(C)])
    mu = np.stack([snap["M"][c][lo.get_rate_index(np.floor(snap["tM"][c]), n_bins)] for c in range(C)])
    lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, 0, br_length=br).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9)
    # the same through the oracle's binned form for a sample of chains
    for c in range(0, C, 97):
        assert lo.calc_likelihood(0, lam[c], mu[c], stats) == pytest.approx(snap["likA"][c], rel=1e-9)
    # (iv) 20,000 iterations on (the chains grow to ~10 rates per process: add / remove moves at every size, several
    # launches, the sums carried from one to the next): the property of (ii) again
    eng.steps(20_000)
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it + 20_000) and float(np.mean(snap["K_l"])) > 4.0 and eng.warnings() == 0
    lam = np.stack([snap["L"][c][lo.get_rate_index(np.floor(snap["tL"][c]), n_bins)] for c in range(C)])
    mu = np.stack([snap["M"][c][lo.get_rate_index(np.floor(snap["tM"][c]), n_bins)] for c in range(C)])
    lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, 0, br_length=br).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9)
    eng.close()


def test_cfg5_ddrate_50k_lineages_256_states():
    """BASELINE.json configs[4]: DDRate likelihood (DD:71-107) on 50k synthetic lineages for 256 parameter
    states: lr_dd_rates + the per-lineage Keiding scan against the oracle's binned likelihood_function on
    create_bins statistics (lib:231-257: last bin dropped)."""
    from literate_amd import ops, synth
    from oracle import literate_oracle as lo
    ts, te, _ = synth.make_lineages(50_000, n_bins=64, n_shifts=6, seed=5)
    origin, present = float(ts.min()), float(te.max())
    o, p, nsp, nex, dt, nb, tr = lo.create_bins(origin, present, ts, te, 0)
    import literate_library as ll
    o2, p2, nsp2, nex2, dt2, nb2, tr2 = ll.create_bins(origin, present, ts, te, 0)
    assert nb2 == nb and np.array_equal(nsp2, nsp) and np.array_equal(nex2, nex) and np.array_equal(dt2, dt)
    rng = np.random.default_rng(8)
    C = 256
    args = np.stack([np.exp(rng.uniform(np.log(.05), np.log(1.2), C)), rng.normal(0, 1.0, C), rng.uniform(0, nb, C),
                     rng.uniform(1, 500, C), rng.uniform(2 * dt.max(), 20 * dt.max(), C),
                     np.exp(rng.uniform(np.log(.02), np.log(.5), C)), rng.uniform(.3, 2, C), rng.uniform(.3, 2, C)], 1)
    b, d, ni, nf = ops.dd_rates(args, dt, 2, 2)
    lik = ops.bd_loglik_batch(ts, te, origin, b, d, 2).cpu().numpy()
    n_checked = 0
    for c in range(C):
        with np.errstate(all="ignore"):
            ref = lo.dd_likelihood_function(args[c], nsp, nex, dt, tr, 2, 2)
        assert np.allclose(b[c].cpu().numpy(), ref[1], rtol=1e-12, equal_nan=True)
        assert np.allclose(d[c].cpu().numpy(), ref[2], rtol=1e-12, equal_nan=True)
        if np.isfinite(ref[0].sum()):
            assert lik[c] == pytest.approx(ref[0].sum(), rel=1e-9)
            n_checked += 1
    assert n_checked > C // 2


@pytest.mark.parametrize("n_bins,unit,engine", [(60, None, "auto"), (60, None, "launch"), (134, None, "auto"),
                                                (134, None, "launch"), (135, None, "auto"), (135, None, "launch"),
                                                (200, False, "auto"), (253, None, "auto"), (254, None, "auto"),
                                                (60, None, "persistent4"), (134, None, "persistent4"),
                                                (253, None, "persistent4"),
                                                (30, None, "spec"), (64, None, "spec"), (65, None, "spec"), (128, None, "spec"), (120, None, "spec"), (129, None, "spec"), (200, None, "spec"), (254, None, "spec"),
                                                (120, False, "spec"),
                                                (300, None, "auto"), (300, None, "persistent4"), (300, None, "persistent2"),
                                                (300, False, "persistent4"), (512, None, "persistent4"), (513, None, "auto"),
                                                (1000, None, "auto"),
                                                # the launch-based engine's packed scan in every table class, unit and general
                                                (30, None, "packed"), (64, None, "packed"), (129, None, "packed"), (254, None, "packed"),
                                                (30, False, "packed"), (120, False, "packed"), (200, False, "packed"),
                                                (300, None, "packed"), (512, None, "packed"), (300, False, "packed")])
def test_engine_shapes_bins(n_bins, unit, engine):
    """Table half-stride classes (H = 40, 72, 136, 264; a class holds n_bins <= 64 x its bins-per-lane count, so 129..134
    bins move up to H = 264; 255..512 bins: H = 520, persistent kernels only) and the generic kernel beyond them
    (n_bins = 513, 1000), unit-resolution and general tables: a few chains against the oracle loop on synthetic data."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    from literate_amd import synth
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    from oracle import mcmc_oracle as mo
    ts, te, _ = synth.make_lineages(4000, n_bins=n_bins, n_shifts=5, seed=n_bins)
    ts = np.concatenate([[0.0], ts]); te = np.concatenate([[float(n_bins) + 0.5], te])   # pin the window to n_bins
    n_it, seed, C = 120, 7, 37
    eng = ChainEngine(ts, te, C, model=0, seed=seed, s_freq=1, n_trace_slots=n_it, unit_resolution=unit, engine=engine)
    assert eng.n_bins == n_bins
    if engine == "persistent4":
        assert eng.layout.persistent == 2      # 37 chains: the last block holds one chain of four
    if engine == "persistent2":
        assert eng.layout.persistent == 1
    if n_bins == 300 and engine == "auto":
        assert eng.layout.persistent != 0      # the H = 520 class
    if n_bins > 512:
        assert eng.layout.persistent == 0
    if engine == "spec":
        assert eng.layout.persistent == 3      # 37 chains: the last block holds one chain of its pair
    if engine == "packed":
        # 37 chains = 19 pairs: four pairs per block up to H = 136, at H = 264 (102 KB of planes) as well - five pair groups,
        # the last one ragged; general times in the pair-general form
        # (255 .. 512 bins: the H = 520 class, 100 KB of planes for TWO pairs per block)
        Hc = {30: 40, 64: 72, 120: 136, 129: 264, 200: 264, 254: 264, 300: 520, 512: 520}[n_bins]
        assert eng.layout.persistent == 0 and eng.layout.packed_scan == 1 and eng.kernel_name().startswith("lr_packscan_kernel<%d, %d, %s>" % (
            2 if Hc == 520 else 4, Hc, "true" if unit is False else "false"))
    eng.init(); eng.steps(n_it)
    tr = eng.trace_rows()
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    for c in (0, 18, 36):
        with np.errstate(all="ignore"):
            ref = mo.run_mcmc(dict(sp=sp, ex=ex, br=br), ts.min(), te.max(), mo.Settings(model_BDI=0),
                              mo.PhiloxDraws(seed, c), n_it, 1, k_max=32)
        for i in range(n_it):
            head, s_row, e_row = split_trace_row(tr[i, c])
            assert np.allclose(head[:13], ref["mcmc"][i][:13], rtol=1e-9, atol=1e-9), (n_bins, c, i, head, ref["mcmc"][i])
    eng.close()


@pytest.mark.parametrize("engine", ["launch", "auto", "persistent4"])
def test_engine_chain_count_shapes(G, engine):
    """Any number of chains: single partition / two partitions, pipelined or not, ragged last block.  The same
    global chains must walk the same path in every engine shape (sums differ only by their tile partition)."""
    from literate_amd.engine import ChainEngine
    name, n_it = "metal_bands", 60
    ref = ChainEngine(G[name + "/ts"], G[name + "/te"], 1, model=2, seed=3, s_freq=1, n_trace_slots=n_it, chain_offset=0)
    ref.init(); ref.steps(n_it)
    first = ref.trace_rows()[:, 0]
    ref.close()
    for C in (1, 2, 5, 16, 17, 31, 32, 33, 47, 100, 129):
        eng = ChainEngine(G[name + "/ts"], G[name + "/te"], C, model=2, seed=3, s_freq=1, n_trace_slots=n_it,
                          engine=engine)
        eng.init(); eng.steps(25); eng.steps(n_it - 25)
        tr = eng.trace_rows()
        assert np.allclose(tr[:, 0], first, rtol=1e-10, atol=1e-9, equal_nan=True), C
        last = ChainEngine(G[name + "/ts"], G[name + "/te"], 1, model=2, seed=3, s_freq=1, n_trace_slots=n_it,
                           chain_offset=C - 1)
        last.init(); last.steps(n_it)
        assert np.allclose(tr[:, C - 1], last.trace_rows()[:, 0], rtol=1e-10, atol=1e-9, equal_nan=True), C
        assert np.all(eng.snapshot()["it"] == n_it)
        eng.close(); last.close()


@pytest.mark.parametrize("engine,C", [("launch", 24), ("packed", 24), ("persistent", 24), ("persistent", 10), ("persistent4", 10), ("spec", 9),
                                      ("spec2", 10), ("spec1x2", 7), ("spec2x1", 9)])
def test_checkpoint_resume_is_bit_identical(G, tmp_path, engine, C):
    """save() after 130 iterations, load() into a fresh engine, 170 more: state, pending proposals and all 300
    trace rows equal an uninterrupted run bit for bit (draws are addressed by (seed, chain, iteration));
    a checkpoint from another configuration is refused."""
    import torch
    from literate_amd.engine import ChainEngine
    name = "metal_bands"
    kw = dict(model=0, seed=77, s_freq=1, n_trace_slots=300, engine=engine)
    if engine == "spec2":
        kw.update(engine="spec", team=2)       # a team of two blocks per chain pair
    if engine == "spec1x2":
        kw.update(engine="spec", team=2, chains_per_team=1)       # a team of two blocks per CHAIN
    if engine == "spec2x1":
        kw.update(engine="spec", team=1, chains_per_team=2)       # a block per chain pair
    full = ChainEngine(G[name + "/ts"], G[name + "/te"], C, **kw)
    full.init(); full.steps(300)
    a = ChainEngine(G[name + "/ts"], G[name + "/te"], C, **kw)
    a.init(); a.steps(130)
    path = str(tmp_path / "run.npz")
    a.save(path)
    a.close()
    b = ChainEngine(G[name + "/ts"], G[name + "/te"], C, **kw)
    b.load(path)
    assert b.iterations == 130
    b.steps(170)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int64)       # bit patterns: the padding of a trace row is NaN
    assert torch.equal(bits(b.trace), bits(full.trace))
    assert torch.equal(bits(b.state_f64), bits(full.state_f64)) and torch.equal(b.state_i32, full.state_i32)
    other = ChainEngine(G[name + "/ts"], G[name + "/te"], C, **dict(kw, seed=78))
    with pytest.raises(ValueError):
        other.load(path)
    for e in (full, b, other):
        e.close()


def test_checkpoints_append_their_trace_rows_and_can_be_written_behind_the_next_window(G, tmp_path):
    """A checkpoint per window: the state goes to <path>.npz (a few MB), the trace rows sampled since the last write are
    APPENDED to <path>.npz.trace (no window rewrites the whole trace buffer); checkpoint_begin() takes the state on the
    device and the write may follow while later windows run.  Resumed from the second of three checkpoints (with rows of a
    later, unfinished write left in the trace file: a kill between the two halves of a write), the run ends bit-identical
    to an uninterrupted one, and its next checkpoint truncates the stale rows."""
    import torch
    from literate_amd import _hip
    from literate_amd.engine import ChainEngine
    name, C = "metal_bands", 12
    kw = dict(model=0, seed=5, s_freq=10, n_trace_slots=40)
    full = ChainEngine(G[name + "/ts"], G[name + "/te"], C, **kw)
    full.init(); full.steps(400)
    a = ChainEngine(G[name + "/ts"], G[name + "/te"], C, **kw)
    a.init()
    path = str(tmp_path / "run.npz")
    row_bytes = C * _hip.LR_TRACE_W * 8
    a.steps(100); t1 = a.checkpoint_begin()
    a.steps(100); t2 = a.checkpoint_begin()          # two windows launched before the first checkpoint is written
    a.check_status()
    a.checkpoint_write(t1, path)
    assert os.path.getsize(path + ".trace") == 10 * row_bytes
    a.checkpoint_write(t2, path)
    assert os.path.getsize(path + ".trace") == 20 * row_bytes
    assert os.path.getsize(path) < a.workspace.numel() - 40 * row_bytes + (1 << 16)         # the .npz holds no trace rows
    keep = open(path, "rb").read()
    a.steps(100); a.save(path)                        # a third checkpoint ...
    assert os.path.getsize(path + ".trace") == 30 * row_bytes
    open(path, "wb").write(keep)                      # ... whose .npz never replaced the second: its rows are stale
    a.close()
    b = ChainEngine(G[name + "/ts"], G[name + "/te"], C, **kw)
    b.load(path)
    assert b.iterations == 200
    b.steps(100); b.save(path)
    assert os.path.getsize(path + ".trace") == 30 * row_bytes
    b.steps(100)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int64)
    assert torch.equal(bits(b.trace), bits(full.trace)) and torch.equal(bits(b.state_f64), bits(full.state_f64))
    c = ChainEngine(G[name + "/ts"], G[name + "/te"], C, **kw)
    c.load(path)
    assert c.iterations == 300 and torch.equal(bits(c.trace[:30]), bits(full.trace[:30]))
    os.truncate(path + ".trace", 29 * row_bytes)
    with pytest.raises(ValueError):
        c.load(path)
    for e in (full, b, c):
        e.close()


@pytest.mark.parametrize("general", [False, True])
def test_four_chain_kernel_does_not_depend_on_how_a_run_is_cut_into_launches(general):
    """The four-chain kernel leaves the scan sums of its last phase for the next launch instead of scoring pair 0 again: a
    run cut into launches of 7 + 1 + 32 iterations equals one launch of 40 bit for bit (60k lineages: several trips per
    scanner lane, the helper waves' share included), and a second init() of the same engine - which sets the state
    from outside - is not served the sums the run before it left."""
    import torch
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    ts, te, _ = synth.make_lineages(60_000, n_bins=128, n_shifts=20, seed=11)
    if general:
        rng = np.random.default_rng(3)
        ts = ts + rng.uniform(0, 0.999, len(ts))
        te = np.maximum(te + rng.uniform(-0.49, 0.49, len(te)), ts + 1e-3)
    kw = dict(model=0, seed=5, s_freq=1, n_trace_slots=40, engine="persistent4")
    one = ChainEngine(ts, te, 22, **kw)
    one.init(); one.steps(40)
    cut = ChainEngine(ts, te, 22, **kw)
    cut.init(); cut.steps(13)                 # a run whose sums must not leak into the next one
    cut.init(); cut.steps(7); cut.steps(1); cut.steps(32)
    torch.cuda.synchronize()
    assert one.layout.persistent == 2 and one.kernel_name().endswith("true, false, false>" if general else "false, false, true>")
    bits = lambda t: t.contiguous().view(torch.int64)
    assert torch.equal(bits(cut.trace), bits(one.trace))
    assert torch.equal(bits(cut.state_f64), bits(one.state_f64)) and torch.equal(cut.state_i32, one.state_i32)
    one.close(); cut.close()


@pytest.mark.parametrize("mb,md,engine", [(2, 2, "auto"), (2, 2, "launch"), (2, 2, "persistent4"), (2, 2, "packed"), (1, 1, "auto"),
                                          (0, 0, "auto"), (2, -1, "auto"), (2, 0, "launch"), (1, 2, "auto"),
                                          (2, -2, "auto")])
def test_ddrate_sampler_follows_oracle(G, golden_dir, mb, md, engine):
    """DDRate.py's sampler (DD:124-241) on the engine (lr_mcmc_config.sampler = 1), metal_bands, 11 chains: every
    sampled log row (scalars AND the 4 x n_bins per-bin columns) against the oracle loop fed the same Philox draws.
    The oracle scores with the reference's binned likelihood, the engine per lineage."""
    from literate_amd.ddrate import DDRateEngine
    from oracle import dd_mcmc_oracle as ddo
    D = np.load(os.path.join(golden_dir, "ddrate.npz"))
    origin, present, _ = D["meta"]
    ts, te = G["metal_bands/lib_ts"], G["metal_bands/lib_te"]
    n_it, seed, C, off = 600, 909, 11, 5
    eng = DDRateEngine(ts, te, origin, present, C, m_birth=mb, m_death=md, seed=seed, s_freq=3,
                       n_trace_slots=n_it // 3, chain_offset=off, engine=engine)
    assert np.array_equal(eng.n_spec, D["N_SPEC"]) and np.array_equal(eng.DT, D["DT"])
    if engine != "auto":
        assert (eng.layout.persistent > 0) == (engine not in ("launch", "packed")) and eng.layout.packed_scan == (1 if engine == "packed" else 0)
    eng.init(); eng.steps(250); eng.steps(n_it - 250)
    with np.errstate(all="ignore"):
        emp = (D["N_SPEC"] / D["DT"], D["N_EXTI"] / D["DT"])
    moved = 0
    for c in (0, 1, 6, 10):
        ref = ddo.run_dd_mcmc(D["N_SPEC"], D["N_EXTI"], D["DT"], D["TIME_RANGE"], origin, present, mb, md,
                              ddo.PhiloxDraws(seed, off + c), n_it, 3, emp=emp)
        got = eng.log_rows(c, emp=emp)
        assert len(got) == len(ref) == n_it // 3
        for i, (g, r) in enumerate(zip(got, ref)):
            assert g[0] == r[0]
            assert np.allclose(g[1:-3], r[1:-3], rtol=1e-9, atol=1e-9, equal_nan=True), (c, i, g[:14], r[:14])
            assert np.allclose(g[-3:], r[-3:], rtol=1e-7, atol=1e-9, equal_nan=True)
        moved += len(set(np.round(np.array(ref)[:, 2], 6)))
    assert moved > 4 * 30
    assert np.all(eng.snapshot()["it"] == n_it)
    eng.close()


def test_cfg1_fixed_two_shifts_engine_vs_reference_run(G, golden_dir):
    """BASELINE.json configs[0] on the device: example_dataTBP, fixed 2 rate shifts (3-rate initial state of the
    golden reference run, const_rates=1).  (i) one chain follows the oracle loop (Philox draws) row by row from that
    state; (ii) the posterior means of the six segment rates over 64 device chains agree with the reference's own
    runMCMC chain (tests/golden/cfg1_fixed_shifts.npz) within Monte-Carlo error."""
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import mcmc_oracle as mo
    T = np.load(os.path.join(golden_dir, "cfg1_fixed_shifts.npz"))
    name, C, n_it, s = "example_TBP", 64, 6000, 10
    eng = ChainEngine(G[name + "/ts"], G[name + "/te"], C, model=0, seed=5, const_rates=1, s_freq=s, n_trace_slots=n_it // s)
    init = [[T["L0"]] * C, [T["M0"]] * C, [T["times0"]] * C, [T["times0"]] * C]
    eng.init(*init)
    eng.steps(n_it)
    tr = eng.trace_rows()
    stats = dict(sp=G[name + "/sp"], ex=G[name + "/ex"], br=G[name + "/br"])
    start, end = G[name + "/start_end"]
    with np.errstate(all="ignore"):
        ref = mo.run_mcmc(stats, start, end, mo.Settings(model_BDI=0, const_rates=1), mo.PhiloxDraws(5, 0), n_it, s,
                          init=(T["L0"], T["M0"], T["times0"], T["times0"]), k_max=32)
    for i in range(n_it // s):
        head, sp, ex = split_trace_row(tr[i, 0])
        assert np.allclose(head[:13], ref["mcmc"][i][:13], rtol=1e-9, atol=1e-9), i
        assert np.allclose(sp, ref["sp"][i], rtol=1e-10) and np.allclose(ex, ref["ex"][i], rtol=1e-10)
    burn = 100
    K = 32
    dev_sp = tr[burn:, :, 13:13 + 3].reshape(-1, 3).mean(0)                    # rates are the first K_MAX entries
    dev_ex = tr[burn:, :, 13 + (2 * K - 1):13 + (2 * K - 1) + 3].reshape(-1, 3).mean(0)
    ref_sp, ref_ex = T["sp"][burn:, :3].mean(0), T["ex"][burn:, :3].mean(0)
    assert np.all(tr[:, :, 6] == 3) and np.all(tr[:, :, 7] == 3)
    assert np.allclose(dev_sp, ref_sp, rtol=0.12) and np.allclose(dev_ex, ref_ex, rtol=0.12), (dev_sp, ref_sp, dev_ex, ref_ex)
    eng.close()


@pytest.mark.parametrize("engine", ["auto", "launch", "persistent4", "persistent2"])
def test_engine_tiny_input_three_lineages(engine):
    """Smallest inputs: three lineages (one extant), 9 unit bins, chains 1..5 - the scan's tile, pair and quad paths all
    run ragged; in the persistent kernels one packed group for 896 / 1024 scanning lanes (all but one score the zero
    groups behind the data, most waves make no trip at all).  Rows against the oracle loop."""
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    from oracle import mcmc_oracle as mo
    ts = np.array([0.0, 2.0, 5.0])
    te = np.array([4.5, 9.5, 7.5])
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    n_it, seed = 200, 3
    for C in (1, 2, 5):
        eng = ChainEngine(ts, te, C, model=0, seed=seed, s_freq=1, n_trace_slots=n_it, engine=engine)
        assert eng.n_bins == len(sp) == 9
        eng.init(); eng.steps(n_it)
        tr = eng.trace_rows()
        for c in range(C):
            with np.errstate(all="ignore"):
                ref = mo.run_mcmc(dict(sp=sp, ex=ex, br=br), ts.min(), te.max(), mo.Settings(model_BDI=0),
                                  mo.PhiloxDraws(seed, c), n_it, 1, k_max=32)
            for i in range(n_it):
                head, s_row, e_row = split_trace_row(tr[i, c])
                assert np.allclose(head[:13], ref["mcmc"][i][:13], rtol=1e-9, atol=1e-9, equal_nan=True), (C, c, i)
        eng.close()


def test_end_to_end_simulate_then_recover_key_innovation():
    """Whole stack on the device: lr_simulate_bd draws a key-innovation history (birth rate 0.10 -> 0.25 at t = 24 of 40,
    death rate 0.08, per-step Bernoulli scheme at scale 4), the RJMCMC engine samples 32 chains on the resulting
    lineages, and the pooled posterior per-bin rates (plotRJforward.v3.py:92-139 definition) recover the history."""
    from literate_amd import logs, synth
    from literate_amd.engine import ChainEngine, split_trace_row
    T, scale = 40, 4
    la, mu = synth.rates_key_innovation(T, .10, .08, .6, .15)
    ts, te, trace = synth.simulate(2000, T, scale, seed=11, rates=(la, mu))
    assert 20_000 < len(ts) < 200_000 and trace[-1] > trace[0]
    C, n_it, s = 32, 8000, 20
    eng = ChainEngine(ts, te, C, model=0, seed=3, s_freq=s, n_trace_slots=n_it // s)
    eng.init(); eng.steps(n_it)
    tr = eng.trace_rows()
    burn = (n_it // s) // 4
    sp_bins, ex_bins = [], []
    for c in range(C):
        for i in range(burn, n_it // s):
            head, sp, ex = split_trace_row(tr[i, c])
            k_l, k_m = int(head[6]), int(head[7])
            sp_bins.append(logs.rates_per_bin(sp[:k_l], sp[k_l:], eng.start_time, eng.n_bins))
            ex_bins.append(logs.rates_per_bin(ex[:k_m], ex[k_m:], eng.start_time, eng.n_bins))
    lam_hat, mu_hat = np.mean(sp_bins, 0), np.mean(ex_bins, 0)
    assert eng.n_bins == T
    assert np.allclose(lam_hat[3:22], .10, rtol=0.3), lam_hat
    assert np.allclose(lam_hat[27:38], .25, rtol=0.3), lam_hat
    assert np.allclose(mu_hat[3:38], .08, rtol=0.35), mu_hat
    assert lam_hat[27:38].mean() > 1.8 * lam_hat[3:22].mean()
    eng.close()


@pytest.mark.parametrize("cb,cd,engine", [(0, 0, "auto"), (0, 0, "launch"), (0, 0, "persistent4"), (0, 0, "packed"), (1, 0, "auto"), (0, 1, "auto")])
def test_trend_rate_sampler_follows_oracle(G, golden_dir, cb, cd, engine):
    """trend_rate.py's sampler (:102-196) on the engine (lr_mcmc_config.sampler = 2), metal_bands + the fixture's
    covariate, 9 chains: every sampled log row against the oracle loop fed the same Philox draws."""
    from literate_amd.trendrate import TrendRateEngine, normalise_trend
    from oracle import trend_mcmc_oracle as tro
    R = np.load(os.path.join(golden_dir, "ratemaps.npz"))
    D = np.load(os.path.join(golden_dir, "ddrate.npz"))
    origin, present, _ = D["meta"]
    trend = normalise_trend(R["trend_raw"])
    assert np.array_equal(trend, R["TREND"])
    ts, te = G["metal_bands/lib_ts"], G["metal_bands/lib_te"]
    n_it, seed, C, off = 600, 411, 9, 3
    eng = TrendRateEngine(ts, te, origin, present, trend, C, const_birth=cb, const_death=cd, seed=seed, s_freq=3,
                          n_trace_slots=n_it // 3, chain_offset=off, engine=engine)
    eng.init(); eng.steps(250); eng.steps(n_it - 250)
    with np.errstate(all="ignore"):
        emp = (R["N_SPEC"] / R["DT"], R["N_EXTI"] / R["DT"])
    moved = 0
    for c in (0, 4, 8):
        ref = tro.run_trend_mcmc(R["N_SPEC"], R["N_EXTI"], R["DT"], R["TREND"], tro.PhiloxDraws(seed, off + c), n_it, 3,
                                 bool(cb), bool(cd), emp=emp)
        got = eng.log_rows(c, emp=emp)
        assert len(got) == len(ref) == n_it // 3
        for i, (g, r) in enumerate(zip(got, ref)):
            assert g[0] == r[0]
            assert np.allclose(g[1:-3], r[1:-3], rtol=1e-9, atol=1e-9, equal_nan=True), (c, i, g[:12], r[:12])
            assert np.allclose(g[-3:], r[-3:], rtol=1e-7, atol=1e-9, equal_nan=True)
        moved += len(set(np.round(np.array(ref)[:, 2], 6)))
    assert moved > 3 * 30
    eng.close()


@pytest.mark.parametrize("kind", ["dd", "trend"])
def test_parametric_samplers_resume_and_sharding(G, golden_dir, tmp_path, kind):
    """The engine services the parametric samplers inherit: a run resumed from a checkpoint is bit-identical to an
    uninterrupted one, and a chain's trajectory does not depend on which shard (chain_offset) hosts it."""
    import torch
    from literate_amd.ddrate import DDRateEngine
    from literate_amd.trendrate import TrendRateEngine
    D = np.load(os.path.join(golden_dir, "ddrate.npz"))
    R = np.load(os.path.join(golden_dir, "ratemaps.npz"))
    origin, present, _ = D["meta"]
    ts, te = G["metal_bands/lib_ts"], G["metal_bands/lib_te"]

    def make(C, off):
        kw = dict(seed=8, s_freq=1, n_trace_slots=200, chain_offset=off)
        if kind == "dd":
            return DDRateEngine(ts, te, origin, present, C, **kw)
        return TrendRateEngine(ts, te, origin, present, R["TREND"], C, **kw)

    bits = lambda t: t.contiguous().view(torch.int64)
    full = make(6, 0)
    full.init(); full.steps(200)
    a = make(6, 0)
    a.init(); a.steps(90)
    path = str(tmp_path / "p.npz")
    a.save(path); a.close()
    b = make(6, 0)
    b.load(path); b.steps(110)
    torch.cuda.synchronize()
    assert torch.equal(bits(b.trace), bits(full.trace)) and torch.equal(bits(b.state_f64), bits(full.state_f64))
    shard = make(2, 4)                       # global chains 4, 5
    shard.init(); shard.steps(200)
    torch.cuda.synchronize()
    assert torch.equal(bits(shard.trace[:, 0]), bits(full.trace[:, 4])) and torch.equal(bits(shard.trace[:, 1]), bits(full.trace[:, 5]))
    for e in (full, b, shard):
        e.close()


@pytest.mark.parametrize("engine,C,team,n_lin", [("spec", 128, 4, 100_000), ("persistent4", 1024, 0, 100_000),
                                                ("spec", 6, 8, 1_300_000), ("persistent4", 24, 0, 1_300_000)])
def test_general_times_off_grid_against_the_oracle_at_size(engine, C, team, n_lin):
    """ARBITRARY fp64 lineage times (uniform jitter, NOT on the 2^-32 grid the packing is exact on) at the size of
    bench.py's cfg4_general (100k lineages: 1024 chains under the four-chain kernel, the 128-chain shard under the
    speculative kernel in teams of 4) and at 1.3 million lineages: the persistent engines carry the in-bin fractions as
    32-bit fixed point (csrc/lr_pack.hip), narrower than the reference's fp64, so the log-likelihood EVERY chain carries
    for its accepted state is checked against the ORACLE's fp64 per-lineage evaluation (BDIx:124-146 form) of that state
    on the raw times, at the north star's 1e-9 relative."""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    from oracle import literate_oracle as lo
    rng = np.random.default_rng(7)
    ts, te, _ = synth.make_lineages(n_lin, n_bins=128, n_shifts=20, seed=0 if n_lin == 100_000 else 4)
    ts = ts + rng.uniform(0.0, 1.0, n_lin) * 0.999                      # as bench.py make_workload("cfg4_general")
    te = np.maximum(np.ceil(te) - 1.0 + rng.uniform(1e-3, 0.999, n_lin), ts + 1e-3)
    assert np.any(np.round(ts * 2.0 ** 32) != ts * 2.0 ** 32)           # off the grid
    n_it = 120 if n_lin == 100_000 else 40
    eng = ChainEngine(ts, te, C, model=0, seed=2026, s_freq=10, n_trace_slots=n_it // 10, engine=engine, team=team)
    assert not eng.unit_resolution and eng.layout.table_mode == 2
    assert eng.layout.persistent == (3 if engine == "spec" else 2)
    if team:
        assert eng.layout.team_blocks == team
    eng.init(); eng.steps(n_it // 2); eng.steps(n_it - n_it // 2)
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it) and np.all(snap["accepted"] > 0)
    br = eng.br_length.cpu().numpy()
    t0o, sp, ex, bro = lo.bin_events_cli(ts, te)
    assert t0o == eng.t0 and np.allclose(br, bro, rtol=1e-12)
    lam, mu = _accepted_rates(snap, eng.n_bins, C)
    pre = lo.lineage_bins(ts, te, float(t0o), eng.n_bins)
    worst = 0.0
    for c in range(C):
        ref = lo.per_lineage_loglik(ts, te, float(t0o), lam[c], mu[c], 0, bro, pre=pre)
        worst = max(worst, abs(snap["likA"][c] - ref) / abs(ref))
    assert worst < 1e-9, worst
    eng.close()


@pytest.mark.parametrize("model", [1, 2, 3])
def test_cfg4_full_size_other_models_under_the_four_chain_kernel(model):
    """Models 1, 2 and 3 at the bench size (1024 chains x 100k lineages, the four-chain persistent kernel; model 0 is
    test_cfg4_full_size_1024_chains_100k_lineages): the accepted log-likelihood of EVERY chain against an independent
    evaluation of its accepted state by lr_bd_loglik_batch, a sample of chains against the oracle's binned
    calc_likelihood (LRF:137-162; model 3 on the te < end_time statistics, LRF:529-546), and two chains row by row
    against the oracle loop."""
    from literate_amd import ops, synth
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    from oracle import mcmc_oracle as mo
    ts, te, _ = synth.make_lineages(100_000, n_bins=128, n_shifts=20, seed=0)
    n_it, seed, C = 100, 2026, 1024
    eng = ChainEngine(ts, te, C, model=model, seed=seed, s_freq=1, n_trace_slots=n_it, engine="persistent4")
    assert eng.layout.persistent == 2 and eng.unit_resolution
    eng.init(); eng.steps(60); eng.steps(n_it - 60)
    tr = eng.trace_rows()
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it) and np.all(snap["accepted"] > 0) and np.all(np.isfinite(snap["likA"]))
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    stats = dict(sp=sp, ex=ex, br=br)
    if model == 3:
        stats["ex_dead"], stats["br_dead"] = lo.bin_events_dead(ts, te, te.max())
    lam, mu = _accepted_rates(snap, eng.n_bins, C)
    lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, model, br_length=br, end_time=eng.end_time).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9)
    for c in range(0, C, 97):
        with np.errstate(all="ignore"):
            assert lo.calc_likelihood(model, lam[c], mu[c], stats) == pytest.approx(snap["likA"][c], rel=1e-9)
    for c in (2, 1021):
        with np.errstate(all="ignore"):
            ref = mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=model), mo.PhiloxDraws(seed, c), n_it, 1, k_max=32)
        for i in range(n_it):
            head, s_row, e_row = split_trace_row(tr[i, c])
            assert np.allclose(head[:13], ref["mcmc"][i][:13], rtol=1e-9, atol=1e-9), (c, i)
    eng.close()


def test_cfg5_ddrate_sampler_at_size():
    """BASELINE.json configs[4] at its size, the SAMPLER (DD:124-241; the likelihood alone is
    test_cfg5_ddrate_50k_lineages_256_states): DDRateEngine on bench.py's cfg5 workload - 50k synthetic lineages,
    256 chains, -m_birth 2 -m_death 2, the engine the bench line is quoted on.  Three chains row by row (scalars and the
    4 x n_bins per-bin columns) against the oracle loop fed the same Philox draws, and all 256 accepted parameter
    vectors re-evaluated by lr_dd_rates + lr_bd_loglik_batch (other kernels) and by the oracle's binned
    likelihood_function (DD:71-107)."""
    from literate_amd import ops, synth
    from literate_amd.ddrate import DDRateEngine
    from oracle import dd_mcmc_oracle as ddo
    from oracle import literate_oracle as lo
    ts, te, _ = synth.make_lineages(50_000, n_bins=64, n_shifts=6, seed=0)
    n_it, s, seed, C = 600, 4, 2026, 256
    eng = DDRateEngine(ts, te, float(ts.min()), float(te.max()), C, m_birth=2, m_death=2, seed=seed, s_freq=s,
                       n_trace_slots=n_it // s)
    assert eng.layout.persistent == 3          # the speculative kernel, as in bench.py's configs.cfg5
    o, p, nsp, nex, dt, nb, tr_range = lo.create_bins(float(ts.min()), float(te.max()), ts, te, 0)
    assert np.array_equal(eng.n_spec, nsp) and np.array_equal(eng.DT, dt) and (eng.origin, eng.present) == (o, p)
    eng.init(); eng.steps(250); eng.steps(n_it - 250)
    with np.errstate(all="ignore"):
        emp = (nsp / dt, nex / dt)
    moved = 0
    for c in (0, 101, 255):
        ref = ddo.run_dd_mcmc(nsp, nex, dt, tr_range, o, p, 2, 2, ddo.PhiloxDraws(seed, c), n_it, s, emp=emp)
        got = eng.log_rows(c, emp=emp)
        assert len(got) == len(ref) == n_it // s
        for i, (g, r) in enumerate(zip(got, ref)):
            assert g[0] == r[0]
            assert np.allclose(g[1:-3], r[1:-3], rtol=1e-9, atol=1e-9, equal_nan=True), (c, i, g[:14], r[:14])
            assert np.allclose(g[-3:], r[-3:], rtol=1e-7, atol=1e-9, equal_nan=True)
        moved += len(set(np.round(np.array(ref)[:, 2], 6)))
    assert moved > 3 * 20
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it)
    args = np.stack([snap["L"][c][:8] for c in range(C)])
    b, d, ni, nf = ops.dd_rates(args, dt, 2, 2)
    lik = ops.bd_loglik_batch(ts, te, o, b, d, 2).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9)
    for c in range(0, C, 17):
        with np.errstate(all="ignore"):
            ref = lo.dd_likelihood_function(args[c], nsp, nex, dt, tr_range, 2, 2)
        assert ref[0].sum() == pytest.approx(snap["likA"][c], rel=1e-9)
    eng.close()


def test_kmax_cap_raises_the_warning_word():
    """The device holds at most LR_KMAX = 32 rates per process (the reference is unbounded, LRF:29-47): an add-shift
    proposed from a state at the cap is rejected and the engine's warning word says so; a run that never gets there
    carries no warning."""
    from literate_amd import _hip, synth
    from literate_amd.engine import ChainEngine
    ts, te, _ = synth.make_lineages(3000, n_bins=200, n_shifts=4, seed=2)
    C = 8
    for engine in ("launch", "persistent4", "spec"):
        eng = ChainEngine(ts, te, C, model=0, seed=4, s_freq=100, n_trace_slots=4, engine=engine, poisson_HP=200.0)
        t = np.linspace(eng.start_time, eng.end_time, 33)          # 32 rates per process: every add-shift hits the cap
        eng.init([np.full(32, .3)] * C, [np.full(32, .1)] * C, [t] * C, [t] * C)
        eng.steps(400)
        assert eng.warnings() & _hip.LR_WARN_KCAP, engine
        assert "truncated" in eng.warning_text()
        eng.init()                                                     # a fresh run clears the word
        eng.steps(50)
        assert eng.warnings() == 0
        eng.close()


def _off_year_grid(ts, te, rng, exact=True):
    """Continuous times from year-resolution ones: births anywhere inside their year, deaths later in theirs; the first
    births and the extant lineages stay where they are, so ORIGIN / PRESENT (lib:196-229) stay integer / unchanged.
    exact: jitter on the 2^-32 grid, where the persistent engines' fixed-point fractions are exact."""
    grid = (lambda x: np.round(x * 2.0 ** 32) / 2.0 ** 32) if exact else (lambda x: x)
    n = len(ts)
    ts2 = ts + grid(rng.uniform(0, 0.999, n))
    ts2[ts == ts.min()] = ts.min()
    te2 = np.maximum(te + grid(rng.uniform(0, 0.4, n)), ts2 + 0.0078125)
    te2[te >= te.max()] = te.max()
    return ts2, te2


@pytest.mark.parametrize("kind,engine", [("dd", "auto"), ("dd", "persistent4"), ("dd", "spec"), ("dd", "packed"), ("trend", "auto"),
                                         ("trend", "persistent4"), ("trend", "spec"), ("trend", "packed")])
def test_parametric_samplers_on_continuous_times(G, golden_dir, kind, engine):
    """`DDRate.py -d <continuous times>` / trend_rate.py select the PARAM x GENERAL instantiations - lr_persist4_kernel<H,
    true, true, .>, lr_spec_kernel<H, T, false, true, .> - which no unit-resolution test reaches (pair-general table
    layout under a parametric sampler).  metal_bands moved off the year grid: every sampled log row against the oracle loop
    run on statistics binned from the SAME jittered data, and every chain's accepted parameter vector re-evaluated by
    lr_dd_rates / lr_trend_rates + lr_bd_loglik_batch (other kernels, fp64 fractions from the raw times)."""
    from literate_amd import ops
    from literate_amd.ddrate import DDRateEngine
    from literate_amd.trendrate import TrendRateEngine
    from oracle import dd_mcmc_oracle as ddo
    from oracle import literate_oracle as lo
    from oracle import trend_mcmc_oracle as tro
    R = np.load(os.path.join(golden_dir, "ratemaps.npz"))
    rng = np.random.default_rng(17)
    ts, te = _off_year_grid(G["metal_bands/lib_ts"], G["metal_bands/lib_te"], rng)
    origin, present = float(ts.min()), float(te.max())
    o, p, nsp, nex, dt, nb, t_range = lo.create_bins(origin, present, ts, te, 0)
    n_it, s, seed, C, off = 450, 3, 77, 9, 2
    kw = dict(seed=seed, s_freq=s, n_trace_slots=n_it // s, chain_offset=off, engine=engine)
    if kind == "dd":
        eng = DDRateEngine(ts, te, origin, present, C, m_birth=2, m_death=2, **kw)
    else:
        assert len(R["TREND"]) == nb
        eng = TrendRateEngine(ts, te, origin, present, R["TREND"], C, **kw)
    assert not eng.unit_resolution
    name = eng.kernel_name()
    if engine == "persistent4":
        assert eng.layout.persistent == 2 and name.startswith("lr_persist4_kernel<") and ", true, true, " in name, name
    elif engine == "spec":
        assert eng.layout.persistent == 3 and name.startswith("lr_spec_kernel<") and ", false, true, " in name, name
    elif engine == "packed":
        # (the launch-based engine under a parametric sampler, its scan over the packed lineages in the pair-general form)
        assert eng.layout.persistent == 0 and eng.layout.packed_scan == 1 and name.startswith("lr_packscan_kernel<") and name.endswith("true>"), name
    if eng.layout.persistent or engine == "packed":
        assert eng.layout.table_mode == 2
    assert np.array_equal(eng.n_spec, nsp) and np.array_equal(eng.n_exti, nex) and np.allclose(eng.DT, dt, rtol=1e-13)
    eng.init(); eng.steps(200); eng.steps(n_it - 200)
    with np.errstate(all="ignore"):
        emp = (nsp / dt, nex / dt)
    moved = 0
    for c in (0, 4, 8):
        if kind == "dd":
            ref = ddo.run_dd_mcmc(nsp, nex, dt, t_range, o, p, 2, 2, ddo.PhiloxDraws(seed, off + c), n_it, s, emp=emp)
        else:
            ref = tro.run_trend_mcmc(nsp, nex, dt, R["TREND"], tro.PhiloxDraws(seed, off + c), n_it, s, False, False, emp=emp)
        got = eng.log_rows(c, emp=emp)
        assert len(got) == len(ref) == n_it // s
        for i, (g, r) in enumerate(zip(got, ref)):
            assert g[0] == r[0]
            assert np.allclose(g[1:-3], r[1:-3], rtol=1e-9, atol=1e-9, equal_nan=True), (c, i, g[:14], r[:14])
            assert np.allclose(g[-3:], r[-3:], rtol=1e-7, atol=1e-9, equal_nan=True)
        moved += len(set(np.round(np.array(ref)[:, 2], 6)))
    assert moved > 3 * 20
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it)
    n_par = 8 if kind == "dd" else 6
    args = np.stack([snap["L"][c][:n_par] for c in range(C)])
    if kind == "dd":
        b, d, _, _ = ops.dd_rates(args, dt, 2, 2)
    else:
        b, d = ops.trend_rates(args, R["TREND"], False, False)
    lik = ops.bd_loglik_batch(ts, te, o, b, d, 2).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9), (lik, snap["likA"])
    eng.close()


@pytest.mark.parametrize("model", [1, 2, 3])
def test_cfg4_general_times_other_models_under_the_four_chain_kernel(model):
    """lr_persist4_kernel<136, true, false, false> (pair-general layout) under models 1, 2 and 3 at the bench size - 1024
    chains x 100k lineages on ARBITRARY fp64 times (bench.py's cfg4_general; model 0 is
    test_general_times_off_grid_against_the_oracle_at_size): the log-likelihood EVERY chain carries for its accepted state
    against (i) the oracle's fp64 per-lineage evaluation of that state on the raw times (models 1, 2; BDIx:124-146 form),
    (ii) the oracle's binned calc_likelihood on statistics binned from the same times - model 3 with its te < end_time
    death half (LRF:141-142, 529-546) -, (iii) lr_bd_loglik_batch (another kernel, fp64 fractions)."""
    from literate_amd import ops, synth
    from literate_amd.engine import ChainEngine
    from oracle import literate_oracle as lo
    rng = np.random.default_rng(7)
    n_lin, C, n_it = 100_000, 1024, 120
    ts, te, _ = synth.make_lineages(n_lin, n_bins=128, n_shifts=20, seed=0)
    ts = ts + rng.uniform(0.0, 1.0, n_lin) * 0.999
    te = np.maximum(np.ceil(te) - 1.0 + rng.uniform(1e-3, 0.999, n_lin), ts + 1e-3)
    eng = ChainEngine(ts, te, C, model=model, seed=2026, s_freq=10, n_trace_slots=n_it // 10, engine="persistent4")
    assert not eng.unit_resolution and eng.layout.table_mode == 2 and eng.layout.persistent == 2
    assert eng.kernel_name().startswith("lr_persist4_kernel<") and ", true, false, " in eng.kernel_name()
    eng.init(); eng.steps(n_it // 2); eng.steps(n_it - n_it // 2)
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it) and np.all(snap["accepted"] > 0) and np.all(np.isfinite(snap["likA"]))
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    stats = dict(sp=sp, ex=ex, br=br)
    if model == 3:
        stats["ex_dead"], stats["br_dead"] = lo.bin_events_dead(ts, te, te.max())
    lam, mu = _accepted_rates(snap, eng.n_bins, C)
    lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, model, br_length=br, end_time=eng.end_time).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9)
    pre = lo.lineage_bins(ts, te, float(t0), eng.n_bins)
    worst = 0.0
    for c in range(C):
        with np.errstate(all="ignore"):
            ref = lo.calc_likelihood(model, lam[c], mu[c], stats)
        worst = max(worst, abs(snap["likA"][c] - ref) / abs(ref))
        if model != 3 and c % 8 == 0:
            ref = lo.per_lineage_loglik(ts, te, float(t0), lam[c], mu[c], model, br, pre=pre)
            worst = max(worst, abs(snap["likA"][c] - ref) / abs(ref))
    assert worst < 1e-9, worst
    eng.close()


@pytest.mark.parametrize("n_lin,C", [(10_000, 256), (100_000, 1024), (30_000, 128)])
def test_planner_self_check_against_a_measurement(monkeypatch, n_lin, C):
    """LR_PLAN_CHECK=1 (ChainEngine.plan_check): the engine the planner picks from its fitted cost models, timed on THIS
    device against every other engine that accepts the configuration - cfg3, cfg4 and a cfg2-sized shape.  The report
    names the planner's kernel and every engine's time; the planner's choice must not lose to the best one by more than
    the check's own tolerance plus what boxes of the pool differ by."""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    ts, te, _ = synth.make_lineages(n_lin, n_bins=128 if n_lin != 30_000 else 32, n_shifts=20 if n_lin != 30_000 else 4, seed=0)
    monkeypatch.setenv("LR_PLAN_CHECK", "1")
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        eng = ChainEngine(ts, te, C, model=0, seed=3, s_freq=100, n_trace_slots=4)
    r = eng.plan_report
    eng.close()
    assert r is not None and r["auto"].startswith("lr_") and set(r["us_per_iter"]) == {"auto", "persistent4", "persistent2", "spec", "packed", "launch"}
    t = r["us_per_iter"]
    assert t["auto"] is not None and t["launch"] is not None and t[r["best"]] == min(v for k, v in t.items() if v is not None and k != "auto")
    # structure is asserted; the timing bound is a WARNING (a shared pool box can be slow for one of the two
    # measurements, and a red here would hide every test behind it under `pytest -x`)
    if t["auto"] > 1.25 * t[r["best"]]:
        warnings.warn("planner self-check: auto %.2f us against %s %.2f us per iteration (n_lin %d, C %d)"
                      % (t["auto"], r["best"], t[r["best"]], n_lin, C))
    assert t["auto"] <= 3.0 * t[r["best"]], r                 # (a wrong engine altogether still fails)
    assert r["ok"] == (not any("LR_PLAN_CHECK" in str(w.message) for w in caught))


_STREAM_RUN = {}


@pytest.mark.parametrize("C,model,general", [(2, 0, False), (5, 2, False), (24, 0, False), (70, 1, False),
                                             (3, 0, True), (12, 2, True), (38, 1, True),
                                             # (... in two partitions on their own streams, as long scans run: forced here)
                                             (24, 2, "parts"), (70, 0, "parts"), (38, 0, "general parts")])
def test_packed_scan_engine_against_the_scan_of_ts_te(C, model, general, monkeypatch):
    """The launch-based engine scanning the packed lineages (lr_packscan.hip: one launch scores every group against all
    chains, four chain pairs per block - here 1, 3, 12 and 35 pairs: one to nine pair groups, the last one ragged) against
    the same engine scanning ts / te: same proposals, same decisions, likelihoods to rounding (the packed form adds a
    group's lineages in another order), however the run is cut (resume: test_checkpoint_resume_is_bit_identical)."""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    parts = 1
    if isinstance(general, str):
        parts, general = 2, general.startswith("general")
        monkeypatch.setenv("LR_PACKED_PARTS", "2")
    ts, te, _ = synth.make_lineages(200_000, n_bins=100, n_shifts=12, seed=9)
    if general:
        # continuous times on the 2^-32 grid: the packed form's fixed-point fractions are exact there (pair-general tables,
        # three more 16-byte arrays per group: lr_packscan_kernel<.., true>)
        ts, te = _off_year_grid(ts, te, np.random.default_rng(2))
    runs = {}
    for engine in ("packed", "launch"):
        eng = ChainEngine(ts, te, C, model=model, seed=31, s_freq=1, n_trace_slots=120, engine=engine)
        assert eng.layout.persistent == 0 and eng.layout.packed_scan == (1 if engine == "packed" else 0) and eng.unit_resolution == (not general)
        if engine == "packed":
            # (never pipelined; one partition: the scans here are short - long ones run in two, on their own streams)
            assert eng.layout.n_parts == parts and eng.layout.pipelined == 0
            assert eng.kernel_name().startswith("lr_packscan_kernel<")
            assert eng.kernel_name().endswith("true>" if general else "false>") and eng.layout.table_mode == (2 if general else 1)
        eng.init()
        for n in (1, 50, 69):
            eng.steps(n)
        runs[engine] = (eng.trace_rows().copy(), eng.snapshot())
        eng.close()
    a, b = runs["packed"][0], runs["launch"][0]
    assert np.array_equal(a[:, :, 6:8], b[:, :, 6:8]) and np.array_equal(a[:, :, 0], b[:, :, 0])          # K_l, K_m: the same decisions
    # (likelihoods of +-5e6 built from terms 100 x larger; general times: the north star's 1e-9; the posterior = likelihood +
    # prior may cancel, so it is held to the likelihood's scale)
    rtol = 1e-9 if general else 1e-10
    assert np.allclose(a[:, :, 2:4], b[:, :, 2:4], rtol=rtol, atol=1e-9)
    assert np.all(np.abs(a[:, :, 1] - b[:, :, 1]) <= 1e-9 + rtol * (np.abs(b[:, :, 2]) + np.abs(b[:, :, 3])))
    assert np.allclose(np.nan_to_num(a[:, :, 13:]), np.nan_to_num(b[:, :, 13:]), rtol=1e-12)
    assert np.array_equal(runs["packed"][1]["accepted"], runs["launch"][1]["accepted"]) and runs["packed"][1]["accepted"].sum() > 10 * C


@pytest.mark.parametrize("cuts", [(1, 1, 1, 37), (40,), (7, 2, 31)])
@pytest.mark.parametrize("general", [False, True])
def test_streaming_kernel_equals_the_launches_however_a_run_is_cut(general, cuts):
    """The resident streaming kernel against the launch-based engine on the same plan (300k lineages x 8 chains, unit
    resolution and general times): trace rows, state rows and the pending proposal's lookup tables are identical bit for
    bit, whatever the calls' lengths - an odd one leaves the pending tables in the kernel's second buffer, from which
    they are copied back."""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    ts, te, _ = synth.make_lineages(300_000, n_bins=100, n_shifts=12, seed=5)
    if general:
        ts, te = _off_year_grid(ts, te, np.random.default_rng(3))
    runs = {}
    for engine in ("stream", "launch"):
        eng = ChainEngine(ts, te, 8, model=0, seed=77, s_freq=1, n_trace_slots=sum(cuts), engine=engine)
        assert eng.layout.persistent == 0 and eng.layout.streaming == (1 if engine == "stream" else 0)
        assert eng.kernel_name().startswith("lr_stream_kernel<8," if engine == "stream" else ("lr_scan_fast_kernel<8," if general else "lr_scan_unit_kernel<8,"))
        eng.init()
        for n in cuts:
            eng.steps(n)
        off, stride = int(eng.layout.tables), int(eng.layout.table_stride) * 16 * 8
        runs[engine] = (eng.trace_rows().copy(), eng.state_f64.cpu().numpy().copy(), eng.state_i32.cpu().numpy().copy(),
                        eng.workspace[off:off + stride].cpu().numpy().copy())
        eng.check_status()
        eng.close()
    for a, b in zip(runs["stream"], runs["launch"]):
        assert np.array_equal(a, b, equal_nan=True)
    assert len(set(np.round(runs["stream"][0][:, 0, 2], 6))) > 5      # the chain moved


@pytest.mark.parametrize("engine", ["stream", "launch", "auto"])
def test_launch_engine_streams_1e7_lineages_from_hbm(engine):
    """Few chains x very many lineages - 16 chains x 1e7 lineages: the planner picks the launch-based engine (a scan and a
    step kernel per iteration) and has its scan read the PACKED lineages (lr_packscan.hip: 11 MB per pass, all sixteen
    chains per group decode); engine="launch" keeps the scan of ts / te (160 MB in every iteration: the HBM-bound form),
    engine="stream" runs that plan's iterations inside the resident streaming kernel (lr_stream.hip: opt-in, measured no
    faster) - those two must give the same run bit for bit, the packed scan the same run to rounding.  Two chains row by row
    against the oracle loop on statistics binned from the same lineages, and every chain's accepted state re-evaluated by
    lr_bd_loglik_batch and by the oracle's binned calc_likelihood."""
    import torch
    from literate_amd import ops, synth
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    from oracle import mcmc_oracle as mo
    ts0, te0, _ = synth.make_lineages(100_000, n_bins=128, n_shifts=20, seed=0)
    reps, C, n_it, seed = 100, 16, 60, 2026
    ts, te = np.tile(ts0, reps), np.tile(te0, reps)
    eng = ChainEngine(ts, te, C, model=0, seed=seed, s_freq=1, n_trace_slots=n_it, engine=engine)
    assert eng.layout.persistent == 0 and eng.unit_resolution
    assert eng.kernel_name().startswith({"stream": "lr_stream_kernel<16,", "launch": "lr_scan_unit_kernel<16,", "auto": "lr_packscan_kernel<4, 136, false>"}[engine])
    assert eng.layout.streaming == (1 if engine == "stream" else 0) and eng.layout.packed_scan == (1 if engine == "auto" else 0)
    eng.init(); eng.steps(25); eng.steps(n_it - 25)      # (an odd cut: the pending tables change buffers in the streaming kernel)
    tr = eng.trace_rows()
    if engine == "stream":
        _STREAM_RUN["trace"], _STREAM_RUN["state"] = tr.copy(), eng.state_f64.cpu().numpy().copy()
    elif engine == "launch" and "trace" in _STREAM_RUN:
        assert np.array_equal(tr, _STREAM_RUN["trace"], equal_nan=True) and np.array_equal(eng.state_f64.cpu().numpy(), _STREAM_RUN["state"], equal_nan=True)
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it) and np.all(np.isfinite(snap["likA"]))
    # the statistics of the tiled data are `reps` times those of one copy (exact: integer counts, half-integer lineage-time)
    t0, sp, ex, br = lo.bin_events_cli(ts0, te0)
    stats = dict(sp=sp * reps, ex=ex * reps, br=br * reps)
    assert np.array_equal(eng.sp_events.cpu().numpy(), stats["sp"]) and np.array_equal(eng.br_length.cpu().numpy(), stats["br"])
    lam, mu = _accepted_rates(snap, eng.n_bins, C)
    lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, 0, br_length=stats["br"]).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9)
    for c in range(C):
        with np.errstate(all="ignore"):
            assert lo.calc_likelihood(0, lam[c], mu[c], stats) == pytest.approx(snap["likA"][c], rel=1e-9)
    for c in (0, 15):
        with np.errstate(all="ignore"):
            ref = mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=0), mo.PhiloxDraws(seed, c), n_it, 1, k_max=32)
        for i in range(n_it):
            head, s_row, e_row = split_trace_row(tr[i, c])
            assert np.allclose(head[:13], ref["mcmc"][i][:13], rtol=1e-9, atol=1e-9), (c, i, head[:6], ref["mcmc"][i][:6])
    eng.close()
    torch.cuda.empty_cache()
