"""The chain engine's kernel-choice map as the tests see it.

The planner (csrc/lr_plan.hip: lr_plan_engine, lr_persist_family, lr_packscan_planned; csrc/lr_loglik.hip:
lr_plan_scan) picks one of five kernel families for a configuration, each compiled for a fixed set of table
half-strides H.  A CELL is (family, H, general, param, extant):

  family   "launch" (the launch-based scans of ts / te), "packed" (lr_packscan_kernel), "persist2" (lr_persist_kernel),
           "persist4" (lr_persist4_kernel), "spec" (lr_spec_kernel)
  H        the table half-stride the kernel is instantiated for (0: the generic launch-based scan, no class)
  general  the kernel reads general-time tables (table_mode 0 or 2) rather than unit-resolution ones (table_mode 1)
  param    a parametric sampler (DDRate, trend_rate) drives the chains instead of the RJ sampler
  extant   model 3: the tables carry the extant block behind the death-side entries

The class rules below restate the code; tests/test_planner_map.py checks the planner against them over a grid of
configurations and derives the cell list from it, and tests/test_hip_edges.py runs every cell against the oracle.
"""
import ctypes as C
import functools
import os
import re

import numpy as np

FAST_H = (40, 72, 136, 264)       # lr_plan_scan's table classes (launch-based scans, every persistent kernel)
H_WIDE = 520                      # LR_H_WIDE: persistent kernels and the packed scan only
ENGINES = {"auto": 0, "launch": 1, "persistent": 2, "persistent4": 3, "persistent2": 4, "spec": 5, "stream": 6, "packed": 7}
FAMILY = {1: "persist2", 2: "persist4", 3: "spec"}
PARAM_MAX_BINS = 256              # lr_check_cfg: LR_DD_MAXP (4) bins per lane x 64 lanes for the parametric samplers


def bins_per_lane(h):
    """lr_bins_per_lane (csrc/lr_device.h)."""
    return 1 if h <= 40 else (2 if h <= 136 else (4 if h <= 264 else 8))


def launch_class(model, n_bins):
    """H of lr_plan_scan's one-class fast path, None for the generic scan: models 0-2 only, n_bins + 2 <= H and at most
    64 lanes x bins_per_lane(H) bins."""
    if model == 3:
        return None
    for h in FAST_H:
        if n_bins + 2 <= h and n_bins <= 64 * bins_per_lane(h):
            return h
    return None


def table_class(model, n_bins):
    """H of the pair tables the persistent kernels and the packed scan read, None where there is none (lr_plan_engine):
    model 3 keeps an extant block behind the death-side entries, so its class needs 2 (n_bins + 2) <= H; models 0-2 take
    the launch class or, above it, H = 520 up to 64 x 8 bins."""
    if model == 3:
        for h in FAST_H + (H_WIDE,):
            if 2 * (n_bins + 2) <= h:
                return h
        return None
    h = launch_class(model, n_bins)
    if h is None and n_bins + 2 <= H_WIDE and n_bins <= 64 * bins_per_lane(H_WIDE):
        h = H_WIDE
    return h


def persistent_capacity(model, sampler):
    """The most bins any persistent kernel takes: the top of the largest class (model 3: 2 (n + 2) <= 520 -> 258; models
    0-2: 64 lanes x 8 bins = 512 <= 520 - 2); the parametric samplers are refused above 256 bins altogether."""
    if sampler != 0:
        return PARAM_MAX_BINS
    return max(n for n in range(1, 1100) if table_class(model, n) is not None)


def class_edges(model, sampler):
    """Bin counts on both sides of every class edge (the top of a class and one bin more)."""
    top = []
    prev = table_class(model, 1)
    for n in range(2, 1100):
        h = table_class(model, n)
        if h != prev:
            top.append(n - 1)
            prev = h
        if h is None:
            break
    out = sorted(set([t for t in top] + [t + 1 for t in top]))
    if sampler != 0:
        out = [n for n in out if n <= PARAM_MAX_BINS]
    return out


def spec_max_h(general):
    """lr_spec_kernel is instantiated for H <= 264 on unit-resolution tables, H <= 136 on pair-general ones."""
    return 136 if general else 264


def engine_runs(engine, model, sampler, unit, n_bins):
    """Whether a FORCED engine runs the configuration as that engine (the mirror of lr_persist_family /
    lr_packscan_eligible at 37 chains); the GPU tests assert the layout agrees."""
    h = table_class(model, n_bins)
    if sampler != 0 and n_bins > PARAM_MAX_BINS:
        return False
    if engine in ("auto", "launch"):
        return True
    if h is None:
        return False
    if engine == "persistent2":
        return unit
    if engine == "spec":
        return h <= spec_max_h(not unit)
    return engine in ("persistent4", "packed")


def make_config(model, sampler, unit, n_bins, n_chains, n_lineages, engine_mode, frac_birth=0.0, frac_death=0.5, team=0,
                chains_per_team=0):
    """(frac_birth, frac_death): the shared in-bin fractions of unit-resolution data, (0, 0.5) for year-resolution input with
    the default death_jitter; general times carry none.  (team, chains_per_team): ChainEngine's request for the
    speculative kernel's team of blocks and its chains per team, 0 = the planner's choice."""
    from literate_amd import _hip
    end = float(n_bins) + 0.5
    return _hip.McmcConfig(
        n_lineages=int(n_lineages), n_bins=int(n_bins), n_chains=int(n_chains), model=int(model), use_rate_HP=1,
        s_freq=10, n_trace_slots=4, update_fraction=0.75, t0=0.0, start_time=0.0, end_time=end, seed=1,
        unit_resolution=int(unit), engine_mode=int(engine_mode), frac_birth=float(frac_birth) if unit else 0.0,
        frac_death=float(frac_death) if unit else 0.0, sampler=int(sampler), m_birth=2 if sampler == 1 else 0,
        m_death=2 if sampler == 1 else 0, team_request=int(team) | (int(chains_per_team) << 8),
        dd_present=end if sampler == 1 else 0.0, dd_init_death=0.1)


def query(model, sampler, unit, n_bins, n_chains, n_lineages, engine_mode, cus=256, frac_birth=0.0, frac_death=0.5, team=0,
          chains_per_team=0):
    """lr_mcmc_query_layout on the host (no device needed), LR_DEVICE_CUS pinned: (rc, layout)."""
    from literate_amd import _hip
    lib = _hip.load()
    cfg = make_config(model, sampler, unit, n_bins, n_chains, n_lineages, engine_mode, frac_birth, frac_death, team,
                      chains_per_team)
    lay = _hip.McmcLayout()
    old = os.environ.get("LR_DEVICE_CUS")
    os.environ["LR_DEVICE_CUS"] = str(cus)
    try:
        return lib.lr_mcmc_query_layout(C.byref(cfg), C.byref(lay)), lay
    finally:
        if old is None:
            os.environ.pop("LR_DEVICE_CUS", None)
        else:
            os.environ["LR_DEVICE_CUS"] = old


def layout_cell(model, sampler, n_bins, lay):
    """The cell a successful layout names."""
    param, extant = sampler != 0, model == 3
    if lay.persistent or lay.packed_scan:
        family = FAMILY[lay.persistent] if lay.persistent else "packed"
        general = lay.table_mode == 2
        return (family, lay.table_stride // (2 if general else 1), general, param, extant)
    return ("launch", launch_class(model, n_bins) or 0, lay.table_mode != 1, param, extant)


def kernel_cell(name, model, sampler):
    """The cell of a kernel name as ChainEngine.kernel_name() prints it."""
    m = re.fullmatch(r"(\w+)<([^>]*)>", name)
    assert m, name
    kern, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    param, extant = sampler != 0, model == 3
    if kern == "lr_spec_kernel":
        assert (args[2] == "false") == param, name
        return ("spec", int(args[0]), args[3] == "true", param, extant)
    if kern == "lr_persist4_kernel":
        assert (args[2] == "true") == param, name
        return ("persist4", int(args[0]), args[1] == "true", param, extant)
    if kern == "lr_persist_kernel":
        return ("persist2", int(args[0]), False, param, extant)
    if kern == "lr_packscan_kernel":
        return ("packed", int(args[1]), args[2] == "true", param, extant)
    if kern in ("lr_stream_kernel", "lr_fused_iter_kernel"):
        return ("launch", int(args[1]), args[2] == "false", param, extant)
    if kern == "lr_scan_wide_kernel":
        return ("launch", int(args[0]), True, param, extant)
    if kern in ("lr_scan_unit_kernel", "lr_scan_fast_kernel"):
        return ("launch", int(args[1]), kern == "lr_scan_fast_kernel", param, extant)
    if kern == "lr_scan_kernel":
        return ("launch", 0, True, param, extant)
    raise AssertionError("unknown kernel %r" % name)


GRID_CHAINS = (3, 10, 37, 128, 1024)
GRID_LINEAGES = (4000, 1_000_000)


def grid():
    """(model, sampler, unit, n_bins, n_chains, n_lineages, engine_mode) of the planner-map grid: every model under the RJ
    sampler, the two parametric samplers (model 2), unit and general times, both sides of every class edge."""
    for model, sampler in [(0, 0), (1, 0), (2, 0), (3, 0), (2, 1), (2, 2)]:
        bins = class_edges(model, sampler)
        if sampler != 0:
            bins = bins + [PARAM_MAX_BINS + 1]          # refused: the limit of the parametric samplers
        for unit in (True, False):
            for n_bins in bins:
                for c in GRID_CHAINS:
                    for n in GRID_LINEAGES:
                        for mode in ENGINES.values():
                            yield model, sampler, unit, n_bins, c, n, mode


def planner_cells():
    """Every cell a configuration of the grid is planned into."""
    cells = set()
    for model, sampler, unit, n_bins, c, n, mode in grid():
        rc, lay = query(model, sampler, unit, n_bins, c, n, mode)
        if rc == 0:
            cells.add(layout_cell(model, sampler, n_bins, lay))
    return cells


def accepted_rates(snap, n_bins, C):
    """Per-bin birth / death rates of every chain's accepted RJ state (a snapshot of ChainEngine)."""
    from oracle import literate_oracle as lo
    lam = np.stack([snap["L"][c][lo.get_rate_index(np.floor(snap["tL"][c]), n_bins)] for c in range(C)])
    mu = np.stack([snap["M"][c][lo.get_rate_index(np.floor(snap["tM"][c]), n_bins)] for c in range(C)])
    return lam, mu


def instantiated(cell):
    """Whether a kernel exists for the cell (the H switches of lr_launch_persistent / lr_spec.hip / lr_packscan.hip and
    the launch-based scans)."""
    family, H, general, param, extant = cell
    if family == "launch":
        # the fast launch-based scans exist for one-class tables; model 3 and wider tables take the generic scan
        return (H in FAST_H and not extant) or (H == 0 and general and not param)
    if H not in FAST_H + (H_WIDE,) or (param and H > 264):
        return False
    if family == "persist2":
        return not general
    if family == "spec":
        return H <= spec_max_h(general)
    return family in ("packed", "persist4")


def instantiated_cells():
    """Every cell a kernel exists for, over the classes the models and samplers reach."""
    out = set()
    for param, extant in [(False, False), (False, True), (True, False)]:
        for family in ("launch", "packed", "persist2", "persist4", "spec"):
            for H in (0,) + FAST_H + (H_WIDE,):
                for general in (False, True):
                    cell = (family, H, general, param, extant)
                    if instantiated(cell):
                        out.add(cell)
    return out


# ---- shared by the oracle comparisons of tests/test_hip_edges.py and tests/test_hip_shared_fractions.py ----------------
ORACLE_CHAINS = (0, 18, 36)       # of 37 chains: the first, a middle one, the ragged last block's


def placed_lineages(n, rng):
    """The lineages placed on purpose on n unit bins, as (birth year, death year) integer pairs - a lineage is born at its
    birth year and dies `death_jitter` after its death year: one over the whole window, born in bin 0 and in the last
    bin, dying in the last bin, 20 extant ones (model 3's extant block), a run of 21 lineages in one birth bin (its groups
    split), and pairs dying d = 0..3 bins apart in the top bins (the largest 16-bit slot offsets of csrc/lr_pack.hip).
    Draws 40 integers from rng."""
    b = rng.integers(0, n, 40)
    extra = [(0, n), (0, 0), (0, n - 1), (n - 1, n - 1), (n - 1, n)]
    extra += [(int(x), n) for x in b[:20]]                                # extant
    extra += [(int(x), n - 1) for x in b[20:]]                            # dying in the last bin
    r = n // 2
    extra += [(r, min(r + (k % 3), n - 1)) for k in range(21)]            # one birth bin, 21 lineages
    top = max(0, n - 8)
    for d in range(4):                                                    # pairs dying d bins apart in the top bins
        extra += [(top, n - 1 - d), (top, n - 1)] * 2
    return extra


def _grid(x, exact):
    return np.round(x * 2.0 ** 32) / 2.0 ** 32 if exact else x


@functools.lru_cache(maxsize=None)
def lineages(n_bins, general, exact=True, n=3000):
    """n synthetic lineages on [0, n_bins + 0.5] (unit resolution: integer births, deaths at .5) plus the placed ones; on
    general times births and deaths move inside their bins (the pinned first birth and the extant lineages stay, so the
    window stays n_bins), on the 2^-32 grid when `exact`."""
    from literate_amd import synth
    nb = int(n_bins)
    ts, te, _ = synth.make_lineages(int(n), n_bins=nb, n_shifts=3, seed=nb + 1000 * general)
    rng = np.random.default_rng(nb)
    extra = [(float(s), k + 0.5) for s, k in placed_lineages(nb, rng)]
    ts = np.concatenate([ts, [s for s, _ in extra]])
    te = np.concatenate([te, [e for _, e in extra]])
    if general:
        keep_s, keep_e = ts == ts.min(), te >= te.max()
        ts = np.where(keep_s, ts, ts + _grid(rng.uniform(0.0, 0.45, len(ts)), exact))
        te = np.where(keep_e, te, te + _grid(rng.uniform(0.0, 0.45, len(te)), exact))
    assert ts.min() == 0.0 and te.max() == nb + 0.5 and np.all(te > ts)
    return ts, te


def rj_stats(ts, te, model, n_bins):
    """Binned statistics of the data (the oracle's own binning)."""
    from oracle import literate_oracle as lo
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    assert t0 == 0 and len(sp) == n_bins
    stats = dict(sp=sp, ex=ex, br=br)
    if model == 3:
        stats["ex_dead"], stats["br_dead"] = lo.bin_events_dead(ts, te, te.max())
    return stats


def rj_trajectory(stats, ts, te, model, seed, n_it, chain):
    """The oracle's sampled rows of one chain, by its GLOBAL id (the draws are keyed by it)."""
    from oracle import mcmc_oracle as mo
    with np.errstate(all="ignore"):
        return mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=model), mo.PhiloxDraws(seed, chain), n_it, 1,
                           k_max=32)["mcmc"]


def rj_reference(ts, te, model, n_bins, seed, n_it, chains=ORACLE_CHAINS):
    """Binned statistics of the data (the oracle's own binning) and the oracle trajectories of `chains`."""
    stats = rj_stats(ts, te, model, n_bins)
    return stats, {c: rj_trajectory(stats, ts, te, model, seed, n_it, c) for c in chains}


def check_forced(engine, cell):
    want = {"packed": "packed", "persistent2": "persist2", "persistent4": "persist4", "spec": "spec"}.get(engine)
    if want:
        assert cell[0] == want, (engine, cell)
    if engine == "launch":
        assert cell[0] == "launch", cell


def reference_loglik(ts, te, lam, mu, model, stats, pre):
    """fp64 log-likelihood of one accepted state on the raw times: the per-lineage form (models 0-2) or the binned
    Keiding form with the death half on the lineages that die in the window (model 3)."""
    from oracle import literate_oracle as lo
    if model == 3:
        return lo.calc_likelihood(3, lam, mu, stats)
    return lo.per_lineage_loglik(ts, te, 0.0, lam, mu, model, stats["br"], pre=pre)


def check_rj_rows(tr, refs, n_it, cell):
    """Trace rows [samples, chains, LR_TRACE_W] against the oracle rows refs = {chain's index in tr: rows}: iteration
    and K columns exact, the head at rtol = atol = 1e-9."""
    from literate_amd.engine import split_trace_row
    for c, ref in refs.items():
        for i in range(n_it):
            head, _, _ = split_trace_row(tr[i, c])
            r = ref[i]
            assert head[0] == r[0] and head[6] == r[6] and head[7] == r[7], (cell, c, i, head[:8], r[:8])
            assert np.allclose(head[:13], r[:13], rtol=1e-9, atol=1e-9), (cell, c, i, head, r)


def check_rj_states(snap, ts, te, model, n_bins, stats, n_it, cell, pre=None):
    """Every chain of a snapshot: n_it iterations done, a finite log-likelihood, and that log-likelihood equal to the fp64
    oracle's for the chain's accepted state on the raw times (rtol 1e-9).  Returns the states' per-bin rates."""
    from oracle import literate_oracle as lo
    C = len(snap["likA"])
    assert np.all(snap["it"] == n_it) and np.all(np.isfinite(snap["likA"]))
    lam, mu = accepted_rates(snap, n_bins, C)
    if pre is None:
        pre = lo.lineage_bins(ts, te, 0.0, n_bins)
    ref = np.array([reference_loglik(ts, te, lam[c], mu[c], model, stats, pre) for c in range(C)])
    assert np.allclose(snap["likA"], ref, rtol=1e-9, atol=0.0), (cell, snap["likA"] - ref)
    return lam, mu


def rescore_rj_on_device(eng, snap, lam, mu, model, stats, cell):
    """Every chain's accepted state (its per-bin rates lam, mu) re-scored by lr_bd_loglik_batch on the engine's lineages."""
    from literate_amd import ops
    lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, model, br_length=stats["br"],
                              end_time=eng.end_time).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9, atol=0.0), (cell, lik - snap["likA"])


def run_rj_against_the_oracle(eng, ts, te, model, n_bins, stats, refs, n_it, cell):
    """n_it iterations of an RJ engine (s_freq 1) in two launches: the chains of refs ({the chain's index in the engine:
    its oracle rows}, rj_reference / rj_trajectory) row by row against oracle/mcmc_oracle.run_mcmc (iteration and K
    columns exact, the head at rtol = atol = 1e-9), and every chain's accepted state re-scored in fp64 by the oracle on
    the raw times and by lr_bd_loglik_batch (rtol 1e-9)."""
    eng.init()
    eng.steps(n_it // 2)
    eng.steps(n_it - n_it // 2)
    check_rj_rows(eng.trace_rows(), refs, n_it, cell)
    snap = eng.snapshot()
    lam, mu = check_rj_states(snap, ts, te, model, n_bins, stats, n_it, cell)
    rescore_rj_on_device(eng, snap, lam, mu, model, stats, cell)
    return snap


def fixed_point_bound(ts, te, lam, mu):
    """Absolute bound of the pair-general tables' 32-bit in-bin fractions (csrc/lr_pack.hip), for one chain's state:
    a birth fraction is rounded to the nearest 2^-32 (its group carries their exact sum: <= 2^-33 per lineage); a death
    fraction likewise, but a PAIR carries the rounded mean of its two rounded fractions, which the doubled slope turns
    back into their sum (<= 2^-33 + 2^-33 per lineage).  Each fraction multiplies the exposure rate of its bin, at most
    (lambda + mu)max, so |error| <= 3 * 2^-33 * N * (lambda + mu)max, plus 64 ulp of the sum of |terms| for the fp64
    summation order (1 % of the bound at these sizes)."""
    R = float(np.max(lam + mu))
    cum = float(np.sum(lam + mu))
    terms = len(ts) * (np.max(np.abs(np.log(np.concatenate([lam, mu])))) + 2 * cum + 2 * R + 10.0)
    return 3.0 * 2.0 ** -33 * len(ts) * R + 64 * 2.0 ** -52 * terms


def param_stats(kind, ts, te, n_bins):
    """create_bins statistics of the lineages and (trend) the covariate, binned by the oracle's own create_bins."""
    from oracle import literate_oracle as lo
    origin, present = float(ts.min()), float(te.max())
    o, p, nsp, nex, dt, nb, t_range = lo.create_bins(origin, present, ts, te, 0)
    assert nb == n_bins
    trend = None
    if kind == "trend":
        x = np.arange(n_bins + 1, dtype=float)
        trend = lo.normalise_trend(np.sin(x / 7.0) + 0.02 * x)
        assert len(trend) == n_bins
    return (o, p, nsp, nex, dt, t_range), trend


def param_reference(kind, bins, trend, n_it, s, seed, off, chains=ORACLE_CHAINS):
    """The oracle loops of the parametric samplers (DDRate -mBirth 2 -mDeath 2, trend_rate) for `chains` (indices in an
    engine created with chain_offset = off: the draws are keyed by off + index)."""
    from oracle import dd_mcmc_oracle as ddo
    from oracle import trend_mcmc_oracle as tro
    o, p, nsp, nex, dt, t_range = bins
    with np.errstate(all="ignore"):
        emp = (nsp / dt, nex / dt)
    refs = {}
    for c in chains:
        if kind == "dd":
            refs[c] = ddo.run_dd_mcmc(nsp, nex, dt, t_range, o, p, 2, 2, ddo.PhiloxDraws(seed, off + c), n_it, s, emp=emp)
        else:
            refs[c] = tro.run_trend_mcmc(nsp, nex, dt, trend, tro.PhiloxDraws(seed, off + c), n_it, s, False, False, emp=emp)
    return emp, refs


def param_engine(kind, ts, te, trend, n_chains, engine, seed, s, n_slots, off):
    from literate_amd.ddrate import DDRateEngine
    from literate_amd.trendrate import TrendRateEngine
    origin, present = float(ts.min()), float(te.max())
    kw = dict(seed=seed, s_freq=s, n_trace_slots=n_slots, chain_offset=off, engine=engine)
    if kind == "dd":
        return DDRateEngine(ts, te, origin, present, n_chains, m_birth=2, m_death=2, **kw)
    return TrendRateEngine(ts, te, origin, present, trend, n_chains, **kw)


def param_rates(kind, snap, dt, trend, n_chains):
    from literate_amd import ops
    if kind == "dd":
        args = np.stack([snap["L"][c][:8] for c in range(n_chains)])
        b, d, _, _ = ops.dd_rates(args, dt, 2, 2)
    else:
        args = np.stack([snap["L"][c][:6] for c in range(n_chains)])
        b, d = ops.trend_rates(args, trend, False, False)
    return [x.cpu().numpy() for x in (b, d)]


def check_param_rows(got, ref, n_rows, cell, c):
    """One chain's log rows against the oracle's: the iteration column exact, 1e-9 on the rest and 1e-7 on the last three
    (adequacy) columns - the tolerances of test_ddrate_sampler_follows_oracle."""
    assert len(got) == len(ref) == n_rows
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0]
        assert np.allclose(g[1:-3], r[1:-3], rtol=1e-9, atol=1e-9, equal_nan=True), (cell, c, i, g[:14], r[:14])
        assert np.allclose(g[-3:], r[-3:], rtol=1e-7, atol=1e-9, equal_nan=True)


def rescore_param_on_device(eng, kind, snap, ts, te, bins, trend, cell):
    """Every chain's accepted parameter vector re-scored by lr_bd_loglik_batch on the raw times."""
    from literate_amd import ops
    o, p, nsp, nex, dt, t_range = bins
    b, d = param_rates(kind, snap, dt, trend, eng.n_chains)
    lik = ops.bd_loglik_batch(ts, te, o, b, d, 2).cpu().numpy()
    assert np.allclose(lik, snap["likA"], rtol=1e-9), (cell, lik - snap["likA"])


def run_param_against_the_oracle(eng, kind, ts, te, bins, trend, emp, refs, n_it, s, cell, chains=ORACLE_CHAINS):
    """n_it iterations of a parametric engine in two launches: the sampled log rows of `chains` (scalars and per-bin
    columns) against the oracle loops with the tolerances of test_ddrate_sampler_follows_oracle, and every chain's
    accepted parameter vector re-scored by lr_bd_loglik_batch."""
    o, p, nsp, nex, dt, t_range = bins
    assert np.array_equal(eng.n_spec, nsp) and np.array_equal(eng.n_exti, nex) and np.allclose(eng.DT, dt, rtol=1e-13)
    eng.init()
    eng.steps(n_it // 2)
    eng.steps(n_it - n_it // 2)
    tr = eng.trace_rows()
    for c in chains:
        check_param_rows(eng.log_rows_from(tr[:, c], emp=emp), refs[c], n_it // s, cell, c)
    snap = eng.snapshot()
    assert np.all(snap["it"] == n_it)
    rescore_param_on_device(eng, kind, snap, ts, te, bins, trend, cell)
    return snap
