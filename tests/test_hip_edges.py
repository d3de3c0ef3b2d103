"""Every kernel cell the planner can select (tests/helpers/edges.py: family x table class H x general x parametric x
model-3 extant block), run at the bin counts on both sides of its class edge against the oracle loops fed the same
Philox draws.

The data: a few thousand synthetic lineages with a window pinned to n_bins, plus lineages placed on purpose - born in
bin 0 and in the last bin, dying in the last bin, extant ones (model 3's extant block), a run of more than 14 lineages in
one birth bin (its groups split), and pairs dying d = 0..3 bins apart in the top bins (the largest 16-bit slot offsets of
csrc/lr_pack.hip).  37 chains leave the last block of every kernel ragged.  The last test checks that the kernels the
cases ran are exactly the planner's cell list, so a new instantiation without an oracle comparison fails the suite."""
import functools

import numpy as np
import pytest

from helpers import edges as E

pytestmark = pytest.mark.gpu

N_IT, C, SEED = 120, 37, 4242
ORACLE_CHAINS = (0, 18, 36)
RAN = {}                                     # cell -> test ids that ran it against the oracle
RJ_ENGINES = ("auto", "launch", "packed", "persistent2", "persistent4", "spec")


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: no ROCm device visible")


def _grid(x, exact):
    return np.round(x * 2.0 ** 32) / 2.0 ** 32 if exact else x


@functools.lru_cache(maxsize=None)
def _lineages(n_bins, general, exact=True):
    """Synthetic lineages on [0, n_bins + 0.5] (unit resolution: integer births, deaths at .5) plus the placed ones; on
    general times births and deaths move inside their bins (the pinned first birth and the extant lineages stay, so the
    window stays n_bins), on the 2^-32 grid when `exact`."""
    from literate_amd import synth
    n = int(n_bins)
    ts, te, _ = synth.make_lineages(3000, n_bins=n, n_shifts=3, seed=n + 1000 * general)
    rng = np.random.default_rng(n)
    b = rng.integers(0, n, 40)
    extra = [(0.0, n + 0.5), (0.0, 0.5), (0.0, n - 0.5), (n - 1.0, n - 0.5), (n - 1.0, n + 0.5)]
    extra += [(float(x), n + 0.5) for x in b[:20]]                        # extant
    extra += [(float(x), n - 0.5) for x in b[20:]]                        # dying in the last bin
    r = n // 2
    extra += [(float(r), min(r + 0.5 + (k % 3), n - 0.5)) for k in range(21)]     # one birth bin, 21 lineages
    top = max(0, n - 8)
    for d in range(4):                                                    # pairs dying d bins apart in the top bins
        extra += [(float(top), n - 0.5 - d), (float(top), n - 0.5)] * 2
    ts = np.concatenate([ts, [s for s, _ in extra]])
    te = np.concatenate([te, [e for _, e in extra]])
    if general:
        keep_s, keep_e = ts == ts.min(), te >= te.max()
        ts = np.where(keep_s, ts, ts + _grid(rng.uniform(0.0, 0.45, len(ts)), exact))
        te = np.where(keep_e, te, te + _grid(rng.uniform(0.0, 0.45, len(te)), exact))
    assert ts.min() == 0.0 and te.max() == n + 0.5 and np.all(te > ts)
    return ts, te


@functools.lru_cache(maxsize=None)
def _rj_reference(model, n_bins, general):
    """Binned statistics of the data (the oracle's own binning) and the oracle trajectories of ORACLE_CHAINS."""
    from oracle import literate_oracle as lo
    from oracle import mcmc_oracle as mo
    ts, te = _lineages(n_bins, general)
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    assert t0 == 0 and len(sp) == n_bins
    stats = dict(sp=sp, ex=ex, br=br)
    if model == 3:
        stats["ex_dead"], stats["br_dead"] = lo.bin_events_dead(ts, te, te.max())
    refs = {}
    for c in ORACLE_CHAINS:
        with np.errstate(all="ignore"):
            refs[c] = mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=model), mo.PhiloxDraws(SEED, c), N_IT, 1,
                                  k_max=32)["mcmc"]
    return stats, refs


def _check_forced(eng, engine, cell):
    want = {"packed": "packed", "persistent2": "persist2", "persistent4": "persist4", "spec": "spec"}.get(engine)
    if want:
        assert cell[0] == want, (engine, cell)
    if engine == "launch":
        assert cell[0] == "launch", cell


def _record(cell, request):
    RAN.setdefault(cell, []).append(request.node.name)


def _reference_loglik(ts, te, lam, mu, model, stats, pre):
    """fp64 log-likelihood of one accepted state on the raw times: the per-lineage form (models 0-2) or the binned
    Keiding form with the death half on the lineages that die in the window (model 3)."""
    from oracle import literate_oracle as lo
    if model == 3:
        return lo.calc_likelihood(3, lam, mu, stats)
    return lo.per_lineage_loglik(ts, te, 0.0, lam, mu, model, stats["br"], pre=pre)


def _rj_cases():
    out = []
    for model in (0, 1, 2, 3):
        engines = RJ_ENGINES if model in (0, 3) else ("auto", "persistent4", "spec")
        for n_bins in E.class_edges(model, 0):
            for general in (False, True):
                for engine in engines:
                    if E.engine_runs(engine, model, 0, not general, n_bins):
                        out.append(pytest.param(model, n_bins, general, engine,
                                                id="m%d-%d-%s-%s" % (model, n_bins, "gen" if general else "unit", engine)))
    return out


@pytest.mark.parametrize("model,n_bins,general,engine", _rj_cases())
def test_rj_sampler_at_the_class_edges(model, n_bins, general, engine, request):
    """The RJ sampler, models 0-3, at both sides of every class edge (model 3 at full capacity, 2 (n_bins + 2) == H, and
    one bin above), unit and general times (jitter on the 2^-32 grid: decisions must equal the oracle's), every engine
    the cell runs: three chains row by row against oracle/mcmc_oracle.run_mcmc (iteration and K columns exact, the head
    at rtol = atol = 1e-9), and every chain's accepted state re-scored in fp64 by the oracle (per lineage for models 0-2,
    binned with the death half on the dead lineages for model 3) and by lr_bd_loglik_batch."""
    _gpu()
    from literate_amd import ops
    from literate_amd.engine import ChainEngine, split_trace_row
    from oracle import literate_oracle as lo
    ts, te = _lineages(n_bins, general)
    stats, refs = _rj_reference(model, n_bins, general)
    eng = ChainEngine(ts, te, C, model=model, seed=SEED, s_freq=1, n_trace_slots=N_IT, engine=engine)
    try:
        assert eng.n_bins == n_bins and eng.unit_resolution == (not general)
        cell = E.kernel_cell(eng.kernel_name(), model, 0)
        assert cell == E.layout_cell(model, 0, n_bins, eng.layout), (eng.kernel_name(), cell)
        _check_forced(eng, engine, cell)
        eng.init()
        eng.steps(N_IT // 2)
        eng.steps(N_IT - N_IT // 2)
        tr = eng.trace_rows()
        for c in ORACLE_CHAINS:
            ref = refs[c]
            for i in range(N_IT):
                head, _, _ = split_trace_row(tr[i, c])
                r = ref[i]
                assert head[0] == r[0] and head[6] == r[6] and head[7] == r[7], (cell, c, i, head[:8], r[:8])
                assert np.allclose(head[:13], r[:13], rtol=1e-9, atol=1e-9), (cell, c, i, head, r)
        snap = eng.snapshot()
        assert np.all(snap["it"] == N_IT) and np.all(np.isfinite(snap["likA"]))
        lam, mu = E.accepted_rates(snap, n_bins, C)
        pre = lo.lineage_bins(ts, te, 0.0, n_bins)
        ref = np.array([_reference_loglik(ts, te, lam[c], mu[c], model, stats, pre) for c in range(C)])
        assert np.allclose(snap["likA"], ref, rtol=1e-9, atol=0.0), (cell, snap["likA"] - ref)
        lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, model, br_length=stats["br"],
                                  end_time=eng.end_time).cpu().numpy()
        assert np.allclose(lik, snap["likA"], rtol=1e-9, atol=0.0), (cell, lik - snap["likA"])
        _record(cell, request)
    finally:
        eng.close()


def _fixed_point_bound(ts, te, lam, mu):
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


def _off_grid_cases():
    out = []
    for model in (0, 1, 2, 3):
        for n_bins in E.class_edges(model, 0):
            h = E.table_class(model, n_bins)
            for engine in ("packed", "persistent4", "spec"):
                if h is None or not E.engine_runs(engine, model, 0, False, n_bins):
                    continue
                # one off-grid case per table-mode-2 cell: the top of each class, model 1 / 2 on the four-chain kernel
                if (model in (1, 2) and engine != "persistent4") or E.table_class(model, n_bins + 1) == h:
                    continue
                out.append(pytest.param(model, n_bins, engine, id="m%d-%d-%s" % (model, n_bins, engine)))
    return out


@pytest.mark.parametrize("model,n_bins,engine", _off_grid_cases())
def test_general_times_off_grid_within_the_fixed_point_bound(model, n_bins, engine, request):
    """Jitter OFF the 2^-32 grid in every table-mode-2 cell: the log-likelihood every chain carries for its accepted
    state against the fp64 oracle of that state on the raw times, within the ABSOLUTE bound of the 32-bit fixed-point
    fractions (_fixed_point_bound: 3 * 2^-33 * N * (lambda + mu)max).  A relative 1e-9 on a log-likelihood of 1e5 would
    hide a hundred times more."""
    _gpu()
    from literate_amd.engine import ChainEngine
    from oracle import literate_oracle as lo
    ts, te = _lineages(n_bins, True, exact=False)
    assert np.any(np.round(ts * 2.0 ** 32) != ts * 2.0 ** 32)
    eng = ChainEngine(ts, te, C, model=model, seed=SEED + 1, s_freq=10, n_trace_slots=6, engine=engine)
    try:
        assert eng.layout.table_mode == 2 and eng.n_bins == n_bins
        cell = E.kernel_cell(eng.kernel_name(), model, 0)
        _check_forced(eng, engine, cell)
        eng.init()
        eng.steps(60)
        snap = eng.snapshot()
        assert np.all(snap["it"] == 60) and np.all(snap["accepted"] > 0)
        t0, sp, ex, br = lo.bin_events_cli(ts, te)
        stats = dict(sp=sp, ex=ex, br=br)
        if model == 3:
            stats["ex_dead"], stats["br_dead"] = lo.bin_events_dead(ts, te, te.max())
        lam, mu = E.accepted_rates(snap, n_bins, C)
        pre = lo.lineage_bins(ts, te, 0.0, n_bins)
        for c in range(C):
            ref = _reference_loglik(ts, te, lam[c], mu[c], model, stats, pre)
            bound = _fixed_point_bound(ts, te, lam[c], mu[c])
            assert abs(snap["likA"][c] - ref) <= bound, (cell, c, snap["likA"][c] - ref, bound)
        _record(cell, request)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _param_data(kind, n_bins, general):
    """Lineages, create_bins statistics and (trend) the covariate, binned by the oracle's own create_bins."""
    from oracle import literate_oracle as lo
    ts, te = _lineages(n_bins, general)
    origin, present = float(ts.min()), float(te.max())
    o, p, nsp, nex, dt, nb, t_range = lo.create_bins(origin, present, ts, te, 0)
    assert nb == n_bins
    trend = None
    if kind == "trend":
        x = np.arange(n_bins + 1, dtype=float)
        trend = lo.normalise_trend(np.sin(x / 7.0) + 0.02 * x)
        assert len(trend) == n_bins
    return ts, te, (o, p, nsp, nex, dt, t_range), trend


@functools.lru_cache(maxsize=None)
def _param_reference(kind, n_bins, general, n_it, s, seed, off):
    from oracle import dd_mcmc_oracle as ddo
    from oracle import trend_mcmc_oracle as tro
    ts, te, (o, p, nsp, nex, dt, t_range), trend = _param_data(kind, n_bins, general)
    with np.errstate(all="ignore"):
        emp = (nsp / dt, nex / dt)
    refs = {}
    for c in ORACLE_CHAINS:
        if kind == "dd":
            refs[c] = ddo.run_dd_mcmc(nsp, nex, dt, t_range, o, p, 2, 2, ddo.PhiloxDraws(seed, off + c), n_it, s, emp=emp)
        else:
            refs[c] = tro.run_trend_mcmc(nsp, nex, dt, trend, tro.PhiloxDraws(seed, off + c), n_it, s, False, False, emp=emp)
    return emp, refs


def _param_engine(kind, n_bins, general, engine, seed, s, n_slots, off, exact=True):
    from literate_amd.ddrate import DDRateEngine
    from literate_amd.trendrate import TrendRateEngine
    if exact:
        ts, te, _, trend = _param_data(kind, n_bins, general)
    else:
        ts, te = _lineages(n_bins, True, exact=False)
        trend = None
    origin, present = float(ts.min()), float(te.max())
    kw = dict(seed=seed, s_freq=s, n_trace_slots=n_slots, chain_offset=off, engine=engine)
    if kind == "dd":
        return ts, te, DDRateEngine(ts, te, origin, present, C, m_birth=2, m_death=2, **kw)
    return ts, te, TrendRateEngine(ts, te, origin, present, trend, C, **kw)


def _param_cases():
    out = []
    for kind in ("dd", "trend"):
        engines = ("auto", "launch", "packed", "persistent2", "persistent4", "spec") if kind == "dd" else \
            ("auto", "packed", "persistent4", "spec")
        for n_bins in E.class_edges(2, 1):
            for general in (False, True):
                for engine in engines:
                    if E.engine_runs(engine, 2, 1, not general, n_bins):
                        out.append(pytest.param(kind, n_bins, general, engine,
                                                id="%s-%d-%s-%s" % (kind, n_bins, "gen" if general else "unit", engine)))
    return out


@pytest.mark.parametrize("kind,n_bins,general,engine", _param_cases())
def test_parametric_samplers_at_the_class_edges(kind, n_bins, general, engine, request):
    """DDRate (-mBirth 2 -mDeath 2) and trend_rate at both sides of every class edge up to their 256-bin limit, unit and
    general times, every engine the cell runs: three chains' sampled log rows (scalars and per-bin columns) against
    oracle/dd_mcmc_oracle.run_dd_mcmc / oracle/trend_mcmc_oracle.run_trend_mcmc, with the tolerances of
    test_ddrate_sampler_follows_oracle, and every chain's accepted parameter vector re-scored by lr_bd_loglik_batch."""
    _gpu()
    from literate_amd import ops
    n_it, s, seed, off = 120, 2, 606, 4
    ts, te, eng = _param_engine(kind, n_bins, general, engine, seed, s, n_it // s, off)
    try:
        assert eng.n_bins == n_bins and eng.unit_resolution == (not general)
        cell = E.kernel_cell(eng.kernel_name(), 2, 1)
        assert cell == E.layout_cell(2, 1, n_bins, eng.layout), (eng.kernel_name(), cell)
        _check_forced(eng, engine, cell)
        _, _, (o, p, nsp, nex, dt, t_range), trend = _param_data(kind, n_bins, general)
        assert np.array_equal(eng.n_spec, nsp) and np.array_equal(eng.n_exti, nex) and np.allclose(eng.DT, dt, rtol=1e-13)
        emp, refs = _param_reference(kind, n_bins, general, n_it, s, seed, off)
        eng.init()
        eng.steps(n_it // 2)
        eng.steps(n_it - n_it // 2)
        for c in ORACLE_CHAINS:
            got = eng.log_rows(c, emp=emp)
            ref = refs[c]
            assert len(got) == len(ref) == n_it // s
            for i, (g, r) in enumerate(zip(got, ref)):
                assert g[0] == r[0]
                assert np.allclose(g[1:-3], r[1:-3], rtol=1e-9, atol=1e-9, equal_nan=True), (cell, c, i, g[:14], r[:14])
                assert np.allclose(g[-3:], r[-3:], rtol=1e-7, atol=1e-9, equal_nan=True)
        snap = eng.snapshot()
        assert np.all(snap["it"] == n_it)
        b, d = _param_rates(kind, snap, dt, trend)
        lik = ops.bd_loglik_batch(ts, te, o, b, d, 2).cpu().numpy()
        assert np.allclose(lik, snap["likA"], rtol=1e-9), (cell, lik - snap["likA"])
        _record(cell, request)
    finally:
        eng.close()


def _param_rates(kind, snap, dt, trend):
    from literate_amd import ops
    if kind == "dd":
        args = np.stack([snap["L"][c][:8] for c in range(C)])
        b, d, _, _ = ops.dd_rates(args, dt, 2, 2)
    else:
        args = np.stack([snap["L"][c][:6] for c in range(C)])
        b, d = ops.trend_rates(args, trend, False, False)
    return [x.cpu().numpy() for x in (b, d)]


def _param_off_grid_cases():
    out = []
    for n_bins in E.class_edges(2, 1):
        h = E.table_class(2, n_bins)
        if n_bins < E.PARAM_MAX_BINS and E.table_class(2, n_bins + 1) == h:
            continue
        for engine in ("packed", "persistent4", "spec"):
            if E.engine_runs(engine, 2, 1, False, n_bins):
                out.append(pytest.param(n_bins, engine, id="dd-%d-%s" % (n_bins, engine)))
    return out


@pytest.mark.parametrize("n_bins,engine", _param_off_grid_cases())
def test_parametric_sampler_off_grid_within_the_fixed_point_bound(n_bins, engine, request):
    """The DDRate sampler on times OFF the 2^-32 grid in every parametric table-mode-2 cell: each chain's accepted
    log-likelihood against the oracle's fp64 per-lineage evaluation of its DD rates, within the fixed-point bound."""
    _gpu()
    from oracle import literate_oracle as lo
    ts, te, eng = _param_engine("dd", n_bins, True, engine, 808, 10, 6, 0, exact=False)
    try:
        assert eng.layout.table_mode == 2 and eng.n_bins == n_bins
        cell = E.kernel_cell(eng.kernel_name(), 2, 1)
        _check_forced(eng, engine, cell)
        eng.init()
        eng.steps(60)
        snap = eng.snapshot()
        assert np.all(snap["it"] == 60)
        b, d = _param_rates("dd", snap, np.asarray(eng.DT), None)
        pre = lo.lineage_bins(ts, te, float(eng.origin), n_bins)
        for c in range(C):
            ref = lo.per_lineage_loglik(ts, te, float(eng.origin), b[c], d[c], 2, pre=pre)
            bound = _fixed_point_bound(ts, te, b[c], d[c])
            assert abs(snap["likA"][c] - ref) <= bound, (cell, c, snap["likA"][c] - ref, bound)
        _record(cell, request)
    finally:
        eng.close()


def test_every_planned_cell_ran_against_the_oracle():
    """The kernels the cases above ran (by ChainEngine.kernel_name()) cover exactly the planner's cell list: every
    instantiation the planner can select has a comparison with the oracle at a class edge, and a new one added without
    one fails here.  (Runs after the cases of this module: run the whole file.)"""
    want = E.planner_cells()
    got = set(RAN)
    assert got == want, dict(missing=sorted(want - got, key=str), unexpected=sorted(got - want, key=str))
    print("%d cells against the oracle" % len(got))
