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
ORACLE_CHAINS = E.ORACLE_CHAINS
RAN = {}                                     # cell -> test ids that ran it against the oracle
RJ_ENGINES = ("auto", "launch", "packed", "persistent2", "persistent4", "spec")


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: no ROCm device visible")


_lineages = E.lineages                      # (the builder: shared with tests/helpers/chain_edges.py)


@functools.lru_cache(maxsize=None)
def _rj_reference(model, n_bins, general):
    """Binned statistics of the data (the oracle's own binning) and the oracle trajectories of ORACLE_CHAINS."""
    ts, te = _lineages(n_bins, general)
    return E.rj_reference(ts, te, model, n_bins, SEED, N_IT)


def _check_forced(eng, engine, cell):
    E.check_forced(engine, cell)


def _record(cell, request):
    RAN.setdefault(cell, []).append(request.node.name)


_reference_loglik = E.reference_loglik


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
    from literate_amd.engine import ChainEngine
    ts, te = _lineages(n_bins, general)
    stats, refs = _rj_reference(model, n_bins, general)
    eng = ChainEngine(ts, te, C, model=model, seed=SEED, s_freq=1, n_trace_slots=N_IT, engine=engine)
    try:
        assert eng.n_bins == n_bins and eng.unit_resolution == (not general)
        cell = E.kernel_cell(eng.kernel_name(), model, 0)
        assert cell == E.layout_cell(model, 0, n_bins, eng.layout), (eng.kernel_name(), cell)
        _check_forced(eng, engine, cell)
        E.run_rj_against_the_oracle(eng, ts, te, model, n_bins, stats, refs, N_IT, cell)
        _record(cell, request)
    finally:
        eng.close()


_fixed_point_bound = E.fixed_point_bound


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
    ts, te = _lineages(n_bins, general)
    bins, trend = E.param_stats(kind, ts, te, n_bins)
    return ts, te, bins, trend


@functools.lru_cache(maxsize=None)
def _param_reference(kind, n_bins, general, n_it, s, seed, off):
    ts, te, bins, trend = _param_data(kind, n_bins, general)
    return E.param_reference(kind, bins, trend, n_it, s, seed, off)


def _param_engine(kind, n_bins, general, engine, seed, s, n_slots, off, exact=True):
    if exact:
        ts, te, _, trend = _param_data(kind, n_bins, general)
    else:
        ts, te = _lineages(n_bins, True, exact=False)
        trend = None
    return ts, te, E.param_engine(kind, ts, te, trend, C, engine, seed, s, n_slots, off)


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
    n_it, s, seed, off = 120, 2, 606, 4
    ts, te, eng = _param_engine(kind, n_bins, general, engine, seed, s, n_it // s, off)
    try:
        assert eng.n_bins == n_bins and eng.unit_resolution == (not general)
        cell = E.kernel_cell(eng.kernel_name(), 2, 1)
        assert cell == E.layout_cell(2, 1, n_bins, eng.layout), (eng.kernel_name(), cell)
        _check_forced(eng, engine, cell)
        _, _, bins, trend = _param_data(kind, n_bins, general)
        emp, refs = _param_reference(kind, n_bins, general, n_it, s, seed, off)
        E.run_param_against_the_oracle(eng, kind, ts, te, bins, trend, emp, refs, n_it, s, cell)
        _record(cell, request)
    finally:
        eng.close()


def _param_rates(kind, snap, dt, trend):
    return E.param_rates(kind, snap, dt, trend, C)


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
