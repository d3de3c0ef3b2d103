"""The planner's map from a configuration to a kernel, on the host (lr_mcmc_query_layout needs no device): every model and
sampler, unit and general times, both sides of every table-class edge, a spread of chain and lineage counts, every
engine_mode.  The class rules and the cell list live in tests/helpers/edges.py; tests/test_hip_edges.py runs each cell
against the oracle."""
import pytest

from helpers import edges as E


@pytest.fixture(scope="module")
def planned():
    """(configuration, rc, layout fields) of every point of the grid."""
    out = []
    for g in E.grid():
        rc, lay = E.query(*g)
        out.append((g, rc, lay))
    return out


def test_class_edges_follow_the_table_rules():
    """The edges the GPU tests sit on: models 0-2 change class above 38, 70, 128, 256 bins and leave the persistent
    kernels above 512; model 3 holds 2 (n_bins + 2) entries per half-stride, so its classes end at 18, 34, 66, 130 and 258
    bins; the parametric samplers stop at 256 bins."""
    assert E.class_edges(0, 0) == [38, 39, 70, 71, 128, 129, 256, 257, 512, 513]
    assert E.class_edges(3, 0) == [18, 19, 34, 35, 66, 67, 130, 131, 258, 259]
    assert E.class_edges(2, 1) == [38, 39, 70, 71, 128, 129, 256]
    for n in (18, 34, 66, 130, 258):                       # full: the extant block's last entry is the half-stride's last
        assert 2 * (n + 2) == E.table_class(3, n)
    assert E.persistent_capacity(0, 0) == E.persistent_capacity(1, 0) == 512
    assert E.persistent_capacity(3, 0) == 258
    assert E.persistent_capacity(2, 1) == E.persistent_capacity(2, 2) == 256


def test_planner_map_invariants(planned):
    """Over the whole grid: the status is LR_OK except for a parametric sampler above 256 bins (LR_ERR_SIZE); table_mode
    follows the time resolution; the packed scan only with persistent == 0; no persistent plan above the model's capacity
    and every persistent or packed plan on the model's own table class; the speculative kernel on general times only up
    to H = 136; a forced engine either runs as asked or falls back to a plan the layout reports, and no layout names a
    kernel without an instantiation."""
    from literate_amd import _hip
    forced = {2: None, 3: "persist4", 4: "persist2", 5: "spec", 7: "packed"}
    names = {3: "persistent4", 4: "persistent2", 5: "spec", 7: "packed"}
    for (model, sampler, unit, n_bins, c, n, mode), rc, lay in planned:
        where = dict(model=model, sampler=sampler, unit=unit, n_bins=n_bins, chains=c, lineages=n, engine_mode=mode)
        if sampler != 0 and n_bins > E.PARAM_MAX_BINS:
            assert rc == _hip.LR_ERR_SIZE, where
            continue
        assert rc == 0, (rc, where)
        cell = E.layout_cell(model, sampler, n_bins, lay)
        family, H = cell[0], cell[1]
        assert E.instantiated(cell), (cell, where)
        # table_mode: unit-resolution data on unit tables wherever a class takes them, general data never on them; the
        # 32-bit fixed-point pair-general form exactly where a persistent kernel or the packed scan reads it
        if unit:
            assert lay.table_mode == (1 if (family != "launch" or E.launch_class(model, n_bins)) else 0), (lay.table_mode, where)
        else:
            assert lay.table_mode == (2 if family != "launch" else 0), (lay.table_mode, where)
        assert not (lay.packed_scan and lay.persistent), where
        assert lay.streaming == 0 or (lay.persistent == 0 and not lay.packed_scan), where
        if lay.persistent or lay.packed_scan:
            assert n_bins <= E.persistent_capacity(model, sampler), where
            assert H == E.table_class(model, n_bins), (H, where)
        else:
            gen_tabs = 2 * (2 if model == 3 else 1) * (n_bins + 2)
            assert lay.table_stride == (H if lay.table_mode == 1 else (2 * H if H else gen_tabs)), (lay.table_stride, where)
        if lay.persistent == 3:
            assert H <= E.spec_max_h(not unit) and lay.team_blocks in (1, 2, 4, 8), where
        if lay.persistent == 1:
            assert unit, where
        if mode == 1 or mode == 6:
            assert family == "launch", where
        if mode in forced and E.table_class(model, n_bins) is not None:
            want = forced[mode]
            if want is None:
                assert lay.persistent != 0, where
            elif c == 37 or c == 10 or c == 128:
                # (the mirror of the planner the GPU tests use to choose their forced engines)
                if E.engine_runs(names[mode], model, sampler, unit, n_bins):
                    assert family == want, (family, where)
                else:
                    assert family != want, (family, where)


def test_forced_engines_fall_back_where_the_cell_has_no_kernel(planned):
    """The fall-backs the planner takes instead of naming a kernel that does not exist: the two-chain kernel has no
    general-time form, the speculative kernel none above H = 136 on general times or above H = 264 at all, and none of
    the persistent kernels or the packed scan takes a configuration beyond the largest class."""
    seen = set()
    for (model, sampler, unit, n_bins, c, n, mode), rc, lay in planned:
        if rc != 0:
            continue
        h = E.table_class(model, n_bins)
        if mode == 4 and not unit:
            assert lay.persistent != 1
            seen.add("persist2-general")
        if mode == 5 and h is not None and h > E.spec_max_h(not unit):
            assert lay.persistent != 3
            seen.add("spec-above")
        if mode in (2, 3, 4, 5, 7) and h is None:
            assert lay.persistent == 0 and lay.packed_scan == 0
            seen.add("beyond")
    assert seen == {"persist2-general", "spec-above", "beyond"}


def test_planner_reaches_every_instantiated_cell(planned):
    """The cells the grid is planned into are exactly the instantiated ones: every kernel instantiation is reachable
    (tests/test_hip_edges.py checks each against the oracle) and the planner never names another."""
    cells = {E.layout_cell(g[0], g[1], g[3], lay) for g, rc, lay in planned if rc == 0}
    assert cells == E.instantiated_cells(), (sorted(cells - E.instantiated_cells(), key=str),
                                             sorted(E.instantiated_cells() - cells, key=str))
    assert cells == E.planner_cells()
    assert len(cells) == 109


def test_parametric_samplers_are_refused_above_256_bins():
    from literate_amd import _hip
    for sampler in (1, 2):
        rc, _ = E.query(2, sampler, True, 256, 37, 4000, 0)
        assert rc == 0
        for mode in E.ENGINES.values():
            rc, _ = E.query(2, sampler, True, 257, 37, 4000, mode)
            assert rc == _hip.LR_ERR_SIZE
