"""The planner's map, value by value: every field of lr_mcmc_layout and the return code of lr_mcmc_query_layout over the
frozen list of configurations (tests/helpers/planner_cases.py) equal what tests/golden/planner_layouts.npz recorded.
tests/test_planner_map.py holds the invariants of the map; this holds its values, on the host (no device needed)."""
import numpy as np
import pytest

from helpers import planner_cases as P


@pytest.fixture(scope="module")
def frozen():
    with np.load(P.FIXTURE) as z:
        return z["layouts"]


def test_fixture_matches_the_case_list(frozen):
    cases = P.cases()
    assert len(cases) == 8960 + 28800 + 270
    assert frozen.shape == (len(cases), len(P.columns())) and frozen.dtype == np.int64
    assert len(P.columns()) == 28


def test_fixture_reaches_every_kind_of_plan(frozen):
    """What the recorded set must contain, so that a shrunken list of cases cannot pass: every kernel family, the packed scan
    in one and in two partitions, the streaming kernel, both schedules, every team size, block width and table mode, and
    the refusals."""
    from literate_amd import _hip
    col = {name: frozen[:, i] for i, name in enumerate(P.columns())}
    ok = col["rc"] == 0
    assert set(np.unique(col["rc"])) == {0, _hip.LR_ERR_SIZE}
    assert int(ok.sum()) == 33102 and int((col["rc"] == _hip.LR_ERR_SIZE).sum()) == 4928

    def reached(name):
        return set(np.unique(col[name][ok]).tolist())

    assert reached("persistent") == {0, 1, 2, 3}
    assert int((ok & (col["packed_scan"] == 1) & (col["n_parts"] == 1)).sum()) == 4280
    assert int((ok & (col["packed_scan"] == 1) & (col["n_parts"] == 2)).sum()) == 2511
    assert int((ok & (col["streaming"] == 1)).sum()) == 168
    assert reached("pipelined") == {0, 1}
    assert reached("team_blocks") >= {1, 2, 4, 8}
    assert reached("spec_chains_per_team") >= {1, 2}
    assert reached("reserved1") == {0, 512, 768, 1024}
    assert reached("table_mode") == {0, 1, 2}
    assert reached("chains_per_block") == {1, 2, 4, 8, 16}


def test_every_field_of_every_row_is_the_librarys_answer(frozen):
    got = P.answers()
    assert got.shape == frozen.shape
    bad = np.flatnonzero((got != frozen).any(axis=1))
    names, cases = P.columns(), P.cases()
    for i in bad[:20]:
        diff = ["%s: %d, recorded %d" % (names[j], got[i, j], frozen[i, j]) for j in np.flatnonzero(got[i] != frozen[i])]
        print("(model, sampler, unit, n_bins, chains, lineages, engine_mode, cus, team_request) = %r: %s" % (cases[i], "; ".join(diff)))
    assert bad.size == 0, "%d of %d rows differ from the recorded map (the first are printed above)" % (bad.size, len(cases))
