"""The planner's answers, frozen: every field of lr_mcmc_layout and the return code of lr_mcmc_query_layout over a fixed list
of configurations, as recorded in tests/golden/planner_layouts.npz (tests/test_planner_frozen_host.py).

tests/test_planner_map.py checks what the planner's map must satisfy; this list pins its VALUES, so that a change to the
planner's code that is meant to change no decision can be shown to change none.  The fixture holds the results only - the
cases are regenerated from the code below - and is recorded from the library as built, with no LR_* variable set:

    python -m helpers.planner_cases --record        (from tests/)

A deliberate change of a threshold or a cost model changes rows of the fixture: record it again with the new library and
say so in the change."""
import ctypes as C
import itertools
import os

import numpy as np

from . import edges

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "golden", "planner_layouts.npz")

MODELS = ((0, 0), (2, 0), (3, 0), (2, 1), (2, 2))          # (model, sampler)
BINS = (20, 100, 200, 400, 600)
CHAINS = (1, 2, 9, 16, 17, 32, 128, 256, 257, 1024, 1536, 4096)
LINEAGES = (1_000, 20_000, 200_000, 3_000_000, 100_000_000, 3_000_000_000)
MODES = (0, 2, 6, 7)
CUS = (256, 64)
TEAM_K, TEAM_CPB, TEAM_CHAINS, TEAM_LINEAGES = (0, 1, 2, 4, 8), (0, 1, 2), (16, 128, 300), (10_000, 100_000, 1_000_000)


def cases():
    """(model, sampler, unit, n_bins, n_chains, n_lineages, engine_mode, cus, team_request) of every frozen point: the
    planner-map grid (both sides of every class edge), a product that reaches every kernel family, both packed partition
    modes, the streaming kernel, both block widths and the error return, and the team requests of the speculative kernel."""
    out = [g + (256, 0) for g in edges.grid()]
    for (model, sampler), unit, n_bins, c, n, mode, cus in itertools.product(MODELS, (True, False), BINS, CHAINS, LINEAGES, MODES, CUS):
        out.append((model, sampler, unit, n_bins, c, n, mode, cus, 0))
    for k, cpb, unit, c, n in itertools.product(TEAM_K, TEAM_CPB, (True, False), TEAM_CHAINS, TEAM_LINEAGES):
        out.append((0, 0, unit, 128, c, n, 0, 256, k | cpb << 8))
    return out


def columns():
    """Names of the recorded columns: the return code, then every field of lr_mcmc_layout in its order."""
    from literate_amd import _hip
    return ["rc"] + [f for f, _ in _hip.McmcLayout._fields_]


def query(case):
    """One row: lr_mcmc_query_layout on the host (no device needed) with LR_DEVICE_CUS pinned, as edges.query does."""
    from literate_amd import _hip
    model, sampler, unit, n_bins, c, n, mode, cus, team = case
    lib = _hip.load()
    cfg = edges.make_config(model, sampler, unit, n_bins, c, n, mode)
    cfg.team_request = team
    lay = _hip.McmcLayout()
    old = os.environ.get("LR_DEVICE_CUS")
    os.environ["LR_DEVICE_CUS"] = str(cus)
    try:
        rc = lib.lr_mcmc_query_layout(C.byref(cfg), C.byref(lay))
    finally:
        if old is None:
            os.environ.pop("LR_DEVICE_CUS", None)
        else:
            os.environ["LR_DEVICE_CUS"] = old
    return [rc] + [getattr(lay, f) for f, _ in _hip.McmcLayout._fields_]


def answers():
    """The library's answers over cases(), int64 [cases][columns]."""
    return np.array([query(case) for case in cases()], dtype=np.int64)


def record(path=FIXTURE):
    set_ = sorted(k for k in os.environ if k.startswith("LR_"))
    if set_:
        raise SystemExit("unset %s first: the fixture is the planner's map with every switch at its default" % ", ".join(set_))
    rows = answers()
    np.savez_compressed(path, layouts=rows)
    return rows


if __name__ == "__main__":
    import sys
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python -m helpers.planner_cases --record")
    sys.path.insert(0, os.path.join(os.path.dirname(FIXTURE), os.pardir, os.pardir))      # the repository: literate_amd
    rows = record()
    print("%d rows of %d columns -> %s (%d bytes)" % (rows.shape + (os.path.normpath(FIXTURE), os.path.getsize(FIXTURE))))
