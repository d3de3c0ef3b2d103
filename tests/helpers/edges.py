"""The chain engine's kernel-choice map as the tests see it.

The planner (csrc/lr_mcmc.hip: lr_plan_engine, lr_persist_variant, lr_packscan_planned; csrc/lr_loglik.hip:
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
    """Whether a FORCED engine runs the configuration as that engine (the mirror of lr_persist_variant /
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


def make_config(model, sampler, unit, n_bins, n_chains, n_lineages, engine_mode):
    from literate_amd import _hip
    end = float(n_bins) + 0.5
    return _hip.McmcConfig(
        n_lineages=int(n_lineages), n_bins=int(n_bins), n_chains=int(n_chains), model=int(model), use_rate_HP=1,
        s_freq=10, n_trace_slots=4, update_fraction=0.75, t0=0.0, start_time=0.0, end_time=end, seed=1,
        unit_resolution=int(unit), engine_mode=int(engine_mode), frac_birth=0.0, frac_death=0.5 if unit else 0.0, sampler=int(sampler), m_birth=2 if sampler == 1 else 0,
        m_death=2 if sampler == 1 else 0, dd_present=end if sampler == 1 else 0.0, dd_init_death=0.1)


def query(model, sampler, unit, n_bins, n_chains, n_lineages, engine_mode, cus=256):
    """lr_mcmc_query_layout on the host (no device needed), LR_DEVICE_CUS pinned: (rc, layout)."""
    from literate_amd import _hip
    lib = _hip.load()
    cfg = make_config(model, sampler, unit, n_bins, n_chains, n_lineages, engine_mode)
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
