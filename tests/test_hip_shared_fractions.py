"""Every engine on unit-resolution data whose shared in-bin fractions are not (0, 0.5) (tests/helpers/shared_fractions.py):
death_jitter 0.25 / 0.75 / 1.0 and births off the year, against the oracle loops fed the same Philox draws and the fp64
per-lineage likelihood on the raw times.

With frac_birth == 0 the birth-side slope frac_birth R of every unit-resolution table entry vanishes (and model 3's
extant block's -frac_birth mu with it), and a kernel that reads 0.5 for frac_death - as the four-chain kernel's specialised
configuration words do on purpose, behind lr_p4_cfg_choice's guard - equals a correct one; tests/test_shared_fractions_host.py
shows that the references used here move by 0.9 % or more between these pairs and (0, 0.5), against the 1e-9 allowed here.
frac_death == 1.0 is death_jitter 0 or 1: deaths ON window edges, lineages with te == ts whose death entry is the bin before
their birth bin, and a whole last bin that holds the extant lineages.

The comparisons, their tolerances and the placed lineages are those of tests/test_hip_edges.py (helpers/edges.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import edges as E
from helpers import shared_fractions as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_IT, C, SEED = 120, 37, 4242
N, N_BINS, DATA_SEED = 3000, 24, 5
GENERIC, BDI, KEIDING = 0, 1, 2
ALL_ENGINES = ("auto", "launch", "packed", "persistent2", "persistent4", "spec", "stream")
P4_HELPER_NAME = "lr_persist4_kernel<%d, false, false, true>"


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: no ROCm device visible")


def _base_bins(window, fd):
    """n_bins of F.lineages for a window of `window` bins."""
    return window - (1 if fd == 1.0 else 0)


@functools.lru_cache(maxsize=None)
def _reference(n, base_bins, pair, model, chains):
    """The case data, its window, the oracle's binning and the oracle trajectories of `chains` (once per case data and
    model: the engines of a case all compare with the same trajectories)."""
    ts, te = F.lineages(n, base_bins, pair[0], pair[1], DATA_SEED)
    n_bins = F.window_bins(base_bins, pair[1])
    stats, refs = E.rj_reference(ts, te, model, n_bins, SEED, N_IT, chains)
    return ts, te, n_bins, stats, refs


def _check_unit_engine(eng, pair, n_bins, model, engine, stats):
    """The engine found the shared fractions by itself, planned the cell the layout names - with unit-resolution tables
    wherever that family has them - and binned the data as the oracle does."""
    assert eng.unit_resolution is True and eng.n_bins == n_bins
    assert eng.cfg.frac_birth == pair[0] and eng.cfg.frac_death == pair[1], (eng.cfg.frac_birth, eng.cfg.frac_death)
    cell = E.kernel_cell(eng.kernel_name(), model, 0)
    assert cell == E.layout_cell(model, 0, n_bins, eng.layout), (eng.kernel_name(), cell)
    E.check_forced(engine, cell)
    if engine == "stream":
        assert cell[0] == "launch", cell
    family, H, general, param, extant = cell
    if eng.n_chains == 1 and family == "launch":
        assert eng.layout.table_mode != 1         # lr_plan_scan: a lone chain scans general tables
    elif E.instantiated((family, H, False, param, extant)):
        assert eng.layout.table_mode == 1 and not general, (cell, eng.layout.table_mode)
    else:
        assert (family, H) == ("launch", 0), cell                     # the generic launch-based scan has no unit form
    assert np.array_equal(eng.sp_events.cpu().numpy(), stats["sp"]) and np.array_equal(eng.ex_events.cpu().numpy(), stats["ex"])
    assert np.allclose(eng.br_length.cpu().numpy(), stats["br"], rtol=1e-12, atol=0.0)
    return cell


def _run_rj(n, window, pair, model, engine, chains, oracle_chains, monkeypatch):
    """One case: engine on the case data, the checks of _check_unit_engine, then tests/test_hip_edges.py's comparison
    (E.run_rj_against_the_oracle); on the four-chain kernel's helper form also the configuration word."""
    _gpu()
    from literate_amd.engine import ChainEngine
    monkeypatch.delenv("LR_P4_GENERIC", raising=False)
    ts, te, n_bins, stats, refs = _reference(n, _base_bins(window, pair[1]), pair, model, oracle_chains)
    assert n_bins == window
    eng = ChainEngine(ts, te, chains, model=model, seed=SEED, s_freq=1, n_trace_slots=N_IT, engine=engine)
    try:
        cell = _check_unit_engine(eng, pair, n_bins, model, engine, stats)
        E.run_rj_against_the_oracle(eng, ts, te, model, n_bins, stats, refs, N_IT, cell)
        if eng.kernel_name() == P4_HELPER_NAME % cell[1]:
            want = GENERIC if (pair != F.CONTROL or model == 3) else (KEIDING if model == 2 else BDI)
            assert eng.p4_config() == want, (pair, model, eng.p4_config())
    finally:
        eng.close()
    return cell


def _rj_cases():
    out = []
    for pair in F.PAIRS + [F.CONTROL]:
        for model in (0, 1, 2, 3):
            for engine in (ALL_ENGINES if model in (0, 3) else ("auto", "persistent4", "spec")):
                out.append(pytest.param(pair, model, engine, id="%s-m%d-%s" % (F.pair_id(pair), model, engine)))
    return out


@pytest.mark.parametrize("pair,model,engine", _rj_cases())
def test_rj_sampler_every_family_at_other_fractions(pair, model, engine, monkeypatch):
    """The RJ sampler in the smallest table class (24 bins, 25 with integer deaths: H = 40, model 3 H = 72), ~3,000
    lineages, 37 chains (every kernel's last block ragged), 120 iterations in two launches, every fraction pair and the
    control, every engine: the fractions in the configuration are the data's, the forced family ran on unit-resolution
    tables, chains 0, 18 and 36 follow the oracle row by row, and every chain's log-likelihood is the fp64 per-lineage
    value of its accepted state on the raw times and lr_bd_loglik_batch's."""
    _run_rj(N, F.window_bins(N_BINS, pair[1]), pair, model, engine, C, E.ORACLE_CHAINS, monkeypatch)


@pytest.mark.parametrize("pair", F.PAIRS + [F.CONTROL], ids=F.pair_id)
def test_unit_binning_at_other_fractions(pair):
    """lr_bin_unit_events on the case data in the caller's order against the CLI's window loop: counts exact, lineage-time
    at 1e-12 (deaths on window edges count in the bin they close; a lineage with te == ts adds a birth, a death in the
    bin before, and no lineage-time)."""
    _gpu()
    from literate_amd import ops
    from oracle import literate_oracle as lo
    ts, te = F.lineages(N, N_BINS, pair[0], pair[1], DATA_SEED)
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    assert t0 == 0 and len(sp) == F.window_bins(N_BINS, pair[1]) and sp.sum() == len(ts)
    got = [x.cpu().numpy() for x in ops.bin_unit_events(np.array(ts), np.array(te), 0.0, len(sp))]
    assert np.array_equal(got[0], sp) and np.array_equal(got[1], ex)
    assert np.allclose(got[2], br, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("model", [0, 2])
@pytest.mark.parametrize("pair", F.REDUCED, ids=F.pair_id)
def test_four_chain_kernel_with_a_helper_share(pair, model, monkeypatch):
    """60,000 lineages on 128 bins (H = 136), 9 chains: the four-chain kernel's helper waves take a share of the scan and
    build the tables (tests/test_hip_p4_specialised.py: the smallest such size)."""
    cell = _run_rj(60_000, 128, pair, model, "persistent4", 9, (0, 4, 8), monkeypatch)
    assert cell == ("persist4", 136, False, False, False)


@pytest.mark.parametrize("window,engine", [(300, "persistent4"), (300, "persistent2"), (300, "packed"), (200, "spec"),
                                           (200, "launch"), (513, "auto")])
@pytest.mark.parametrize("pair", F.REDUCED, ids=F.pair_id)
def test_wider_table_classes(pair, window, engine, monkeypatch):
    """The wide class (300 bins, H = 520) on the persistent kernels and the packed scan, H = 264 (200 bins) on the
    speculative kernel and the launch-based scans, and 513 bins - above every class - on the generic launch-based scan."""
    cell = _run_rj(N, window, pair, 0, engine, C, E.ORACLE_CHAINS, monkeypatch)
    assert cell[1] == {300: 520, 200: 264, 513: 0}[window], cell


@pytest.mark.parametrize("pair", F.REDUCED, ids=F.pair_id)
def test_one_chain_on_the_launch_based_scan(pair, monkeypatch):
    """lr_plan_scan drops a lone chain to general tables: the configuration still carries the shared fractions, the scan
    takes them from the times."""
    _run_rj(N, F.window_bins(N_BINS, pair[1]), pair, 0, "launch", 1, (0,), monkeypatch)


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("pair", F.PAIRS + [F.CONTROL], ids=F.pair_id)
def test_other_fractions_run_the_generic_configuration_word(pair, model, monkeypatch):
    """The four-chain kernel's specialised words compile the fractions (0, 0.5) in (csrc/lr_step.h: LR_P4_FRAC_*): only
    the control may run them; every other pair runs the generic instantiation of the same helper-wave kernel."""
    _gpu()
    from literate_amd.engine import ChainEngine
    monkeypatch.delenv("LR_P4_GENERIC", raising=False)
    monkeypatch.delenv("LR_P4_HELP", raising=False)
    ts, te = F.lineages(N, N_BINS, pair[0], pair[1], DATA_SEED)
    eng = ChainEngine(ts, te, 6, model=model, seed=SEED, s_freq=1, n_trace_slots=4, engine="persistent4")
    try:
        eng.init()
        eng.steps(4)
        assert eng.layout.persistent == 2 and eng.kernel_name() == P4_HELPER_NAME % 40, eng.kernel_name()
        want = GENERIC if pair != F.CONTROL else (KEIDING if model == 2 else BDI)
        assert eng.p4_config() == want, (pair, model, eng.p4_config())
    finally:
        eng.close()


@pytest.mark.parametrize("model", [0, 3])
@pytest.mark.parametrize("engine", ["launch", "packed", "persistent4", "spec"])
def test_off_grid_jitter_falls_back_to_general_times(engine, model):
    """death_jitter 0.1: year + 0.1 rounds differently from year to year, the fractions differ by ulps and the engine must
    take the general-times path by itself.  Every chain's log-likelihood after 60 iterations against the fp64 oracle of
    its accepted state on the raw times: rtol 1e-9 on the launch-based scan (fp64 fractions), the fixed-point bound of
    tests/test_hip_edges.py on the packed families.  (No trajectories: off the 2^-32 grid a near-tie may go either way.)"""
    _gpu()
    from literate_amd.engine import ChainEngine
    from oracle import literate_oracle as lo
    ts, te = F.lineages(N, N_BINS, F.OFF_GRID[0], F.OFF_GRID[1], DATA_SEED)
    assert E.engine_runs(engine, model, 0, False, N_BINS)
    eng = ChainEngine(ts, te, C, model=model, seed=SEED + 1, s_freq=10, n_trace_slots=6, engine=engine)
    try:
        assert eng.unit_resolution is False and eng.n_bins == N_BINS
        assert eng.cfg.frac_birth == 0.0 and eng.cfg.frac_death == 0.0
        cell = E.kernel_cell(eng.kernel_name(), model, 0)
        assert cell == E.layout_cell(model, 0, N_BINS, eng.layout), (eng.kernel_name(), cell)
        E.check_forced(engine, cell)
        assert cell[2] and eng.layout.table_mode == (0 if engine == "launch" else 2), (cell, eng.layout.table_mode)
        eng.init()
        eng.steps(60)
        snap = eng.snapshot()
        assert np.all(snap["it"] == 60) and np.all(snap["accepted"] > 0)
        stats = F.stats_of(ts, te, model)
        lam, mu = E.accepted_rates(snap, N_BINS, C)
        pre = lo.lineage_bins(ts, te, 0.0, N_BINS)
        for c in range(C):
            ref = E.reference_loglik(ts, te, lam[c], mu[c], model, stats, pre)
            if engine == "launch":
                assert np.isclose(snap["likA"][c], ref, rtol=1e-9, atol=0.0), (cell, c, snap["likA"][c] - ref)
            else:
                bound = E.fixed_point_bound(ts, te, lam[c], mu[c])
                assert abs(snap["likA"][c] - ref) <= bound, (cell, c, snap["likA"][c] - ref, bound)
    finally:
        eng.close()


PARAM_PAIRS = [(0.0, 0.25), (0.0, 1.0)]
PARAM_IT, PARAM_S, PARAM_SEED, PARAM_OFF = 120, 2, 606, 4


@functools.lru_cache(maxsize=None)
def _param_reference(kind, pair):
    """create_bins statistics (24 bins either way: create_bins drops the last bin, whole or partial) and oracle loops."""
    ts, te = F.lineages(N, N_BINS, pair[0], pair[1], DATA_SEED)
    bins, trend = E.param_stats(kind, ts, te, N_BINS)
    emp, refs = E.param_reference(kind, bins, trend, PARAM_IT, PARAM_S, PARAM_SEED, PARAM_OFF)
    return ts, te, bins, trend, emp, refs


@pytest.mark.parametrize("engine", ["auto", "persistent4", "spec", "packed"])
@pytest.mark.parametrize("pair", PARAM_PAIRS, ids=F.pair_id)
@pytest.mark.parametrize("kind", ["dd", "trend"])
def test_parametric_samplers_at_other_fractions(kind, pair, engine):
    """DDRate (-mBirth 2 -mDeath 2) and trend_rate on 24 bins of create_bins statistics at death_jitter 0.25 and 1.0 (the
    deaths of the last year then fall behind the window's last edge), the comparison of
    test_parametric_samplers_at_the_class_edges."""
    _gpu()
    assert E.engine_runs(engine, 2, 1, True, N_BINS)
    ts, te, bins, trend, emp, refs = _param_reference(kind, pair)
    eng = E.param_engine(kind, ts, te, trend, C, engine, PARAM_SEED, PARAM_S, PARAM_IT // PARAM_S, PARAM_OFF)
    try:
        assert eng.n_bins == N_BINS and eng.unit_resolution is True
        assert eng.cfg.frac_birth == pair[0] and eng.cfg.frac_death == pair[1]
        cell = E.kernel_cell(eng.kernel_name(), 2, 1)
        assert cell == E.layout_cell(2, 1, N_BINS, eng.layout), (eng.kernel_name(), cell)
        E.check_forced(engine, cell)
        assert eng.layout.table_mode == 1 and not cell[2], (cell, eng.layout.table_mode)
        E.run_param_against_the_oracle(eng, kind, ts, te, bins, trend, emp, refs, PARAM_IT, PARAM_S, cell)
    finally:
        eng.close()


def test_checkpoint_from_other_fractions_is_refused(tmp_path):
    """A checkpoint of a run on the control data is not loaded into an engine on the same lineages at death_jitter 0.25:
    the fractions are part of the configuration a checkpoint must agree on."""
    _gpu()
    from literate_amd.engine import ChainEngine
    kw = dict(model=0, seed=77, s_freq=1, n_trace_slots=40, engine="persistent4")
    ts, te = F.lineages(N, N_BINS, F.CONTROL[0], F.CONTROL[1], DATA_SEED)
    ts2, te2 = F.lineages(N, N_BINS, 0.0, 0.25, DATA_SEED)
    assert np.array_equal(ts, ts2) and np.array_equal(te - 0.5, te2 - 0.25)
    a = ChainEngine(ts, te, 6, **kw)
    b = ChainEngine(ts2, te2, 6, **kw)
    same = ChainEngine(ts, te, 6, **kw)
    try:
        a.init()
        a.steps(30)
        path = str(tmp_path / "run.npz")
        a.save(path)
        assert bytes(a.layout) == bytes(b.layout)
        with pytest.raises(ValueError, match="frac_death"):
            b.load(path)
        same.load(path)
        assert same.iterations == 30
    finally:
        for e in (a, b, same):
            e.close()


CLI_IT, CLI_S, CLI_SEED, CLI_CHAINS = 200, 10, 31, 2
CLI_JITTERS = {"quarter": 0.25, "zero": 0.0, "default": 0.5}


@functools.lru_cache(maxsize=None)
def _cli_years():
    """A tiny year-resolution input: integer births and deaths, some in the same year."""
    from literate_amd import synth
    s, k, _ = synth.make_lineages(400, n_bins=20, n_shifts=2, seed=9, jitter=0.0)
    assert np.count_nonzero(s == k) > 0
    return s, k


@functools.lru_cache(maxsize=None)
def _cli_engine_rows(jitter):
    """The sampled heads [samples, chains, 13] of a ChainEngine built directly on te + jitter."""
    from literate_amd.engine import ChainEngine, split_trace_row
    s, k = _cli_years()
    eng = ChainEngine(s, k + jitter, CLI_CHAINS, model=0, seed=CLI_SEED, s_freq=CLI_S, n_trace_slots=CLI_IT // CLI_S)
    try:
        assert eng.unit_resolution is True and eng.cfg.frac_death == (jitter if jitter > 0 else 1.0)
        eng.init()
        eng.steps(CLI_IT)
        tr = eng.trace_rows()
        return np.array([[split_trace_row(tr[i, c])[0][:13] for c in range(CLI_CHAINS)] for i in range(CLI_IT // CLI_S)])
    finally:
        eng.close()


@pytest.mark.parametrize("which", list(CLI_JITTERS))
def test_cli_death_jitter_end_to_end(which, tmp_path):
    """LiteRateForward.py with -death_jitter 0.25, with -death_jitter 0 and with the default: the sampled rows of every
    chain's log are those of an engine built on te + jitter with the same seed (the tolerance of test_cli_end_to_end),
    and the three conventions give three different likelihood columns."""
    _gpu()
    jitter = CLI_JITTERS[which]
    s, k = _cli_years()
    data = tmp_path / "years.tsv"
    with open(data, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, b) in enumerate(zip(s, k)):
            f.write("%d\t%d\t%d\n" % (i, a, b))
    cmd = [sys.executable, os.path.join(ROOT, "LiteRateForward.py"), "-d", str(data), "-n", str(CLI_IT), "-s", str(CLI_S),
           "-p", "100", "-seed", str(CLI_SEED), "-model_BDI", "0", "--chains", str(CLI_CHAINS)]
    if which != "default":
        cmd += ["-death_jitter", repr(jitter)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
    logdir = tmp_path / "literate_mcmc_logs"
    want = _cli_engine_rows(jitter)
    for c in range(CLI_CHAINS):
        mc = np.loadtxt(logdir / ("years_BD_c%d_mcmc.log" % c), skiprows=1)
        assert mc.shape == (CLI_IT // CLI_S, 16)
        assert np.allclose(mc[:, :13], want[:, c], rtol=1e-9), (which, c)
    lik = {w: _cli_engine_rows(j)[:, :, 2] for w, j in CLI_JITTERS.items()}
    for w in CLI_JITTERS:
        if w != which:
            assert not np.any(np.isclose(lik[w], lik[which], rtol=1e-6, atol=0.0)), (which, w)
