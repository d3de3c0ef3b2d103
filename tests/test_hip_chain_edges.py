"""Every engine kernel at its chain-count edges against the oracle loops (the cases and their classes: tests/helpers/
chain_edges.py; the boundaries themselves are pinned on the host by tests/test_chain_edges_host.py).

The chain count decides the table grouping cb (1, 2, 4, 8, 16 from 1, 2, 3, 5, 9 chains), what a lone chain runs on,
which slots of the last block stay empty (a lone chain, a pair, a pair and a lone chain in lr_persist4_kernel's quad; a
half-filled lr_persist_kernel block; a lone chain in lr_spec_kernel's last team; a ragged last pair group of
lr_packscan_kernel<PAIRS>), the team form of lr_spec_kernel (a team per chain up to the CUs, per pair up to twice as
many, forced teams of k blocks up to cpb * floor(CUs / k)), and the launches' schedule (pipelined halves, two partitions,
the wide scan on general times).  Seven configurations reach every kernel family on unit and pair-general tables, with
the extant block, at H = 520, under the parametric samplers, and on scans long enough for lr_spec_kernel's mode 3 and the
1024-thread lr_persist_kernel.

Each case asserts from the engine's layout and kernel name that it hits the class it names (CE.expected_signature:
restated rules, not the planner's answer), runs 60 iterations at
s_freq = 1 in two launches of 25 + 35 and checks: chains {0, 1, C // 2, C - 2, C - 1} row by row against the oracle loop
fed the same Philox draws (by global chain id under a chain_offset), every chain's accepted state re-scored in fp64,
every chain at iteration 60 with a finite log-likelihood and a counting iteration column, and no two chains ending in the
same state.  The last test checks that every class the host walk finds over all configurations and engines was run,
but for the pairs without a case that CE.EXCLUDED lists (held to the walk by the host test)."""
import numpy as np
import pytest

from helpers import chain_edges as CE
from helpers import edges as E

pytestmark = pytest.mark.gpu

RAN = {}                                     # (configuration, engine) -> signatures run against the oracle


def _device_cus():
    """Compute units of the device (read inside a test, never at collection)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: no ROCm device visible")
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


CASES = CE.cases()                            # chain counts that follow the device stay symbolic (CUs+1, cap-1) here


def _engine(case):
    from literate_amd.engine import ChainEngine
    cfg, kw = CE.CONFIGS[case.config], CE.engine_kwargs(case.kwargs)
    if cfg.sampler == 0:
        ts, te = CE.data(case.config)
        return ChainEngine(ts, te, case.chains, model=cfg.model, seed=CE.SEED, s_freq=1, n_trace_slots=CE.N_IT,
                           engine=case.engine, **kw)
    assert set(kw) <= {"chain_offset"}
    ts, te, _, trend = CE.param_data(case.config)
    return E.param_engine(CE.KIND[cfg.sampler], ts, te, trend, case.chains, case.engine, CE.SEED, 1, CE.N_IT,
                          kw.get("chain_offset", 0))


@pytest.mark.parametrize("case", CASES, ids=[CE.case_id(c) for c in CASES])
def test_chain_count_edge(case):
    cus = _device_cus()
    case = CE.resolved(case, cus)
    cfg, cid, C = CE.CONFIGS[case.config], CE.case_id(case), case.chains
    off = case.kwargs.get("chain_offset", 0)
    with CE.environment(case.kwargs):
        eng = _engine(case)
        try:
            assert eng.n_bins == cfg.n_bins and eng.unit_resolution == (not cfg.general) and eng.n_chains == C
            # the class the case names (restated rules, not the planner's answer), from the layout and the kernel name
            sig = CE.check_class(case, eng.layout, eng.kernel_name(), cus)
            eng.init()
            if sig.family == 3 and sig.team == 1 and sig.cpb == 1:
                # a block per chain: planes by scanners up to 3 trips of the eight scanner waves (1536 groups), else mode 3
                assert eng.kernel_name().endswith(", 3>" if case.config == "G" else ", 2>"), (cid, eng.kernel_name())
            eng.steps(CE.FIRST)
            eng.steps(CE.N_IT - CE.FIRST)
            assert eng.iterations == CE.N_IT
            tr, snap = eng.trace_rows(), eng.snapshot()
            if cfg.sampler == 0:
                lam, mu = CE.check_rj_case(tr, snap, case.config, off, cid)
                E.rescore_rj_on_device(eng, snap, lam, mu, cfg.model, CE.rj_stats(case.config), cid)
            else:
                ts, te, bins, trend = CE.param_data(case.config)
                assert np.array_equal(eng.n_spec, bins[2]) and np.array_equal(eng.n_exti, bins[3])
                assert np.allclose(eng.DT, bins[4], rtol=1e-13)
                rows = {c: eng.log_rows_from(tr[:, c], emp=CE.param_emp(case.config)) for c in CE.followed(C)}
                CE.check_param_case(rows, tr, snap, case.config, off, cid)
                E.rescore_param_on_device(eng, CE.KIND[cfg.sampler], snap, ts, te, bins, trend, cid)
            RAN.setdefault((case.config, case.engine), set()).add(sig)
        finally:
            eng.close()


def test_every_walked_class_ran_against_the_oracle():
    """Every signature the host walk (tests/test_chain_edges_host.py, here with the device's compute units) finds for a
    (configuration, engine) was run by at least one case above; the pairs without a case are exactly the written list
    CE.EXCLUDED.  (Runs after the cases of this module: run the whole file.)"""
    bad = CE.uncovered(RAN, _device_cus())
    assert not bad, bad
    print("%d cases ran %d classes against the oracle" % (len(CASES), sum(len(v) for v in RAN.values())))
