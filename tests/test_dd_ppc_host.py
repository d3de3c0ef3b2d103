"""The host side of DDRate.py's and trend_rate.py's posterior predictive check: the two new declarations, the argument
errors of lr_simulate_dd_batch (all returned before any launch, so they need no device), the numpy restatement
tests/helpers/dd_sim_ref.py against the simulators the project already has where the models coincide, the restated check
tests/helpers/dd_ppc_ref.py on its replicate numbering, what the two new entry points of literate_amd/ppc.py refuse, and the
flags of the two CLIs."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import dd_ppc_ref, dd_sim_cases, dd_sim_ref, ppc_ref
from helpers.sim_batch_cases import NB, SPB, counts_from_run, mixed_rates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_binds_the_dd_simulator():
    from literate_amd import _hip, build
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        text = f.read()
    for name in ("lr_simulate_dd_batch_workspace_bytes", "lr_simulate_dd_batch"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["lr_simulate_dd_batch"][1]) == 15 and len(_hip.SIGNATURES["lr_simulate_dd_batch_workspace_bytes"][1]) == 4
    assert "lr_simbatch.hip" in build.SOURCES and "lr_dd.h" in build.HEADERS      # the kernel's unit and the rate map it shares
    with open(os.path.join(ROOT, "literate_amd", "csrc", "lr_simbatch.hip")) as f:
        src = f.read()
    assert 'extern "C" int lr_simulate_dd_batch(' in src and "lr_dd_bin_rates(" in src


def test_size_query_and_argument_errors_need_no_device():
    """the size query is host arithmetic and equals lr_simulate_bd_batch's; NULL, SIZE, MODEL and WORKSPACE errors come before
    any device call (the pointers below are host memory that is never read)"""
    from literate_amd import _hip
    lib = _hip.load()
    q, qb = lib.lr_simulate_dd_batch_workspace_bytes, lib.lr_simulate_bd_batch_workspace_bytes
    lds, groups = _hip.LR_SIMBATCH_LDS_SLOTS, _hip.LR_SIMBATCH_GROUPS
    assert q(3, 5, 4, 1000) == q(3, 5, 4, lds) == 256
    assert q(3, 5, 4, lds + 64) == 256 + 3 * 64 * 4
    assert q(10 * groups, 5, 4, lds + 64) == 256 + groups * 64 * 4
    for a in ((3, 5, 4, 1000), (700, 24, 8, 1 << 20), (1, 1, 1, (1 << 31) - 1)):
        assert q(*a) == qb(*a) > 0
    for bad in ((0, 5, 4, 10), (3, 0, 4, 10), (3, 5, 0, 10), (3, _hip.LR_MAX_BINS + 1, 4, 10), (3, 5, 4, 0), (3, 5, 4, 1 << 31)):
        assert q(*bad) == _hip.LR_ERR_SIZE, bad
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(par=p, x=p, mb=2, md=2, R=3, nb=5, spb=4, start=p, cap=1 << 20, counts=p, totals=p, work=p, nbytes=0):
        return lib.lr_simulate_dd_batch(par, x, mb, md, R, nb, spb, start, cap, 1, counts, totals, work, nbytes, None)

    assert lib.lr_simulate_dd_batch(None, None, 2, 2, 3, 5, 4, None, 10, 1, None, None, None, 0, None) == _hip.LR_ERR_NULL
    for kw in (dict(par=None), dict(x=None), dict(start=None), dict(counts=None), dict(totals=None), dict(work=None)):
        assert call(**kw) == _hip.LR_ERR_NULL, kw
    for kw in (dict(R=0), dict(nb=0), dict(spb=0), dict(nb=_hip.LR_MAX_BINS + 1), dict(cap=0), dict(cap=1 << 31)):
        assert call(**kw) == _hip.LR_ERR_SIZE, kw
    for kw in (dict(mb=-1), dict(mb=3), dict(md=-3), dict(md=3)):
        assert call(**kw) == _hip.LR_ERR_MODEL, kw
    for mb in (0, 1, 2):
        for md in (-2, -1, 0, 1, 2):                                    # every accepted pair gets as far as the workspace check
            assert call(mb=mb, md=md, nbytes=255) == _hip.LR_ERR_WORKSPACE, (mb, md)
    assert call(cap=lds + 64, nbytes=256 + 3 * 64 * 4 - 1) == _hip.LR_ERR_WORKSPACE


def test_restatement_on_constant_rates_equals_the_oracle_simulator():
    """GPU test 1's case on the CPU: under m_birth 0, m_death 0 the restated rate map is l_max, m_max, and the restated
    step loop must then be oracle/sim_oracle.py's on constant rows"""
    la, mu = mixed_rates()
    par = dd_sim_cases.const_params(la[:, 0], mu[:, 0], 12)
    counts, totals, closest = dd_sim_ref.simulate(par, dd_sim_cases.X, SPB, 300, 1000, 0, 0)
    oc, ot = ppc_ref.oracle_simulator(np.repeat(la[:, :1], NB, 1), np.repeat(mu[:, :1], NB, 1), SPB, np.full(12, 300), 1000, 1 << 20)
    assert np.array_equal(counts, oc) and np.array_equal(totals, ot)
    assert totals[:, 0].min() > 300 and np.all(closest > 0)
    counts, totals, _ = dd_sim_ref.simulate(dd_sim_cases.const_params(.02, .6, 3), dd_sim_cases.X, SPB, 50, 3, 0, 0)
    oc, ot = ppc_ref.oracle_simulator(np.full((3, NB), .02), np.full((3, NB), .6), SPB, np.full(3, 50), 3, 1 << 20)
    assert np.array_equal(counts, oc) and np.array_equal(totals, ot) and totals[:, 3].tolist() == [59, 77, 46]


def test_restatement_with_a_fixed_niche_and_unit_exponents_equals_the_mode_1_oracle():
    """GPU test 3's case on the CPU, with the figures the device is held to"""
    from oracle import sim_oracle
    c = dd_sim_cases.MODE1
    counts, totals, closest = dd_sim_ref.simulate(np.tile(c["par"], (4, 1)), dd_sim_cases.X, SPB, c["n_start"], c["seed"], 1, 1)
    assert closest.min() >= dd_sim_cases.FLOOR
    assert totals[:, 0].tolist() == c["created"] and totals[:, 1].tolist() == c["living"]
    for r in range(4):
        ts, te, trace = sim_oracle.simulate_bd(c["n_start"], NB * SPB, c["seed"] + r, mode=1, l0=.5, m0=.1, K=500., scale=float(SPB))
        oc, ot = counts_from_run(ts, te, trace, c["n_start"], NB, SPB)
        assert np.array_equal(counts[r], oc) and np.array_equal(totals[r], ot), r


def test_restatement_figures_of_the_gpu_cases():
    """what the GPU cases pin comes from the committed restatement: the (2, 2) branch case and the start above the niche,
    whose first steps sit on the 1e-15 floor (no birth while frac > 1)"""
    counts, totals, closest = dd_sim_ref.simulate(dd_sim_cases.branch_params(), dd_sim_cases.X, SPB, 30, 2000, 2, 2)
    assert totals[:, 0].tolist() == dd_sim_cases.CREATED_2[(2, 2)] and counts[:, 2].max() == 2204 and closest.min() >= dd_sim_cases.FLOOR
    c = dd_sim_cases.ABOVE
    counts, totals, closest = dd_sim_ref.simulate(np.tile(c["par"], (3, 1)), dd_sim_cases.X, SPB, c["n_start"], c["seed"], 1, 1)
    assert totals[:, 0].tolist() == c["created"] and totals[:, 1].tolist() == c["living"] and closest.min() >= dd_sim_cases.FLOOR
    assert dd_sim_ref.dd_rates_at(c["par"], 0.0, 400.0, 1, 1) == (1e-15, .2 + .2 * 4.0)
    assert not counts[:, 0, 0].any() and counts[:, 1, 0].min() > 100       # bin 0: 400 lineages above a niche of 100


def test_restated_rate_map_equals_the_oracles_dd_rates():
    from oracle import literate_oracle as lo
    par = dd_sim_cases.branch_params()
    for mb, md in ((2, 2), (1, 1), (1, 0), (2, -1), (2, 1), (0, 2), (0, -2)):
        for r in (0, 5, 11):
            for n in (1.0, 30.0, 2500.0):
                b, d, _, _ = lo.dd_rates(par[r], np.full(NB, n), dd_sim_cases.X, mb, md)
                for k in (0, 7, 23):
                    assert dd_sim_ref.dd_rates_at(par[r], float(k), n, mb, md) == (b[k], d[k]), (mb, md, r, n, k)


def test_restated_check_numbers_its_replicates_as_the_docstring_says():
    """free-running: draw i from div_obs[b0] over x = time_range[b0:], seed + i; one step ahead: replicate (b - b0) * R + i is
    one bin from div_obs[b] at x = time_range[b] under draw i, seed + R + that index; an empty bin is not simulated"""
    sp, ex = np.array([0, 3, 2, 0, 0, 4]), np.array([0, 0, 1, 4, 0, 1])          # div_obs 0 0 3 4 0 0 3
    R, spb, seed = 6, 2, 40
    par = dd_sim_cases.branch_params()[:R]
    x = np.arange(6.) + 3
    out = dd_ppc_ref.check(par, sp, ex, x, 2, 2, spb, seed, capacity=1000)
    assert out["start_bin"] == 2 and out["div_obs"].tolist() == [0, 0, 3, 4, 0, 0, 3]
    fc, ft, d = dd_sim_ref.simulate(par, x[2:], spb, 3, seed, 2, 2, 1000)
    assert np.array_equal(out["free"]["counts"], fc) and np.array_equal(out["free"]["totals"], ft)
    closest = [d.min()]
    for b in range(2, 6):
        for i in range(R):
            j = (b - 2) * R + i
            c1, t1, d1 = dd_sim_ref.simulate_one(par[i], x[b:b + 1], spb, out["div_obs"][b], seed + R + j, 2, 2, 1000)
            assert np.array_equal(out["step"]["counts"][b - 2, i], c1[:, 0]) and np.array_equal(out["step"]["totals"][b - 2, i], t1), (b, i)
            closest.append(d1)
    assert out["closest"] == min(closest)
    assert out["step"]["simulated"].tolist() == [True, True, False, False]
    assert np.all(out["step"]["totals"][2:, :, 2] == 1) and np.isnan(out["table"][4:, 2:6]).all()
    rows = np.zeros((5, 3, 139))
    rows[..., 4:12] = np.arange(15 * 8).reshape(5, 3, 8)
    ref = dd_ppc_ref.posterior_predictive_dd(np.concatenate([rows[..., :4], np.tile(par[0], (5, 3, 1)), rows[..., 12:]], axis=2),
                                             sp, ex, x, 0, 0, 4, spb, seed, capacity=1000)
    assert ref["draw_rows"].tolist() == [0, 3, 7, 11] and np.array_equal(ref["params"], np.tile(par[0], (4, 1)))


def test_entry_points_refuse_bad_arguments_before_the_gpu_is_touched():
    import torch
    from literate_amd import ppc
    from literate_amd._hip import LR_TRACE_W
    sp, ex = np.array([0, 0, 2, 1, 0, 3]), np.array([0, 0, 0, 3, 0, 1])          # div_obs 0 0 0 2 0 0 2
    DT, x = np.ones(6), np.arange(6.)
    rows = torch.zeros((4, 2, LR_TRACE_W), dtype=torch.float64)
    for M, n in ((8, 4), (8, 50), (1000, 333)):
        assert np.array_equal(ppc.draw_indices(M, n), ppc_ref.draw_indices(M, n))
    with pytest.raises(ValueError, match="LR_TRACE_W"):
        ppc.posterior_predictive_dd(rows[..., :20], sp, ex, DT, x, 2, 2, 4, 10, 1)
    with pytest.raises(ValueError, match="one entry per bin"):
        ppc.posterior_predictive_dd(rows, sp, ex, DT[:5], x, 2, 2, 4, 10, 1)
    with pytest.raises(ValueError, match="one entry per bin"):
        ppc.posterior_predictive_dd(rows, sp, ex, DT, x[:5], 2, 2, 4, 10, 1)
    for bad in (0, 4, 6):                                               # nobody at its left edge / no such bin
        with pytest.raises(ValueError, match="start_bin"):
            ppc.posterior_predictive_dd(rows, sp, ex, DT, x, 2, 2, 4, 10, 1, start_bin=bad)
        with pytest.raises(ValueError, match="start_bin"):
            ppc.posterior_predictive_rates(np.ones((4, 6)), np.ones((4, 6)), sp, ex, 10, 1, start_bin=bad)
    with pytest.raises(ValueError, match="nothing to simulate"):
        ppc.posterior_predictive_dd(rows, [0, 0, 0], [0, 0, 0], DT[:3], x[:3], 2, 2, 4, 10, 1)
    with pytest.raises(ValueError, match="draws, n_bins"):
        ppc.posterior_predictive_rates(np.ones((4, 5)), np.ones((4, 5)), sp, ex, 10, 1)
    with pytest.raises(ValueError, match="draws, n_bins"):
        ppc.posterior_predictive_rates(np.ones((4, 6)), np.ones((3, 6)), sp, ex, 10, 1)
    with pytest.raises(ValueError, match="no draws"):
        ppc.posterior_predictive_rates(np.ones((0, 6)), np.ones((0, 6)), sp, ex, 10, 1)
    assert ppc.dd_arg_error(0.2, 0, 100, 10) is None and ppc.dd_arg_error(0.0, 0.0) is None
    assert "burn-in" in ppc.dd_arg_error(1.0, 0) and "burn-in" in ppc.dd_arg_error(-0.5, 0)
    assert "-rm_first_bin" in ppc.dd_arg_error(0.2, 1.0)
    assert "at least 1" in ppc.dd_arg_error(0.2, 0, 0, 10) and "at least 1" in ppc.dd_arg_error(0.2, 0, 10, 0)


@pytest.mark.parametrize("cli", ["DDRate", "trend_rate"])
def test_cli_parsers_take_the_ppc_flags(cli):
    sys.path.insert(0, ROOT)
    try:
        mod = __import__(cli)
    finally:
        sys.path.remove(ROOT)
    a = mod.build_parser().parse_args(["-d", "x.tsv", "--ppc", "0.25", "--ppc_draws", "50", "--ppc_scale", "10", "--ppc_start_bin", "3"])
    assert (a.ppc, a.ppc_draws, a.ppc_scale, a.ppc_start_bin) == (0.25, 50, 10, 3)
    d = mod.build_parser().parse_args(["-d", "x.tsv"])
    assert (d.ppc, d.ppc_draws, d.ppc_scale, d.ppc_start_bin) == (-1.0, 1000, 100, -1)


@pytest.mark.parametrize("cli", ["DDRate", "trend_rate"])
@pytest.mark.parametrize("flags,said", [(["--ppc", "0.2", "-rm_first_bin", "1"], "-rm_first_bin"), (["--ppc", "1.0"], "burn-in"),
                                        (["--ppc", "0.2", "--ppc_draws", "0"], "at least 1"),
                                        (["--ppc", "0.2", "--ppc_scale", "0"], "at least 1")])
def test_cli_refuses_before_the_gpu_is_touched(cli, flags, said):
    code = ("import sys; sys.path.insert(0, %r)\nimport %s as cli\n"
            "try:\n    cli.main(['-d', 'no_such_file.tsv'] + %r)\nexcept SystemExit as e:\n"
            "    assert 'torch' not in sys.modules, 'torch was imported'\n    print('REFUSED', e)\n" % (ROOT, cli, flags))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0 and "REFUSED --ppc" in out.stdout and said in out.stdout, out.stdout + out.stderr
