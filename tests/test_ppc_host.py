"""The host side of the posterior predictive check (literate_amd/ppc.py): its numpy restatement tests/helpers/ppc_ref.py on
hand-built counts (a made-up simulator whose every number can be worked out by hand), ppc.py's own host functions against
it, the flag combinations LiteRateForward.py refuses before it touches the GPU, and the two new declarations."""
import os
import re
import sys

import numpy as np
import pytest

from helpers import ppc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fake_simulator(calls):
    """births of replicate r in bin b = (seed + r) % 5 + b, deaths = (seed + r) % 3; living follows; overflow when more
    than `capacity` lineages were created; a start < 1 is refused"""
    def sim(lam, mu, spb, n_start, seed, capacity):
        n, nb = np.shape(lam)
        calls.append(dict(lam=np.array(lam), mu=np.array(mu), spb=spb, n_start=np.array(n_start), seed=seed, capacity=capacity))
        counts, totals = np.zeros((n, 4, nb), dtype=np.int64), np.zeros((n, 4), dtype=np.int64)
        for r in range(n):
            if n_start[r] < 1 or n_start[r] > capacity:
                totals[r] = (0, 0, 1, -1)
                continue
            alive = int(n_start[r])
            for b in range(nb):
                counts[r, 0, b], counts[r, 1, b] = (seed + r) % 5 + b, min((seed + r) % 3, alive)
                counts[r, 2, b], counts[r, 3, b] = alive, alive * spb
                alive += counts[r, 0, b] - counts[r, 1, b]
            created = int(n_start[r] + counts[r, 0].sum())
            totals[r] = (created, alive, int(created > capacity), -1)
        return counts, totals
    return sim


def rates(R, n_bins):
    return np.arange(R * n_bins, dtype=float).reshape(R, n_bins) / 100, np.full((R, n_bins), .5)


def test_draw_indices():
    assert ppc_ref.draw_indices(10, 4).tolist() == [0, 2, 5, 7]
    assert ppc_ref.draw_indices(3, 50).tolist() == [0, 1, 2]            # n_draws > M: every row once
    assert ppc_ref.draw_indices(7, 7).tolist() == list(range(7))
    from literate_amd import ppc
    for M, n in ((10, 4), (3, 50), (7, 7), (1000, 333), (12345, 1000)):
        assert np.array_equal(ppc.draw_indices(M, n), ppc_ref.draw_indices(M, n))
    with pytest.raises(ValueError):
        ppc.draw_indices(0, 5)


def test_observed_diversity_and_start_bin():
    from literate_amd import ppc
    sp, ex = [0, 0, 2, 1, 0, 3], [0, 0, 0, 3, 0, 1]
    d = ppc_ref.div_obs_of(sp, ex)
    assert d.tolist() == [0, 0, 0, 2, 0, 0, 2]
    assert np.array_equal(ppc.observed_diversity(sp, ex), d)
    assert ppc_ref.start_bin_of(d) == 3 == ppc.pick_start_bin(d)        # div_obs[1] = 0: b0 > 1
    assert ppc_ref.start_bin_of(d, 3) == 3 == ppc.pick_start_bin(d, 3)
    for bad in (0, 4, 6, 9):                                            # nobody at its left edge / no such bin
        with pytest.raises(ValueError):
            ppc_ref.start_bin_of(d, bad)
        with pytest.raises(ValueError):
            ppc.pick_start_bin(d, bad)
    d1 = ppc_ref.div_obs_of([1, 2], [0, 0])
    assert ppc_ref.start_bin_of(d1) == 1 and ppc_ref.start_bin_of(d1, 1) == 1
    with pytest.raises(ValueError):
        ppc.pick_start_bin(np.array([0, 0, 0]))


def test_replicate_numbering_seeds_and_tables_on_hand_built_counts():
    sp, ex = np.array([0, 0, 2, 1, 0, 3]), np.array([0, 0, 0, 3, 0, 1])      # div_obs 0 0 0 2 0 0 2: interior empty bins
    R, nb = 4, 6
    lam, mu = rates(R, nb)
    calls = []
    out = ppc_ref.check(lam, mu, sp, ex, 10, 100, fake_simulator(calls), capacity=1000, start_time=5.0)
    assert out["start_bin"] == 3 and out["capacity"] == 1000
    free, step = calls
    assert free["seed"] == 100 and free["n_start"].tolist() == [2] * 4 and np.array_equal(free["lam"], lam[:, 3:])
    assert step["seed"] == 104 and step["lam"].shape == (12, 1)
    assert step["n_start"].tolist() == [2] * 4 + [0] * 4 + [0] * 4           # replicate (b - b0) * R + i
    assert step["lam"][:, 0].tolist() == [lam[i, b] for b in (3, 4, 5) for i in range(4)]
    assert out["step"]["simulated"].tolist() == [True, False, False]
    t = out["table"]
    assert t[:, 0].tolist() == [5, 6, 7, 8, 9, 10]
    assert t[:, 1].tolist() == sp.tolist() and t[:, 6].tolist() == ex.tolist() and t[:, 11].tolist() == [0, 0, 0, 2, 0, 0]
    assert np.isnan(t[:3, 2:6]).all() and np.isnan(t[:3, 7:11]).all() and np.isnan(t[:4, 12:16]).all()
    assert np.isnan(t[4:, 2:6]).all() and np.isnan(t[4:, 7:11]).all()        # empty bins: observed only
    # one step ahead in bin 3: births (104 + i) % 5 = 4, 0, 1, 2; observed 1 -> mean 1.75, p_ge 3/4; HPD of 4 values: n_in 4
    assert t[3, 1:6].tolist() == [1, 1.75, 0, 4, .75]
    # deaths (104 + i) % 3 = 2, 0, 1, 2; observed 3 -> p_ge 0
    assert t[3, 6:11].tolist() == [3, 1.25, 0, 2, 0]
    # free-running, seeds 100 .. 103: births per bin k = i + k, deaths (100 + i) % 3 = 1, 2, 0, 1
    # diversity at bin 4 = 2 + i - d = 1, 1, 4, 4; observed 0
    assert t[4, 11:16].tolist() == [0, 2.5, 1, 4, 1]
    f = out["fit"]
    assert (f["draws"], f["start_bin"], f["n_start"], f["free_kept"], f["step_kept"], f["step_overflowed"]) == (4, 3, 2, 4, 4, 0)
    # total births 3 i + 3 = 3, 6, 9, 12; observed 1 + 0 + 3 = 4: p_ge 3/4
    assert (f["total_births_obs"], f["total_births_mean"], f["total_births_p_ge"]) == (4, 7.5, .75)
    assert f["coverage_sp_events"] == 1.0 and f["coverage_ex_events"] == 0.0
    a, b = ppc_ref.file_text(t, f)
    assert a.splitlines()[0].split("\t") == ppc_ref.PPC_HEAD and len(a.splitlines()) == 7
    assert a.splitlines()[4].split("\t")[:6] == ["8.0", "1.0", "1.75", "0.0", "4.0", "0.75"]
    assert b.splitlines()[1].split("\t")[:4] == ["4", "10", "3", "2"]


def test_ties_at_the_observed_value_count_as_greater_or_equal():
    s = ppc_ref.stats_of(np.array([[3.], [3.], [3.], [2.], [5.]]), np.array([3.]))
    assert s[0].tolist() == [3, 3.2, 2, 5, .8]
    assert ppc_ref.coverage(np.array([[2., 1, 2, 5, 0], [6., 1, 2, 5, 0], [5., 1, 2, 5, 0], [0., np.nan, np.nan, np.nan, np.nan]])) == 2 / 3


def test_overflowed_draws_leave_both_tables_and_all_overflowed_is_an_error():
    sp, ex = np.array([3, 2, 1, 1]), np.array([0, 1, 1, 0])
    lam, mu = rates(40, 4)
    calls = []
    # capacity 16: free-running replicates with (100 + i) % 5 >= 3 create 3 + 3 b + 3 + ... > 16 lineages
    out = ppc_ref.check(lam, mu, sp, ex, 2, 100, fake_simulator(calls), capacity=16)
    fr = out["free"]
    assert out["start_bin"] == 1 and 0 < fr["kept"].sum() < 40
    assert np.array_equal(fr["kept"], fr["totals"][:, 2] == 0)
    assert out["fit"]["free_overflowed"] == 40 - fr["kept"].sum() and out["fit"]["step_overflowed"] == 0
    with pytest.raises(ValueError):
        ppc_ref.check(lam, mu, sp, ex, 2, 100, fake_simulator([]), capacity=4)     # every free-running replicate overflows
    # a draw any of whose one-bin replicates overflowed leaves the one-step tables as a whole
    def sim(lam_, mu_, spb, n_start, seed, capacity):
        counts, totals = fake_simulator([])(lam_, mu_, spb, n_start, seed, capacity)
        if np.shape(lam_)[1] == 1:
            totals[40 + 7, 2] = 1                                       # bin b0 + 1, draw 7
        return counts, totals
    out = ppc_ref.check(lam, mu, sp, ex, 2, 100, sim, capacity=1000)
    assert out["step"]["kept"].sum() == 39 and not out["step"]["kept"][7] and out["fit"]["step_overflowed"] == 1


def test_ppc_writer_and_coverage_agree_with_the_restatement(tmp_path):
    from literate_amd import ppc
    sp, ex = np.array([0, 0, 2, 1, 0, 3]), np.array([0, 0, 0, 3, 0, 1])
    lam, mu = rates(30, 6)
    out = ppc_ref.check(lam, mu, sp, ex, 10, 7, fake_simulator([]), capacity=1000, start_time=-3.0)
    assert ppc.PPC_HEAD == ppc_ref.PPC_HEAD and ppc.FIT_HEAD == ppc_ref.FIT_HEAD
    ppc.write_tables(str(tmp_path / "x"), out["table"], out["fit"])
    a, b = ppc_ref.file_text(out["table"], out["fit"])
    assert open(tmp_path / "x_PPC.tsv").read() == a and open(tmp_path / "x_PPC_fit.tsv").read() == b
    for c in (slice(1, 6), slice(6, 11), slice(11, 16)):
        got, want = ppc.coverage(out["table"][:, c]), ppc_ref.coverage(out["table"][:, c])
        assert got == want or (np.isnan(got) and np.isnan(want))
    assert ppc.default_capacity(sp) == 1 << 16 and ppc.default_capacity([30217]) == 8 * 30217


@pytest.mark.parametrize("flags", [["--ppc", "1.0"], ["--ppc", "-0.5"], ["--ppc", "0.2", "-model_BDI", "1"],
                                   ["--ppc", "0.2", "-pyrate_output"], ["--ppc", "0.2", "--ppc_draws", "0"],
                                   ["--ppc", "0.2", "--ppc_scale", "0"]])
def test_cli_refuses_before_the_gpu_is_touched(flags):
    import subprocess
    code = ("import sys; sys.path.insert(0, %r)\nimport LiteRateForward as cli\n"
            "try:\n    cli.main(['-d', 'no_such_file.tsv'] + %r)\nexcept SystemExit as e:\n"
            "    assert 'torch' not in sys.modules, 'torch was imported'\n    print('REFUSED', e)\n" % (ROOT, flags))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0 and "REFUSED --ppc" in out.stdout, out.stdout + out.stderr


def test_header_declares_and_binding_binds_the_batched_simulator():
    from literate_amd import _hip
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        text = f.read()
    for name in ("lr_simulate_bd_batch_workspace_bytes", "lr_simulate_bd_batch"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["lr_simulate_bd_batch"][1]) == 13 and len(_hip.SIGNATURES["lr_simulate_bd_batch_workspace_bytes"][1]) == 4
    for name, value in (("LR_SIMBATCH_GROUPS", _hip.LR_SIMBATCH_GROUPS), ("LR_SIMBATCH_LDS_SLOTS", _hip.LR_SIMBATCH_LDS_SLOTS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == value
    with open(os.path.join(ROOT, "literate_amd", "build.py")) as f:
        assert '"lr_simbatch.hip"' in f.read()


def test_size_query_and_argument_errors_need_no_device():
    """the size query is host arithmetic, and the argument checks come before any device call"""
    from literate_amd import _hip
    lib = _hip.load()
    q = lib.lr_simulate_bd_batch_workspace_bytes
    lds, groups = _hip.LR_SIMBATCH_LDS_SLOTS, _hip.LR_SIMBATCH_GROUPS
    assert q(3, 5, 4, 1000) == q(3, 5, 4, lds) == 256                       # the whole list fits LDS: only the ticket
    assert q(3, 5, 4, lds + 64) == 256 + 3 * 64 * 4                         # one slice per work-group, not per replicate
    assert q(10 * groups, 5, 4, lds + 64) == q(groups, 5, 4, lds + 64) == 256 + groups * 64 * 4
    for bad in ((0, 5, 4, 10), (3, 0, 4, 10), (3, 5, 0, 10), (3, _hip.LR_MAX_BINS + 1, 4, 10), (3, 5, 4, 0), (3, 5, 4, 1 << 31)):
        assert q(*bad) == _hip.LR_ERR_SIZE, bad
    assert q(3, _hip.LR_MAX_BINS, 4, (1 << 31) - 1) > 0
    assert lib.lr_simulate_bd_batch(None, None, 3, 5, 4, None, 10, 1, None, None, None, 0, None) == _hip.LR_ERR_NULL
