"""Host side of the posterior rates-through-time summary (lr_rtt_summary): the ABI declaration and binding, the argument
checks the library makes before it touches a device, the TSV writer and the CLI's refusals.  No GPU needed."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rtt_entry_points_declared_and_bound():
    from literate_amd import _hip
    header = open(os.path.join(ROOT, "include", "literate_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(lr_\w+)\s*\(", header, flags=re.M))
    for name in ("lr_rtt_summary_workspace_bytes", "lr_rtt_summary"):
        assert name in declared and name in _hip.SIGNATURES
        assert hasattr(_hip.load(), name)


def test_rtt_workspace_query_rejects_what_the_reference_cannot_summarise():
    from literate_amd import _hip
    q = _hip.load().lr_rtt_summary_workspace_bytes
    # b - a integer valued: np.arange gives int(b - a) + 1 edges, one bin short of the nbins the reference indexes
    assert q(1000, 1, 1968.0, 2000.0, 0.2, 0) == _hip.LR_ERR_SIZE
    # fewer than one bin, reversed ages, NaN
    assert q(1000, 1, 0.0, 0.5, 0.2, 0) == _hip.LR_ERR_SIZE
    assert q(1000, 1, 2000.5, 1968.0, 0.2, 0) == _hip.LR_ERR_SIZE
    assert q(1000, 1, float("nan"), 2000.5, 0.2, 0) == _hip.LR_ERR_SIZE
    # burn-in outside [0, 1)
    assert q(1000, 1, 1968.0, 2000.5, 1.0, 0) == _hip.LR_ERR_SIZE
    assert q(1000, 1, 1968.0, 2000.5, -0.1, 0) == _hip.LR_ERR_SIZE
    # calcHPD raises below two samples in the window: n = 2 -> round(1.9) = 2 is enough, n = 1 is not
    assert q(2, 1, 0.0, 3.5, 0.0, 0) != _hip.LR_ERR_SIZE
    assert q(1, 1, 0.0, 3.5, 0.0, 0) == _hip.LR_ERR_SIZE
    assert q(3, 1, 0.0, 3.5, 0.5, 0) != _hip.LR_ERR_SIZE       # int(1.5) = 1 row dropped, 2 left
    assert q(3, 1, 0.0, 3.5, 0.7, 0) == _hip.LR_ERR_SIZE       # int(2.1) = 2 dropped: one row, n_in = 1
    assert q(10, 1, 0.0, 3.5, 0.95, 0) == _hip.LR_ERR_SIZE     # per chain: int(9.5) = 9 dropped (the cap is 9 too)
    assert q(10, 2, 0.0, 3.5, 0.95, 1) != _hip.LR_ERR_SIZE     # pooled: 2 chains x (10 - 9) rows = 2
    assert q(20, 1, 0.0, 3.5, 0.95, 0) != _hip.LR_ERR_SIZE     # per chain: min(int(19.0), int(18.0)) = 18 -> 2 rows
    assert q(20, 1, 0.0, 3.5, 0.95, 1) == _hip.LR_ERR_SIZE     # pooled, no cap: 19 dropped, 1 row


def test_rtt_python_round_matches_the_library_threshold():
    """n_in = round(0.95 n), half to even: n = 30 gives 28.5 -> 28 (Python), not 29."""
    assert int(round(0.95 * 30)) == 28 and int(round(0.95 * 10)) == 10 and int(round(0.95 * 2)) == 2


def test_rtt_summary_has_no_cpu_path(monkeypatch):
    import torch
    from literate_amd import _hip, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.HipLibraryError):
        ops.rtt_summary(np.zeros((4, 1, _hip.LR_TRACE_W)), 4, 0.0, 3.5)


def test_rtt_time_vector_is_get_marginal_rates_time_frames():
    from literate_amd import ops
    t = ops.rtt_time(1968.0, 2000.5)
    assert np.array_equal(t, np.arange(1968.5, 2000.5, 1.0)) and t.size == 32
    edges = np.arange(0.3, 7.9)
    assert np.array_equal(ops.rtt_time(0.3, 7.9), (edges - abs(edges[1] - edges[0]) / 2.)[1:])


def test_rtt_tables_format(tmp_path):
    from literate_amd import logs
    nb = 3
    time = np.array([0.5, 1.5, 2.5])
    rates = np.arange(27, dtype=float).reshape(3, 3, nb) / 7.0
    freq = np.array([[0.0, 0.25, 1e-05], [0.5, 0.0, 0.0]])
    kc = np.zeros((2, 32), dtype=np.int64)
    kc[0, 0], kc[1, 2] = 5, 7
    stem = str(tmp_path / "x_BD")
    logs.write_rtt_tables(stem, time, rates, freq, kc)
    lines = open(stem + "_RTT.tsv").read().splitlines()
    assert lines[0].split("\t") == ["time", "birth_rate", "birth_minHPD", "birth_maxHPD", "death_rate", "death_minHPD",
                                    "death_maxHPD", "net_rate", "net_minHPD", "net_maxHPD", "birth_counts", "death_counts"]
    assert len(lines) == nb + 1
    for i in range(nb):
        want = [time[i]] + [rates[k, s, i] for k in range(3) for s in range(3)] + [freq[0, i], freq[1, i]]
        assert lines[i + 1].split("\t") == [str(float(v)) for v in want]
    assert lines[3].split("\t")[-2] == "1e-05"
    k = open(stem + "_RTT_K.tsv").read().splitlines()
    assert k[0] == "n_rates\tK_l\tK_m" and len(k) == 33
    assert k[1] == "1\t5\t0" and k[3] == "3\t0\t7"


def test_cli_refuses_rtt_with_pyrate_output_and_bad_burnin():
    import LiteRateForward as cli
    assert cli.build_parser().parse_args(["-d", "x.tsv"]).rtt < 0          # off by default
    with pytest.raises(SystemExit, match="pyrate_output"):
        cli.main(["-d", "x.tsv", "--rtt", "0.2", "-pyrate_output"])
    with pytest.raises(SystemExit, match="burn-in"):
        cli.main(["-d", "x.tsv", "--rtt", "1.0"])
