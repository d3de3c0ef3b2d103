"""Host side of the convergence summary (lr_ess_summary): the ABI declaration and binding, the argument checks the size
query makes without a device, the numpy restatement on the worked example, the TSV writers and the CLIs' refusals of a
bad --ess.  No GPU needed."""
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

from helpers import ess_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ess_entry_points_declared_bound_and_exported():
    from literate_amd import _hip
    header = open(os.path.join(ROOT, "include", "literate_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(lr_\w+)\s*\(", header, flags=re.M))
    for name in ("lr_ess_summary_workspace_bytes", "lr_ess_summary"):
        assert name in declared and name in _hip.SIGNATURES
        assert hasattr(_hip.load(), name)
    # the LDS cut-over the tests sit on both sides of is the library's
    assert int(re.search(r"#define LR_ESS_LDS_ROWS (\d+)", header).group(1)) == _hip.LR_ESS_LDS_ROWS


def _query(S, C=2, width=139, cols=(1, 5), burnin=0.1, max_lag=2000):
    from literate_amd import _hip
    c = np.ascontiguousarray(np.asarray(cols, dtype=np.int32))
    return _hip.load().lr_ess_summary_workspace_bytes(S, C, width, c.ctypes.data_as(_hip.c_vp) if c.size else None,
                                                       int(c.size), burnin, max_lag)


def test_ess_workspace_query_refusals():
    from literate_amd import _hip
    E = _hip.LR_ERR_SIZE
    # n = S - int(burnin S) >= 4: both sides of 4
    assert _query(4, burnin=0.0) > 0 and _query(3, burnin=0.0) == E
    assert _query(5, burnin=0.2) > 0                  # int(1.0) = 1 dropped, 4 kept
    assert _query(5, burnin=0.4) == E                 # int(2.0) = 2 dropped, 3 kept
    assert _query(1000, burnin=0.996) > 0 and _query(1000, burnin=0.997) == E
    # burn-in outside [0, 1), NaN
    for b in (1.0, -0.1, 1.5, float("nan")):
        assert _query(1000, burnin=b) == E, b
    # columns: none, negative, past the row
    assert _query(1000, cols=()) == E
    assert _query(1000, cols=(1, -1)) == E
    assert _query(1000, width=13, cols=(1, 13)) == E and _query(1000, width=13, cols=(0, 12)) > 0
    # max_lag >= 1, chains >= 1
    assert _query(1000, max_lag=0) == E and _query(1000, max_lag=1) > 0
    assert _query(1000, C=0) == E


def test_ess_workspace_grows_past_the_lds_cut_over():
    from literate_amd import _hip
    cut = _hip.LR_ESS_LDS_ROWS
    small = _query(cut, burnin=0.0)
    big = _query(cut + 1, burnin=0.0)
    assert small == _query(5, burnin=0.0)             # the half-chain statistics only
    assert big >= small + 8 * 2 * 2 * (cut + 1)       # + a centred copy of every series


def test_restatement_reproduces_the_worked_example_exactly():
    x = np.array([F(v) for v in (1, 3, 2, 4, 3, 5, 4, 6)], dtype=object)
    r = er.series(x, 2000)
    assert r["mean"] == F(7, 2)
    assert [er.autocov(r["d"], t) for t in range(5)] == [F(9, 4), F(9, 28), F(17, 12), F(-17, 20), F(1, 4)]
    assert r["V"] == F(481, 84) and r["stop_lag"] == 4
    assert r["act"] == F(481, 189) and r["ess"] == F(1512, 481) and r["se2"] == F(481, 672)
    assert r["se_mean"] == pytest.approx(0.846034, abs=1e-6) and float(r["ess"]) == pytest.approx(3.143451, abs=1e-6)
    assert er.rhat_of([x])[1] == F(39, 20) and er.rhat_of([x])[0] == pytest.approx(1.396424, abs=1e-6)
    y = np.array([F(v) for v in (2, 2, 3, 3, 4, 4, 5, 5)], dtype=object)
    ry = er.series(y, 2000)
    assert float(ry["ess"]) == pytest.approx(2.584615, abs=1e-6) and ry["stop_lag"] == 4
    assert float(r["ess"] + ry["ess"]) == pytest.approx(5.728067, abs=1e-6)
    assert er.rhat_of([x, y])[1] == F(25, 12) and er.rhat_of([x, y])[0] == pytest.approx(1.443376, abs=1e-6)
    # in float64 through the whole-call restatement
    rows = np.stack([np.array(v, dtype=float) for v in ([1, 3, 2, 4, 3, 5, 4, 6], [2, 2, 3, 3, 4, 4, 5, 5])], 1)[:, :, None]
    s = er.summary(rows, 8, [0], burnin=0.0)
    assert s["stop_lag"][:, 0].tolist() == [4, 4]
    assert s["pooled_ess"][0] == pytest.approx(5.728067, abs=1e-6) and s["rhat"][0] == pytest.approx(1.443376, abs=1e-6)


def test_restatement_edges():
    """constant series (the value as its mean even where sum / n is not), max_lag 1, max_lag before the stop"""
    n = next(n for n in range(4, 64) if np.full(n, 0.1).sum() / n != 0.1)
    x = np.full(n, 0.1)
    r = er.series(x, 2000)
    assert r["mean"] == 0.1 and r["stop_lag"] == 0 and np.isnan(r["ess"]) and r["se_mean"] == 0
    z = np.cumsum(np.ones(50))                            # a ramp: every pair sum positive up to n - 1
    assert er.series(z, 1)["stop_lag"] == 1 and er.series(z, 1)["ess"] == 50
    assert er.series(z, 6)["stop_lag"] == 6
    rh = er.rhat_of([np.full(8, 2.0), np.full(8, 2.0)])
    assert np.isnan(rh[0])


def test_ess_tables_format(tmp_path):
    from literate_amd import logs, ops
    ess = np.array([[300.5, np.nan], [150.25, np.nan], [150.25, np.nan]])
    act = np.array([[2.0, np.nan], [3.0, np.nan], [3.5, np.nan]])
    res = ops.EssSummary(np.full((3, 2), 0.1), ess, act, np.full((3, 2), 1e-05), np.array([[4, 0], [6, 0], [6, 0]]),
                         np.array([0.1, 0.3]), np.array([601.0, np.nan]), np.array([1.01, np.nan]), 10)
    stem = str(tmp_path / "x_BD")
    line = logs.write_ess_tables(stem, ["posterior", "K_l"], res, 1000)
    top = open(stem + "_ESS.tsv").read().splitlines()
    assert top[0].split("\t") == ["parameter", "mean", "ess_pooled", "ess_min", "chain_ess_min", "rhat",
                                  "chains_ess_below_200", "chains_constant"]
    assert top[1].split("\t") == ["posterior", "0.1", "601.0", "150.25", "1", "1.01", "2", "0"]
    assert top[2].split("\t") == ["K_l", "0.3", "nan", "nan", "nan", "nan", "0", "3"]
    ch = open(stem + "_ESS_chains.tsv").read().splitlines()
    assert ch[0].split("\t") == ["chain", "parameter", "mean", "ess", "act", "se_mean", "stop_lag"]
    assert len(ch) == 7
    assert ch[1].split("\t") == ["0", "posterior", "0.1", "300.5", "2000.0", "1e-05", "4"]
    assert ch[2].split("\t") == ["0", "K_l", "0.1", "nan", "nan", "1e-05", "0"]
    assert ch[5].split("\t")[4] == str(3.5 * 1000)
    assert "150.25 (posterior, chain 1)" in line and "1.01 (posterior)" in line and "2 of 3 chains" in line


@pytest.mark.parametrize("cli", ["LiteRateForward", "DDRate", "trend_rate"])
def test_clis_refuse_a_bad_ess_before_touching_a_device(cli, monkeypatch):
    import importlib
    import torch
    from literate_amd import _hip

    def no_device(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(_hip, "require_gpu", no_device)
    mod = importlib.import_module(cli)
    assert mod.build_parser().parse_args(["-d", "x.tsv"]).ess == -1.0          # off by default
    for bad in ("1.0", "-0.5", "1.5", "nan"):
        with pytest.raises(SystemExit, match="burn-in fraction"):
            mod.main(["-d", "x.tsv", "--ess", bad])
    # ceil(n / s) - int(BURNIN ceil(n / s)) < 4
    with pytest.raises(SystemExit, match="at least 4"):
        mod.main(["-d", "x.tsv", "-n", "30", "-s", "10", "--ess", "0.0"])      # 3 samples
    with pytest.raises(SystemExit, match="at least 4"):
        mod.main(["-d", "x.tsv", "-n", "41", "-s", "10", "--ess", "0.4"])      # 5 samples, int(2.0) dropped
    with pytest.raises(SystemExit, match="at least 4"):
        mod.main(["-d", "x.tsv", "-n", "0", "--ess", "0.1"])
    from literate_amd.logs import ess_arg_error
    assert ess_arg_error(0.2, 41, 10) is None and ess_arg_error(0.0, 31, 10) is None     # 4 kept: accepted


def test_ess_summary_has_no_cpu_path(monkeypatch):
    import torch
    from literate_amd import _hip, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.HipLibraryError):
        ops.ess_summary(np.zeros((8, 2, 13)), 8, [1, 2])
