"""Host side of the posterior summary of the parametric samplers (lr_col_summary, lr_curve_summary): the numpy restatement
against the reference's own output, the ABI declaration and binding, the argument checks the library makes before it
touches a device, the TSV writer and the CLIs' refusals.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import summary_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lr_col_summary_workspace_bytes", "lr_col_summary", "lr_curve_summary_workspace_bytes", "lr_curve_summary")


def test_restatement_reproduces_make_vec_dict_on_the_shipped_log(golden_dir):
    """tests/golden/plotdd_shipped.npz: plotDD.py make_vec_dict run by the reference on its shipped DDRate log"""
    P = np.load(os.path.join(golden_dir, "plotdd_shipped.npz"))
    for cols, mean, lo, hi in (("l", "birth_rate", "birth_minHPD", "birth_maxHPD"),
                               ("m", "death_rate", "death_minHPD", "death_maxHPD"),
                               ("niche_cols", "niche", "niche_minHPD", "niche_maxHPD")):
        X = P[cols]
        assert X.shape == (1000, 32)
        t = sr.triples(X)
        assert np.array_equal(t[:, 1], P[lo]) and np.array_equal(t[:, 2], P[hi]), cols
        assert np.allclose(t[:, 0], P[mean], rtol=1e-12, atol=0), cols
        one = np.array([sr.triple(X[:, i]) for i in range(0, 32, 5)])          # the scan as the reference writes it
        assert np.array_equal(one[:, 1:], t[::5, 1:]) and np.allclose(one[:, 0], t[::5, 0], rtol=1e-12, atol=0)
    # the grouping rules on the same columns: one chain, no burn-in is the table itself
    g = sr.col_summary(P["l"][:, None, :], 1000, range(32), 0.0, True)
    assert g.shape == (1, 32, 3) and np.array_equal(g[0, :, 1], P["birth_minHPD"])


def test_restatement_rules():
    assert [sr.n_in_of(n) for n in (2, 10, 30, 1)] == [2, 10, 28, 1]           # round half to even: 28.5 -> 28
    t = sr.triple([1.0] + [2.0] * 18 + [3.0])                                  # two windows of width 1: the first
    assert t.tolist() == [2.0, 1.0, 2.0]
    assert np.isnan(sr.triple([1.0, np.nan, 2.0])).all()
    assert sr.triple([5.0, 5.0, 5.0]).tolist() == [5.0, 5.0, 5.0]
    with pytest.raises(RuntimeError):
        sr.triple([1.0])
    T = np.arange(24, dtype=float).reshape(4, 3, 2)                            # [S, C, K]: pooled = chain after chain
    g = sr.groups(T, 4, 0.5, True)[0]
    assert g[:, 0].tolist() == [12.0, 18.0, 14.0, 20.0, 16.0, 22.0]
    assert [x[:, 0].tolist() for x in sr.groups(T, 4, 0.5, False)] == [[12.0, 18.0], [14.0, 20.0], [16.0, 22.0]]


def test_summary_entry_points_declared_and_bound():
    from literate_amd import _hip
    header = open(os.path.join(ROOT, "include", "literate_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(lr_\w+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in _hip.SIGNATURES
        assert hasattr(_hip.load(), name)


def _cols(*c):
    a = np.asarray(c, dtype=np.int32)
    return a, a.ctypes.data_as(__import__("ctypes").c_void_p), len(c)


def test_col_summary_query_checks_its_arguments_on_the_host():
    from literate_amd import _hip
    q = _hip.load().lr_col_summary_workspace_bytes
    keep, p, k = _cols(0, 3)
    E = _hip.LR_ERR_SIZE
    assert q(1000, 4, 12, p, k, 1.0, 1, 0) == E and q(1000, 4, 12, p, k, -0.1, 1, 0) == E     # burn-in outside [0, 1)
    assert q(1000, 4, 12, p, k, float("nan"), 1, 0) == E
    assert q(0, 4, 12, p, k, 0.2, 1, 0) == E and q(1000, 0, 12, p, k, 0.2, 1, 0) == E and q(1000, 4, 0, p, k, 0.2, 1, 0) == E
    assert q(1000, 4, 3, p, k, 0.2, 1, 0) == E                                                 # column 3 of 3
    assert q(1000, 4, 12, p, 0, 0.2, 1, 0) == E
    assert q(1000, 4, 12, None, 2, 0.2, 1, 0) == _hip.LR_ERR_NULL
    assert q(1000, 4, 12, p, k, 0.2, 1, 3) == E                                                # 3 columns per pass of 2
    # calcHPD raises below two samples in the window; no 0.9 cap on the burn-in
    assert q(1, 1, 12, p, k, 0.0, 0, 0) == E
    assert q(3, 1, 12, p, k, 0.7, 0, 0) == E                    # int(2.1) = 2 dropped: one row
    assert q(20, 1, 12, p, k, 0.95, 0, 0) == E                  # 19 dropped (plotRJforward's cap would keep 2)
    assert q(20, 4, 12, p, k, 0.95, 0, 0) == E                  # per chain: one row each
    # the same shapes with enough rows pass the argument checks: a size, or LR_ERR_STATE where no device answers
    for ok in (q(2, 1, 12, p, k, 0.0, 0, 0), q(3, 1, 12, p, k, 0.5, 0, 0), q(20, 4, 12, p, k, 0.95, 1, 0),
               q(1000, 4, 12, p, k, 0.2, 1, 1)):
        assert ok > 0 or ok == _hip.LR_ERR_STATE
    assert keep.size == 2


def test_curve_summary_query_checks_its_arguments_on_the_host():
    from literate_amd import _hip
    q = _hip.load().lr_curve_summary_workspace_bytes
    E = _hip.LR_ERR_SIZE
    for sampler in (0, 3, -1):
        assert q(1000, 4, 139, 4, sampler, 32, 0.2, 1, 0) == _hip.LR_ERR_MODEL
    assert q(1000, 4, 139, 4, 1, 0, 0.2, 1, 0) == E and q(1000, 4, 139, 4, 1, _hip.LR_MAX_BINS + 1, 0.2, 1, 0) == E
    assert q(1000, 4, 12, 5, 1, 32, 0.2, 1, 0) == E             # 8 parameters from column 5 of 12
    assert q(1000, 4, 12, 4, 1, 32, 0.2, 1, 0) != E and q(1000, 4, 10, 4, 2, 32, 0.2, 1, 0) != E
    assert q(1000, 4, 9, 4, 2, 32, 0.2, 1, 0) == E and q(1000, 4, 139, -1, 2, 32, 0.2, 1, 0) == E
    assert q(1000, 4, 139, 4, 1, 32, 1.0, 1, 0) == E and q(1000, 4, 139, 4, 1, 32, 0.2, 1, 33) == E
    assert q(20, 1, 139, 4, 1, 32, 0.95, 1, 0) == E and q(20, 2, 139, 4, 1, 32, 0.95, 1, 0) != E
    ok = q(1000, 256, 139, 4, 1, 128, 0.2, 1, 0)
    assert ok > 0 or ok == _hip.LR_ERR_STATE


def test_summaries_have_no_cpu_path(monkeypatch):
    import torch
    from literate_amd import _hip, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_hip.HipLibraryError):
        ops.col_summary(np.zeros((4, 1, 12)), 4, [1, 2])
    with pytest.raises(_hip.HipLibraryError):
        ops.curve_summary(np.zeros((4, 1, 12)), 4, 1, np.ones(8), 2, 2)


def test_summary_geometry_is_the_library_rule():
    from literate_amd import ops
    assert ops.summary_geometry(1000, 256, 0.2, True) == (200, 204800, 194560)
    assert ops.summary_geometry(30, 5, 0.0, False) == (0, 30, 28)
    assert ops.summary_geometry(20, 2, 0.95, True) == (19, 2, 2)
    assert ops.CURVE_KINDS == {1: ("birth", "death", "net", "niche", "nicheFrac"), 2: ("birth", "death", "net")}


@pytest.mark.parametrize("kinds", [("birth", "death", "net", "niche", "nicheFrac"), ("birth", "death", "net")])
def test_summary_tables_round_trip(tmp_path, kinds):
    from literate_amd import logs
    nb = 4
    rng = np.random.default_rng(5)
    values = rng.gamma(2.0, 0.1, (len(kinds), 3, nb))
    values[0, 0, 1], values[1, 2, 3] = 1e-05, 1.5e+16
    values[2, :, 2] = np.nan
    DT = np.array([3.0, 7.5, 11.0, 0.0])
    n_spec, n_exti = np.array([1, 2, 0, 4]), np.array([0, 1, 1, 0])
    names = ["posterior", "likelihood", "prior", "a", "b"]
    params = rng.normal(0, 10, (5, 3))
    stem = str(tmp_path / "run_7_X")
    logs.write_summary_tables(stem, 1968.0, DT, n_spec, n_exti, kinds, values, names, params)
    lines = open(stem + "_summary.tsv").read().splitlines()
    head = lines[0].split("\t")
    want = ["time", "net_diversity", "emp_birth", "emp_death", "birth_rate", "birth_minHPD", "birth_maxHPD", "death_rate",
            "death_minHPD", "death_maxHPD"]
    if "niche" in kinds:
        want += ["niche", "niche_minHPD", "niche_maxHPD"]
    want += ["net_rate", "net_minHPD", "net_maxHPD"]
    if "nicheFrac" in kinds:
        want += ["nicheFrac", "nicheFrac_minHPD", "nicheFrac_maxHPD"]
    assert head == want and len(lines) == nb + 1
    tab = np.array([[float(x) for x in l.split("\t")] for l in lines[1:]])
    assert tab[:, 0].tolist() == [1968.5, 1969.5, 1970.5, 1971.5] and np.array_equal(tab[:, 1], DT)
    assert np.isnan(tab[0, 2]) and np.isnan(tab[0, 3])                                   # plotDD.py:16-17
    assert tab[1:3, 2].tolist() == [2 / 7.5, 0.0] and tab[3, 2] == np.inf and tab[1, 3] == 1 / 7.5
    for k, kind in enumerate(kinds):
        c = head.index(logs.SUMMARY_KIND_HEAD[kind][0])
        assert head[c:c + 3] == logs.SUMMARY_KIND_HEAD[kind]
        assert np.array_equal(tab[:, c:c + 3], values[k].T, equal_nan=True)              # str(float) round-trips
    assert lines[2].split("\t")[head.index("birth_rate")] == "1e-05"
    assert lines[4].split("\t")[head.index("death_maxHPD")] == "1.5e+16"
    plines = [l.split("\t") for l in open(stem + "_summary_params.tsv").read().splitlines()]
    assert plines[0] == ["parameter", "mean", "minHPD", "maxHPD"] and [p[0] for p in plines[1:]] == names
    assert np.array_equal(np.array([[float(x) for x in p[1:]] for p in plines[1:]]), params)


def test_summary_arg_error():
    from literate_amd.logs import summary_arg_error
    assert summary_arg_error(0.2, 1000, 10, 4) is None and summary_arg_error(0.0, 20, 10, 1) is None
    assert "burn-in" in summary_arg_error(1.0, 1000, 10, 4) and "burn-in" in summary_arg_error(-0.5, 1000, 10, 4)
    assert "at least 2" in summary_arg_error(0.95, 200, 10, 1)          # 20 samples, 19 dropped: one left
    assert summary_arg_error(0.95, 200, 10, 2) is None                  # pooled: two left, window round(1.9) = 2
    assert "at least 2" in summary_arg_error(0.2, 0, 10, 4)


@pytest.mark.parametrize("cli,extra", [("DDRate.py", []), ("trend_rate.py", ["-trend_data", "none.tsv"])])
def test_clis_refuse_summary_arguments_before_any_gpu_import(cli, extra):
    """in a child process whose torch import would raise: the refusal comes first"""
    code = ("import sys, runpy\n"
            "sys.modules['torch'] = None\n"                       # `import torch` now raises ImportError
            "sys.argv = %r\n"
            "runpy.run_path(%r, run_name='__main__')\n")
    for args, msg in ((["--summary", "1.0"], "burn-in fraction"), (["--summary", "0.95", "-n", "200", "-s", "10"], "at least 2")):
        argv = [cli, "-d", "none.tsv"] + extra + args
        out = subprocess.run([sys.executable, "-c", code % (argv, os.path.join(ROOT, cli))], capture_output=True, text=True,
                             timeout=120, cwd=ROOT)
        assert out.returncode != 0 and msg in out.stderr and "ImportError" not in out.stderr, out.stderr
    import importlib
    mod = importlib.import_module(cli[:-3])
    assert mod.build_parser().parse_args(["-d", "x.tsv"] + extra).summary < 0          # off by default
