"""lr_col_summary / lr_curve_summary on the device: mean and 95 % HPD of log columns and of the per-bin curves of DDRate.py
and trend_rate.py (what plotDD.py make_vec_dict and logAverager.py take of the logs) against the numpy restatement
tests/helpers/summary_ref.py - on the reference's own output, engine runs against their own log columns, hand-built
edges, chunked calls, cfg5's shape and the CLIs.  Every case runs in a child process under a time limit
(tests/helpers/post_summary_cases.py); HPD ends must be bit-identical, means within rtol 1e-12."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "post_summary_cases.py")


@pytest.fixture(scope="module")
def G(golden_dir):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return np.load(os.path.join(golden_dir, "binning_lik.npz"))


def _env():
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def run_case(*args, timeout=300):
    out = subprocess.run([sys.executable, CASES] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout,
                         env=_env(), cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "case %s ok" % " ".join(str(a) for a in args) in out.stdout


# ---- 1. the reference's own output ---------------------------------------------------------------------------------
def test_col_summary_matches_make_vec_dict_on_the_shipped_log(G):
    run_case("golden")


# ---- 2. curves against the log -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb,md", [(2, 2), (1, 1), (0, 0), (2, 0), (1, 2)])
def test_ddrate_engine_summary_is_the_summary_of_its_log_columns(G, mb, md):
    run_case("dd_engine", mb, md)


@pytest.mark.parametrize("cb,cd", [(0, 0), (1, 0), (0, 1)])
def test_trend_engine_summary_is_the_summary_of_its_log_columns(G, cb, cd):
    run_case("trend_engine", cb, cd)


# ---- 3. - 5. edges, chunking, size ------------------------------------------------------------------------------------
def test_summary_edges(G):
    run_case("edges")


def test_summary_chunked_calls_are_bitwise_the_full_call(G):
    run_case("chunking")


def test_curve_summary_cfg5_shape_pooled_under_a_1_gib_cap(G):
    run_case("cfg5", timeout=900)


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------
def _bands_data(G, tmp_path):
    ts, te = G["metal_bands/lib_ts"], G["metal_bands/lib_te"] - 0.5
    data = tmp_path / "bands.tsv"
    with open(data, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, c) in enumerate(zip(ts, te)):
            f.write("%d\t%g\t%g\n" % (i, a, c))
    return data


def test_ddrate_cli_summary_matches_restatement_on_its_logs(G, tmp_path):
    from helpers import post_summary_cases as pc
    from literate_amd.ddrate import LOG_HEAD
    data = _bands_data(G, tmp_path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "DDRate.py"), "-d", str(data), "-n", "800", "-s", "10", "-p", "400",
                          "-seed", "21", "--chains", "4", "--summary", "0.2"], check=True, capture_output=True, text=True,
                         timeout=300, env=_env()).stdout
    stem = str(tmp_path / "bands_21_LDDN_MDDN")
    assert "posterior summary of 256 samples (4 chains pooled)" in out
    origin = float(out.split()[0])                                   # the CLI prints ORIGIN and PRESENT first (DD:33)
    tab, S = pc.check_cli_tables(stem, [stem + "_c%d.log" % c for c in range(4)], ("l_%s", "m_%s", "niche_%s", "nicheFrac_%s"),
                                 ["posterior", "likelihood", "prior"] + LOG_HEAD[6:14], origin)
    assert S == 80 and tab.shape[1] == 4 + 15


def test_trend_rate_cli_summary_matches_restatement_on_its_logs(G, golden_dir, tmp_path):
    from helpers import post_summary_cases as pc
    from literate_amd.trendrate import LOG_HEAD
    R = np.load(os.path.join(golden_dir, "ratemaps.npz"))
    data = _bands_data(G, tmp_path)
    trend_file = tmp_path / "trend.tsv"
    with open(trend_file, "w") as f:
        f.write("year\ttrend\n")
        for i, v in enumerate(R["trend_raw"]):
            f.write("%d\t%r\n" % (i, float(v)))
    subprocess.run([sys.executable, os.path.join(ROOT, "trend_rate.py"), "-d", str(data), "-n", "800", "-s", "10", "-p", "400",
                    "-seed", "23", "-trend_data", str(trend_file), "-trend_index", "1", "--chains", "4", "--summary", "0.2"],
                   check=True, stdout=subprocess.DEVNULL, timeout=300, env=_env())
    tab, S = pc.check_cli_tables(str(tmp_path / "bands_23_EXPB_EXPD_1"),
                                 [str(tmp_path / ("bands_23_EXPB_EXPD_c%d_1.trendrate.log" % c)) for c in range(4)],
                                 ("l_%s", "m_%s"), ["posterior", "likelihood", "prior"] + LOG_HEAD[6:12])
    assert S == 80 and tab.shape[1] == 4 + 9
