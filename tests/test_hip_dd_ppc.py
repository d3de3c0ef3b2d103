"""DDRate.py's and trend_rate.py's posterior predictive check on the device (literate_amd/ppc.py posterior_predictive_dd,
posterior_predictive_rates; --ppc of the two CLIs) against the numpy restatements: tests/helpers/dd_ppc_ref.py - the restated
check on the restated diversity-dependent simulator - on a DDRateEngine run of the example TBP data (same trace rows) and
through DDRate.py (the rows of the logs the run wrote, the two files compared byte for byte) under the model pairs (2, 2)
and (1, 0); tests/helpers/ppc_ref.py with oracle/sim_oracle.py for trend_rate.py.  Draws, starts, counts, HPD ends and p_ge
must be identical, means within rtol 1e-12; the comparisons with the restated simulator are conditional on its draws
staying 1e-11 clear of its thresholds (tests/helpers/dd_sim_cases.py).  Every case runs in a child process under a time
limit (tests/helpers/dd_ppc_cases.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "dd_ppc_cases.py")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def run_case(*args, timeout=300):
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, CASES] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout,
                         env=env, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "case %s ok" % " ".join(str(a) for a in args) in out.stdout


def test_posterior_predictive_dd_on_an_engine_run_equals_the_restatement():
    run_case("engine")


def test_ddrate_cli_ppc_files_equal_the_restatement_on_the_runs_own_logs():
    run_case("cli_dd", 2, 2, -1)


def test_ddrate_cli_ppc_under_a_fixed_niche_and_constant_deaths():
    run_case("cli_dd", 1, 0, -1)


def test_trend_rate_cli_ppc_equals_the_fixed_rate_restatement():
    run_case("cli_trend")
