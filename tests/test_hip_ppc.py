"""The posterior predictive check on the device (literate_amd/ppc.py, LiteRateForward.py --ppc) against its numpy
restatement tests/helpers/ppc_ref.py with oracle/sim_oracle.py as the simulator: on an engine run of the example TBP data
(same trace rows), and through the CLI (the rows of the logs the run wrote), under two models and a chosen start bin.
Draws, starts, counts, HPD ends and p_ge must be identical, means within rtol 1e-12.  Every case runs in a child process
under a time limit (tests/helpers/ppc_cases.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "ppc_cases.py")


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


def test_posterior_predictive_on_an_engine_run_equals_the_restatement():
    run_case("engine")


def test_cli_ppc_files_equal_the_restatement_on_the_runs_own_logs():
    run_case("cli", 0, -1)


def test_cli_ppc_under_the_keiding_model():
    run_case("cli", 2, -1)


def test_cli_ppc_from_a_chosen_start_bin():
    run_case("cli", 0, 5)
