"""lr_simulate_bd_batch on the device: every replicate of a batch against the single runs it is defined by -
oracle/sim_oracle.py and ops.simulate_bd with seed + r - on mixed rates, under a capacity one replicate exceeds, on a
list that outgrows LDS in mid-run, on extinction, per-replicate starts, more replicates than workgroups, the scheme's
exact expectation, and every argument error.  Integer outputs are compared with array_equal.  Every case runs in a child
process under a time limit (tests/helpers/sim_batch_cases.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "sim_batch_cases.py")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def run_case(name, timeout=300):
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, CASES, name], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "case %s ok" % name in out.stdout


def test_mixed_rates_equal_the_oracle_and_the_single_runs():
    run_case("mixed")


def test_overflow_stays_with_the_one_replicate_that_exceeds_the_capacity():
    run_case("overflow")


def test_a_list_that_outgrows_lds_in_mid_run():
    run_case("beyond_lds", timeout=600)


def test_extinct_replicates_carry_zeros_on():
    run_case("extinction")


def test_per_replicate_starts_and_refused_starts():
    run_case("starts")


def test_a_replicate_does_not_depend_on_the_batch_around_it():
    run_case("independence")


def test_mean_diversity_follows_the_schemes_expectation():
    run_case("expectation")


def test_argument_errors_are_reported_before_any_launch():
    run_case("arguments")
