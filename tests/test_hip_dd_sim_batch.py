"""lr_simulate_dd_batch on the device: exact against lr_simulate_bd_batch where the rate map is constant (m_birth 0,
m_death 0), every branch of the rate map against the numpy restatement tests/helpers/dd_sim_ref.py, the fixed niche with
exponents 1 against the mode-1 simulators, a start above the niche (the 1e-15 floor), a list that outgrows LDS under
feedback, batch behaviour (more replicates than workgroups, per-replicate and refused starts, a second call, the shared
x_bins form) and every argument error.  Integer outputs are compared with array_equal; every comparison with the
restatement is conditional on the restatement's draws staying 1e-11 clear of its thresholds (asserted first; the
reasoning is in tests/helpers/dd_sim_cases.py, 400 times the bound the rate maps are held to).  Every case runs in a
child process under a time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "dd_sim_cases.py")


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


def test_constant_rates_equal_the_fixed_rate_kernel_bit_for_bit():
    run_case("exact")


@pytest.mark.parametrize("pair", [(2, 2), (1, 1), (1, 0), (2, -1), (2, 1)])
def test_every_branch_of_the_rate_map_equals_the_restatement(pair):
    run_case("branches", *pair)


def test_fixed_niche_with_unit_exponents_equals_the_mode_1_simulators():
    run_case("mode1")


def test_a_start_above_the_niche_sits_on_the_rate_floor():
    run_case("above_niche")


def test_a_list_that_outgrows_lds_under_feedback():
    run_case("beyond_lds", timeout=600)


def test_batch_behaviour():
    run_case("batch")


def test_argument_errors_are_reported_before_any_launch():
    run_case("arguments")
