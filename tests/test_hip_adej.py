"""The joint sampler of (death-rate skyline, Weibull shape) on the device (tests/helpers/adej_cases.py, every case in a child
process under a time limit): lr_adej_loglik against the numpy restatement tests/helpers/adej_ref.py within 1e-9 of the sum of
the absolute class terms - 1, 2, 40, 64, 65 and 128 bins, shapes 1/8, 1 and 8, rates scaled by 1e-12 and 1e6, a class in every
cell and a single class, counts beyond 32 bits - with the same bits from a second call on dirty outputs; flagged rows beside
good ones; every argument error of the four entry points, in order, before any launch; chains 0, 64 and 129 of a 130-chain run
against the restatement iteration by iteration (K and the accepted proposals equal, every used column within rtol 1e-9,
atol 1e-9, the restatement's smallest decision margin at least 1e-6) at 12, 40 and 128 bins, with one rate only, with counts
that do not fit the LDS copies, and up to the cap of LR_KMAX rates; a run cut into launches or into groups of chains bit for
bit; exact-size guarded buffers; the exact posterior at one rate and the number of rates under the prior alone with the bounds
and the ESS floor of tests/test_adej_host.py; recovery of a simulated shape; and two command lines end to end with the other
post-run flags' files byte-identical beside --ade_joint and without it."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "adej_cases.py")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def run_case(*args, timeout=300):
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_PPC_AGE_SLICES", "LR_WAIC_SLICES"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, CASES] + list(args), capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "case %s ok" % " ".join(args) in out.stdout


def test_the_likelihood_against_the_restatement_and_again_on_dirty_outputs():
    run_case("loglik")


def test_flagged_rows_leave_the_others_bit_identical():
    run_case("flags")


def test_argument_errors_are_reported_in_order_before_any_launch():
    run_case("arguments")


@pytest.mark.parametrize("name", ["a12", "a40", "a128", "a12_const", "big12", "cap128"])
def test_chains_follow_the_restatement_iteration_by_iteration(name):
    run_case("trajectory", name)


def test_the_run_is_a_function_of_its_arguments():
    run_case("function")


def test_the_buffer_contract_on_exact_size_guarded_buffers():
    run_case("contract")


def test_the_exact_posterior_at_one_rate():
    run_case("exact")


def test_the_number_of_rates_under_the_prior_alone():
    run_case("prior_k")


def test_a_simulated_shape_is_recovered_with_and_without_an_age_effect():
    run_case("recovery")


def test_cli_literate_forward_and_the_other_flags_files_beside_it():
    run_case("cli_lrf", timeout=600)


def test_cli_ddrate_and_the_other_flags_files_beside_it():
    run_case("cli_dd", timeout=600)
