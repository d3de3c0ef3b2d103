"""lr_ade_classes and lr_ade_profile on the device (tests/helpers/ade_cases.py, every case in a child process under a time
limit): the class counts with np.array_equal against the numpy restatement on lineage counts around a wave, a block and a
trip, bin counts on both sides of the LDS table's limit, year-resolution and continuous times, the edge lineages, and a
second call on dirty outputs; the profile against the restatement within 1e-9 of the sum of the absolute class terms (c^
within 1e-7 relative) on the smallest and the largest tables, with more classes than the threads keep in registers, under
rates scaled by 1e-12 and 1e6, scale invariance on the device itself, the same bits from a second call; counts beyond 32 bits, exactly 2^28 times the table's own result; the two degenerate
cases; flagged draws and bad shapes beside good ones; every argument error; the buffer contract on exact-size guarded
buffers; fit_rates on the device against fit_rates on the restatement; and the three command lines end to end, with the
other post-run flags' files byte-identical beside --ade and without it."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "ade_cases.py")


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


def test_the_classes_equal_the_restatement_and_again_on_dirty_outputs():
    run_case("classes")


@pytest.mark.parametrize("group", ["small", "scaled", "large"])
def test_the_profile_against_the_restatement_and_again_on_dirty_outputs(group):
    run_case("profile", group)


def test_counts_beyond_32_bits_scale_the_profile_exactly():
    run_case("big_counts")


def test_no_deaths_and_no_finite_maximiser():
    run_case("degenerate")


def test_flagged_draws_and_bad_shapes_leave_the_others_bit_identical():
    run_case("flags")


def test_argument_errors_are_reported_in_order_before_any_launch():
    run_case("arguments")


def test_the_buffer_contract_on_exact_size_guarded_buffers():
    run_case("contract")


def test_fit_rates_on_the_device_reproduces_the_host_recovery():
    run_case("recovery")


def test_cli_literate_forward_and_the_other_flags_files_beside_it():
    run_case("cli_lrf", timeout=600)


def test_cli_ddrate_and_the_other_flags_files_beside_it():
    run_case("cli_dd", timeout=600)


def test_cli_trend_rate_and_the_other_flags_files_beside_it():
    run_case("cli_trend", timeout=600)
