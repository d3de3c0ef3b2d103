"""lr_shift_prior on the device against its numpy restatement (tests/helpers/shift_prior_ref.py) on the same Philox draws:
all four integer outputs compared with array_equal - over spans from one bin to LR_MAX_BINS, replicate counts from one to
beyond a grid pass, a seed with high bits, a replicate range across 2^32, accumulation over sharded ranges, fixed Poisson
rates below and above the cap on K, repeat launches, every argument error, and one end-to-end --rtt_bf run of the command
line.  Every case runs in a child process under a time limit (tests/helpers/shift_prior_cases.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "shift_prior_cases.py")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def run_case(name, *args, timeout=300):
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, CASES, name] + [str(a) for a in args], capture_output=True, text=True,
                         timeout=timeout, env=env, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "case %s ok" % name in out.stdout


def test_spans_from_fifty_bins_down_to_one():
    run_case("spans")


def test_the_most_bins():
    run_case("most_bins")


def test_replicate_counts_from_one_to_beyond_a_grid_pass():
    run_case("counts")


def test_a_seed_with_high_bits_and_a_range_across_2_to_the_32():
    run_case("seed_and_range")


def test_sharded_ranges_accumulate_to_the_whole():
    run_case("additivity")


def test_fixed_poisson_rates_below_and_above_the_cap():
    run_case("fixed_lambda")


def test_two_launches_give_equal_bits():
    run_case("repeatable")


def test_argument_errors_are_reported_before_any_launch():
    run_case("arguments")


def test_cli_rtt_bf_writes_the_tables_and_leaves_the_rtt_tables_alone(tmp_path):
    run_case("cli", tmp_path, timeout=600)
