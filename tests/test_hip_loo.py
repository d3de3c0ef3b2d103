"""lr_loo_pointwise and lr_psis_rows on the device (tests/helpers/loo_cases.py, every case in a child process under a time
limit): the rows' entry point on host-built matrices at every draw count around the rule's and the sort's edges - tail
length, tail membership and k = +inf exactly, the values within 16 times the float64 restatement's own error (at least 8
units) of the longdouble restatement -, ties at the cutoff and inside the tail; from rates under models 0, 2 and 3; the
exact properties (subset, permutation, batches, repetition, the two stages apart, identical draws) and lppd beside WAIC's;
the flag rule; every argument error of both entry points; and the three command lines end to end with
`python -m literate_amd.loo` on their files."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "loo_cases.py")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def run_case(*args, timeout=300):
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_WAIC_SLICES", "LR_LOO_BATCH"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, CASES] + list(args), capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "case %s ok" % " ".join(args) in out.stdout


@pytest.mark.parametrize("group", ["small", "mid", "cap"])
def test_rows_structure_exactly_and_values_within_the_bound(group):
    run_case("rows", group)


def test_rows_with_ties_at_the_cutoff_and_inside_the_tail():
    run_case("ties")


@pytest.mark.parametrize("model", ["0", "2", "3"])
def test_from_rates_against_the_longdouble_restatement(model):
    run_case("rates", model)


def test_exact_properties():
    run_case("exact")


def test_flagged_lineages_are_nan_and_the_others_keep_their_bits():
    run_case("flags")


def test_argument_errors_are_reported_before_any_launch():
    run_case("arguments")


def test_cli_literate_forward_with_waic_beside_it():
    run_case("cli_lrf", "2")


def test_cli_ddrate_two_models_and_the_comparison():
    run_case("cli_dd", timeout=600)


def test_cli_trend_rate():
    run_case("cli_trend")
