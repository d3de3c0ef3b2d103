"""lr_waic_pointwise on the device (tests/helpers/waic_cases.py, every case in a child process under a time limit): against
the longdouble restatement at every table-size edge, draw count around the LDS chunk, lineage count, kind of times, order
and alignment under models 0, 2 and 3, within 16 times the float64 restatement's own error (at least 8 units); the exact
properties (identical draws, independence of the other lineages, repeated calls); draw slices; draws 1500 nats apart and
draws that differ in the 12th digit; the flag rule; every argument error; and the three command lines end to end with
`python -m literate_amd.waic` on their files.  The sharded path (chains over several ranks) reaches WAIC through
ppc._gathered_rows, which the posterior predictive checks cover; no two-rank rehearsal is run here."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "waic_cases.py")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def run_case(*args, timeout=300):
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_WAIC_SLICES"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, CASES] + list(args), capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "case %s ok" % " ".join(args) in out.stdout


@pytest.mark.parametrize("group", ["a", "b", "c", "d"])
@pytest.mark.parametrize("model", ["0", "2", "3"])
def test_against_the_longdouble_restatement(model, group):
    run_case("against", model, group)


def test_exact_properties():
    run_case("exact")


def test_draw_slices_agree_within_the_bound():
    run_case("slices")


def test_draws_far_apart_and_draws_that_differ_in_the_12th_digit():
    run_case("range")


def test_flagged_lineages_are_nan_and_the_others_keep_their_bits():
    run_case("flags")


def test_argument_errors_are_reported_before_any_launch():
    run_case("arguments")


def test_cli_literate_forward():
    run_case("cli_lrf", "2")


def test_cli_ddrate_two_models_and_the_comparison():
    run_case("cli_dd", timeout=600)


def test_cli_trend_rate():
    run_case("cli_trend")
