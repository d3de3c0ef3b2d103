"""lr_ppc_age on the device (tests/helpers/ppc_age_cases.py, every case in a child process under a time limit): np.array_equal
of obs, rep and totals against the numpy restatement on every case of the table - lineage counts around a tile, draw counts
around a chunk and a slice, bin counts at every LDS regime, year-resolution and continuous times, the edge lineages, zero,
tiny and huge rates, flagged draws -, the same bits under 1, 2 and as many slices as draws and from a second call on dirty
outputs; a flagged draw leaves the other draws' rows alone; every argument error; the distribution of the simulated
lifespans; the buffer contract on exact-size guarded buffers; and the three command lines end to end, with the other
post-run flags' files byte-identical beside --ppc_age and without it."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "helpers", "ppc_age_cases.py")


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


@pytest.mark.parametrize("group", ["lineages", "draws", "bins", "lds"])
def test_against_the_restatement_under_every_slicing_and_on_dirty_outputs(group):
    run_case("against", group)


def test_a_flagged_draw_leaves_the_other_draws_rows_unchanged():
    run_case("flags")


def test_argument_errors_are_reported_in_order_before_any_launch():
    run_case("arguments")


def test_the_simulated_lifespans_follow_the_exponential_law():
    run_case("distribution")


def test_the_buffer_contract_on_exact_size_guarded_buffers():
    run_case("contract")


def test_cli_literate_forward_and_the_other_flags_files_beside_it():
    run_case("cli_lrf", timeout=900)


def test_cli_ddrate():
    run_case("cli_dd")


def test_cli_trend_rate():
    run_case("cli_trend")
