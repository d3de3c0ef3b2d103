"""The buffer contract of include/literate_hip.h on the device (tests/helpers/abi_cases.py, every case in a child process of
its own under a time limit): every entry point on workspaces of exactly the queried size and outputs of exactly the
documented size, each between two guards of 256 KiB and filled with 0x00 and with 0xFF before the call - the guards intact,
the defined outputs bit-identical to plain ops and to each other, a second call on the dirty buffers identical again, and an
error return (one byte short, one argument error per entry point) leaving every byte alone.  The engines run 200 iterations
on such a workspace and once more through a restore into a workspace of 0xFF.  A child that ends at its time limit is a hang:
it is not retried."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import abi_cases as A  # noqa: E402

CASES = os.path.join(ROOT, "tests", "helpers", "abi_cases.py")

# (case, arguments ...); "loglik <model> 1" runs with LR_LOGLIK_SMALL=0, which the library reads once per process
CHILDREN = ([("loglik", str(m), t) for m in range(4) for t in ("0", "1")]
            + [("bin_events",), ("bin_unit",), ("chain_maps",), ("rate_maps",), ("shift_prior",), ("simulate_bd",), ("sim_batch",),
               ("dd_batch",), ("summaries",), ("ess",)]
            + [("waic", str(m)) for m in (0, 2, 3)] + [("loo",), ("psis",)]
            + [("engine",) + tuple(r) for r in A.ENGINE_RUNS])


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def run_case(*args, timeout=120):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_WAIC_SLICES", "LR_LOO_BATCH", "LR_LOGLIK_SMALL", "LR_SHARED_DEVICE", "LR_RTT_WORKSPACE"):
        env.pop(k, None)
    if args[0] == "loglik" and args[2] == "1":
        env["LR_LOGLIK_SMALL"] = "0"
    out = subprocess.run([sys.executable, CASES] + list(args), capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "case %s ok" % " ".join(args) in out.stdout


@pytest.mark.parametrize("args", CHILDREN, ids=["-".join(c) for c in CHILDREN])
def test_buffer_contract(args):
    run_case(*args)
