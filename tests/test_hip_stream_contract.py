"""The stream contract of include/literate_hip.h on the device (tests/helpers/stream_cases.py, every case in a child process
of its own under a time limit): "`stream` is a hipStream_t passed as void* (NULL = default stream); every call is asynchronous
on it and returns after enqueueing".  Every entry point that takes the stream runs on a side stream that is non-blocking
against the null stream and busy with a delay, behind copies of its inputs over a valid decoy: its outputs, and clones of
them enqueued behind the call without a host synchronisation, must have the bits of the default-stream run, and the call
must return while the stream is still busy unless its header sentence says that it blocks.  The first child holds the
harness itself to fakes that break the contract one way each.  A child that ends at its time limit is a hang: it is not
retried."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import stream_cases as S  # noqa: E402

CASES = os.path.join(ROOT, "tests", "helpers", "stream_cases.py")

CHILDREN = ([("selftest",), ("bin_events",), ("bin_unit",), ("chain_maps",), ("rate_maps",)]
            + [("loglik", w) for w in S.LOGLIK_SHAPES]
            + [(c, d) for c in ("waic", "loo") for d in S.WALK_DRAWS]
            + [("psis",), ("simulate_bd",), ("sim_batch",), ("dd_batch",), ("shift_prior",), ("ppc_age",), ("ade",), ("adej",), ("mlik",),
               ("summaries",)]
            + [("engine",) + tuple(r) for r in S.ENGINE_RUNS])


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def run_case(*args, timeout=120):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_WAIC_SLICES", "LR_LOO_BATCH", "LR_LOGLIK_SMALL", "LR_SHARED_DEVICE", "LR_RTT_WORKSPACE",
              "LR_GRAPH_ITERS", "LR_PIPELINE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, CASES] + list(args), capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-6000:]
    assert "case %s ok" % " ".join(args) in out.stdout


@pytest.mark.parametrize("args", CHILDREN, ids=["-".join(c) for c in CHILDREN])
def test_stream_contract(args):
    run_case(*args)
