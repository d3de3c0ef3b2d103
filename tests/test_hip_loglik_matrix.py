"""The values of lr_bd_loglik_batch on every scan kernel it can launch (tests/helpers/loglik_cases.py: the families, the
restated plan, the child's main; tests/helpers/loglik_ref.py: the longdouble reference and the derived bound;
tests/test_loglik_matrix_host.py: what the cases mean).  A family runs in a child process of its own - LR_LOGLIK_SMALL and
LR_SCAN_WIDE are read once per process - under a time limit; the child prints error / tolerance per case and ends with
`family X ok: worst ratio R`, R <= 1.  A child that ends at its time limit is a hang: it is not retried."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import loglik_cases as K  # noqa: E402

CASES = os.path.join(ROOT, "tests", "helpers", "loglik_cases.py")
# seconds; a child takes 2 to 3 s on an MI355X (most of it the interpreter, torch and the references)
TIME_LIMIT = dict(A=120, B=120, C=120, D=120, E=120, F=120)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def run_family(fam):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_WAIC_SLICES", "LR_LOO_BATCH", "LR_LOGLIK_SMALL", "LR_SHARED_DEVICE", "LR_RTT_WORKSPACE",
              "LR_SCAN_WIDE", "LR_SCAN_BLOCKS"):
        env.pop(k, None)
    env.update(K.FAMILY_ENV[fam])
    out = subprocess.run([sys.executable, CASES, fam], capture_output=True, text=True, timeout=TIME_LIMIT[fam], env=env, cwd=ROOT)
    print(out.stdout[-20000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-6000:]
    assert "family %s ok: worst ratio" % fam in out.stdout


@pytest.mark.parametrize("fam", sorted(K.FAMILIES))
def test_loglik_values(fam):
    run_family(fam)
