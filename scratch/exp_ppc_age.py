"""ops.ppc_age at 1e5 lineages x 1000 draws x 40 bins and x 512 bins: device events around the call, one warm-up call, seven
timed (median, min, max), the plan's slicing and 1 .. 32 forced slices (three timed each); beside it ops.loo_pointwise and
ops.waic_pointwise on the first shape.

    python scratch/exp_ppc_age.py          # the device timings, one JSON object
    python scratch/exp_ppc_age.py host     # the numpy restatement (tests/helpers/ppc_age_ref.py) on the first shape, one core"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if sys.argv[1:] == ["host"]:
    from helpers import ppc_age_ref
    rng = np.random.default_rng(7)
    ts = 5.0 + rng.random(100000) * 40
    te = ts + 0.001 + rng.exponential(5.0, 100000)
    mu = np.exp(rng.normal(size=(1000, 40)) * 0.3 - 1.6)
    t = time.time()
    w = ppc_age_ref.ppc_age(ts, te, 5.0, mu, 11)
    print("numpy restatement, 1e5 x 1000 x 40: %.1f s (%.1f deaths per draw)" % (time.time() - t, w["rep"][:, 0].sum(1).mean()))
    sys.exit(0)

import torch  # noqa: E402

from literate_amd import ops  # noqa: E402


def timed(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return dict(median_ms=out[len(out) // 2], min_ms=out[0], max_ms=out[-1])

res = {}
for nb in (40, 512):
    rng = np.random.default_rng(7)
    n, S = 100000, 1000
    ts = 5.0 + rng.random(n) * nb
    te = ts + 0.001 + rng.exponential(5.0, n)
    mu = np.exp(rng.normal(size=(S, nb)) * 0.3 - 1.6)
    lam = np.exp(rng.normal(size=(S, nb)) * 0.3 - 1.6)
    tsd, ted, mud, lamd = (torch.as_tensor(x, device="cuda") for x in (ts, te, mu, lam))
    out = ops.ppc_age(tsd, ted, 5.0, mud, 11)
    plan = out[3]
    first = [t.clone() for t in out[:3]]
    r = timed(lambda: ops.ppc_age(tsd, ted, 5.0, mud, 11, out=out[:3]))
    assert all(torch.equal(a, b) for a, b in zip(first, out[:3]))
    r["plan"] = plan
    r["deaths_per_draw"] = float(out[1][:, 0].sum(1).double().mean())
    res["ppc_age_%d" % nb] = r
    for sl in ("1", "2", "4", "8", "16", "32"):
        os.environ["LR_PPC_AGE_SLICES"] = sl
        res["ppc_age_%d_slices%s" % (nb, sl)] = timed(lambda: ops.ppc_age(tsd, ted, 5.0, mud, 11, out=out[:3]), 3)
    os.environ.pop("LR_PPC_AGE_SLICES")
    if nb == 40:
        res["loo_40"] = timed(lambda: ops.loo_pointwise(tsd, ted, 5.0, lamd, mud, model=2, end_time=float(te.max())))
        res["waic_40"] = timed(lambda: ops.waic_pointwise(tsd, ted, 5.0, lamd, mud, model=2, end_time=float(te.max())))
    print(json.dumps(res, indent=1))
    sys.stdout.flush()
