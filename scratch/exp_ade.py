"""ops.ade_classes and ops.ade_profile at 1e5 lineages x 1000 draws x 40 bins (65 and 129 shapes: the two passes of
literate_amd.ade) and x 512 bins: device events around the call, one warm-up call, seven timed (median, min, max); and
ade.fit_rates as a whole (wall clock, transfers included).

    python scratch/exp_ade.py          # the device timings, one JSON object
    python scratch/exp_ade.py host     # the numpy restatement (tests/helpers/ade_ref.py) on ten draws x 65 shapes, one core"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def data(nb, n=100000, S=1000):
    rng = np.random.default_rng(7)
    ts = 5.0 + rng.random(n) * nb
    te = ts + 0.001 + rng.exponential(5.0, n)
    return ts, te, np.exp(rng.normal(size=(S, nb)) * 0.3 - 1.6)


if sys.argv[1:] == ["host"]:
    from helpers import ade_ref
    from literate_amd import ade
    ts, te, mu = data(40)
    dead, cens, _ = ade_ref.classes(ts, te, 5.0, 40)
    t = time.time()
    ade_ref.profile(dead, cens, mu[:10], ade.coarse_shapes())
    dt = time.time() - t
    print("numpy restatement, %d classes, 10 draws x 65 shapes: %.2f s, %.1f ms per (draw, shape): 1000 draws x (65 + 129) "
          "shapes would take %.0f s" % ((dead > 0).sum(), dt, dt / 650 * 1e3, dt / 650 * 1000 * 194))
    sys.exit(0)

import torch  # noqa: E402

from literate_amd import ade, ops  # noqa: E402


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
    ts, te, mu = data(nb)
    tsd, ted, mud = (torch.as_tensor(x, device="cuda") for x in (ts, te, mu))
    cls = ops.ade_classes(tsd, ted, 5.0, nb)
    res["classes_%d" % nb] = dict(timed(lambda: ops.ade_classes(tsd, ted, 5.0, nb, out=cls)), classes=int((cls[0] > 0).sum()),
                                  deaths=int(cls[0].sum()))
    for G, shapes in ((65, ade.coarse_shapes()), (129, np.exp(np.linspace(-0.2, 0.2, 129)))):
        sh = torch.as_tensor(shapes, device="cuda")
        out = ops.ade_profile(cls[0], cls[1], mud, sh)
        first = [t.clone() for t in out]
        r = timed(lambda: ops.ade_profile(cls[0], cls[1], mud, sh, out=out), 7 if nb == 40 else 3)
        assert all(torch.equal(a, b) or bool((torch.isnan(a) == torch.isnan(b)).all()) for a, b in zip(first, out))
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(first, out))
        res["profile_%d_shapes%d" % (nb, G)] = r
    if nb == 40:
        ade.fit_rates(tsd, ted, 5.0, mud)
        torch.cuda.synchronize()
        t = time.time()
        fit = ade.fit_rates(tsd, ted, 5.0, mud).fit
        res["fit_rates_40_wall_ms"] = (time.time() - t) * 1e3
        res["fit_40"] = {k: fit[k] for k in ("shape_median", "shape_q025", "shape_q975", "lr_mean", "const_shape_ml", "edge_mass")}
    print(json.dumps(res, indent=1))
    sys.stdout.flush()
