"""ops.loo_pointwise, its two stages apart, ops.waic_pointwise on the same shape, and the numpy restatement on one host core.

    python scratch/exp_loo.py [a] [b] [c] [host]

a: 1e5 synthetic lineages (literate_amd.synth.make_lineages) x 1000 draws x 40 bins
b: 3e4 x 1000 x 32
c: 1e5 x 4000 x 40
host: the float64 restatement (tests/helpers/loo_ref.py) on 2000 rows of each shape's draw count, one core, scaled to the
      shape's lineage count

Timing: device events around the call, two warm-up calls, then 7 timed ones (median, min, max).  The stages apart: the
second stage is ops.psis_loo_rows on a slab of one batch's size (plan[2] lineages of terms, as the first stage wrote them)
times the number of batches; the first stage is the whole call minus that."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from literate_amd import ops
from literate_amd.synth import make_lineages

what = sys.argv[1:] or ["a", "b", "c", "host"]
SHAPES = {"a": (100000, 1000, 40), "b": (30000, 1000, 32), "c": (100000, 4000, 40)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def stats(fn, warm=2, reps=7):
    for _ in range(warm):
        timed(fn)
    t = [timed(fn)[0] for _ in range(reps)]
    return statistics.median(t), min(t), max(t)


def draws(S, nb, seed=3):
    rng = np.random.default_rng(seed)
    base_l, base_m = np.exp(rng.normal(size=nb) * 0.5 - 1.2), np.exp(rng.normal(size=nb) * 0.5 - 1.6)
    lam = base_l * np.exp(rng.normal(size=(S, nb)) * 0.05)
    mu = base_m * np.exp(rng.normal(size=(S, nb)) * 0.05)
    return torch.as_tensor(lam, device="cuda"), torch.as_tensor(mu, device="cuda")


def measure(name, n, S, nb):
    ts, te = make_lineages(n, n_bins=nb, n_shifts=4, seed=0)[:2]       # (the default 20 shifts do not fit 32 bins)
    t0 = float(int(np.min(ts)))
    ts, te = torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda")
    lam, mu = draws(S, nb)
    plan = ops.loo_plan(n, nb, S, 2)
    whole = stats(lambda: ops.loo_pointwise(ts, te, t0, lam, mu, model=2))
    pw, tot, _ = ops.loo_pointwise(ts, te, t0, lam, mu, model=2)
    B = plan[2]
    slab = ops.loo_pointwise(ts[:B], te[:B], t0, lam, mu, model=2, return_terms=True)[3]
    rows = stats(lambda: ops.psis_loo_rows(slab))
    stage2 = tuple(v * n / B for v in rows)
    waic = stats(lambda: ops.waic_pointwise(ts, te, t0, lam, mu, model=2))
    terms = float(n) * S
    print("%s: %d lineages x %d draws x %d bins, plan (M, m, batch, batches) %s" % (name, n, S, nb, plan))
    print("   loo_pointwise   median %.3f ms (min %.3f, max %.3f) = %.3g terms/s" % (whole[0] * 1e3, whole[1] * 1e3, whole[2] * 1e3, terms / whole[0]))
    print("   second stage    median %.3f ms (min %.3f, max %.3f) scaled from %d rows; first stage by difference %.3f ms"
          % (stage2[0] * 1e3, stage2[1] * 1e3, stage2[2] * 1e3, B, (whole[0] - stage2[0]) * 1e3))
    print("   waic_pointwise  median %.3f ms (min %.3f, max %.3f): loo / waic = %.2f" % (waic[0] * 1e3, waic[1] * 1e3, waic[2] * 1e3, whole[0] / waic[0]))
    k = pw[:, 1]
    print("   elpd_loo %.6f, p_loo %.4f, k > 0.7: %d, unsmoothed %d, max k %.3f, flagged %d" %
          (float(tot[2]), float(tot[4]), int(tot[7]), int(tot[8]), float(tot[9]), int(tot[1])), flush=True)
    return slab


for key in ("a", "b", "c"):
    if key in what:
        n, S, nb = SHAPES[key]
        slab = measure(key, n, S, nb)
        if "host" in what:
            from helpers import loo_ref
            L = slab[:2000].cpu().numpy()
            t = time.perf_counter()
            loo_ref.psis(L)
            dt = time.perf_counter() - t
            print("   numpy float64 restatement, one core: %.2f s for 2000 rows -> %.1f s for %d" % (dt, dt * n / 2000, n), flush=True)
