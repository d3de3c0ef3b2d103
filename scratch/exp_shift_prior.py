"""lr_shift_prior timed on the device, beside the --rtt summary it completes and the reference's host loop.

    python scratch/exp_shift_prior.py

Kernel time between two HIP events on the launch's stream (torch.cuda.Event), one warm-up launch, then 7 timed launches
(median, min, max), at 2^16 .. 2^24 replicates of the span (1960, 2010.5), hyper-prior mode; the same at 2^24 for the fixed
rate 2 and for a span of 500 bins.  Beside it: ops.rtt_summary of 1000 samples x 8 and x 100 chains over the same span
(rows of K = 3 with random shift times: its cost depends on the sample count, not on what the rows hold), timed the same
way, and the reference's own seconds per get_prior_shift call (100 000 replicates) as recorded in
tests/golden/shift_prior_reference.json.  Prints the counts' headline figures so that a run can be checked against the
restatement (tests/helpers/shift_prior_ref.py)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from literate_amd import _hip, ops, shift_bf


def event_ms(fn, reps=7):
    fn()                                   # warm-up launch
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


a, b = 1960.0, 2010.5
for lg in (16, 18, 20, 22, 24):
    n = 1 << lg
    med, lo, hi = event_ms(lambda: ops.shift_prior(a, b, n_reps=n, seed=1))
    r = ops.shift_prior(a, b, n_reps=n, seed=1)
    tot = r.totals.cpu().numpy()
    ps = shift_bf.prior_s(r.shift_hist.cpu().numpy(), tot[0])
    print("2^%d replicates (1960, 2010.5): median %.3f ms (min %.3f, max %.3f) = %.2f ns per replicate; accepted %.4f, "
          "prior_s %.6f, bf2 %.6f, bf6 %.6f" % ((lg, med, lo, hi, med * 1e6 / n, tot[0] / n, ps) + shift_bf.thresholds(ps)),
          flush=True)
n = 1 << 24
med, lo, hi = event_ms(lambda: ops.shift_prior(a, b, n_reps=n, seed=1, poi_lambda=2.0))
print("2^24 replicates, fixed rate 2: median %.3f ms (min %.3f, max %.3f)" % (med, lo, hi), flush=True)
med, lo, hi = event_ms(lambda: ops.shift_prior(0.0, 500.5, n_reps=n, seed=1))
print("2^24 replicates, (0, 500.5): median %.3f ms (min %.3f, max %.3f)" % (med, lo, hi), flush=True)

rng = np.random.default_rng(3)
for C in (8, 100):
    S = 1000
    T = np.zeros((S, C, _hip.LR_TRACE_W))
    T[:, :, 6:8] = 3
    T[:, :, 8], T[:, :, 9] = a, b
    L0, TL0 = _hip.LR_TRACE_HEAD, _hip.LR_TRACE_HEAD + _hip.LR_KMAX
    M0 = _hip.LR_TRACE_HEAD + 2 * _hip.LR_KMAX - 1
    TM0 = M0 + _hip.LR_KMAX
    T[:, :, L0:L0 + 3] = rng.gamma(2, 0.2, (S, C, 3))
    T[:, :, M0:M0 + 3] = rng.gamma(2, 0.1, (S, C, 3))
    T[:, :, TL0:TL0 + 2] = np.sort(rng.uniform(a + 1, b - 1, (S, C, 2)), axis=2)
    T[:, :, TM0:TM0 + 2] = np.sort(rng.uniform(a + 1, b - 1, (S, C, 2)), axis=2)
    Td = torch.as_tensor(T, device="cuda")
    med, lo, hi = event_ms(lambda: ops.rtt_summary(Td, S, a, b, burnin=0.2, pooled=True))
    print("ops.rtt_summary, %d samples x %d chains pooled, 50 bins: median %.3f ms (min %.3f, max %.3f)" % (S, C, med, lo, hi),
          flush=True)

with open(os.path.join(ROOT, "tests", "golden", "shift_prior_reference.json")) as f:
    fx = json.load(f)
for c in fx["cases"]:
    runs = np.array(c["runs"])
    print("reference get_prior_shift (%s, %s): %.2f s per call of %d replicates on the host (min %.2f, max %.2f); prior_s "
          "%.6f +- %.6f over 16 runs" % (c["a"], c["b"], statistics.median(c["seconds"]), fx["reps"], min(c["seconds"]),
                                       max(c["seconds"]), runs[:, 0].mean(), runs[:, 0].std(ddof=1)))
