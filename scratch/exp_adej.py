"""The joint sampler of (death-rate skyline, Weibull shape), ops.adej_steps: microseconds per iteration of all chains at
1024 chains x 40 bins (783 classes), 1024 chains x 128 bins and 64 chains x 40 bins - device events around one launch of
ITERS iterations, one warm-up launch, seven timed (median, min, max), every launch from the same burnt-in state.

    python scratch/exp_adej.py          # the device timings, one JSON object
    python scratch/exp_adej.py host     # the numpy restatement (tests/helpers/adej_ref.py) on the same data, one core

A library built with LR_EXTRA_FLAGS=-DLR_ADEJ_REBUILD_ALL rebuilds w and M for every proposal instead of keeping the accepted
state's: the difference is what the cache saves."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import ade_ref  # noqa: E402

ITERS = 2000


def tables(nb, n=100000):
    rng = np.random.default_rng(7)
    ts = 5.0 + rng.random(n) * nb
    te = ts + 0.001 + rng.exponential(5.0, n)
    return ade_ref.classes(ts, te, 5.0, nb)[:2]


if sys.argv[1:] == ["host"]:
    from helpers import adej_ref as ref
    for nb in (40, 128):
        dead, cens = tables(nb)
        data = ref.Data(dead, cens)
        for name, draws in (("Philox in Python", ref.PhiloxDraws(1, 0)), ("numpy Generator", ref.NumpyDraws(np.random.default_rng(1)))):
            t = time.time()
            ref.run(data, 5.0, ref.Settings(), draws, ITERS, 10)
            dt = time.time() - t
            print("numpy restatement, %d bins, %d classes, draws by %s: %.0f iterations per second" % (nb, len(data.n), name, ITERS / dt))
    sys.exit(0)

import torch  # noqa: E402

from literate_amd import ops  # noqa: E402

res = {}
for nb, C in ((40, 1024), (128, 1024), (40, 64)):
    dead, cens = tables(nb)
    data = ops.adej_prepare(torch.as_tensor(dead, device="cuda"), torch.as_tensor(cens, device="cuda"))
    st = ops.AdejSettings()
    rows, state0 = ops.adej_run(data, 5.0, C, ITERS, 10, 1, st)           # burnt in: K has grown to where it stays
    out = (torch.empty_like(rows),)
    times = []
    for rep in range(8):
        state = state0.clone()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.adej_steps(data, 5.0, state, ITERS, ITERS, 10, 1, st, out=out)
        b.record()
        torch.cuda.synchronize()
        if rep:
            times.append(a.elapsed_time(b))
    times.sort()
    prop = state[:, 6:11].sum(0) - state0[:, 6:11].sum(0)
    acc = state[:, 11:16].sum(0) - state0[:, 11:16].sum(0)
    res["%d_chains_%d_bins" % (C, nb)] = dict(
        classes=int((dead > 0).sum()), us_per_iteration=dict(median=times[3] * 1e3 / ITERS, min=times[0] * 1e3 / ITERS, max=times[-1] * 1e3 / ITERS),
        chain_iterations_per_second=C * ITERS / (times[3] * 1e-3), K_mean=float(state[:, 0].mean()),
        share_of_proposals=dict(zip(ops.ADEJ_MOVES, (prop / prop.sum()).tolist())), acceptance=dict(zip(ops.ADEJ_MOVES, (acc / prop).tolist())))
    print(json.dumps(res, indent=1))
    sys.stdout.flush()
