"""The power-posterior chains of trend_rate.py --mlik, ops.tmlik_steps: microseconds per iteration of ALL chains at 16
temperatures x 8 replicates and 40 bins, for M = 1 and M = 31 models in one launch (EXPB_EXPD, EXPB_COND, CONB_EXPD on ten
covariates and the null) - device events around one launch of ITERS iterations, one warm-up launch, seven timed (median, min,
max), every launch from the same burnt-in state, windows as trend_mlik tunes them (0.3 here: the order of the tuned values at
beta = 1).  Beside it ops.mlik_steps (the DDRate sampler, model (2, 2)) at 16 x 8 on statistics of the same size.

    python scratch/exp_tmlik.py          # one JSON object
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from literate_amd import mlik, ops  # noqa: E402

ITERS, T, R, BINS, S_FREQ = 2000, 16, 8, 40, 10


def timed(fn):
    times = []
    for rep in range(8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep:
            times.append(a.elapsed_time(b))
    times.sort()
    return dict(median=times[3] * 1e3 / ITERS, min=times[0] * 1e3 / ITERS, max=times[-1] * 1e3 / ITERS)


rng = np.random.default_rng(7)
DT = np.abs(200.0 + np.cumsum(rng.normal(size=BINS) * 20.0)) + 10.0
n_spec, n_exti = rng.poisson(0.05 * DT).astype(float), rng.poisson(0.04 * DT).astype(float)
raw = np.cumsum(rng.normal(size=(10, BINS)), axis=1)
trends = (raw - raw.min(axis=1, keepdims=True)) / (raw.max(axis=1, keepdims=True) - raw.min(axis=1, keepdims=True))
trends[trends == 0] = 1e-15
betas = mlik.temperatures(T, 0.3)
scales = mlik.window_scales(betas, 8.0)
data = ops.TmlikData(n_spec, n_exti, DT, trends)
res = {}
for M in (1, 31):
    col = [0] + [c for c in range(10) for _ in range(3)]
    flags = [3] + [f for _ in range(10) for f in (0, 2, 1)]
    if M == 1:
        col, flags = [0], [0]
    grid = ops.TmlikGrid(col[:M], flags[:M], [m * R for m in range(M)], betas, scales, R)
    wins = torch.full((M, T), 0.3, dtype=torch.float64, device="cuda")
    rows, state0 = ops.tmlik_run(data, grid, wins, ITERS, S_FREQ, 1)
    state = state0.clone()

    def steps():
        state.copy_(state0)
        ops.tmlik_steps(data, grid, wins, state, ITERS, ITERS, S_FREQ, 1, rows=rows)

    t = timed(steps)
    S = ops.TMLIK_STATE
    prop = (state - state0)[..., S["proposed"]:S["proposed"] + 2].sum((0, 1, 2))
    acc = (state - state0)[..., S["accepted"]:S["accepted"] + 2].sum((0, 1, 2))
    res["tmlik_%d_models_%dx%d_chains_%d_bins" % (M, T, R, BINS)] = dict(
        us_per_iteration_of_all_chains=t, chains=M * T * R, chain_iterations_per_second=M * T * R * ITERS / (t["median"] * ITERS * 1e-6),
        acceptance=dict(zip(("mult", "add"), (acc / prop).tolist())))
dd = ops.MlikData(n_spec, n_exti, DT, -float(BINS) - 3.0, -2.0, 2, 2)
dd_rows, dd_state0 = ops.mlik_run(dd, betas, scales, R, ITERS, S_FREQ, 1)
dd_state, dd_out = dd_state0.clone(), (torch.empty_like(dd_rows),)


def dd_steps():
    dd_state.copy_(dd_state0)
    ops.mlik_steps(dd, betas, scales, dd_state, ITERS, ITERS, S_FREQ, 1, out=dd_out)


res["mlik_%dx%d_chains_%d_bins" % (T, R, BINS)] = dict(us_per_iteration_of_all_chains=timed(dd_steps), chains=T * R)
print(json.dumps(res, indent=1))
