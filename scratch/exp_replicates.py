"""Replicate data sets in one launch (literate_amd/replicates.py, csrc/lr_rjbin.hip) against the only way to do the same job
without it: one ChainEngine per replicate, one after another.  Whole-job wall clock, set-up included (binning, planning,
packing, init, the run, the trace rows on the host), at R = 100 replicates x 1 chain and R = 32 x 32 chains; every replicate
30,000 lineages on 32 bins (literate_amd/synth.py) with the death times of the dead lineages re-drawn, 100,000 iterations,
a sample every 1000.  Beside them the kernel alone: microseconds per iteration of ALL chains (device events around a launch
of 20,000 iterations, one warm-up launch, five timed: median).

    python scratch/exp_replicates.py [ITERS]          # one JSON object
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from literate_amd import synth  # noqa: E402
from literate_amd.engine import ChainEngine  # noqa: E402
from literate_amd.replicates import ReplicateEngine, Replicates  # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
S_FREQ, N, BINS, SEED, KERNEL_ITERS = 1000, 30000, 32, 5, 20000


def imputations(R):
    """R replicates of one data set: the dead lineages' death years re-drawn within +-2 years (inside their bins' window)"""
    ts, te, _ = synth.make_lineages(N, n_bins=BINS, n_shifts=3, seed=1)
    rng = np.random.default_rng(2)
    dead = te < te.max()
    out = []
    for _ in range(R):
        te_r = te.copy()
        te_r[dead] = np.clip(np.floor(te[dead]) + rng.integers(-2, 3, int(dead.sum())), np.floor(ts[dead]), BINS - 1) + 0.5
        out.append((ts, te_r))
    return out


def new_path(data, cpr):
    t = time.perf_counter()
    eng = ReplicateEngine(Replicates.from_lineages(data), len(data) * cpr, seed=SEED, s_freq=S_FREQ, n_trace_slots=ITERS // S_FREQ)
    eng.init()
    eng.steps(ITERS)
    rows = eng.trace_rows()
    wall = time.perf_counter() - t
    # the kernel alone, from the burnt-in state
    times = []
    for rep in range(6):
        eng.iterations = 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.steps(KERNEL_ITERS)
        b.record()
        torch.cuda.synchronize()
        if rep:
            times.append(a.elapsed_time(b))
    eng.close()
    return wall, rows, sorted(times)[2] * 1e3 / KERNEL_ITERS


def sequential(data, cpr):
    t = time.perf_counter()
    rows = []
    for r, (ts, te) in enumerate(data):
        eng = ChainEngine(ts, te, cpr, seed=SEED, s_freq=S_FREQ, n_trace_slots=ITERS // S_FREQ, chain_offset=r * cpr)
        eng.init()
        eng.steps(ITERS)
        rows.append(eng.trace_rows())
        eng.close()
    return time.perf_counter() - t, np.concatenate(rows, axis=1)


res = {}
# (a first use of each path loads its kernels: not part of either timing)
warm = imputations(1)
ReplicateEngine(Replicates.from_lineages(warm), 1, seed=SEED, s_freq=10, n_trace_slots=1).init()
for cpr in (1, 32):
    e = ChainEngine(warm[0][0], warm[0][1], cpr, seed=SEED, s_freq=10, n_trace_slots=1)
    e.init(), e.steps(10), e.check_status(), e.close()
for R, cpr in ((100, 1), (32, 32)):
    data = imputations(R)
    w_new, rows_new, us = new_path(data, cpr)
    w_seq, rows_seq = sequential(data, cpr)
    same = bool(np.allclose(rows_new[:, :, :13], rows_seq[:, :, :13], rtol=1e-6, atol=1e-6))
    res["R%d_x_%d_chains" % (R, cpr)] = dict(
        lineages=N, bins=BINS, iterations=ITERS, chains=R * cpr, one_launch_wall_s=w_new, sequential_engines_wall_s=w_seq,
        speedup=w_seq / w_new, kernel_us_per_iteration_of_all_chains=us, trace_heads_agree_1e_6=same)
print(json.dumps(res, indent=1))
