"""The power-posterior chains of --mlik, ops.mlik_steps: microseconds per iteration of all chains at 16 x 64 and 64 x 64
(temperatures x replicates) chains, 40, 256 and 512 bins, model (2, 2) - device events around one launch of ITERS iterations, one
warm-up launch, seven timed (median, min, max), every launch from the same burnt-in state; ops.mlik_estimate on the rows of
such a run; and, for context, the DD engine (the per-lineage sampler of DDRate.py, 20 000 lineages) at the same chain counts
and bins - up to the 256 bins it takes.

    python scratch/exp_mlik.py          # the device timings, one JSON object
    python scratch/exp_mlik.py host     # the numpy restatement (tests/helpers/mlik_ref.py) on the same statistics, one core
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import mlik_ref as ref  # noqa: E402

ITERS = 2000
N_LINEAGES = 20000


def lineages(nb):
    rng = np.random.default_rng(7)
    ts = rng.random(N_LINEAGES) * (nb - 1)
    te = np.minimum(ts + 0.001 + rng.exponential(5.0, N_LINEAGES), float(nb))
    return ts, te


def ladder(T):
    betas = ref.temperatures(T, 0.3)
    return betas, ref.window_scales(betas, 8.0)


def stats_host(nb):
    """create_bins' statistics of the lineages above, in numpy (what the engine computes on the device)"""
    ts, te = lineages(nb)
    n = nb - 1                                   # create_bins drops the last bin
    lo_e = np.arange(n, dtype=float)
    n_spec = np.histogram(ts, bins=np.arange(n + 1))[0]
    n_exti = np.histogram(te[te < nb], bins=np.arange(n + 1))[0]
    DT = np.array([np.sum(np.clip(np.minimum(te, b + 1) - np.maximum(ts, b), 0, None)) for b in lo_e])
    return ref.Model(n_spec, n_exti, DT, 0.0, float(nb), 2, 2)


if sys.argv[1:] == ["host"]:
    for nb in (41, 513):
        M = stats_host(nb)
        betas, scales = ladder(16)
        t = time.time()
        ref.run_vec(M, betas, scales, 4, 500, 10, np.random.default_rng(1))
        dt = time.time() - t
        print("numpy restatement, %d bins, 64 chains at once on a numpy Generator: %.0f chain iterations per second"
              % (len(M.DT), 64 * 500 / dt))
        from oracle.dd_mcmc_oracle import PhiloxDraws
        t = time.time()
        ref.run_chain(M, 1.0, 1.0, PhiloxDraws(1, 0), 500, 10)
        print("numpy restatement, %d bins, one chain, draws by Philox in Python: %.0f iterations per second"
              % (len(M.DT), 500 / (time.time() - t)))
    sys.exit(0)

import torch  # noqa: E402

from literate_amd import ops  # noqa: E402
from literate_amd.ddrate import DDRateEngine  # noqa: E402


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
    return times


res = {}
for nb in (41, 257, 513):
    ts, te = lineages(nb)
    M = stats_host(nb)
    for T, R in ((16, 64), (64, 64)):
        eng = None
        if nb - 1 <= 256:
            eng = DDRateEngine(ts, te, 0.0, float(nb), T * R, m_birth=2, m_death=2, seed=1, s_freq=1 << 30, n_trace_slots=2)
            assert np.array_equal(eng.n_spec, M.n_spec) and np.array_equal(eng.n_exti, M.n_exti) and np.allclose(eng.DT, M.DT, rtol=1e-12)
        data = ops.MlikData(M.n_spec, M.n_exti, M.DT, M.origin, M.present, 2, 2)
        betas, scales = ladder(T)
        rows, state0 = ops.mlik_run(data, betas, scales, R, ITERS, 10, 1)
        out = (torch.empty_like(rows),)
        state = state0.clone()

        def steps():
            state.copy_(state0)
            ops.mlik_steps(data, betas, scales, state, ITERS, ITERS, 10, 1, out=out)

        times = timed(steps)
        est = timed(lambda: ops.mlik_estimate(rows, betas, row0=ITERS // 50))
        engine = [float("nan")] * 7
        if eng is not None:
            eng.init()
            eng.steps(ITERS)
            engine = timed(lambda: eng.steps(ITERS))
            eng.close()
        prop = (state[:, :, 10:12] - state0[:, :, 10:12]).sum((0, 1))
        acc = (state[:, :, 12:14] - state0[:, :, 12:14]).sum((0, 1))
        res["%dx%d_chains_%d_bins" % (T, R, data.n_bins)] = dict(
            us_per_iteration=dict(median=times[3] * 1e3 / ITERS, min=times[0] * 1e3 / ITERS, max=times[-1] * 1e3 / ITERS),
            chain_iterations_per_second=T * R * ITERS / (times[3] * 1e-3),
            estimate_us=dict(median=est[3] * 1e3, min=est[0] * 1e3, max=est[-1] * 1e3, rows=int(rows.shape[0])),
            dd_engine_us_per_iteration=dict(median=engine[3] * 1e3 / ITERS, min=engine[0] * 1e3 / ITERS, max=engine[-1] * 1e3 / ITERS,
                                            lineages=N_LINEAGES),
            acceptance=dict(zip(("mult", "slide"), (acc / prop).tolist())))
        print(json.dumps(res, indent=1))
        sys.stdout.flush()
