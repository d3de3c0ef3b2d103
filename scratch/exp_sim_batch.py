"""lr_simulate_bd_batch against the only other way to the same numbers, sequential ops.simulate_bd calls, and the
posterior predictive check end to end on the metal-bands lineages beside that run's own sampling time.

    python scratch/exp_sim_batch.py [batch] [ppc]

batch: 256 and 1024 replicates of a list that outgrows LDS (32 bins x 100 steps, 20 founders, 67k lineages created,
37k alive at the peak); one warm-up call, then 5 timed calls each (median, min, max; wall clock around a device
synchronisation).  Yardstick: 8 sequential ops.simulate_bd runs of the same replicates (seeds 7 .. 14), timed once after
one warm-up run, and scaled to the batch's replicate count.
ppc: ChainEngine on the 30,217 metal-bands lineages (model 2, 64 chains, 20,000 iterations, a sample every 100), then
ppc.posterior_predictive with 1000 draws, 100 steps per bin, burn-in 0.2."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from literate_amd import ops, ppc

what = sys.argv[1:] or ["batch", "ppc"]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


if "batch" in what:
    la = np.array([.45] * 10 + [.35] * 12 + [.2] * 10)
    mu = np.full(32, .1)
    spb, n_steps = 100, 3200
    for R in (256, 1024):
        lam_b, mu_b = torch.as_tensor(np.tile(la, (R, 1)), device="cuda"), torch.as_tensor(np.tile(mu, (R, 1)), device="cuda")
        call = lambda: ops.simulate_bd_batch(lam_b, mu_b, spb, 20, 7)
        _, (counts, totals) = timed(call)
        ts = [timed(call)[0] for _ in range(5)]
        lineage_steps = int(counts[:, 3].sum())
        med = statistics.median(ts)
        print("batch %4d replicates: median %.4f s (min %.4f, max %.4f) = %.3f us per replicate-step, %.1f G draws/s; created "
              "%d .. %d, overflowed %d" % (R, med, min(ts), max(ts), med / (R * n_steps) * 1e6, lineage_steps / med / 1e9,
                                          int(totals[:, 0].min()), int(totals[:, 0].max()), int(totals[:, 2].sum())), flush=True)
        if R == 256:
            lam_s, mu_s = np.repeat(la, spb) / spb, np.repeat(mu, spb) / spb
            timed(lambda: ops.simulate_bd(20, n_steps, 7, lam_s, mu_s))
            t8, _ = timed(lambda: [ops.simulate_bd(20, n_steps, 7 + r, lam_s, mu_s) for r in range(8)])
            print("yardstick: 8 sequential ops.simulate_bd runs %.3f s = %.4f s per replicate (%.1f us per step)"
                  % (t8, t8 / 8, t8 / 8 / n_steps * 1e6), flush=True)
        print("  scaled yardstick for %d replicates %.1f s: the batch is %.0f x faster" % (R, t8 / 8 * R, t8 / 8 * R / med), flush=True)

if "ppc" in what:
    from literate_amd.engine import ChainEngine
    G = np.load(os.path.join(ROOT, "tests", "golden", "binning_lik.npz"))
    eng = ChainEngine(G["metal_bands/lib_ts"], G["metal_bands/lib_te"], 64, model=2, seed=31, s_freq=100, n_trace_slots=200)
    eng.init()
    t_run, _ = timed(lambda: eng.steps(20000))
    S = eng.samples_done()
    rows = eng.trace[int(0.2 * S):S]
    sp, ex = eng.sp_events.cpu().numpy(), eng.ex_events.cpu().numpy()
    run = lambda: ppc.posterior_predictive(rows, sp, ex, 1000, 100, 31)
    t1, res = timed(run)
    t2, res = timed(run)
    f = res.fit
    n_step = int(res.step["simulated"].sum()) * f["draws"]
    print("metal bands: %d lineages, %d bins; sampling 20000 iterations x 64 chains %.2f s; posterior predictive check of %d "
          "draws (%d free-running + %d one-bin replicates, 100 steps per bin) %.2f s first call, %.2f s second"
          % (sp.sum(), len(sp), t_run, f["draws"], f["draws"], n_step, t1, t2))
    print("  ", {k: f[k] for k in ppc.FIT_HEAD}, flush=True)
    eng.close()
