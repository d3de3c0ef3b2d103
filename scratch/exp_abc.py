"""lr_abc_simulate beside lr_simulate_dd_batch, and the ABC command end to end.

    python scratch/exp_abc.py [sim] [cli]

Method: wall clock around a device synchronisation; one warm-up call, then five timed calls; median with min and max.

sim: 32 bins x 100 steps at diversities near 100 and near 10 000.  lr_abc_simulate under the fixed niche theta = (0.6, 0.05, K, K,
    0, 0) started at its equilibrium K / 2 (K = 200, 20 000), counts not asked for; beside it lr_simulate_dd_batch under the
    pair (1, 1) with [.6, 1, 0, div_0, L, .05, 1, 1] started at ITS equilibrium 0.846 (div_0 + L) (118 and 11 818 in all) on
    the same number of replicates and steps - a different but equally costly rate map, and the only way to such counts
    without the new kernel.  Then lr_abc_simulate alone at 2^20 simulations, with and without counts.
cli: python -m literate_amd.abc on the example TBP data (24 bins, 75 births), the README's command: --model niche --sims
    1048576 --keep 0.01 --rounds 4, whole process, twice."""
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from literate_amd import ops

args = sys.argv[1:] or ["sim", "cli"]
NB, SPB = 32, 100


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def five(fn):
    _, out = timed(fn)
    ts = []
    for _ in range(5):
        t, out = timed(fn)
        ts.append(t)
    return ts, out


def say(ts):
    return "median %.4f s (min %.4f, max %.4f)" % (statistics.median(ts), min(ts), max(ts))


if "sim" in args:
    tab = torch.zeros((3, NB), dtype=torch.float64, device="cuda")
    obs = torch.full((3, NB), 0.1, dtype=torch.float64, device="cuda")
    for K, R, cap in ((200, 16384, 4096), (20000, 1024, 1 << 17)):
        n0 = K // 2
        theta = torch.as_tensor(np.tile([.6, .05, K, K, 0., 0.], (R, 1)), device="cuda")
        ta, a = five(lambda: ops.abc_simulate(theta, n0, obs, obs, SPB, 8 * K, 7))
        full = ops.abc_simulate(theta, n0, obs, obs, SPB, 8 * K, 7, counts=True)
        niche = K / 2 / ((.6 - .05) / (.6 + .05))
        par = torch.as_tensor(np.tile([.6, 1, 0, niche * 0.1, niche * 0.9, .05, 1, 1], (R, 1)), device="cuda")
        x = torch.arange(NB, dtype=torch.float64, device="cuda") + 40.0          # (far past the midpoint: the niche is full)
        tb, (counts, totals) = five(lambda: ops.simulate_dd_batch(par, x, SPB, n0, 7, 1, 1, capacity=cap))
        ma, mb = statistics.median(ta), statistics.median(tb)
        print("diversity near %d, %d replicates x %d steps: lr_abc_simulate %s = %.4f us per replicate-step, flagged %d, mean living "
              "%.0f; lr_simulate_dd_batch %s = %.4f us per replicate-step, overflowed %d, mean living %.0f; dd / abc %.1f"
              % (n0, R, NB * SPB, say(ta), ma / (R * NB * SPB) * 1e6, int((a.flags != 0).sum()), float(full.counts[:, 2].double().mean()),
                 say(tb), mb / (R * NB * SPB) * 1e6, int(totals[:, 2].sum()), float(counts[:, 2].double().mean()), mb / ma), flush=True)
        R = 1 << 20
        theta = torch.as_tensor(np.tile([.6, .05, K, K, 0., 0.], (R, 1)), device="cuda")
        for with_counts in (False, True):
            ts, a = five(lambda: ops.abc_simulate(theta, n0, obs, obs, SPB, 8 * K, 7, counts=with_counts))
            m = statistics.median(ts)
            print("diversity near %d, 2^20 simulations%s: %s = %.3g simulations/s, %.5f us per simulation-step, flagged %d"
                  % (n0, " with counts" if with_counts else "", say(ts), R / m, m / (R * NB * SPB) * 1e6, int((a.flags != 0).sum())), flush=True)

if "cli" in args:
    G = np.load(os.path.join(ROOT, "tests", "golden", "binning_lik.npz"))
    ts_, te_ = G["example_TBP/ts"], G["example_TBP/te"] - 0.5
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "example.tsv")
        with open(data, "w") as f:
            f.write("id\tts\tte\n" + "".join("%d\t%g\t%g\n" % (i, 24.0 - a, 24.0 - b) for i, (a, b) in enumerate(zip(ts_, te_))))
        cmd = [sys.executable, "-m", "literate_amd.abc", "-d", data, "-TBP", "--model", "niche", "--sims", "1048576", "--keep", "0.01",
               "--rounds", "4", "--out", os.path.join(tmp, "example")]
        for _ in range(2):
            t0 = time.perf_counter()
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=ROOT, timeout=240).stdout
            print("python -m literate_amd.abc, example TBP data, 4 rounds of 2^20 simulations, whole process: %.2f s" % (time.perf_counter() - t0))
        print(out.replace(tmp, "."), flush=True)
