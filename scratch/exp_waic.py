"""ops.waic_pointwise against the plain torch formulation of the same numbers, on the same GPU.

    python scratch/exp_waic.py [cfg4] [example] [big] [slices]

cfg4:    1e5 synthetic lineages (literate_amd.synth.make_lineages) x 1000 draws x 128 bins
example: the metal-bands lineages of tests/golden/binning_lik.npz (30,217) x 1000 draws at their own window
big:     1e7 lineages x 1000 draws x 128 bins (1e10 terms: 80 GB as a float64 matrix)
slices:  cfg4's and the example's size under 1, 2, 4, ... draw slices (LR_WAIC_SLICES) beside the plan's own count

Timing: device events around the call (tables, scan, merge and totals kernels), one warm-up call, then 5 timed ones
(median, min, max).  Achieved LDS gathers: 2 x 16 B per (lineage, draw) against the peak DESIGN.md uses, 256 B/clk/CU x
256 CUs x 2.4 GHz = 157.3 TB/s.  Yardstick: the [S, n] matrix gathered with torch indexing from the same tables, in slices
of draws that fit 2 GB, reduced with torch.logsumexp / mean / var per slice and merged (running logaddexp, Chan moments);
timed the same way, once after a warm-up, and compared with the kernel's results."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from literate_amd import ops
from literate_amd.synth import make_lineages

what = sys.argv[1:] or ["cfg4", "example", "big", "slices"]
LDS_PEAK = 256 * 256 * 2.4e9


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def torch_waic(ts, te, t0, lam, mu, slice_bytes=2 << 30):
    """model 2, the definition on a materialised matrix, a slice of draws at a time"""
    S, nb = lam.shape
    n = ts.numel()
    R = lam + mu
    cum = torch.cat([torch.zeros(S, 1, dtype=R.dtype, device=R.device), torch.cumsum(R, 1)], 1)
    z = torch.zeros(S, 1, dtype=R.dtype, device=R.device)
    SA = torch.cat([z, torch.log(lam) + cum[:, :-1], cum[:, -1:]], 1)
    EA = torch.cat([z, torch.log(mu) - cum[:, :-1], -cum[:, -1:]], 1)
    SR = torch.cat([z, R, z], 1)
    fl, ce = torch.floor(ts), torch.ceil(te)
    js = torch.clamp(fl - t0 + 1, 0, nb + 1).long()
    je = torch.clamp(ce - t0, 0, nb + 1).long()
    fs, fe = ts - fl, te - (ce - 1)
    per = max(1, int(slice_bytes // (8 * n * 4)))
    m = torch.full((n,), -float("inf"), dtype=R.dtype, device=R.device)
    lse = m.clone()
    cnt, mean, M2 = 0, torch.zeros_like(m), torch.zeros_like(m)
    for a in range(0, S, per):
        b = min(a + per, S)
        L = SA[a:b][:, js] + fs * SR[a:b][:, js] + EA[a:b][:, je] - fe * SR[a:b][:, je]        # [slice, n]
        lse = torch.logaddexp(lse, torch.logsumexp(L, 0))
        k = b - a
        mb = L.mean(0)
        vb = ((L - mb) ** 2).sum(0)
        d = mb - mean
        tot = cnt + k
        mean = mean + d * (k / tot)
        M2 = M2 + vb + d * d * (cnt * k / tot)
        cnt = tot
    return torch.stack([lse - np.log(S), mean, M2 / (S - 1)], 1)


def draws(S, nb, seed=3):
    rng = np.random.default_rng(seed)
    base_l, base_m = np.exp(rng.normal(size=nb) * 0.5 - 1.2), np.exp(rng.normal(size=nb) * 0.5 - 1.6)
    lam = base_l * np.exp(rng.normal(size=(S, nb)) * 0.05)
    mu = base_m * np.exp(rng.normal(size=(S, nb)) * 0.05)
    return torch.as_tensor(lam, device="cuda"), torch.as_tensor(mu, device="cuda")


def measure(name, ts, te, t0, nb, S=1000, yardstick=True):
    ts, te = torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda")
    lam, mu = draws(S, nb)
    n = ts.numel()
    call = lambda: ops.waic_pointwise(ts, te, t0, lam, mu, model=2)
    _, (pw, tot, plan) = timed(call)
    t = [timed(call)[0] for _ in range(5)]
    med = statistics.median(t)
    terms = float(n) * S
    print("%s: %d lineages x %d draws x %d bins, plan (tile, chunk, slices, tiles) %s: median %.3f ms (min %.3f, max %.3f) = "
          "%.3g terms/s, %.3g gathers/s = %.2f of the LDS gather peak; elpd_waic %.6f, p_waic %.4f, flagged %d"
          % (name, n, S, nb, plan, med * 1e3, min(t) * 1e3, max(t) * 1e3, terms / med, 2 * terms / med, 32 * terms / med / LDS_PEAK,
             float(tot[4]), float(tot[3]), int(tot[1])), flush=True)
    if yardstick:
        timed(lambda: torch_waic(ts, te, t0, lam, mu))
        ty, ref = timed(lambda: torch_waic(ts, te, t0, lam, mu))
        err = (pw - ref).abs().max(0).values
        print("   torch on a materialised matrix in 2 GB slices: %.3f ms = %.1f x the kernel; largest |difference| lppd %.3g, "
              "mean %.3g, var %.3g" % (ty * 1e3, ty / med, float(err[0]), float(err[1]), float(err[2])), flush=True)
    return med


def example():
    G = np.load(os.path.join(ROOT, "tests", "golden", "binning_lik.npz"))
    ts, te = np.asarray(G["metal_bands/lib_ts"], float), np.asarray(G["metal_bands/lib_te"], float)
    t0 = float(int(ts.min()))
    return ts, te, t0, int(te.max()) - int(t0)


if "cfg4" in what:
    ts, te = make_lineages(100000, n_bins=128, seed=0)[:2]
    measure("cfg4", ts, te, float(int(np.min(ts))), 128)
if "example" in what:
    ts, te, t0, nb = example()
    measure("example", ts, te, t0, nb)
if "big" in what:
    ts, te = make_lineages(10 ** 7, n_bins=128, seed=0)[:2]
    measure("big", ts, te, float(int(np.min(ts))), 128)
if "slices" in what:
    for name, (ts, te, t0, nb) in (("cfg4", (*make_lineages(100000, n_bins=128, seed=0)[:2], None, 128)), ("example", example())):
        t0 = float(int(np.min(ts))) if t0 is None else t0
        for k in (None, 1, 2, 4, 8, 16, 32):
            if k is None:
                os.environ.pop("LR_WAIC_SLICES", None)
            else:
                os.environ["LR_WAIC_SLICES"] = str(k)
            measure("%s, slices %s" % (name, "of the plan" if k is None else k), ts, te, t0, nb, yardstick=False)
        os.environ.pop("LR_WAIC_SLICES", None)
