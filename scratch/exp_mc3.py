"""Measurements of the Metropolis-coupled RJ sampler (profiles/EXPERIMENTS.md, "Heated chains that swap"), on one MI355X.

    python scratch/exp_mc3.py cost [PARENT_LIB]   us per iteration of lr_rjmc3_steps at 256 x 4 and 128 x 8 waves, 40 and 256 bins,
                                                  swap_every 0 / 100 / 10, beside lr_rjbin_steps on 1024 chains - this commit's
                                                  and, where the path of a parent commit's libliterate_hip.so is given, that one's,
                                                  alternating in the same process
    python scratch/exp_mc3.py ess                 ESS of K_l + K_m and of the likelihood, cold chains of 64 ladders x 4 against 256
                                                  plain chains, per 1000 iterations and per second

Times are HIP events around one launch, one warm-up launch first, the median of five.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch          # noqa: E402

from literate_amd import _hip, mc3, ops          # noqa: E402


def stats(n_bins, seed, step=None):
    """lineage-time as in the tests' make_stats; step: the birth rate rises and the death rate falls by this factor half way"""
    rng = np.random.default_rng(seed)
    br = np.abs(15.0 + np.cumsum(rng.normal(size=n_bins) * 2.0)) + 0.5 + rng.random(n_bins)
    lam, mu = np.full(n_bins, 0.3), np.full(n_bins, 0.2)
    if step:
        lam[: n_bins // 2] /= step
        mu[n_bins // 2:] /= step
    return rng.poisson(lam * br).astype(float), rng.poisson(mu * br).astype(float), br, 5.05, 5.0 + n_bins + 0.27


def timed(fn, reps=5):
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
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def cost(parent_path):
    lib = _hip.load()
    parent = None
    if parent_path:
        parent = C.CDLL(parent_path)
        parent.lr_rjbin_steps.restype, parent.lr_rjbin_steps.argtypes = _hip.SIGNATURES["lr_rjbin_steps"]
    n_it, s = 50000, 1000
    print("| bins | kernel | waves | swap_every | us per iteration (median of 5; min - max) |")
    print("|---|---|---|---|---|")
    for n_bins in (40, 256):
        sp, ex, br, t0, t1 = stats(n_bins, 3)
        data = ops.RjbinData(sp, ex, br, [t0], [t1], 1024)
        state = ops.rjbin_init(data, 5)
        ops.rjbin_steps(data, state, 0, 20000, s, 5)          # burn in
        rows = ops.alloc_output((n_it // s, 1024, _hip.LR_TRACE_W), torch.float64, data.device)
        prob = ops.rjbin_problem(data, state, 5)

        def plain(fn):
            return lambda: _hip.launch_problem(fn, data.device, prob, 20000, n_it, s, _hip.ptr(rows), n_it // s, 0)
        sides = [("lr_rjbin_steps, this commit", plain(lib.lr_rjbin_steps))] + ([("lr_rjbin_steps, parent commit", plain(parent.lr_rjbin_steps))] if parent else [])
        for _ in range(2):          # alternating: each side twice
            for name, fn in sides:
                med, lo, hi = timed(fn)
                print("| %d | %s | 1024 | - | %.3f (%.3f - %.3f) |" % (n_bins, name, med * 1e3 / n_it, lo * 1e3 / n_it, hi * 1e3 / n_it), flush=True)
        for G, T in ((256, 4), (128, 8)):
            betas = mc3.ladder_betas(T, 0.1)
            d = ops.RjbinData(sp, ex, br, [t0], [t1], G)
            st, sw = ops.rjmc3_init(d, 5, betas)
            ops.rjmc3_steps(d, st, sw, 0, 20000, s, 5, betas, 100)
            r2 = ops.alloc_output((n_it // s, G, _hip.LR_TRACE_W), torch.float64, d.device)
            l2 = ops.alloc_output((n_it // s, G, T, 4), torch.float64, d.device)
            for every in (0, 100, 10):
                med, lo, hi = timed(lambda: ops.rjmc3_steps(d, st, sw, 20000, n_it, s, 5, betas, every, rows=r2, ladder=l2))
                print("| %d | lr_rjmc3_steps | %d x %d | %d | %.3f (%.3f - %.3f) |" % (n_bins, G, T, every, med * 1e3 / n_it, lo * 1e3 / n_it, hi * 1e3 / n_it), flush=True)


def ess():
    n_it, s, seed = 200000, 10, 78
    S = n_it // s
    print("| problem | sampler | waves | logged chains | column | mean ESS per chain | total ESS per 1000 iterations | total ESS per second | run, s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, (sp, ex, br, t0, t1) in (("test 7's (constant generating rates)", stats(40, 62)), ("a 3x rate step half way", stats(40, 63, step=3.0))):
        for label, T in (("256 plain chains", 1), ("64 ladders x 4, dt 0.3, every 20", 4), ("64 ladders x 4, dt 0.1, every 100", 4)):
            G = 256 if T == 1 else 64
            data = ops.RjbinData(sp, ex, br, [t0], [t1], G)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if T == 1:
                state = ops.rjbin_init(data, seed)
                ops.rjbin_steps(data, state, 0, 1000, s, seed)          # (loads the kernel)
                state = ops.rjbin_init(data, seed)
                a.record()
                rows = ops.rjbin_steps(data, state, 0, n_it, s, seed)
                b.record()
            else:
                dt, every = (0.3, 20) if "0.3" in label else (0.1, 100)
                betas = mc3.ladder_betas(T, dt)
                state, sw = ops.rjmc3_init(data, seed, betas)
                ops.rjmc3_steps(data, state, sw, 0, 1000, s, seed, betas, every)
                state, sw = ops.rjmc3_init(data, seed, betas)
                a.record()
                rows, _ = ops.rjmc3_steps(data, state, sw, 0, n_it, s, seed, betas, every, with_ladder=False)
                b.record()
            torch.cuda.synchronize()
            secs = a.elapsed_time(b) / 1e3
            cols = torch.stack([rows[:, :, 6] + rows[:, :, 7], rows[:, :, 2]], dim=2).contiguous()
            res = ops.ess_summary(cols, S, [0, 1], burnin=0.2)
            e = res.ess.cpu().numpy()
            for k, col in enumerate(("K_l + K_m", "likelihood")):
                tot = float(np.nansum(e[:, k]))
                print("| %s | %s | %d | %d | %s | %.0f | %.1f | %.0f | %.3f |" % (name, label, G * T, G, col, float(np.nanmean(e[:, k])), tot / (n_it / 1000.0),
                                                                               tot / secs, secs), flush=True)
            if T > 1:
                swn = sw.sum(dim=0).cpu().numpy()
                print("  swap rates per pair: %s; mean K_l + K_m %.3f" % (" ".join("%.3f" % r for r in swn[:, 1] / swn[:, 0]), float(cols[S // 5:, :, 0].mean())), flush=True)
            else:
                print("  mean K_l + K_m %.3f" % float(cols[S // 5:, :, 0].mean()), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "cost":
        cost(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "ess":
        ess()
    else:
        raise SystemExit(__doc__)
