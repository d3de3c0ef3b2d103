"""Measurements of the trait-dependent sampler (profiles/EXPERIMENTS.md, "Trait-dependent rates"): lr_trait_weights at 1e5
lineages x 1024 states x 40 bins and at 1e7 x 16 against the read-only yardstick lr_debug_stream2; a whole cycle at
--trait_every 10 beside the plain lr_rjbin iteration; the numpy restatement's trait move on one core; the LiteTraitRate.py job
end to end on the example data with a synthetic trait file.  Device times: HIP events around `reps` calls after a warm-up,
the median of 5 such windows.  python scratch/exp_trait.py OUT.json"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, fn, reps, windows=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def lineages(n, n_bins, seed):
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.uniform(0.0, n_bins - 0.5, n))
    te = np.minimum(ts + rng.exponential(6.0, n), n_bins + 1.0)
    return ts, te, rng.normal(size=n)


def main(out_path):
    import torch
    from helpers import trait_ref as tr
    from literate_amd import _hip, ops
    lib = _hip.load()
    res = {"device": torch.cuda.get_device_name(0)}
    nb = 40
    # ---- A: the weights pass
    res["weights"] = []
    for n, C, reps in ((100000, 1024, 10), (10000000, 16, 5)):
        ts, te, x = [torch.as_tensor(v, device="cuda") for v in lineages(n, nb, 1)]
        P = torch.as_tensor(np.random.default_rng(2).normal(size=(C, 2)), device="cuda")
        out = ops.trait_weights(ts, te, x, 0.0, nb, P)
        ms = timed(torch, lambda: ops.trait_weights(ts, te, x, 0.0, nb, P, out=out), reps)
        plan = ops.trait_weights_plan(n, nb, C)
        sink = torch.zeros(1, dtype=torch.float64, device="cuda")
        s2 = timed(torch, lambda: _hip.launch(lib.lr_debug_stream2, ts.device, _hip.ptr(ts), _hip.ptr(te), n, _hip.ptr(sink)), 20)
        res["weights"].append(dict(lineages=n, states=C, bins=nb, ms=ms[0], ms_min=ms[1], ms_max=ms[2], plan=plan,
                                   GBs=24.0 * n * plan["passes"] / (ms[0] * 1e-3) / 1e9, stream2_GBs=16.0 * n / (s2[0] * 1e-3) / 1e9,
                                   pair_evals_per_s=float(n) * C / (ms[0] * 1e-3), ns_per_pair=ms[0] * 1e6 / (float(n) * C)))
        del ts, te, x, out
    # ---- B: a whole cycle beside the plain iteration
    res["cycle"] = []
    for n, C in ((2000, 256), (100000, 256)):
        ts, te, x = lineages(n, nb, 3)
        data = ops.TraitData(ts, te, x, 0.0, nb)
        row = dict(lineages=n, chains=C, bins=nb)
        for every in (0, 10, 2):
            st = ops.TraitSettings(trait_every=every, x0_lo=-5.0, x0_hi=5.0)
            state = ops.trait_init(data, C, 1, st)
            ops.trait_steps(data, state, 0, 1000, 1000, 1, st)
            ms = timed(torch, lambda: ops.trait_steps(data, state, 1000, 1000, 1000, 1, st), 1, 3)
            row["us_per_iteration_every_%d" % every] = ms[0]          # ms per 1000 iterations = us per iteration
        WL, _, _ = ops.trait_weights(ts, te, x, 0.0, nb, np.zeros((1, 2)))
        tile = lambda v: v.reshape(1, -1).repeat(C, 1).contiguous()
        rj = ops.RjbinData(tile(data.sp), tile(data.ex), tile(WL), [data.start_time] * C, [data.end_time] * C, 1)
        rstate = ops.rjbin_init(rj, 1)
        ops.rjbin_steps(rj, rstate, 0, 1000, 1000, 1)
        row["us_per_iteration_rjbin"] = timed(torch, lambda: ops.rjbin_steps(rj, rstate, 1000, 1000, 1000, 1), 3)[0]
        P = torch.zeros(C, 2, dtype=torch.float64, device="cuda")
        dts = [data.ts, data.te, data.x]
        out = ops.trait_weights(*dts, 0.0, nb, P)
        row["us_per_weights_pass"] = timed(torch, lambda: ops.trait_weights(*dts, 0.0, nb, P, out=out), 50)[0] * 1e3
        res["cycle"].append(row)
    # ---- C: the restatement's trait move on one core
    for n in (2000, 100000):
        ts, te, x = lineages(n, nb, 3)
        e = tr.overlaps(ts, te, 0.0, nb)
        t = time.perf_counter()
        for _ in range(20):
            tr.weights(ts, te, x, 0.0, nb, [[0.1, 0.5]], e)
        res.setdefault("numpy_move_ms", {})[n] = (time.perf_counter() - t) / 20 * 1e3
    # ---- D: the job end to end
    import LiteTraitRate as cli
    G = np.load(os.path.join(ROOT, "tests", "golden", "binning_lik.npz"))
    ts, te = G["example_TBP/ts"], G["example_TBP/te"] - 0.5
    rng = np.random.default_rng(10)
    with tempfile.TemporaryDirectory() as d:
        data, traits = os.path.join(d, "example.tsv"), os.path.join(d, "traits.tsv")
        with open(data, "w") as f, open(traits, "w") as g:
            f.write("id\tts\tte\n"), g.write("id\tsize\n")
            for i, (a, b) in enumerate(zip(ts, te)):
                f.write("sp%d\t%g\t%g\n" % (i, 1990.0 + a, 1990.0 + b))
                g.write("sp%d\t%r\n" % (i, float(3.0 + 2.0 * rng.normal() + 0.1 * (b - a))))
        res["cli"] = []
        for every in (10, 2):
            t = time.perf_counter()
            cli.main(["-d", data, "-trait_data", traits, "-n", "200000", "-s", "100", "-p", "50000", "-seed", "3", "--chains", "64",
                      "--trait_every", str(every), "--ess", "0.1"])
            el = time.perf_counter() - t
            ess = [l.split("\t") for l in open(os.path.join(d, "literate_mcmc_logs", "example_trait_ESS.tsv")).read().splitlines()[1:]]
            eff = [l.split("\t") for l in open(os.path.join(d, "literate_mcmc_logs", "example_trait_effect.tsv")).read().splitlines()[1:]]
            res["cli"].append(dict(lineages=len(ts), chains=64, n=200000, trait_every=every, seconds=el,
                                   ess_pooled={r[0]: float(r[2]) for r in ess}, effect={r[0]: [float(v) for v in r[1:]] for r in eff}))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(sys.argv[1])
