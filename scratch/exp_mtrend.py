"""Measurements of the joint covariate sampler (profiles/EXPERIMENTS.md, "Joint covariate model"): microseconds per iteration
of all chains of lr_mtrend_steps at 1024 chains for 40 bins x 6 covariates with selection, the same with every covariate
included, 512 bins x 16 covariates with every covariate included, and the constant model; beside them lr_parbin_steps
sampler 2 at 1024 chains x 40 bins, the yardstick for a wave-per-chain O(bins) iteration; the numpy restatement's iteration on
one core; the whole MultiTrendRate.py command on the metal-bands lineages (tests/golden/binning_lik.npz) with six seeded
random-walk columns, 256 chains and a million iterations.  Device times: HIP events around one launch of `iters` iterations
after a warm-up launch, the median of 5.  python scratch/exp_mtrend.py OUT.json"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, fn, windows=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(min(out)), float(max(out))


def main(out_path):
    import torch
    from helpers import mtrend_ref as mr
    from helpers import parbin_ref as pr
    from literate_amd import ops
    res = {"device": torch.cuda.get_device_name(0)}
    iters, C = 20000, 1024
    # ---- A: the kernel at 1024 chains
    res["kernel"] = []
    sel, big = mr.selection_data(), mr.synthetic(512, 16, 1)
    S = ops.MtrendSettings
    shapes = [("40 bins x 6, bvs", sel, S(bvs=1, bvs_from=0, pI=0.1, win=(0.05, 0.05))),
              ("40 bins x 6, all included", sel, S(bvs=0, win=(0.05, 0.05))),
              ("512 bins x 16, all included", big, S(bvs=0, win=(0.02, 0.02))),
              ("40 bins, constant model", sel, S(m_birth=1, m_death=1))]
    for label, D, st in shapes:
        data = ops.MtrendData(D.n[0], D.n[1], D.DT, D.X, C)
        state = ops.mtrend_init(data, 1, st)
        rows = ops.mtrend_steps(data, state, 0, 1, 1, 1, st)
        ms = timed(torch, lambda: ops.mtrend_steps(data, state, 1, iters, iters + 7, 1, st, rows=rows))
        h = state.cpu().numpy()
        o = ops.MTREND_STATE
        prop, acc = h[:, o["proposed"]:o["proposed"] + 6].sum(axis=0), h[:, o["accepted"]:o["accepted"] + 6].sum(axis=0)
        included = float(h[:, o["I_l"]:o["I_l"] + 16].sum() + h[:, o["I_m"]:o["I_m"] + 16].sum()) / C
        res["kernel"].append(dict(shape=label, chains=C, bins=D.n_bins, P=D.P, us_per_iteration=1e3 * ms[0] / iters, us_min=1e3 * ms[1] / iters,
                                  us_max=1e3 * ms[2] / iters, included_at_the_end=included,
                                  acceptance=[float(a / p) if p else None for a, p in zip(acc, prop)]))
        print(res["kernel"][-1], flush=True)
    # ---- B: lr_parbin_steps sampler 2 at 1024 chains x 40 bins
    Dp = pr.synthetic(C, 40, 3)
    pdata = ops.ParbinData(Dp.n_spec, Dp.n_exti, Dp.DT, Dp.origin, Dp.present, 1, Dp.trend)
    pst = ops.ParbinSettings(2, 0, 0, 0.1)
    pstate = ops.parbin_init(pdata, 1, pst)
    prow = ops.parbin_steps(pdata, pstate, 0, 1, 1, 1, pst)
    ms = timed(torch, lambda: ops.parbin_steps(pdata, pstate, 1, iters, iters + 7, 1, pst, rows=prow))
    res["parbin"] = dict(sampler=2, chains=C, bins=40, us_per_iteration=1e3 * ms[0] / iters, us_min=1e3 * ms[1] / iters, us_max=1e3 * ms[2] / iters)
    print(res["parbin"], flush=True)
    # ---- C: the numpy restatement on one core
    res["numpy"] = []
    for label, D, kw in (("40 bins x 6, bvs", sel, dict(bvs=1, bvs_from=0)), ("512 bins x 16, all included", big, dict(bvs=0))):
        ch = mr.Chain(D, mr.Settings(**kw), mr.Stream(1, 0))
        t = time.perf_counter()
        for it in range(2000):
            ch.step(it)
        res["numpy"].append(dict(shape=label, us_per_iteration_one_chain=1e6 * (time.perf_counter() - t) / 2000))
        print(res["numpy"][-1], flush=True)
    # ---- D: the whole command
    G = np.load(os.path.join(ROOT, "tests", "golden", "binning_lik.npz"))
    ts, te = G["metal_bands/lib_ts"], G["metal_bands/lib_te"] - 0.5
    tmp = tempfile.mkdtemp()
    data_file, trend_file = os.path.join(tmp, "bands.tsv"), os.path.join(tmp, "trend.tsv")
    with open(data_file, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, c) in enumerate(zip(ts, te)):
            f.write("%d\t%g\t%g\n" % (i, a, c))
    from literate_amd.literate_library import parse_ts_te
    _, _, present, origin = parse_ts_te(data_file, False, -1, -1, .5)
    n_rows = len(np.arange(origin, present + 1)) - 1          # one row per window of create_bins: the last is dropped
    g = np.random.default_rng(7)
    walks = np.cumsum(g.normal(size=(n_rows, 6)), axis=0)
    with open(trend_file, "w") as f:
        f.write("year\t" + "\t".join("x%d" % j for j in range(6)) + "\n")
        for i in range(n_rows):
            f.write("%d\t%s\n" % (i, "\t".join(repr(float(v)) for v in walks[i])))
    for n in (100000, 1000000):
        t = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "MultiTrendRate.py"), "-d", data_file, "-trend_data", trend_file, "--columns",
                            "1,2,3,4,5,6", "--chains", "256", "-n", str(n), "-s", "1000", "-seed", "1", "--summary", "0.2", "--ess", "0.2"],
                           capture_output=True, text=True, timeout=500)
        wall = time.perf_counter() - t
        line = [ln for ln in r.stdout.splitlines() if " iterations x " in ln]
        res.setdefault("command", []).append(dict(n=n, columns=6, chains=256, returncode=r.returncode, wall_s=wall,
                                                  sampler_line=line[-1] if line else (r.stdout[-300:] + r.stderr[-500:])))
        print(res["command"][-1], flush=True)
    mt = os.path.join(tmp, "bands_joint_MT.tsv")
    if os.path.exists(mt):
        with open(mt) as f:
            res["command_MT"] = f.read().splitlines()
    shutil.rmtree(tmp, ignore_errors=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "exp_mtrend.json")
