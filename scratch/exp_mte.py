"""Measurements of the multi-trait extinction sampler (profiles/EXPERIMENTS.md, "Multi-trait extinction"): microseconds per
iteration of all chains of lr_mte_steps at 1024 chains on the example's shape (the example file in six slices: 392
combinations, 6 traits) and at 1024 combinations x 16 traits (128 categories); beside them lr_parbin_steps at 1024 chains x 40
bins, the nearest existing one-wave-per-chain kernel; the numpy restatement's iteration on one core; the whole MTEmodel.py
command on the example file with six slices x 16 chains.  Device times: HIP events around one launch of `iters` iterations
after a warm-up launch, the median of 5.  python scratch/exp_mte.py OUT.json"""
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

EDGES = "33,23,16,12,8,3,0"


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
    from helpers import mte_ref as mr
    from helpers import parbin_ref as pr
    from literate_amd import ops
    res = {"device": torch.cuda.get_device_name(0)}
    iters = 20000
    ts, te, traits, names = mr.read_example()
    e = [float(x) for x in EDGES.split(",")]
    slices = list(zip(e[:-1], e[1:]))
    # ---- A: the kernel at 1024 chains
    res["kernel"] = []
    shapes = [("example: 6 slices", ops.MteData.from_lineages(ts, te, traits, slices, chains_per_problem=1024 // 6 + 1)),
              ("1024 combinations x 16 traits", None)]
    big = mr.synthetic(2, 1024, mr.T16, 1)[0]
    shapes[1] = (shapes[1][0], ops.MteData(big.code, big.n_states, big.n, big.E, big.B, 512))
    for label, data in shapes:
        for sname, st in (("bvs", ops.MteSettings()), ("constant", ops.MteSettings(1, 1, 1001, 0.05))):
            state = ops.mte_init(data, 1, st)
            rows = ops.mte_steps(data, state, 0, 1, 1, 1, st)
            ms = timed(torch, lambda: ops.mte_steps(data, state, 1, iters, iters + 7, 1, st, rows=rows))
            res["kernel"].append(dict(shape=label, model=sname, chains=data.n_chains, G=data.G, T=data.T, cats=data.n_cats,
                                      us_per_iteration=1e3 * ms[0] / iters, us_min=1e3 * ms[1] / iters, us_max=1e3 * ms[2] / iters))
            print(res["kernel"][-1], flush=True)
    # ---- B: lr_parbin_steps at 1024 chains x 40 bins
    D = pr.synthetic(1024, 40, 3)
    for sampler, mb, md in ((1, 2, 2), (2, 0, 0)):
        pdata = ops.ParbinData(D.n_spec, D.n_exti, D.DT, D.origin, D.present, 1, D.trend if sampler == 2 else None)
        pst = ops.ParbinSettings(sampler, mb, md, 0.1)
        pstate = ops.parbin_init(pdata, 1, pst)
        prow = ops.parbin_steps(pdata, pstate, 0, 1, 1, 1, pst)
        ms = timed(torch, lambda: ops.parbin_steps(pdata, pstate, 1, iters, iters + 7, 1, pst, rows=prow))
        res.setdefault("parbin", []).append(dict(sampler=sampler, chains=1024, bins=40, us_per_iteration=1e3 * ms[0] / iters))
        print(res["parbin"][-1], flush=True)
    # ---- C: the numpy restatement on one core
    res["numpy"] = []
    for label, Dn in (("example: slice 23-16", mr.Data(shapes[0][1].tables["code"], shapes[0][1].tables["n_states"], shapes[0][1].tables["n"][1:2],
                                                     shapes[0][1].tables["E"][1:2], shapes[0][1].tables["B"][1:2])),
                      ("1024 combinations x 16 traits", big)):
        ch = mr.Chain(Dn, 0, (1, 0, 10, 0.05), mr.Stream(1, 0))
        t = time.perf_counter()
        for it in range(300):
            ch.step(it)
        res["numpy"].append(dict(shape=label, us_per_iteration_one_chain=1e6 * (time.perf_counter() - t) / 300))
        print(res["numpy"][-1], flush=True)
    # ---- D: the whole command
    tmp = tempfile.mkdtemp()
    src = os.path.join(tmp, "example.txt")
    shutil.copy(mr.FIXTURE, src)
    for n in (100000, 1000000):
        t = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "MTEmodel.py"), "-d", src, "--slice_edges", EDGES, "--chains", "16", "-n", str(n),
                            "-s", "100", "-seed", "1", "--summary", "0.2", "--ess", "0.2"], capture_output=True, text=True, timeout=500)
        wall = time.perf_counter() - t
        line = [ln for ln in r.stdout.splitlines() if " iterations x " in ln]
        res.setdefault("command", []).append(dict(n=n, slices=6, chains=16, returncode=r.returncode, wall_s=wall, sampler_line=line[-1] if line else r.stderr[-500:]))
        print(res["command"][-1], flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "exp_mte.json")
