"""A/B of two builds of the library over the --ade and --ade_joint entry points (the library is swapped between runs the
way scratch/ab.sh swaps it: cp scratch/ab/<name>.so literate_amd/csrc/libliterate_hip.so).

    python scratch/ade_ab.py dump OUT.npz   # the raw bytes of what the entry points compute, as uint8 arrays
    python scratch/ade_ab.py time           # device time of four calls, one JSON object

dump: ops.ade_profile on ade_cases.PROFILE's a1, a2, a3, a40, a65, a512; ops.adej_loglik on every table of
adej_cases.LOGLIK_TABLES; rows and state of ops.adej_run for every entry of adej_cases.TRAJ, all 130 chains.

time: HIP events around one call, every timed call after one untimed call of the same shape, the median (and the smallest
and largest) of REPS timed calls: ade_profile at 128 bins x 1000 draws x 129 shapes and at 512 bins x 1000 draws x 65 shapes,
adej_prepare at 128 bins, adej_run of 256 chains x 4000 iterations (a row every 10) on a128."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from helpers import ade_cases, adej_cases  # noqa: E402
from literate_amd import ops  # noqa: E402

REPS = 21
PROFILE_DUMPED = ("a1", "a2", "a3", "a40", "a65", "a512")


def raw(t):
    return np.frombuffer(np.ascontiguousarray(t.cpu().numpy()).tobytes(), dtype=np.uint8)


def dump(path):
    out = {}
    for name in PROFILE_DUMPED:
        for what, t in zip(("ll", "c", "flag"), ade_cases.dev_profile(*ade_cases.profile_inputs(name))):
            out["profile_%s_%s" % (name, what)] = raw(t)
    for name in adej_cases.LOGLIK_TABLES:
        dead, cens, mu, sh = adej_cases.loglik_inputs(name)
        for what, t in zip(("ll", "flag"), ops.adej_loglik(adej_cases.dev_data(dead, cens), mu, sh)):
            out["loglik_%s_%s" % (name, what)] = raw(t)
    for name, (tab, kw, seed, n_it, _) in adej_cases.TRAJ.items():
        data = adej_cases.dev_data(*adej_cases.traj_table(tab))
        for what, t in zip(("rows", "state"), ops.adej_run(data, 0.0, adej_cases.TRAJ_CHAINS, n_it, 1, seed, adej_cases.settings(**kw))):
            out["traj_%s_%s" % (name, what)] = raw(t)
    np.savez(path, **out)
    print("%d arrays, %d bytes -> %s" % (len(out), sum(v.size for v in out.values()), path))


def timed(call):
    """milliseconds of REPS calls, each behind an untimed one of the same shape -> (median, min, max)"""
    ms = []
    for _ in range(REPS):
        call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def lineage_table(A):
    rng = np.random.default_rng(7)
    ts = 5.0 + rng.random(100000) * A
    return [torch.as_tensor(x, device="cuda") for x in ade_cases.ref.classes(ts, ts + 0.001 + rng.exponential(5.0, 100000), 5.0, A)[:2]]


def time_all():
    res = {}
    for A, S, G in ((128, 1000, 129), (512, 1000, 65)):
        dead, cens = lineage_table(A)
        mu = torch.as_tensor(ade_cases.rates(np.random.default_rng(8), S, A), device="cuda")
        sh = torch.as_tensor(ade_cases.grid(G), device="cuda")
        out = ops.ade_profile(dead, cens, mu, sh)
        res["ade_profile_%d_bins_%d_draws_%d_shapes" % (A, S, G)] = timed(lambda: ops.ade_profile(dead, cens, mu, sh, out=out))
    dead, cens = (torch.as_tensor(x, device="cuda") for x in adej_cases.table("a128"))
    data = ops.adej_prepare(dead, cens)
    res["adej_prepare_128_bins"] = timed(lambda: ops.adej_prepare(dead, cens, out=data))
    res["adej_run_256_chains_4000_iterations_a128"] = timed(lambda: ops.adej_run(data, 0.0, 256, 4000, 10, 1))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if sys.argv[1:2] == ["dump"] and len(sys.argv) == 3:
        dump(sys.argv[2])
    elif sys.argv[1:] == ["time"]:
        time_all()
    else:
        sys.exit(__doc__)
