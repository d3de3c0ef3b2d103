"""lr_simulate_dd_batch beside lr_simulate_bd_batch, and what templating the walk did to the latter.

    python scratch/exp_sim_dd_batch.py [old PARENT_LIB] [dd] [cli]

Method throughout: wall clock around a device synchronisation; one warm-up call per version, then five timed calls per
version, the two versions ALTERNATED within one process; median with min and max.

old PARENT_LIB: (a) lr_simulate_bd_batch of the parent commit's library (a path to its libliterate_hip.so) against this
    tree's, through the C ABI on the same buffers, on scratch/exp_sim_batch.py's own shape (32 bins x 100 steps, 20
    founders, rates .45 / .35 / .2 over .1; 256 and 1024 replicates).  The outputs are compared bit for bit as well.
    The acceptable difference is the min-max spread of the five calls.
dd: (b) lr_simulate_dd_batch under the pair (0, 0) against lr_simulate_bd_batch on identical replicates (the same
    thresholds, so the same walk: the outputs are compared), at the shape of the beyond-LDS test case (parameters [.6, 1,
    0, 1000, 39000, .05, 1, 1], 32 bins x 100 steps, 20 founders) times 1000 replicates.  Under (0, 0) nothing levels these
    rates off: every replicate grows until it overflows the default capacity of 2^20 lineages, in both kernels at the same
    step - the walk is the same, long lists in the workspace included.  The added work of the new kernel is one lr_log and
    two exp per thread and step, against one Philox per lineage.  Then the pair (1, 1) on the same parameters, the case as
    the test runs it (33,901 living at the end), for the time per replicate-step under feedback.
cli: (c) DDRate.py on the example TBP data, 8 chains, 20,000 iterations, with and without --ppc 0.2 at 1000 draws and 100
    steps per bin: the difference is the check end to end."""
import ctypes as C
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
from literate_amd import _hip, ops

args = sys.argv[1:] or ["dd", "cli"]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def alternate(a, b, n=5):
    """one warm-up each, then n timed calls each, alternated -> (times a, times b, last outputs)"""
    _, oa = timed(a)
    _, ob = timed(b)
    ta, tb = [], []
    for _ in range(n):
        t, oa = timed(a)
        ta.append(t)
        t, ob = timed(b)
        tb.append(t)
    return ta, tb, oa, ob


def say(name, ts):
    return "%s median %.4f s (min %.4f, max %.4f)" % (name, statistics.median(ts), min(ts), max(ts))


def bind(path):
    lib = C.CDLL(path)
    for name in ("lr_simulate_bd_batch_workspace_bytes", "lr_simulate_bd_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _hip.SIGNATURES[name]
    return lib


def abi_call(lib, lam, mu, spb, n0, cap, seed):
    R, nb = lam.shape
    need = lib.lr_simulate_bd_batch_workspace_bytes(R, nb, spb, cap)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    counts = torch.empty((R, 4, nb), dtype=torch.int64, device="cuda")
    totals = torch.empty((R, 4), dtype=torch.int64, device="cuda")

    def call():
        rc = lib.lr_simulate_bd_batch(_hip.ptr(lam), _hip.ptr(mu), R, nb, spb, _hip.ptr(n0), cap, seed, _hip.ptr(counts),
                                      _hip.ptr(totals), _hip.ptr(ws), need, _hip.stream_ptr())
        assert rc == 0, rc
        return counts, totals
    return call


if "old" in args:
    parent = bind(args[args.index("old") + 1])
    this = _hip.load()
    la = np.array([.45] * 10 + [.35] * 12 + [.2] * 10)
    mu = np.full(32, .1)
    for R in (256, 1024):
        lam_b, mu_b = torch.as_tensor(np.tile(la, (R, 1)), device="cuda"), torch.as_tensor(np.tile(mu, (R, 1)), device="cuda")
        n0 = torch.full((R,), 20, dtype=torch.int64, device="cuda")
        a, b = abi_call(parent, lam_b, mu_b, 100, n0, 1 << 20, 7), abi_call(this, lam_b, mu_b, 100, n0, 1 << 20, 7)
        ta, tb, oa, ob = alternate(a, b)
        # (the two calls write into buffers of their own)
        same = bool(torch.equal(oa[0], ob[0]) and torch.equal(oa[1], ob[1]))
        ma, mb = statistics.median(ta), statistics.median(tb)
        print("(a) %4d replicates: %s; %s; this / parent %.4f; parent's spread %.1f %%, this tree's %.1f %%; outputs identical: %s"
              % (R, say("parent", ta), say("this tree", tb), mb / ma, (max(ta) - min(ta)) / ma * 100,
                 (max(tb) - min(tb)) / mb * 100, same), flush=True)

if "dd" in args:
    R, nb, spb = 1000, 32, 100
    par = torch.as_tensor(np.tile([.6, 1, 0, 1000, 39000, .05, 1, 1], (R, 1)), device="cuda")
    x = torch.arange(nb, dtype=torch.float64, device="cuda")
    lam_b = torch.full((R, nb), .6, dtype=torch.float64, device="cuda")
    mu_b = torch.full((R, nb), .05, dtype=torch.float64, device="cuda")
    ta, tb, oa, ob = alternate(lambda: ops.simulate_bd_batch(lam_b, mu_b, spb, 20, 7),
                               lambda: ops.simulate_dd_batch(par, x, spb, 20, 7, 0, 0))
    same = bool(torch.equal(oa[1], ob[1]))
    ma, mb = statistics.median(ta), statistics.median(tb)
    print("(b) %d replicates, pair (0, 0): %s; %s; dd / bd %.4f; totals identical: %s; overflowed %d of %d"
          % (R, say("lr_simulate_bd_batch", ta), say("lr_simulate_dd_batch", tb), mb / ma, same, int(ob[1][:, 2].sum()), R), flush=True)
    call = lambda: ops.simulate_dd_batch(par, x, spb, 20, 7, 1, 1)
    _, (counts, totals) = timed(call)
    ts = [timed(call)[0] for _ in range(5)]
    med = statistics.median(ts)
    steps = int(counts[:, 3].sum())
    print("(b) %d replicates, pair (1, 1): %s = %.3f us per replicate-step, %.1f G draws/s; created %d .. %d, living at the end "
          "%d .. %d, overflowed %d" % (R, say("lr_simulate_dd_batch", ts), med / (R * nb * spb) * 1e6, steps / med / 1e9,
                                       int(totals[:, 0].min()), int(totals[:, 0].max()), int(totals[:, 1].min()),
                                       int(totals[:, 1].max()), int(totals[:, 2].sum())), flush=True)

if "cli" in args:
    G = np.load(os.path.join(ROOT, "tests", "golden", "binning_lik.npz"))
    ts_, te_ = G["example_TBP/ts"], G["example_TBP/te"] - 0.5
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "example.tsv")
        with open(data, "w") as f:
            f.write("id\tts\tte\n" + "".join("%d\t%g\t%g\n" % (i, 24.0 - a, 24.0 - b) for i, (a, b) in enumerate(zip(ts_, te_))))
        base = [sys.executable, os.path.join(ROOT, "DDRate.py"), "-d", data, "-TBP", "-n", "20000", "-s", "100", "-p", "10000",
                "-seed", "31", "--chains", "8"]
        check = ["--ppc", "0.2", "--ppc_draws", "1000", "--ppc_scale", "100"]
        times = {}
        for name, cmd in (("without", base), ("with --ppc", base + check), ("without", base), ("with --ppc", base + check)):
            t0 = time.perf_counter()
            out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
            times.setdefault(name, []).append(time.perf_counter() - t0)
            line = [l for l in out.splitlines() if l.startswith("posterior predictive check:")]
        print("(c) DDRate.py, example TBP data, 8 chains x 20000 iterations, whole process: without %s s; with --ppc 0.2 at 1000 "
              "draws x 100 steps per bin %s s" % (", ".join("%.2f" % t for t in times["without"]),
                                                  ", ".join("%.2f" % t for t in times["with --ppc"])))
        print("   ", line[0].replace(tmp, "."), flush=True)
