"""Generate tests/golden/abc_sim.npz: the diversity trajectory of the reference's own forward simulator under a fixed niche.

    python tests/golden/make_abc_sim_golden.py <reference checkout>

Runs where a checkout of the reference is at hand; the tests only read the npz.  simulateRateABC.v2.py plots when imported
(and imports scipy and matplotlib), so only its `Simulator` class is executed here: the module is parsed, every other
top-level statement dropped, and the class body run in a namespace that holds what it takes from its star imports - numpy's
names and get_br, for which the project's restatement (oracle.literate_oracle.get_br, lib:74-79) stands in.

Settings: theoretical_only = False; fixed niche K = div_0 + L = 200; l0 0.5, m0 0.2; 5 founders; 4 bins x scale 100; the size
constraints relaxed so that the first pass is returned (minSP 2 lets the loop start on its one-entry placeholder and end on
the 5 founders, maxSP 1e9, minEX_SP 0).  RUNS passes, pass r after np.random.seed(SEED0 + r).  Stored: the per-bin mean and
variance (ddof 1) of st_diversity - the living count at the start of each bin - and the run count.  About a minute."""
import ast
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RUNS, SEED0 = 4000, 20181113
L0, M0, K, FOUNDERS, BINS, SCALE = 0.5, 0.2, 200.0, 5, 4, 100


def load_simulator(path):
    from oracle.literate_oracle import get_br
    tree = ast.parse(open(path).read(), path)
    tree.body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Simulator"]
    ns = {k: getattr(np, k) for k in dir(np) if not k.startswith("_")}
    ns.update(np=np, get_br=get_br, __name__="simulateRateABC_Simulator", max=max, min=min, round=round, range=range, list=list,
              int=int, len=len, print=print)
    exec(compile(tree, path, "exec"), ns)
    return ns["Simulator"]


def main(ref):
    Simulator = load_simulator(os.path.join(ref, "simulateRateABC.v2.py"))
    sim = Simulator()
    sim.theoretical_only = False
    sim.s_species, sim.minSP, sim.maxSP, sim.minEX_SP = FOUNDERS, 2, 10 ** 9, 0
    sim.scale, sim.time_frame = SCALE, BINS
    sim.logistic_params["div_0"], sim.logistic_params["L"] = 0.0, K
    sim.si_params["l0"], sim.si_params["m0"] = L0, M0
    div = np.empty((RUNS, BINS))
    for r in range(RUNS):
        np.random.seed(SEED0 + r)
        with contextlib.redirect_stdout(io.StringIO()):
            out = sim.simulate()
        div[r] = out[5]
        if r % 500 == 0:
            print("run", r, div[r])
            sys.stdout.flush()
    path = os.path.join(HERE, "abc_sim.npz")
    np.savez(path, mean=div.mean(0), var=div.var(0, ddof=1), runs=np.int64(RUNS),
             settings=np.array([L0, M0, K, FOUNDERS, BINS, SCALE], dtype=np.float64))
    print(path, os.path.getsize(path), "bytes", div.mean(0), div.var(0, ddof=1))


if __name__ == "__main__":
    main(sys.argv[1])
