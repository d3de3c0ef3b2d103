"""Generate tests/golden/shift_prior_reference.json: the reference's own Monte Carlo prior on rate-shift times.

    python tests/golden/make_shift_prior_golden.py <reference checkout>

Runs where a checkout of the reference is at hand (it needs pandas, as the reference does); the tests only read the json.
plotRJforward.v3.py parses its command line and plots when imported, so only its imports and function definitions are
executed here (the module is parsed and every other top-level statement dropped, as make_plotdd_golden.py does); the two
names the dropped statements rebind, min and max, are set to the builtins as the script sets them.

get_prior_shift (plotRJforward.v3.py:58-89) is called as get_r_plot calls it (:168, :184) - t_start = the death_age end b,
t_end = the root_age end a, bins np.arange(a, b) - RUNS times per time span, each after np.random.seed(SEED0 + 1000 * case
+ run).  Stored per span: a, b, the seeds, runs [RUNS][prior_s, bf2, bf6] and the host seconds of each call (100 000
replicates of the script's loop).  Recorded numbers only; about five minutes."""
import ast
import builtins
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SPANS = [(1960.0, 2010.5), (0.0, 12.5)]
RUNS = 16
SEED0 = 20200206
REPS = 100000          # the script's hard-coded loop count


def load_functions(path):
    """The module at `path` with only its imports and function definitions executed."""
    tree = ast.parse(open(path).read(), path)
    tree.body = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom, ast.FunctionDef))]
    ns = {"__name__": "plotRJforward_functions"}
    exec(compile(tree, path, "exec"), ns)
    ns["min"], ns["max"] = builtins.min, builtins.max
    return ns


def main(ref):
    fns = load_functions(os.path.join(ref, "plotRJforward.v3.py"))
    cases = []
    for ci, (a, b) in enumerate(SPANS):
        seeds, runs, secs = [], [], []
        for r in range(RUNS):
            seed = SEED0 + 1000 * ci + r
            np.random.seed(seed)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                res = fns["get_prior_shift"](b, a, np.arange(a, b))
            secs.append(round(time.perf_counter() - t0, 3))
            seeds.append(seed)
            runs.append([float(v) for v in res])
            print("span (%s, %s) run %d: prior_s %.6f bf2 %.6f bf6 %.6f, %.2f s" % (a, b, r, res[0], res[1], res[2], secs[-1]))
            sys.stdout.flush()
        cases.append({"a": a, "b": b, "seeds": seeds, "runs": runs, "seconds": secs})
    out = {"source": "plotRJforward.v3.py get_prior_shift", "reps": REPS, "columns": ["prior_s", "bf2", "bf6"], "cases": cases}
    path = os.path.join(HERE, "shift_prior_reference.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
