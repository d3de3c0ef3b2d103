"""Generate tests/golden/plotdd_shipped.npz: the reference's own posterior summary of its shipped DDRate log.

    python tests/golden/make_plotdd_golden.py <reference checkout>

Runs where a checkout of the reference is at hand (it needs pandas, as the reference does); the tests only read the npz.
plotDD.py calls its __main__() when imported (argument parsing, then Rscript), so only its imports and function definitions
are executed here: the module is parsed and every other top-level statement dropped.  make_vec_dict (plotDD.py:11-57) is
then applied, as the script applies it to a single log (no burn-in), to
example_data/metal_bands/single_run/DD_Rate/all_bands_1_8898_LDDN_MDDN.log (1000 rows, 32 time bins).

Stored: birth_rate / birth_minHPD / birth_maxHPD, death_*, niche / niche_minHPD / niche_maxHPD [32] as make_vec_dict returned
them, and the log columns they came from, l [1000, 32], m, niche_cols, as the float64 values pandas parsed (all 96 columns:
the compressed file stays under the size allowed for a committed file, so no bins are left out)."""
import ast
import os
import sys

import numpy as np

LOG = os.path.join("example_data", "metal_bands", "single_run", "DD_Rate", "all_bands_1_8898_LDDN_MDDN.log")
HERE = os.path.dirname(os.path.abspath(__file__))


def load_functions(path):
    """The module at `path` with only its imports and function definitions executed."""
    tree = ast.parse(open(path).read(), path)
    tree.body = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom, ast.FunctionDef))]
    ns = {"__name__": "plotDD_functions"}
    exec(compile(tree, path, "exec"), ns)
    return ns


def main(ref):
    import pandas as pd
    sys.path.insert(0, ref)
    fns = load_functions(os.path.join(ref, "plotDD.py"))
    D = np.load(os.path.join(HERE, "ddrate.npz"))           # the bins of the same data set (time / empirical vectors only)
    origin, present = D["meta"][:2]
    log = os.path.join(ref, LOG)
    vec = fns["make_vec_dict"](log, 0, origin, present, D["N_SPEC"].astype(float), D["N_EXTI"].astype(float),
                               D["DT"].astype(float))
    table = pd.read_csv(log, sep="\t", header=0)
    n = len(D["DT"])
    out = {k: np.asarray(vec[k], dtype=np.float64) for k in (
        "birth_rate", "birth_minHPD", "birth_maxHPD", "death_rate", "death_minHPD", "death_maxHPD", "niche", "niche_minHPD",
        "niche_maxHPD")}
    for key, name in (("l", "l_%d"), ("m", "m_%d"), ("niche_cols", "niche_%d")):
        out[key] = np.stack([table[name % i].to_numpy(dtype=np.float64) for i in range(n)], axis=1)
    assert out["l"].shape == (1000, 32) and all(v.shape == (n,) for k, v in out.items() if v.ndim == 1)
    path = os.path.join(HERE, "plotdd_shipped.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
