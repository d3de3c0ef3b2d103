"""The GPU cases of tests/test_hip_ppc.py, each run in a child process of its own (under the test's time limit):

    python tests/helpers/ppc_cases.py CASE [ARGS...]

A case prints its figures, asserts, and exits 0 - or raises.  The yardstick is tests/helpers/ppc_ref.py fed with the same
rows (or the rows of the written logs) and oracle/sim_oracle.py as its simulator."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import ppc_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DRAWS, SPB = 50, 10


def same(what, got, want):
    ok = np.array_equal(got, want, equal_nan=True) if np.asarray(got).dtype.kind == "f" else np.array_equal(got, want)
    print("%s: %s" % (what, "identical" if ok else "DIFFER"))
    sys.stdout.flush()
    assert ok, (what, got, want)


def check_table(table, fit, ref):
    """obs, HPD ends and p_ge identical (nan where nan), means within rtol 1e-12; the counts of the fit row identical"""
    table, want = np.asarray(table, dtype=float), ref["table"]
    assert table.shape == want.shape
    mean_cols = [2, 7, 12]
    rest = [c for c in range(16) if c not in mean_cols]
    same("table: time, obs, HPD ends, p_ge", table[:, rest], want[:, rest])
    fin = np.isfinite(want[:, mean_cols])
    same("table: where the means are reported", np.isfinite(table[:, mean_cols]), fin)
    rel = np.abs(table[:, mean_cols][fin] - want[:, mean_cols][fin]) / np.maximum(np.abs(want[:, mean_cols][fin]), 1e-300)
    print("table: %d means, largest relative difference %.3g" % (fin.sum(), rel.max() if rel.size else 0.0))
    assert np.allclose(table[:, mean_cols][fin], want[:, mean_cols][fin], rtol=1e-12, atol=0)
    for k in ppc_ref.FIT_HEAD:
        a, b = float(fit[k]), float(ref["fit"][k])
        if k.endswith("_mean"):
            assert np.isclose(a, b, rtol=1e-12, atol=0), (k, a, b)
        else:
            assert a == b or (np.isnan(a) and np.isnan(b)), (k, a, b)
    print("fit row: %s" % {k: fit[k] for k in ppc_ref.FIT_HEAD})
    sys.stdout.flush()


def case_engine():
    """ppc.posterior_predictive on an engine run of the example TBP data against the restatement on the same rows"""
    from literate_amd import ppc
    from literate_amd.engine import ChainEngine
    G = np.load(os.path.join(GOLDEN, "binning_lik.npz"))
    eng = ChainEngine(G["example_TBP/ts"], G["example_TBP/te"], 8, model=0, seed=21, s_freq=10, n_trace_slots=300)
    eng.init()
    eng.steps(3000)
    S = eng.samples_done()
    assert S == 300
    rows = eng.trace[int(0.2 * S):S]
    sp, ex = eng.sp_events.cpu().numpy(), eng.ex_events.cpu().numpy()
    t0 = float(np.floor(eng.start_time))
    res = ppc.posterior_predictive(rows, sp, ex, DRAWS, SPB, 77, start_time=t0)
    host = rows.cpu().numpy()
    eng.close()
    assert len(sp) == 24 and sp.sum() == 75 and res.div_obs[1] == 2 and res.start_bin == 1
    ref = ppc_ref.posterior_predictive(host, sp, ex, DRAWS, SPB, 77, ppc_ref.oracle_simulator, start_time=t0)
    same("draws", res.draw_rows, ref["draw_rows"])
    same("birth rates per bin", res.lam_bins, ref["lam_bins"])
    same("death rates per bin", res.mu_bins, ref["mu_bins"])
    same("div_obs", res.div_obs, ref["div_obs"])
    assert (res.start_bin, res.n_start, res.capacity, res.seeds) == (ref["start_bin"], 2, ref["capacity"], (77, 77 + DRAWS))
    for name, got in (("free-running", res.free), ("one step ahead", res.step)):
        want = ref["free" if name[0] == "f" else "step"]
        same(name + ": overflow flags", got["totals"][..., 2], want["totals"][..., 2])
        same(name + ": kept draws", got["kept"], want["kept"])
        ok = want["totals"][..., 2] == 0
        same(name + ": counts", got["counts"][ok], want["counts"][ok])
        same(name + ": totals", got["totals"][ok], want["totals"][ok])
    same("bins simulated one step ahead", res.step["simulated"], ref["step"]["simulated"])
    check_table(res.table, res.fit, ref)


def _write_example(path):
    G = np.load(os.path.join(GOLDEN, "binning_lik.npz"))
    ts, te = G["example_TBP/ts"], G["example_TBP/te"] - 0.5
    with open(path, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, b) in enumerate(zip(ts, te)):
            f.write("%d\t%g\t%g\n" % (i, 24.0 - a, 24.0 - b))


def case_cli(model, start_bin):
    """LiteRateForward.py --ppc against the restatement fed with the rows of the logs the same run wrote"""
    from literate_amd import logs
    model, start_bin = int(model), (None if int(start_bin) < 0 else int(start_bin))
    C, n, s, seed = 8, 3000, 10, 31
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "example.tsv")
        _write_example(data)
        cmd = [sys.executable, os.path.join(ROOT, "LiteRateForward.py"), "-d", data, "-TBP", "-n", str(n), "-s", str(s), "-p", "1000",
               "-seed", str(seed), "-model_BDI", str(model), "--chains", str(C), "--ppc", "0.2", "--ppc_draws", str(DRAWS),
               "--ppc_scale", str(SPB)] + ([] if start_bin is None else ["--ppc_start_bin", str(start_bin)])
        env = dict(os.environ)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=280, env=env).stdout
        line = [l for l in out.splitlines() if l.startswith("posterior predictive check:")]
        print(line)
        assert len(line) == 1 and "_PPC.tsv" in line[0] and "_PPC_fit.tsv" in line[0] and "%d draws" % DRAWS in line[0]
        stem = logs.log_paths(data, model)[1]["div"][:-len("_div.log")]
        div = np.loadtxt(stem + "_div.log", skiprows=1)
        sp, ex = div[:, 0].astype(np.int64), div[:, 1].astype(np.int64)
        n_bins, S = len(sp), n // s
        burn = int(0.2 * S)
        per_chain = []
        for c in range(C):
            paths = logs.log_paths(data, model, chain=c)[1]
            mc = np.loadtxt(paths["mcmc"], skiprows=1)
            sp_rows = [np.array(l.split(), float) for l in open(paths["sp_rates"])]
            ex_rows = [np.array(l.split(), float) for l in open(paths["ex_rates"])]
            assert len(mc) == S == len(sp_rows) == len(ex_rows)
            per_chain.append([(logs.rates_per_bin(a[:(len(a) + 1) // 2], a[(len(a) + 1) // 2:], m[8], n_bins),
                               logs.rates_per_bin(b[:(len(b) + 1) // 2], b[(len(b) + 1) // 2:], m[8], n_bins))
                              for m, a, b in zip(mc, sp_rows, ex_rows)])
        flat = [per_chain[c][k] for k in range(burn, S) for c in range(C)]           # sample-major, chain-minor
        idx = ppc_ref.draw_indices(len(flat), DRAWS)
        lam, mu = np.array([flat[k][0] for k in idx]), np.array([flat[k][1] for k in idx])
        ref = ppc_ref.check(lam, mu, sp, ex, SPB, seed, ppc_ref.oracle_simulator, start_bin=start_bin, start_time=0.0)
        tab = np.loadtxt(stem + "_PPC.tsv", skiprows=1)
        with open(stem + "_PPC.tsv") as f:
            assert f.readline().rstrip("\n").split("\t") == ppc_ref.PPC_HEAD
        with open(stem + "_PPC_fit.tsv") as f:
            head, vals = [l.rstrip("\n").split("\t") for l in f]
        assert head == ppc_ref.FIT_HEAD and all("." not in v for v in vals[:len(ppc_ref.FIT_INTS)])
        fit = dict(zip(head, [float(v) for v in vals]))
        assert fit["start_bin"] == (1 if start_bin is None else start_bin) and fit["draws"] == DRAWS
        check_table(tab, fit, ref)
        # (a draw whose free-running replicate outgrows the capacity is dropped, and said so: the restatement drops the same)
        assert "overflowed: %d free-running, %d one-step" % (ref["fit"]["free_overflowed"], ref["fit"]["step_overflowed"]) in line[0]


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
