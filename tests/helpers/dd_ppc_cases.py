"""The GPU cases of tests/test_hip_dd_ppc.py, each run in a child process of its own (under the test's time limit):

    python tests/helpers/dd_ppc_cases.py CASE [ARGS...]

A case prints its figures, asserts, and exits 0 - or raises.  Yardsticks: tests/helpers/dd_ppc_ref.py (the restated check on
the restated diversity-dependent simulator) fed the same trace rows, or the rows of the logs the CLI run wrote; for
trend_rate.py, tests/helpers/ppc_ref.check with oracle/sim_oracle.py as the simulator.  Draws, starts, counts, HPD ends
and p_ge identical, means within rtol 1e-12 (tests/test_hip_ppc.py's tolerances).  Every comparison with the restated
simulator carries the condition of tests/helpers/dd_sim_cases.py, asserted first: no draw of the restatement within 1e-11
of a threshold."""
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

from helpers import dd_ppc_ref, ppc_ref  # noqa: E402
from helpers.dd_sim_cases import clear_of_thresholds  # noqa: E402
from helpers.ppc_cases import GOLDEN, _write_example, check_table, same  # noqa: E402

DRAWS, SPB = 100, 10
C, N_IT, S_FREQ = 8, 3000, 50           # 60 samples a chain, 48 after the burn-in: 384 rows to draw from


def example():
    G = np.load(os.path.join(GOLDEN, "binning_lik.npz"))
    ts, te = np.asarray(G["example_TBP/ts"], dtype=float), np.asarray(G["example_TBP/te"], dtype=float)
    return ts, te, float(ts.min()), float(te.max())


def compare_sets(res, ref):
    for name, got in (("free-running", res.free), ("one step ahead", res.step)):
        want = ref["free" if name[0] == "f" else "step"]
        same(name + ": overflow flags", got["totals"][..., 2], want["totals"][..., 2])
        same(name + ": kept draws", got["kept"], want["kept"])
        ok = want["totals"][..., 2] == 0
        same(name + ": counts", got["counts"][ok], want["counts"][ok])
        same(name + ": totals", got["totals"][ok], want["totals"][ok])
    same("bins simulated one step ahead", res.step["simulated"], ref["step"]["simulated"])


def case_engine():
    """ppc.posterior_predictive_dd on a DDRateEngine run of the example TBP data against the restatement on the same rows"""
    from literate_amd import ops, ppc
    from literate_amd.ddrate import DDRateEngine
    ts, te, origin, present = example()
    eng = DDRateEngine(ts, te, origin, present, C, m_birth=2, m_death=2, seed=21, s_freq=S_FREQ, n_trace_slots=N_IT // S_FREQ)
    eng.init()
    eng.steps(N_IT)
    S = eng.samples_done()
    assert S == N_IT // S_FREQ
    rows = eng.trace[int(0.2 * S):S]
    sp, ex, DT, x = eng.n_spec, eng.n_exti, eng.DT, eng.time_range
    res = ppc.posterior_predictive_dd(rows, sp, ex, DT, x, 2, 2, DRAWS, SPB, 77, start_time=float(eng.origin))
    host = rows.cpu().numpy()
    eng.close()
    print("bins %d, events %d / %d, start bin %d from %d lineages" % (len(sp), sp.sum(), ex.sum(), res.start_bin, res.n_start))
    ref = dd_ppc_ref.posterior_predictive_dd(host, sp, ex, x, 2, 2, DRAWS, SPB, 77, start_time=float(origin))
    clear_of_thresholds("both sets", ref["closest"])
    same("draws", res.draw_rows, ref["draw_rows"])
    same("div_obs", res.div_obs, ref["div_obs"])
    assert (res.start_bin, res.n_start, res.capacity, res.seeds) == (ref["start_bin"], int(ref["div_obs"][ref["start_bin"]]),
                                                                     ref["capacity"], (77, 77 + DRAWS))
    assert len(res.draw_rows) == DRAWS and res.start_bin == 1
    # lam_bins / mu_bins: the rates at the OBSERVED DT, for the reader
    b, d = [v.cpu().numpy() for v in ops.dd_rates(ref["params"], DT, 2, 2)[:2]]
    same("birth rates at the observed DT", res.lam_bins, b)
    same("death rates at the observed DT", res.mu_bins, d)
    compare_sets(res, ref)
    check_table(res.table, res.fit, ref)


def _run_cli(script, data, extra, n_draws):
    cmd = [sys.executable, os.path.join(ROOT, script), "-d", data, "-TBP", "-n", str(N_IT), "-s", str(S_FREQ), "-p", "1000",
           "-seed", "31", "--chains", str(C), "--ppc", "0.2", "--ppc_draws", str(n_draws), "--ppc_scale", str(SPB)] + extra
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=280, env=env).stdout
    line = [l for l in out.splitlines() if l.startswith("posterior predictive check:")]
    print(line)
    assert len(line) == 1 and "_PPC.tsv" in line[0] and "_PPC_fit.tsv" in line[0] and "%d draws" % n_draws in line[0]
    return line[0]


def _drawn_log_rows(paths, n_draws):
    """the rows of the chains' logs after the burn-in, sample-major and chain-minor as the trace holds them, and the draws"""
    logs = [np.loadtxt(p, skiprows=1) for p in paths]
    S = N_IT // S_FREQ
    assert all(len(l) == S for l in logs)
    flat = np.array([logs[c][k] for k in range(int(0.2 * S), S) for c in range(C)])
    return flat[ppc_ref.draw_indices(len(flat), n_draws)]


def _binned(data):
    """what the CLIs bin the data into: (n_spec, n_exti, origin, n_bins)"""
    from literate_amd.literate_library import create_bins, parse_ts_te
    TS, TE, PRESENT, ORIGIN = parse_ts_te(data, True, -1, -1, .5)
    origin, _, n_spec, n_exti, DT, n_bins, x = create_bins(ORIGIN, PRESENT, np.asarray(TS, float), np.asarray(TE, float), 0)
    return np.asarray(n_spec).astype(np.int64), np.asarray(n_exti).astype(np.int64), float(origin), n_bins, x


def _files(stem):
    with open(stem + "_PPC.tsv") as f:
        a = f.read()
    with open(stem + "_PPC_fit.tsv") as f:
        b = f.read()
    tab = np.loadtxt(stem + "_PPC.tsv", skiprows=1)
    head, vals = [l.split("\t") for l in b.splitlines()]
    assert a.splitlines()[0].split("\t") == ppc_ref.PPC_HEAD and head == ppc_ref.FIT_HEAD
    assert all("." not in v for v in vals[:len(ppc_ref.FIT_INTS)])
    return a, b, tab, dict(zip(head, [float(v) for v in vals]))


def case_cli_dd(mb, md, start_bin):
    """DDRate.py --ppc against the restatement fed the rows of the logs the same run wrote.  The log holds the parameters
    in a shifted form (midpoint_x0 = x0 + ORIGIN, maxCarryingCap = L + div_0): undone here."""
    from literate_amd.ddrate import model_suffix
    mb, md, start_bin = int(mb), int(md), (None if int(start_bin) < 0 else int(start_bin))
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "example.tsv")
        _write_example(data)
        line = _run_cli("DDRate.py", data, ["-m_birth", str(mb), "-m_death", str(md)]
                        + ([] if start_bin is None else ["--ppc_start_bin", str(start_bin)]), DRAWS)
        stem = os.path.join(tmp, "example_31" + model_suffix(mb, md))
        sp, ex, origin, n_bins, x = _binned(data)
        par = _drawn_log_rows(["%s_c%d.log" % (stem, c) for c in range(C)], DRAWS)[:, 6:14].copy()
        par[:, 2] -= origin
        par[:, 4] -= par[:, 3]
        ref = dd_ppc_ref.check(par, sp, ex, x, mb, md, SPB, 31, start_bin=start_bin, start_time=origin)
        clear_of_thresholds("both sets", ref["closest"])
        a, b, tab, fit = _files(stem)
        assert fit["start_bin"] == (1 if start_bin is None else start_bin) and fit["draws"] == DRAWS
        check_table(tab, fit, ref)
        assert "overflowed: %d free-running, %d one-step" % (ref["fit"]["free_overflowed"], ref["fit"]["step_overflowed"]) in line
        ra, rb = ppc_ref.file_text(ref["table"], ref["fit"])
        print("files: %d and %d bytes" % (len(a), len(b)))
        assert a == ra, "the _PPC.tsv files differ"
        assert b == rb, "the _PPC_fit.tsv files differ"


def case_cli_trend():
    """trend_rate.py --ppc with a synthetic covariate against ppc_ref.check fed the rates ops.trend_rates gives for the
    drawn log rows, with oracle/sim_oracle.py as the simulator"""
    from literate_amd import ops
    from literate_amd.trendrate import model_suffix, normalise_trend
    n_draws = 50
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "example.tsv")
        _write_example(data)
        sp, ex, origin, n_bins, _ = _binned(data)
        raw = 3.0 + np.sin(np.arange(n_bins + 1) / 4.0) + np.arange(n_bins + 1) / 10.0
        trend_file = os.path.join(tmp, "trend.tsv")
        with open(trend_file, "w") as f:
            f.write("year\tcovariate\n" + "".join("%d\t%r\n" % (i, float(v)) for i, v in enumerate(raw)))
        line = _run_cli("trend_rate.py", data, ["-trend_data", trend_file, "-trend_index", "1"], n_draws)
        stem = os.path.join(tmp, "example_31" + model_suffix(False, False))
        par = _drawn_log_rows(["%s_c%d_1.trendrate.log" % (stem, c) for c in range(C)], n_draws)[:, 6:12]
        lam, mu = [v.cpu().numpy() for v in ops.trend_rates(par, normalise_trend(raw), False, False)]
        ref = ppc_ref.check(lam, mu, sp, ex, SPB, 31, ppc_ref.oracle_simulator, start_time=origin)
        a, b, tab, fit = _files(stem + "_1")
        assert fit["start_bin"] == 1 and fit["draws"] == n_draws
        check_table(tab, fit, ref)
        assert "overflowed: %d free-running, %d one-step" % (ref["fit"]["free_overflowed"], ref["fit"]["step_overflowed"]) in line


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
