"""lr_ess_summary on the device: per-chain ESS (Tracer's estimator), pooled ESS and split R-hat against the numpy
restatement in tests/helpers/ess_ref.py - on AR(1) series on both sides of the LDS cut-over, constant columns, engine
runs of the three samplers, cfg4's shape and the three CLIs."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import ess_ref as er

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 139
PHIS = (-0.5, 0.0, 0.5, 0.9, 0.99, 0.999)
COLS = (3, 17, 40, 77, 101, 138)                 # scattered columns of 139-wide rows, NaN everywhere else


@pytest.fixture(scope="module")
def G(golden_dir):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return np.load(os.path.join(golden_dir, "binning_lik.npz"))


def rows_for(n, C, burnin, seed):
    """[S, C, W] rows whose kept part (S - int(burnin S) = n rows) holds AR(1) series of every phi in COLS"""
    S = n
    while S - int(burnin * S) != n:
        S += 1
    rng = np.random.default_rng(seed)
    R = np.full((S, C, W), np.nan)
    for k, phi in enumerate(PHIS):
        e = rng.standard_normal((S, C))
        x = np.empty((S, C))
        x[0] = e[0] / np.sqrt(max(1e-6, 1 - phi * phi))
        for s in range(1, S):
            x[s] = phi * x[s - 1] + e[s]
        R[:, :, COLS[k]] = 3.0 * k - 5.0 + (k + 1) * 0.37 * x
    return R, S


def _cases():
    from literate_amd import _hip
    cut = _hip.LR_ESS_LDS_ROWS
    return [(4, 3, 0.0, 2000), (5, 64, 0.1, 2), (6, 1, 0.5, 7), (7, 3, 0.1, 1), (64, 64, 0.0, 7), (64, 3, 0.5, 2000),
            (901, 64, 0.1, 2000), (901, 3, 0.0, 2), (2001, 3, 0.1, 2000), (2002, 1, 0.5, 2000), (2002, 3, 0.0, 7),
            (cut - 1, 3, 0.1, 2000), (cut, 1, 0.0, 2000), (cut + 1, 3, 0.5, 2000), (40_000, 1, 0.1, 2000)]


@pytest.mark.parametrize("n,C,burnin,max_lag", _cases())
def test_ess_ar1_against_restatement(G, n, C, burnin, max_lag):
    from literate_amd import ops
    R, S = rows_for(n, C, burnin, seed=n * 7 + C)
    res = ops.ess_summary(R, S, COLS, burnin=burnin, max_lag=max_lag)
    assert res.n == n and res.ess.shape == (C, len(COLS)) and res.rhat.shape == (len(COLS),)
    er.check(res, R, S, COLS, burnin, max_lag)
    stop = res.stop_lag.cpu().numpy()
    L = min(n - 1, max_lag)
    assert stop.max() <= L and stop.min() >= 1
    if max_lag == 7 and n >= 64:
        assert (stop[:, -1] == L).mean() > 0.5       # phi = 0.999: max_lag is mostly reached before the pair rule stops
    ess = res.ess.cpu().numpy()
    assert np.all((ess > 0) & (ess <= n))


def test_ess_constant_columns(G):
    """a column constant in every chain and one constant in one chain only: NaN ESS and ACT, SE 0, stop lag 0, the value
    as the mean; pooled_ess skips the constant chain; R-hat NaN where W = 0"""
    from literate_amd import ops
    R, S = rows_for(300, 4, 0.1, seed=5)
    R[:, :, 50] = 0.1                              # the sum of 270 copies of 0.1 over 270 is not 0.1
    R[:, 2, 3] = 7.25
    burn = S - 300
    R[:burn, 1, 17] = -3.0                         # constant after burn-in only
    R[burn:, 1, 17] = 2.5
    cols = [3, 17, 50, 40]
    res = ops.ess_summary(R, S, cols, burnin=0.1)
    er.check(res, R, S, cols, 0.1)
    ess, act, se, stop, mean = (getattr(res, k).cpu().numpy() for k in ("ess", "act", "se_mean", "stop_lag", "mean"))
    for c, k, v in [(c, 2, 0.1) for c in range(4)] + [(2, 0, 7.25), (1, 1, 2.5)]:
        assert np.isnan(ess[c, k]) and np.isnan(act[c, k]) and se[c, k] == 0 and stop[c, k] == 0 and mean[c, k] == v
    assert np.isfinite(ess[[0, 1, 3], 0]).all() and stop[3, 0] >= 1
    pe, rh, pm = res.pooled_ess.cpu().numpy(), res.rhat.cpu().numpy(), res.pooled_mean.cpu().numpy()
    assert pe[0] == pytest.approx(ess[[0, 1, 3], 0].sum(), rel=1e-12)
    assert np.isnan(pe[2]) and np.isnan(rh[2]) and pm[2] == 0.1
    assert np.isfinite(rh[[0, 1, 3]]).all()


def test_ess_refuses_bad_arguments(G):
    from literate_amd import ops
    R, S = rows_for(10, 2, 0.0, seed=1)
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        ops.ess_summary(R, S, [3, W], burnin=0.0)
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        ops.ess_summary(R, S, [3], burnin=0.7)          # 3 rows kept
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        ops.ess_summary(R, S, [3], burnin=0.1, max_lag=0)


# ---- engine runs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", [("example_TBP", 0), ("metal_bands", 2)])
def test_ess_chain_engine_matches_restatement(G, name, model):
    from literate_amd.engine import ChainEngine
    eng = ChainEngine(G[name + "/ts"], G[name + "/te"], 32, model=model, seed=29, s_freq=4, n_trace_slots=750)
    eng.init()
    eng.steps(3000)
    res, names = eng.ess_summary(burnin=0.1)
    T = eng.trace_rows()
    view = eng.trace
    again = eng.ess_summary(burnin=0.1)[0]
    from literate_amd import ops
    copy = ops.ess_summary(view[:750].clone(), 750, [1, 2, 3, 4, 5, 6, 7, 10, 11, 12], burnin=0.1)
    eng.close()
    assert names == ["posterior", "likelihood", "prior", "lambda_avg", "mu_avg", "K_l", "K_m", "gamma_rate_hp_BI",
                     "gamma_rate_hp_D", "poisson_rate_hp"]
    assert T.shape == (750, 32, W)
    er.check(res, T, 750, [1, 2, 3, 4, 5, 6, 7, 10, 11, 12], 0.1)
    # the same bits twice, and on the trace view and a contiguous copy
    for x, y, z in zip(res, again, copy):
        if hasattr(x, "cpu"):
            a, b, c = (v.cpu().numpy() for v in (x, y, z))
            assert a.tobytes() == b.tobytes() == c.tobytes()


def _dd_data(G, golden_dir):
    D = np.load(os.path.join(golden_dir, "ddrate.npz"))
    origin, present, _ = D["meta"]
    return G["metal_bands/lib_ts"], G["metal_bands/lib_te"], origin, present


def test_ess_ddrate_engine_on_logged_values(G, golden_dir):
    """DDRate: the diagnosed values are the log's (midpoint_x0 = arg + ORIGIN, maxCarryingCap = arg4 + arg3)"""
    from literate_amd.ddrate import DDRateEngine, LOG_HEAD
    ts, te, origin, present = _dd_data(G, golden_dir)
    eng = DDRateEngine(ts, te, origin, present, 32, m_birth=2, m_death=2, seed=17, s_freq=3, n_trace_slots=1000)
    eng.init()
    eng.steps(3000)
    res, names = eng.ess_summary(burnin=0.1)
    T = eng.trace_rows()
    table = eng.log_table_from(T)                  # [S, C, log columns] as DDRate.py writes them
    eng.close()
    log_cols = [1, 2, 5] + list(range(6, 14))
    assert names == [LOG_HEAD[i] for i in log_cols]
    assert not np.array_equal(table[:, :, 8], T[:, :, 6])          # (the transform is not the identity)
    er.check(res, table, 1000, log_cols, 0.1)


def test_ess_trend_engine_matches_restatement(G, golden_dir):
    from literate_amd.trendrate import LOG_HEAD, TrendRateEngine
    R = np.load(os.path.join(golden_dir, "ratemaps.npz"))
    ts, te, origin, present = _dd_data(G, golden_dir)
    eng = TrendRateEngine(ts, te, origin, present, R["TREND"], 32, seed=19, s_freq=3, n_trace_slots=1000)
    eng.init()
    eng.steps(3000)
    res, names = eng.ess_summary(burnin=0.1)
    T = eng.trace_rows()
    table = eng.log_table_from(T)
    eng.close()
    log_cols = [1, 2, 5] + list(range(6, 12))
    assert names == [LOG_HEAD[i] for i in log_cols]
    er.check(res, table, 1000, log_cols, 0.1)


def test_ess_cfg4_shape(G):
    """1024 chains x 1001 samples x 10 columns of a short cfg4-size run (100k synthetic lineages) at s = 20: R-hat and the
    pooled values on every column, the per-chain values on a sample of chains; two calls bitwise equal."""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    ts, te, _ = synth.make_lineages(100_000, n_bins=128, n_shifts=20, seed=0)
    eng = ChainEngine(ts, te, 1024, model=0, seed=5, s_freq=20, n_trace_slots=1001)
    eng.init()
    eng.steps(20_001)
    r1, names = eng.ess_summary(burnin=0.1)
    r2, _ = eng.ess_summary(burnin=0.1)
    T = eng.trace_rows()
    eng.close()
    assert T.shape[:2] == (1001, 1024) and r1.n == 901 and len(names) == 10
    for x, y in zip(r1[:-1], r2[:-1]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    cols = [1, 2, 3, 4, 5, 6, 7, 10, 11, 12]
    er.check(r1, T, 1001, cols, 0.1, chains=[0, 1, 2, 255, 511, 512, 777, 1023])


# ---- CLIs ----------------------------------------------------------------------------------------------------------------
def _example_data(G, tmp_path):
    ts, te = G["example_TBP/ts"], G["example_TBP/te"] - 0.5
    data = tmp_path / "example.tsv"
    with open(data, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, b) in enumerate(zip(ts, te)):
            f.write("%d\t%g\t%g\n" % (i, 24.0 - a, 24.0 - b))
    return data


def _bands_data(G, tmp_path):
    ts, te = G["metal_bands/lib_ts"], G["metal_bands/lib_te"] - 0.5
    data = tmp_path / "bands.tsv"
    with open(data, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, c) in enumerate(zip(ts, te)):
            f.write("%d\t%g\t%g\n" % (i, a, c))
    return data


def _env():
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def read_tables(stem, s_freq):
    """<stem>_ESS.tsv / <stem>_ESS_chains.tsv -> (column names, an EssSummary-like object of host arrays, the _ESS rows)"""
    from literate_amd import logs, ops
    lines = open(stem + "_ESS_chains.tsv").read().splitlines()
    assert lines[0].split("\t") == logs.ESS_CHAIN_HEAD
    recs = [l.split("\t") for l in lines[1:]]
    names = []
    for r in recs:
        if r[1] not in names:
            names.append(r[1])
    C, K = len(recs) // len(names), len(names)
    assert len(recs) == C * K and [int(r[0]) for r in recs] == [c for c in range(C) for _ in range(K)]
    v = np.array([[float(x) for x in r[2:6]] for r in recs]).reshape(C, K, 4)
    stop = np.array([int(r[6]) for r in recs]).reshape(C, K)
    top = [l.split("\t") for l in open(stem + "_ESS.tsv").read().splitlines()]
    assert top[0] == logs.ESS_HEAD and [t[0] for t in top[1:]] == names
    col = np.array([[float(t[1]), float(t[2]), float(t[5])] for t in top[1:]])
    res = ops.EssSummary(v[..., 0], v[..., 1], v[..., 2] / s_freq, v[..., 3], stop, col[:, 0], col[:, 1], col[:, 2], None)
    return names, res, top[1:]


def check_tables(stem, s_freq, rows, n_samples, cols, burnin):
    names, res, top = read_tables(stem, s_freq)
    X, _ = er.kept(rows, n_samples, cols, burnin)
    er.check(res._replace(n=X.shape[2]), rows, n_samples, cols, burnin)
    for k, t in enumerate(top):
        e = res.ess[:, k]
        fin = np.isfinite(e)
        if fin.any():
            assert float(t[3]) == e[fin].min() and int(t[4]) == int(np.argmin(np.where(fin, e, np.inf)))
        else:
            assert t[3] == "nan" and t[4] == "nan"
        assert int(t[6]) == int((fin & (e < 200)).sum()) and int(t[7]) == int((res.stop_lag[:, k] == 0).sum())
    return names


def test_cli_ess_matches_restatement_on_the_logs(G, tmp_path):
    from literate_amd import logs
    data = _example_data(G, tmp_path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "LiteRateForward.py"), "-d", str(data), "-TBP", "-n", "3000",
                          "-s", "5", "-p", "1000", "-seed", "7", "--chains", "5", "--ess", "0.1"], check=True,
                         capture_output=True, text=True, timeout=300, env=_env()).stdout
    assert "lowest ESS" in out and "highest R-hat" in out
    logdir = tmp_path / "literate_mcmc_logs"
    rows = np.stack([np.loadtxt(logs.log_paths(str(data), 0, "", c)[1]["mcmc"], skiprows=1, ndmin=2) for c in range(5)], 1)
    assert rows.shape[:2] == (600, 5) and rows.shape[2] >= 13        # (+ the adequacy columns)
    cols = [1, 2, 3, 4, 5, 6, 7, 10, 11, 12]
    stem = logs.log_paths(str(data), 0, "")[1]["div"][:-len("_div.log")]
    names = check_tables(stem, 5, rows, 600, cols, 0.1)
    assert names == [logs.MCMC_HEAD[c] for c in cols]
    shutil.rmtree(logdir)


def test_cli_ess_two_ranks_and_resume_are_byte_identical(G, tmp_path):
    """The sharded run (two gloo ranks on one GPU, rows gathered to rank 0 once) and a run resumed from --checkpoint
    write the one-process run's ESS tables byte for byte."""
    data = _example_data(G, tmp_path)
    args = [os.path.join(ROOT, "LiteRateForward.py"), "-d", str(data), "-TBP", "-n", "600", "-s", "20", "-p", "200", "-seed", "31",
            "-model_BDI", "2", "--chains", "5", "--block", "130", "--ess", "0.1"]
    env = _env()
    subprocess.run([sys.executable] + args + ["-out", "_one"], check=True, stdout=subprocess.DEVNULL, timeout=300, env=env)
    ck = str(tmp_path / "ck")
    subprocess.run([sys.executable] + args + ["-out", "_res", "--checkpoint", ck], check=True, stdout=subprocess.DEVNULL,
                   timeout=300, env=env)
    out = subprocess.run([sys.executable] + args + ["-out", "_res", "--checkpoint", ck], check=True, capture_output=True,
                         text=True, timeout=300, env=env)
    assert "resumed from" in out.stdout
    env2 = dict(env, LR_DIST_BACKEND="gloo")
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                    "127.0.0.1", "--master-port", "29563"] + args + ["-out", "_two"], check=True, stdout=subprocess.DEVNULL,
                   timeout=300, env=env2)
    logdir = tmp_path / "literate_mcmc_logs"
    for suffix in ("_ESS.tsv", "_ESS_chains.tsv"):
        one = open(logdir / ("example_BDk_one" + suffix), "rb").read()
        assert len(one) > 200
        assert open(logdir / ("example_BDk_two" + suffix), "rb").read() == one, suffix
        assert open(logdir / ("example_BDk_res" + suffix), "rb").read() == one, suffix
    shutil.rmtree(logdir)


def _table_log(path):
    head = open(path).readline().rstrip("\n").split("\t")
    return head, np.loadtxt(path, skiprows=1, ndmin=2)


def test_ddrate_cli_ess_matches_restatement(G, tmp_path):
    data = _bands_data(G, tmp_path)
    subprocess.run([sys.executable, os.path.join(ROOT, "DDRate.py"), "-d", str(data), "-n", "600", "-s", "10", "-p", "300",
                    "-seed", "21", "--chains", "3", "--ess", "0.2"], check=True, stdout=subprocess.DEVNULL, timeout=300,
                   env=_env())
    stem = str(tmp_path / "bands_21_LDDN_MDDN")
    logs_ = [_table_log(stem + "_c%d.log" % c) for c in range(3)]
    head = logs_[0][0]
    want = ["posterior", "likelihood", "prior", "l_max", "steepness_k", "midpoint_x0", "initCarryingCap", "maxCarryingCap",
            "m_max", "nuB", "nuD"]
    cols = [head.index(w) for w in want]
    rows = np.stack([t for _, t in logs_], 1)
    assert rows.shape[:2] == (60, 3)
    assert check_tables(stem, 10, rows, 60, cols, 0.2) == want


def test_trend_rate_cli_ess_matches_restatement(G, golden_dir, tmp_path):
    R = np.load(os.path.join(golden_dir, "ratemaps.npz"))
    data = _bands_data(G, tmp_path)
    trend_file = tmp_path / "trend.tsv"
    with open(trend_file, "w") as f:
        f.write("year\ttrend\n")
        for i, v in enumerate(R["trend_raw"]):
            f.write("%d\t%r\n" % (i, float(v)))
    subprocess.run([sys.executable, os.path.join(ROOT, "trend_rate.py"), "-d", str(data), "-n", "600", "-s", "10", "-p", "300",
                    "-seed", "23", "-trend_data", str(trend_file), "-trend_index", "1", "--chains", "3", "--ess", "0.2"],
                   check=True, stdout=subprocess.DEVNULL, timeout=300, env=_env())
    logs_ = [_table_log(str(tmp_path / ("bands_23_EXPB_EXPD_c%d_1.trendrate.log" % c))) for c in range(3)]
    head = logs_[0][0]
    want = ["posterior", "likelihood", "prior", "l_min", "m_min", "alpha", "beta", "delta", "gamma"]
    cols = [head.index(w) for w in want]
    rows = np.stack([t for _, t in logs_], 1)
    assert check_tables(str(tmp_path / "bands_23_EXPB_EXPD_1"), 10, rows, 60, cols, 0.2) == want
