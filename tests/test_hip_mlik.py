"""Marginal likelihoods of the DDRate models on the device (include/literate_hip_mlik.h): the chains against the numpy
restatement tests/helpers/mlik_ref.py iteration by iteration - every (m_birth, m_death) combination, 1, 2, 63, 64, 65 and 512
bins, 2, 3 and 5 temperatures in 2, 9 and 15 chains (a last workgroup partly empty), the coldest-to-hottest ladder with its
window scales, the hottest chain against the oracle's DDRate loop as well - within rtol 1e-9, atol 1e-9; a run cut into
launches or into groups of replicates bit for bit; exact-size, dirty, guarded buffers; every argument error in the header's
order with the buffers untouched; the closed-form marginal likelihood of the constant-rate model with the bound and the
restatement's sd of tests/test_mlik_host.py; lr_mlik_estimate against the restatement at rtol 1e-12; and the command line end
to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import mlik_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IT = 300
BINS = (1, 2, 63, 64, 65, 512)
LADDERS = ((2, 1), (3, 3), (5, 3))          # (T, replicates): 2, 9 and 15 chains, four to a workgroup


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def synthetic(n_bins, seed, m_birth, m_death):
    """seeded statistics of n_bins bins: a diversity trajectory with its births and deaths"""
    rng = np.random.default_rng(seed)
    DT = np.abs(20.0 + np.cumsum(rng.normal(size=n_bins) * 3.0)) + 1.0 + rng.random(n_bins)
    n_spec, n_exti = rng.poisson(0.3 * DT), rng.poisson(0.2 * DT)
    origin = -float(n_bins) - 3.0
    return ref.Model(n_spec, n_exti, DT, origin, origin + n_bins + 1.0, m_birth, m_death, init_death=0.15)


def golden(m_birth, m_death):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ratemaps.npz"))
    return ref.Model(z["N_SPEC"], z["N_EXTI"], z["DT"], -32.0, 1.0, m_birth, m_death)


def dev_data(M):
    from literate_amd import ops
    return ops.MlikData(M.n_spec, M.n_exti, M.DT, M.origin, M.present, M.m_birth, M.m_death, M.init_death)


def ladder(T):
    betas = ref.temperatures(T, 0.3)
    return betas, ref.window_scales(betas, 8.0)


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    same_inf = np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(got)], want[np.isinf(want)])
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / (1e-9 + 1e-9 * np.abs(want[fin]))
    worst = float(err.max()) if err.size else 0.0
    print("%s: largest error %.3g of the tolerance" % (what, worst))
    if not (same_inf and worst <= 1.0 and np.isfinite(got[fin]).all()):
        at = np.argwhere(~np.isclose(got, want, rtol=1e-9, atol=1e-9))[:3]
        raise AssertionError("%s: differs first at %s: %s against %s" % (what, at.tolist(), got[tuple(at[0])], want[tuple(at[0])]))


# (e) every model once, the bin counts and ladders cycling under them so that each is met by several models
E_CASES = [(mb, md, BINS[i % 6], LADDERS[i % 3]) for i, (mb, md) in enumerate(ref.MODELS)] + \
          [(2, 2, 512, (5, 3)), (2, -1, 65, (2, 1)), (1, 2, 1, (3, 3))]


@pytest.mark.parametrize("m_birth,m_death,n_bins,shape", E_CASES)
def test_e_the_chains_follow_the_restatement_iteration_by_iteration(m_birth, m_death, n_bins, shape):
    from literate_amd import ops
    from oracle.dd_mcmc_oracle import PhiloxDraws, run_dd_mcmc
    T, R = shape
    M = synthetic(n_bins, 100 + n_bins, m_birth, m_death)
    betas, scales = ladder(T)
    seed, rep0 = 7 + n_bins, (0 if T == 2 else 4)
    rows, state = ops.mlik_run(dev_data(M), betas, scales, R, N_IT, 1, seed, rep0=rep0)
    rows, state = rows.cpu().numpy(), state.cpu().numpy()
    want_rows, want_state = ref.run(M, betas, scales, R, N_IT, 1, seed, rep0=rep0)
    assert rows.shape == (N_IT, R, T, ref.ROW_W) and state.shape == (R, T, ref.STATE_W)
    close(rows, want_rows, "rows")
    close(state, want_state, "state")
    assert np.array_equal(state[:, :, 10:14], want_state[:, :, 10:14])            # proposals made and accepted
    assert np.array_equal(rows[:, :, :, 1], np.broadcast_to(betas, (N_IT, R, T)))
    acc = want_state[:, :, 12:14].sum()
    assert acc > 0.2 * N_IT * R * T, "the restatement's chains hardly move: the case tests little"
    # the hottest chain is DDRate.py's own
    assert betas[-1] == 1.0 and scales[-1] == 1.0
    for r in range(R):
        with np.errstate(all="ignore"):
            o = np.array([w[:14] for w in run_dd_mcmc(M.n_spec, M.n_exti, M.DT, M.time_range, M.origin, M.present, m_birth, m_death,
                                                      PhiloxDraws(seed, (rep0 + r) * T + T - 1), N_IT, 1, init_death=M.init_death)])
        logged = rows[:, r, T - 1, 4:].copy()
        logged[:, 2] += M.origin
        logged[:, 4] += logged[:, 3]
        close(np.column_stack([rows[:, r, T - 1, 2:4], logged]), np.column_stack([o[:, 2], o[:, 5], o[:, 6:14]]),
              "replicate %d at beta 1 against run_dd_mcmc" % r)


@pytest.mark.parametrize("model", [(2, 2), (0, 0), (1, -1)])
def test_e_on_the_golden_statistics(model):
    from literate_amd import ops
    M = golden(*model)
    betas, scales = ladder(3)
    rows, state = ops.mlik_run(dev_data(M), betas, scales, 2, N_IT, 1, 3)
    want_rows, want_state = ref.run(M, betas, scales, 2, N_IT, 1, 3)
    close(rows.cpu().numpy(), want_rows, "rows")
    close(state.cpu().numpy(), want_state, "state")


def bits(ts):
    return [np.ascontiguousarray(t.cpu().numpy()).tobytes() for t in ts]


def test_f_a_run_cut_into_launches_or_groups_of_replicates_is_the_same_run():
    import torch
    from literate_amd import ops
    M = synthetic(65, 9, 2, 2)
    data = dev_data(M)
    betas, scales = ladder(3)
    R, s, seed = 5, 7, 21                                  # s divides none of the cuts 100, 101
    rows, state = ops.mlik_run(data, betas, scales, R, N_IT, s, seed)
    st = ops.mlik_init(data, betas, scales, R, seed)
    parts = [ops.mlik_steps(data, betas, scales, st, a, b - a, s, seed) for a, b in ((0, 100), (100, 101), (101, N_IT))]
    assert [int(p.shape[0]) for p in parts] == [15, 0, 28] and rows.shape[0] == 43
    assert bits([torch.cat(parts), st]) == bits([rows, state])
    a_rows, a_state = ops.mlik_run(data, betas, scales, 2, N_IT, s, seed, rep0=0)
    b_rows, b_state = ops.mlik_run(data, betas, scales, 3, N_IT, s, seed, rep0=2)
    assert bits([torch.cat([a_rows, b_rows], dim=1), torch.cat([a_state, b_state])]) == bits([rows, state])
    one = ops.mlik_steps(data, betas, scales, ops.mlik_init(data, betas, scales, R, seed), 0, 0, s, seed)
    assert one.shape[0] == 0


@pytest.mark.parametrize("n_bins,shape", [(1, (2, 1)), (64, (3, 3)), (512, (5, 3))])
def test_f_the_buffer_contract_on_exact_size_guarded_buffers(n_bins, shape):
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    T, R = shape
    M = synthetic(n_bins, 5, 2, 2)
    data = dev_data(M)
    betas, scales = ladder(T)

    def whole():
        state = ops.mlik_init(data, betas, scales, R, 9)
        first = ops.mlik_steps(data, betas, scales, state, 0, 25, 3, 9)
        rows = ops.mlik_steps(data, betas, scales, state, 25, 40, 3, 9)           # rows of iterations 27, 30, .. 63
        est = ops.mlik_estimate(rows, betas, row0=2)
        return (first, rows, state) + tuple(est)

    out = contract(ops, torch, whole, label="mlik bins %d" % n_bins)
    assert out[0].shape[0] == 9 and out[1].shape[0] == 13 and out[1][0, 0, 0, 0] == 27 and out[1][-1, 0, 0, 0] == 63


def test_f_argument_errors_in_the_headers_order_leave_the_buffers_untouched():
    import torch
    from helpers.abi_cases import refuses
    from literate_amd import _hip, ops
    lib = _hip.load()
    M = synthetic(8, 5, 2, 2)
    data = dev_data(M)
    betas, scales = ladder(3)
    big = dev_data(synthetic(513, 5, 2, 2))
    bad0, desc, one = np.array([0.1, 0.5, 1.0]), np.array([0.0, 0.7, 0.6, 1.0]), np.array([1.0])
    inf_s = np.array([1.0, np.inf, 1.0])
    for what, call, code in (
            ("513 bins", lambda: ops.mlik_init(big, betas, scales, 2, 1), "LR_ERR_SIZE"),
            ("513 bins before the betas", lambda: ops.mlik_init(big, bad0, scales, 2, 1), "LR_ERR_SIZE"),
            ("T = 1", lambda: ops.mlik_init(data, one, one, 2, 1), "LR_ERR_SIZE"),
            ("T = 1 before the model", lambda: ops.mlik_init(dev_data(synthetic(8, 5, 3, 2)), one, one, 2, 1), "LR_ERR_SIZE"),
            ("m_birth 3", lambda: ops.mlik_init(dev_data(synthetic(8, 5, 3, 2)), betas, scales, 2, 1), "LR_ERR_MODEL"),
            ("betas[0] != 0", lambda: ops.mlik_init(data, bad0, scales, 2, 1), "LR_ERR_MODEL"),
            ("descending betas", lambda: ops.mlik_init(data, desc, np.ones(4), 2, 1), "LR_ERR_MODEL"),
            ("a scale not finite", lambda: ops.mlik_init(data, betas, inf_s, 2, 1), "LR_ERR_MODEL"),
            ("rep0 < 0", lambda: ops.mlik_init(data, betas, scales, 1, 1, rep0=-1), "LR_ERR_SIZE")):
        refuses(ops, torch, call, code, label=what, entry="lr_mlik_init")
    state = ops.mlik_init(data, betas, scales, 2, 1)
    for what, call, code in (
            ("steps: descending betas", lambda: ops.mlik_steps(data, desc[:3], scales, state, 0, 10, 1, 1), "LR_ERR_MODEL"),
            ("steps: a scale not finite", lambda: ops.mlik_steps(data, betas, inf_s, state, 0, 10, 1, 1), "LR_ERR_MODEL")):
        before = state.clone()
        refuses(ops, torch, call, code, label=what, entry="lr_mlik_steps")
        assert torch.equal(before, state)
    # n_rows too small, and the order NULL < SIZE < MODEL < the counts: straight at the library, on buffers of a known fill
    rows = torch.full((9, 2, 3, ref.ROW_W), 7.0, dtype=torch.float64, device="cuda")
    before = state.clone()
    bp, sp = (x.ctypes.data_as(_hip.c_vp) for x in (betas, scales))
    b0 = bad0.ctypes.data_as(_hip.c_vp)

    def steps(d=data, b=bp, st=state, n_rows=10, rows_=rows, it0=0, n_it=10, s=1):
        return _hip.launch(lib.lr_mlik_steps, d.device, _hip.ptr(d.n_spec), _hip.ptr(d.n_exti), _hip.ptr(d.DT), d.n_bins, d.origin,
                           d.present, d.m_birth, d.m_death, d.init_death, b, sp, 3, 1, 0, 2, _hip.ptr(st), it0, n_it, s, _hip.ptr(rows_),
                           n_rows)

    assert steps(n_rows=9) == _hip.LR_ERR_SIZE and steps(b=b0, n_rows=9) == _hip.LR_ERR_MODEL
    assert steps(s=0) == steps(it0=-1) == steps(n_it=-1) == _hip.LR_ERR_SIZE and steps(b=b0, s=0) == _hip.LR_ERR_MODEL
    assert steps(d=big, b=b0) == _hip.LR_ERR_SIZE and steps(d=big, st=None) == _hip.LR_ERR_NULL and steps(rows_=None) == _hip.LR_ERR_NULL
    torch.cuda.synchronize()
    assert torch.equal(before, state) and bool((rows == 7.0).all())
    # the estimator's
    good = torch.zeros((6, 2, 3, ref.ROW_W), dtype=torch.float64, device="cuda")
    for what, call, code in (("row0 = n_rows", lambda: ops.mlik_estimate(good, betas, row0=6), "LR_ERR_SIZE"),
                             ("row0 < 0", lambda: ops.mlik_estimate(good, betas, row0=-1), "LR_ERR_SIZE"),
                             ("betas[0] != 0", lambda: ops.mlik_estimate(good, bad0), "LR_ERR_MODEL"),
                             ("descending betas", lambda: ops.mlik_estimate(good, desc[:3]), "LR_ERR_MODEL")):
        refuses(ops, torch, call, code, label=what, entry="lr_mlik_estimate")


def test_g_the_constant_rate_models_marginal_likelihood_on_the_device():
    """The run of tests/test_mlik_host.py (b) on the device: |mean_r ss - exact| <= 4 sd_r / sqrt(R), and sd_r at most twice the
    restatement's 0.1844.  The device's run (Philox seed 20261019) gives mean_r ss = -218.4745, sd_r = 0.1826 (se 0.0323), the pooled
    stones -218.4595; exact -218.4567 (profiles/EXPERIMENTS.md)."""
    from literate_amd import ops
    H = ref
    EXACT = ref.const_log_z(H.B, H.D, H.S)
    M = ref.const_model(H.B, H.D)
    betas = ref.temperatures(H.T, H.ALPHA)
    scales = ref.window_scales(betas, H.WIDEN)
    rows, state = ops.mlik_run(dev_data(M), betas, scales, H.R, H.N_IT, H.S_FREQ, H.SEED)
    n = int(rows.shape[0])
    est = ops.mlik_estimate(rows, betas, row0=int(H.BURN * n))
    ss = est.ss.cpu().numpy()
    mean, sd = float(np.mean(ss)), float(np.std(ss, ddof=1))
    print("exact %.4f, mean ss %.4f, sd %.4f, se %.4f, pooled %.4f, ti %.4f"
          % (EXACT, mean, sd, sd / math.sqrt(H.R), float(est.pooled[-1]), float(est.ti.mean())))
    assert abs(mean - EXACT) <= 4 * sd / math.sqrt(H.R)
    assert sd <= 2 * H.REF_SD
    want = ref.const_mean_lik(betas, H.B, H.D, H.S)
    lm = est.lik_mean.cpu().numpy()
    assert (np.abs(lm.mean(axis=0) - want) <= 5 * np.std(lm, axis=0, ddof=1) / math.sqrt(H.R)).all()


@pytest.mark.parametrize("n_rows,R,T,row0", [(300, 3, 4, 0), (300, 3, 4, 41), (1, 2, 2, 0), (700, 1, 5, 13), (5, 1, 2, 4)])
def test_h_the_estimator_against_the_restatement(n_rows, R, T, row0):
    from literate_amd import ops
    rng = np.random.default_rng(n_rows + T)
    betas = ref.temperatures(T, 0.3)
    rows = rng.normal(size=(n_rows, R, T, ref.ROW_W))
    rows[:, :, :, ref.R_LIK] = -6e5 + 1e3 * rng.normal(size=(n_rows, R, T))
    if n_rows > 100:
        rows[row0 + 3, 0, 1, ref.R_LIK] = -np.inf            # one -inf entry
        rows[:, R - 1, 0, ref.R_LIK] = -np.inf               # an all -inf stone
    est = ops.mlik_estimate(rows, betas, row0=row0)
    want = ref.estimate(rows, betas, row0)
    for k in ("stone", "ss", "lik_mean", "lik_var", "ti", "pooled"):
        got, w = getattr(est, k).cpu().numpy(), want[k]
        assert got.shape == w.shape, k
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(got), np.isnan(w)) and np.array_equal(got[np.isinf(w)], w[np.isinf(w)]), (k, got, w)
        np.testing.assert_allclose(got[fin], w[fin], rtol=1e-12, atol=0, err_msg=k)
    if n_rows > 100:
        assert want["stone"][R - 1, 0] == -np.inf and np.isfinite(want["stone"][0, 1]) and want["ss"][R - 1] == -np.inf
    if n_rows - row0 == 1:
        assert np.isnan(want["lik_var"]).all()


def test_i_the_command_line_end_to_end(tmp_path):
    from helpers import waic_cases as W
    from literate_amd import mlik
    from literate_amd.ddrate import model_suffix
    from literate_amd.literate_library import create_bins, parse_ts_te
    data = W._data(str(tmp_path))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    files = []
    for mb, md in ((2, 2), (0, 0)):
        cmd = [sys.executable, os.path.join(ROOT, "DDRate.py"), "-d", data, "-TBP", "-n", "3000", "-s", "10", "-p", "1000", "-seed", "31",
               "--chains", "4", "-m_birth", str(mb), "-m_death", str(md), "--mlik", "0.2", "--mlik_temps", "5", "--mlik_reps", "3"]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=280, env=env)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        line = [l for l in out.stdout.splitlines() if l.startswith("MLIK:")]
        assert len(line) == 1 and "_MLIK.tsv" in line[0]
        stem = os.path.join(str(tmp_path), "example_31" + model_suffix(mb, md))
        assert all(os.path.exists(stem + k) for k in ("_MLIK.tsv", "_MLIK_temps.tsv", "_MLIK.npz"))
        fit = mlik.read_fit(stem)
        TS, TE, PRESENT, ORIGIN = parse_ts_te(data, True, -1, -1, .5)
        origin, present, n_spec, n_exti, DT, n_bins, _ = create_bins(ORIGIN, PRESENT, np.asarray(TS, float), np.asarray(TE, float), 0)
        res = mlik.run(n_spec, n_exti, DT, origin, present, mb, md, 0.1, 5, 3, 3000, 10, 31, 0.2, 0.3, 8.0)
        print(fit)
        assert list(fit) == mlik.FIT_HEAD and fit["model"] == model_suffix(mb, md) and fit["bins"] == n_bins
        for k in mlik.FIT_HEAD:
            assert fit[k] == res.fit[k] or (isinstance(fit[k], float) and math.isnan(fit[k]) and math.isnan(res.fit[k])), k
        assert math.isfinite(fit["logZ_ss"]) and fit["logZ_ss_se"] > 0 and fit["samples_kept"] == 240
        with open(stem + "_MLIK_temps.tsv") as f:
            temps = [l.rstrip("\n").split("\t") for l in f]
        assert temps[0] == mlik.TEMPS_HEAD and len(temps) == 6 and float(temps[1][1]) == 0.0 and float(temps[5][1]) == 1.0
        with np.load(stem + "_MLIK.npz") as z:
            assert z["ss"].shape == (3,) and float(z["logZ_ss"]) == fit["logZ_ss"] and z["fingerprint"][0] == len(TS)
        files.append(stem + "_MLIK.npz")
    out = subprocess.run([sys.executable, "-m", "literate_amd.mlik"] + files, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    table = [l.split("\t") for l in out.stdout.strip().splitlines()]
    print(out.stdout)
    assert table[0] == mlik.COMPARE_HEAD and len(table) == 3
    assert float(table[1][4]) == 0.0 and float(table[2][4]) == 2.0 * (float(table[2][2]) - float(table[1][2])) < 0
    # the run is refused beyond the bins the sampler takes, with a message that says so
    assert "512" in mlik.arg_error(0.2, 5, 3, 3000, 10, 0.3, 8.0, n_bins=513)
