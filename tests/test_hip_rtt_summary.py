"""lr_rtt_summary on the device: posterior rates through time (mean and 95 % HPD of birth, death and net rates per unit
bin, shift frequencies, K histograms) against the reference's get_marginal_rates / plot_net_rate / get_r_plot /
get_K_values (plotRJforward.v3.py) as the oracle restates them, on the reference's own output, engine runs, hand-built
edge cases, chunked calls, cfg4's shape and the CLI."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, KM = 139, 13, 32
L0, TL0, M0, TM0 = H, H + KM, H + 2 * KM - 1, H + 3 * KM - 1


@pytest.fixture(scope="module")
def G(golden_dir):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    return np.load(os.path.join(golden_dir, "binning_lik.npz"))


# ---- building traces and the reference's answers -----------------------------------------------------------------
def make_trace(rows, a, b):
    """rows[s][c] = (sp_row, ex_row) in the *_rates.log layout (K rates then K - 1 shift times) -> [S, C, W] trace."""
    S, C = len(rows), len(rows[0])
    T = np.full((S, C, W), np.nan)
    for s in range(S):
        for c in range(C):
            sp, ex = (np.asarray(r, dtype=float) for r in rows[s][c])
            kl, km = (len(sp) + 1) // 2, (len(ex) + 1) // 2
            T[s, c, 6], T[s, c, 7], T[s, c, 8], T[s, c, 9] = kl, km, a, b
            T[s, c, L0:L0 + kl], T[s, c, TL0:TL0 + kl - 1] = sp[:kl], sp[kl:]
            T[s, c, M0:M0 + km], T[s, c, TM0:TM0 + km - 1] = ex[:km], ex[km:]
    return T


def trace_rows(T, c):
    """(sp rows, ex rows) of chain c, as the logs hold them"""
    from literate_amd.engine import split_trace_row
    out = [split_trace_row(T[s, c]) for s in range(T.shape[0])]
    return [o[1] for o in out], [o[2] for o in out]


def reference_group(sp_rows, ex_rows, a, b, burnin):
    """The reference's summary of one log (or COMBINED log) -> dict of ascending-time arrays (oracle restatement)."""
    from oracle import literate_oracle as lo
    ms, los, his, mat_s = lo.marginal_rates_from_rows(sp_rows, b, a, burnin)
    me, loe, hie, mat_e = lo.marginal_rates_from_rows(ex_rows, b, a, burnin)
    net = mat_s - mat_e                                          # plot_net_rate
    hn = np.array([lo.calcHPD(net[:, i], 0.95) for i in range(net.shape[1])])
    n = mat_s.shape[0]
    burn = len(sp_rows) - n
    edges = np.arange(a, b)
    freq, kc = [], []
    for rows in (sp_rows, ex_rows):
        shifts = [t for r in rows[burn:] for t in r[(len(r) + 1) // 2:]]
        h = np.histogram(shifts, bins=edges)[0] / float(n) if len(shifts) > 1 else np.zeros(len(edges) - 1)
        freq.append(h)
        kc.append(np.bincount([(len(r) + 1) // 2 for r in rows[burn:]], minlength=KM + 1)[1:KM + 1])
    # (get_marginal_rates returns the most recent bin first; the device, like the R vectors, ascending time)
    rates = np.array([[ms, los, his], [me, loe, hie], [net.mean(0), hn[:, 0], hn[:, 1]]])[:, :, ::-1]
    return dict(rates=rates, freq=np.array(freq), k=np.array(kc), n=n, mat_s=mat_s, mat_e=mat_e)


def check_group(res, g, ref):
    """device result of group g against the reference: HPD ends bit-identical, means to 1e-12, counts exact"""
    rates = res.rates[g].cpu().numpy()
    R = ref["rates"]
    for k in range(3):
        assert np.array_equal(rates[k, 1], R[k, 1]) and np.array_equal(rates[k, 2], R[k, 2]), k
    assert np.allclose(rates[:2, 0], R[:2, 0], rtol=1e-12, atol=0)
    scale = np.abs(ref["mat_s"]).mean(0)[::-1] + np.abs(ref["mat_e"]).mean(0)[::-1]     # net means may cancel to ~0
    assert np.all(np.abs(rates[2, 0] - R[2, 0]) <= 1e-12 * scale)
    assert np.array_equal(res.shift_freq[g].cpu().numpy(), ref["freq"])
    assert np.array_equal(res.k_counts[g].cpu().numpy(), ref["k"])


# ---- 1. the reference's own output ---------------------------------------------------------------------------------
def test_rtt_matches_get_marginal_rates_on_shipped_logs(G, golden_dir):
    """tests/golden/marginal_rates.npz: get_marginal_rates run by the reference on the shipped metal_bands rate logs."""
    from literate_amd import ops
    M = np.load(os.path.join(golden_dir, "marginal_rates.npz"))
    b, a = M["ages"]
    sp = [r[~np.isnan(r)] for r in M["sp/rows"]]
    ex = [r[~np.isnan(r)] for r in M["ex/rows"]]
    T = make_trace([[(s, e)] for s, e in zip(sp, ex)], a, b)
    res = ops.rtt_summary(T, T.shape[0], a, b, burnin=0.2, pooled=False)
    assert res.n_samples == 800 == int(M["sp/n_samples"])
    assert np.array_equal(res.time, M["sp/time_frames"])
    rates = res.rates[0].cpu().numpy()
    for k, kind in enumerate(("sp", "ex")):
        assert np.array_equal(rates[k, 1], M[kind + "/hpd_lo"][::-1])
        assert np.array_equal(rates[k, 2], M[kind + "/hpd_hi"][::-1])
        assert np.allclose(rates[k, 0], M[kind + "/mean"][::-1], rtol=1e-12, atol=0)
    check_group(res, 0, reference_group(sp, ex, a, b, 0.2))


# ---- 2. engine runs against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", [("example_TBP", 0), ("metal_bands", 2)])
def test_rtt_engine_per_chain_and_pooled_match_oracle(G, name, model):
    from literate_amd.engine import ChainEngine
    eng = ChainEngine(G[name + "/ts"], G[name + "/te"], 16, model=model, seed=21, s_freq=5, n_trace_slots=300)
    eng.init()
    eng.steps(1500)
    T = eng.trace_rows()
    a, b = eng.start_time, eng.end_time
    per = eng.rtt_summary(burnin=0.2, pooled=False)
    pool = eng.rtt_summary(burnin=0.2, pooled=True)
    eng.close()
    assert per.rates.shape == (16, 3, 3, per.time.size) and pool.rates.shape == (1, 3, 3, per.time.size)
    assert T[:, :, 6].max() > 1 and T[:, :, 7].max() > 1            # shifts were sampled
    sp_all, ex_all = [], []
    for c in range(16):
        sp, ex = trace_rows(T, c)
        check_group(per, c, reference_group(sp, ex, a, b, 0.2))
        burn = int(0.2 * len(sp))                                   # combine_logs, then burnin = 0
        sp_all += sp[burn:]
        ex_all += ex[burn:]
    assert pool.n_samples == len(sp_all) == 16 * 240
    check_group(pool, 0, reference_group(sp_all, ex_all, a, b, 0))


# ---- 3. edges --------------------------------------------------------------------------------------------------------
def _summ(rows, a, b, burnin=0.0, pooled=False, **kw):
    from literate_amd import ops
    T = make_trace(rows, a, b)
    return ops.rtt_summary(T, T.shape[0], a, b, burnin=burnin, pooled=pooled, **kw)


def test_rtt_constant_rates():
    """-const_rates: K = 1 in every sample, rates[0] in every bin; no shift ever sampled"""
    a, b = 10.0, 16.5
    rng = np.random.default_rng(1)
    rows = [[([rng.gamma(2, 0.1)], [rng.gamma(2, 0.05)])] for _ in range(40)]
    res = _summ(rows, a, b)
    ref = reference_group([r[0][0] for r in rows], [r[0][1] for r in rows], a, b, 0.0)
    check_group(res, 0, ref)
    assert np.all(res.shift_freq.cpu().numpy() == 0) and res.k_counts[0, :, 0].tolist() == [40, 40]


def test_rtt_shift_on_an_edge_and_in_the_last_partial_year():
    """a shift at e_3 changes the rate from bin 3 on; one at e_nbins counts in the last bin; one in the partial year
    (e_nbins, b] or before e_0 in none (np.histogram drops it); a lone shift time in a group gives no shift frequencies"""
    a, b = 100.0, 105.5                                    # edges 100 .. 105, 5 bins; time 100.5 .. 104.5
    rows = []
    for i in range(40):
        sp = [0.1, 0.2, 0.3, 103.0, 105.0] if i % 2 else [0.4, 0.5, 100.0]
        ex = [0.05, 0.07, 105.2] if i % 3 else [0.09, 0.03, 99.5]
        rows.append([(sp, ex)])
    res = _summ(rows, a, b)
    ref = reference_group([r[0][0] for r in rows], [r[0][1] for r in rows], a, b, 0.0)
    check_group(res, 0, ref)
    f = res.shift_freq[0].cpu().numpy()
    assert f[0, 3] == 20 / 40 and f[0, 4] == 20 / 40 and f[0, 0] == 20 / 40 and np.all(f[1] == 0)
    lone = [[([0.1, 0.2, 101.0], [0.1])]] + [[([0.1], [0.1])] for _ in range(9)]
    res = _summ(lone, a, b)
    assert np.all(res.shift_freq.cpu().numpy() == 0)
    check_group(res, 0, reference_group([r[0][0] for r in lone], [r[0][1] for r in lone], a, b, 0.0))


def test_rtt_equal_minimum_widths_take_the_first():
    """n = 20, n_in = 19: windows [d0, d18] and [d1, d19] of equal width -> the first"""
    a, b = 0.0, 1.5
    vals = np.array([1.0] + [2.0] * 18 + [3.0])           # d18 - d0 = 1.0 = d19 - d1
    rows = [[([v], [0.5])] for v in np.random.default_rng(2).permutation(vals)]
    res = _summ(rows, a, b)
    r = res.rates[0].cpu().numpy()
    assert r[0, 1, 0] == 1.0 and r[0, 2, 0] == 2.0
    check_group(res, 0, reference_group([x[0][0] for x in rows], [x[0][1] for x in rows], a, b, 0.0))


@pytest.mark.parametrize("burnin", [0.0, 0.95])
def test_rtt_burnin_per_chain_and_pooled(burnin):
    """per chain: min(int(beta S), int(0.9 S)) rows dropped; pooled: int(beta S) from every chain, no cap"""
    a, b = 0.25, 8.75
    rng = np.random.default_rng(3)
    S, C = 100, 3
    rows = []
    for s in range(S):
        row = []
        for c in range(C):
            k = int(rng.integers(1, 4))
            t = np.sort(rng.uniform(a - 0.5, b, k - 1))
            row.append((list(rng.gamma(2, 0.1, k)) + list(t), list(rng.gamma(2, 0.05, 2)) + [rng.uniform(a, b)]))
        rows.append(row)
    T = make_trace(rows, a, b)
    from literate_amd import ops
    per = ops.rtt_summary(T, S, a, b, burnin=burnin, pooled=False)
    pool = ops.rtt_summary(T, S, a, b, burnin=burnin, pooled=True)
    keep = S - min(int(burnin * S), int(0.9 * S))
    assert per.n_samples == keep
    assert pool.n_samples == C * (S - int(burnin * S))
    sp_all, ex_all = [], []
    for c in range(C):
        sp, ex = trace_rows(T, c)
        check_group(per, c, reference_group(sp, ex, a, b, burnin))
        sp_all += sp[int(burnin * S):]
        ex_all += ex[int(burnin * S):]
    check_group(pool, 0, reference_group(sp_all, ex_all, a, b, 0))


def test_rtt_too_few_samples_and_integer_span_raise():
    rows = [[([0.1], [0.1])] for _ in range(3)]
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        _summ(rows, 0.0, 3.5, burnin=0.7)                 # one row left: round(0.95) = 1 < 2 (calcHPD raises)
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        _summ(rows, 0.0, 3.0)                              # b - a integer valued: the reference indexes past its matrix
    with pytest.raises(ValueError, match="LR_ERR_WORKSPACE"):
        _summ(rows, 0.0, 3.5, workspace_bytes=64)


# ---- 4. chunking and size ----------------------------------------------------------------------------------------------
def _random_trace(S, C, a, b, seed):
    rng = np.random.default_rng(seed)
    T = np.full((S, C, W), np.nan)
    for kind, (r0, t0) in enumerate(((L0, TL0), (M0, TM0))):
        K = rng.integers(1, 9, (S, C))
        T[:, :, 6 + kind] = K
        T[:, :, r0:r0 + KM] = rng.gamma(2, 0.1, (S, C, KM))
        t = np.sort(rng.uniform(a - 1, b + 1, (S, C, KM - 1)), axis=-1)
        t[np.arange(KM - 1)[None, None, :] >= (K[:, :, None] - 1)] = np.nan
        T[:, :, t0:t0 + KM - 1] = t
    T[:, :, 8], T[:, :, 9] = a, b
    return T


def test_rtt_chunked_call_is_bitwise_the_full_call(G):
    from literate_amd import _hip, ops
    a, b = 3.0, 2003.5                                     # 2000 bins
    S, C = 24, 64
    T = _random_trace(S, C, a, b, 4)
    full = _hip.load().lr_rtt_summary_workspace_bytes(S, C, a, b, 0.2, 0)
    assert full > 0
    one = ops.rtt_summary(T, S, a, b, burnin=0.2, pooled=False)
    small = ops.rtt_summary(T, S, a, b, burnin=0.2, pooled=False, workspace_bytes=full // 3 - 4096)   # >= 4 chunks
    for x, y in zip(one[1:4], small[1:4]):
        assert np.array_equal(x.cpu().numpy().view(np.int64), y.cpu().numpy().view(np.int64))
    sp, ex = trace_rows(T, 5)
    check_group(one, 5, reference_group(sp, ex, a, b, 0.2))


def numpy_rtt(T, S, a, b, burnin, bins_per_pass=8):
    """Vectorised restatement of the pooled summary (combine_logs, then get_marginal_rates / plot_net_rate /
    get_r_plot / get_K_values with burnin 0) for many rows: -> (rates [3, 3, nb], freq [2, nb], k [2, KMAX])."""
    burn = int(burnin * S)
    R = np.ascontiguousarray(T[burn:S].transpose(1, 0, 2).reshape(-1, W))
    n = R.shape[0]
    edges = np.arange(a, b)
    nb = edges.size - 1
    n_in = int(round(0.95 * n))
    rates, c, freq, kc = [], [], [], []
    for r0, t0, kcol in ((L0, TL0, 6), (M0, TM0, 7)):
        K = R[:, kcol].astype(np.int64)
        t = R[:, t0:t0 + KM - 1]
        live = np.arange(KM - 1)[None, :] < (K[:, None] - 1)
        inside = live & (t >= edges[0]) & (t <= edges[-1])
        idx = np.where(inside, np.minimum(np.searchsorted(edges, np.where(inside, t, edges[0]), side="right") - 1, nb - 1), nb)
        hist = np.zeros((n, nb + 1), dtype=np.int8)
        rows = np.arange(n)
        for k in range(KM - 1):
            hist[rows, idx[:, k]] += 1
        c.append(np.cumsum(hist[:, :nb], axis=1, dtype=np.int8))      # c_i = #{shifts in bins <= i}
        rates.append(R[:, r0:r0 + KM])
        f = hist[:, :nb].sum(0) / float(n)
        freq.append(f if live.sum() > 1 else np.zeros(nb))
        kc.append(np.bincount(K, minlength=KM + 1)[1:KM + 1])
    out = np.zeros((3, 3, nb))
    for i0 in range(0, nb, bins_per_pass):
        i1 = min(nb, i0 + bins_per_pass)
        vb = np.take_along_axis(rates[0], c[0][:, i0:i1].astype(np.int64), axis=1)
        vd = np.take_along_axis(rates[1], c[1][:, i0:i1].astype(np.int64), axis=1)
        for k, v in enumerate((vb, vd, vb - vd)):
            d = np.sort(np.ascontiguousarray(v.T), axis=1)
            # (pairwise summation along the contiguous axis: np.mean down the columns of [n, bins] adds n values one after
            # the other, ~1e-12 relative of rounding at n ~ 1e6 - more than the device's fixed-order sum of sorted values)
            out[k, 0, i0:i1] = d.mean(axis=1)
            w = d[:, n_in - 1:] - d[:, :n - n_in + 1]
            j = np.argmin(w, axis=1)
            out[k, 1, i0:i1] = d[np.arange(i1 - i0), j]
            out[k, 2, i0:i1] = d[np.arange(i1 - i0), j + n_in - 1]
    return out, np.array(freq), np.array(kc)


def test_rtt_cfg4_shape_pooled(G):
    """1024 chains x 1000 rows of a real cfg4 engine run (100k synthetic lineages, 123 unit bins), pooled: against the
    vectorised restatement (itself checked against the oracle on four chains); two calls bitwise equal."""
    from literate_amd import ops, synth
    from literate_amd.engine import ChainEngine
    ts, te, _ = synth.make_lineages(100_000, n_bins=128, n_shifts=20, seed=0)
    eng = ChainEngine(ts, te, 1024, model=0, seed=5, s_freq=20, n_trace_slots=1000)
    eng.init()
    eng.steps(20_000)
    a, b = eng.start_time, eng.end_time
    r1 = eng.rtt_summary(burnin=0.2, pooled=True)
    r2 = eng.rtt_summary(burnin=0.2, pooled=True)
    T = eng.trace_rows()
    eng.close()
    assert T.shape[:2] == (1000, 1024) and r1.n_samples == 1024 * 800
    for x, y in zip(r1[1:4], r2[1:4]):
        assert np.array_equal(x.cpu().numpy().view(np.int64), y.cpu().numpy().view(np.int64))
    # the restatement against the oracle on a subset
    sub = T[:, :4]
    ro, fo, ko = numpy_rtt(sub, 1000, a, b, 0.2)
    sp_all, ex_all = [], []
    for c in range(4):
        sp, ex = trace_rows(sub, c)
        sp_all += sp[200:]
        ex_all += ex[200:]
    ref = reference_group(sp_all, ex_all, a, b, 0)
    assert np.array_equal(ro[:, 1:], ref["rates"][:, 1:]) and np.allclose(ro[:, 0], ref["rates"][:, 0], rtol=1e-12, atol=1e-15)
    assert np.array_equal(fo, ref["freq"]) and np.array_equal(ko, ref["k"])
    # the device against the restatement on all 1024 chains
    rn, fn, kn = numpy_rtt(T, 1000, a, b, 0.2)
    rd = r1.rates[0].cpu().numpy()
    assert np.array_equal(rd[:, 1:], rn[:, 1:])
    assert np.allclose(rd[:2, 0], rn[:2, 0], rtol=1e-12, atol=0)
    assert np.allclose(rd[2, 0], rn[2, 0], rtol=1e-12, atol=1e-12 * np.abs(rn[0, 0]).max())
    assert np.array_equal(r1.shift_freq[0].cpu().numpy(), fn) and np.array_equal(r1.k_counts[0].cpu().numpy(), kn)


# ---- 5. CLI ----------------------------------------------------------------------------------------------------------
def _example_data(G, tmp_path):
    ts, te = G["example_TBP/ts"], G["example_TBP/te"] - 0.5
    data = tmp_path / "example.tsv"
    with open(data, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, b) in enumerate(zip(ts, te)):
            f.write("%d\t%g\t%g\n" % (i, 24.0 - a, 24.0 - b))
    return data


def _env():
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def test_cli_rtt_matches_combined_logs(G, tmp_path):
    """--chains 8 --combine 0.2 --rtt 0.2: the TSVs are what the reference's script computes from the COMBINED logs the
    same run wrote (get_marginal_rates with burnin 0, plot_net_rate, get_r_plot's shift counts, get_K_values)"""
    from literate_amd import logs
    data = _example_data(G, tmp_path)
    subprocess.run([sys.executable, os.path.join(ROOT, "LiteRateForward.py"), "-d", str(data), "-TBP", "-n", "1200", "-s", "20",
                    "-p", "400", "-seed", "7", "--chains", "8", "--combine", "0.2", "--rtt", "0.2"], check=True,
                   stdout=subprocess.DEVNULL, timeout=300, env=_env())
    logdir = tmp_path / "literate_mcmc_logs"
    tab = np.loadtxt(logdir / "example_BD_RTT.tsv", skiprows=1, ndmin=2)
    head = open(logdir / "example_BD_RTT.tsv").readline().split()
    assert head == logs.RTT_HEAD
    mc = np.loadtxt(logdir / "COMBINED_mcmc.log", skiprows=1, ndmin=2)
    mhead = open(logdir / "COMBINED_mcmc.log").readline().split()
    a, b = np.mean(mc[:, mhead.index("root_age")]), np.mean(mc[:, mhead.index("death_age")])
    sp = [np.array(l.split(), float) for l in open(logdir / "COMBINED_sp_rates.log")]
    ex = [np.array(l.split(), float) for l in open(logdir / "COMBINED_ex_rates.log")]
    assert len(sp) == 8 * (60 - 12)
    frames, ms, los, his, mat_s = logs.marginal_rates(sp, b, a, burnin=0)
    _, me, loe, hie, mat_e = logs.marginal_rates(ex, b, a, burnin=0)
    net = mat_s - mat_e
    hn = np.array([logs.calcHPD(net[:, i]) for i in range(net.shape[1])])
    assert np.array_equal(tab[:, 0], frames)
    for col, want in ((2, los), (3, his), (5, loe), (6, hie)):
        assert np.array_equal(tab[:, col], want[::-1]), col
    assert np.array_equal(tab[:, 8], hn[::-1, 0]) and np.array_equal(tab[:, 9], hn[::-1, 1])
    assert np.allclose(tab[:, 1], ms[::-1], rtol=1e-12) and np.allclose(tab[:, 4], me[::-1], rtol=1e-12)
    assert np.allclose(tab[:, 7], net.mean(0)[::-1], rtol=1e-12, atol=1e-12 * np.abs(ms).max())
    edges = np.arange(a, b)
    for col, rows in ((10, sp), (11, ex)):
        shifts = [t for r in rows for t in r[(len(r) + 1) // 2:]]
        want = np.histogram(shifts, bins=edges)[0] / float(len(rows)) if len(shifts) > 1 else np.zeros(len(edges) - 1)
        assert np.array_equal(tab[:, col], want), col
    K = np.loadtxt(logdir / "example_BD_RTT_K.tsv", skiprows=1, dtype=np.int64, ndmin=2)
    assert K[:, 0].tolist() == list(range(1, 33))
    for col, name in ((1, "K_l"), (2, "K_m")):
        u, n = np.unique(mc[:, mhead.index(name)], return_counts=True)
        want = np.zeros(32, dtype=np.int64)
        want[u.astype(int) - 1] = n
        assert np.array_equal(K[:, col], want), name
    shutil.rmtree(logdir)


def test_cli_rtt_two_ranks_and_resume_are_byte_identical(G, tmp_path):
    """The sharded run (two gloo ranks on one GPU, rows gathered to rank 0 once) and a run resumed from --checkpoint
    write the one-process run's TSVs byte for byte."""
    data = _example_data(G, tmp_path)
    args = [os.path.join(ROOT, "LiteRateForward.py"), "-d", str(data), "-TBP", "-n", "600", "-s", "20", "-p", "200", "-seed", "31",
            "-model_BDI", "2", "--chains", "5", "--block", "130", "--rtt", "0.2"]
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
                    "127.0.0.1", "--master-port", "29561"] + args + ["-out", "_two"], check=True, stdout=subprocess.DEVNULL,
                   timeout=300, env=env2)
    logdir = tmp_path / "literate_mcmc_logs"
    for suffix in ("_RTT.tsv", "_RTT_K.tsv"):
        one = open(logdir / ("example_BDk_one" + suffix), "rb").read()
        assert len(one) > 200
        assert open(logdir / ("example_BDk_two" + suffix), "rb").read() == one, suffix
        assert open(logdir / ("example_BDk_res" + suffix), "rb").read() == one, suffix
    shutil.rmtree(logdir)
