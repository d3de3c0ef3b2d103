"""The GPU cases of tests/test_hip_post_summary.py, each run in a child process of its own (under the test's time limit):

    python tests/helpers/post_summary_cases.py CASE [ARGS...]

A case prints its figures, asserts, and exits 0 - or raises.  The yardstick is the numpy restatement
tests/helpers/summary_ref.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import summary_ref as sr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _np(t):
    return t.cpu().numpy()


def col_triples(res):
    """ops.ColSummary -> [G, K, 3]"""
    return np.stack([_np(res.mean), _np(res.lo), _np(res.hi)], axis=-1)


def curve_triples(res):
    """ops.CurveSummary -> [G, kinds, n_bins, 3]"""
    return np.moveaxis(_np(res.values), 2, -1)


def _max_rel(a, b):
    ok = np.isfinite(a) & np.isfinite(b) & (b != 0)
    return float((np.abs(a - b)[ok] / np.abs(b[ok])).max()) if ok.any() else 0.0


def check(what, got, want):
    """print the figures, then assert: HPD ends bit-identical, means within rtol 1e-12, NaN where NaN (sr.check)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape:
        ends = np.array_equal(got[..., 1:], want[..., 1:], equal_nan=True)
        print("%s: %d triples, %d NaN; HPD ends %s; largest relative difference of the means %.3g" % (
            what, want[..., 0].size, int(np.isnan(want[..., 0]).sum()), "identical" if ends else "DIFFER",
            _max_rel(got[..., 0], want[..., 0])))
        sys.stdout.flush()
    sr.check(got, want, what)


# ---- 1. the reference's own output -------------------------------------------------------------------------------------
def case_golden():
    """plotdd_shipped.npz: make_vec_dict run by the reference on its shipped log; one chain, burn-in 0"""
    from literate_amd import ops
    P = np.load(os.path.join(GOLDEN, "plotdd_shipped.npz"))
    rows = np.concatenate([P["l"], P["m"], P["niche_cols"]], axis=1)[:, None, :]          # [1000, 1, 96]
    for pooled in (False, True):
        res = ops.col_summary(rows, 1000, range(96), burnin=0.0, pooled=pooled)
        assert res.n == 1000
        t = col_triples(res)[0]
        for k, (mean, lo, hi) in enumerate((("birth_rate", "birth_minHPD", "birth_maxHPD"),
                                            ("death_rate", "death_minHPD", "death_maxHPD"),
                                            ("niche", "niche_minHPD", "niche_maxHPD"))):
            want = np.stack([P[mean], P[lo], P[hi]], axis=-1)
            check("reference %s pooled=%d" % (mean, pooled), t[32 * k:32 * (k + 1)], want)
    check("restatement", t[None], sr.col_summary(rows, 1000, range(96), 0.0, True))


# ---- 2. curves against the log ---------------------------------------------------------------------------------------
def _dd_data():
    G = np.load(os.path.join(GOLDEN, "binning_lik.npz"))
    D = np.load(os.path.join(GOLDEN, "ddrate.npz"))
    origin, present, _ = D["meta"]
    return G["metal_bands/lib_ts"], G["metal_bands/lib_te"], origin, present


def _engine_case(eng, heads, param_names):
    """posterior_summary per chain and pooled against the restatement applied to log_table_from(trace): the columns the log
    files hold.  heads: the log's per-bin column names of birth and death (and niche, nicheFrac)."""
    eng.init()
    eng.steps(1500)
    S = eng.samples_done()
    assert S == 300
    per = eng.posterior_summary(burnin=0.2, pooled=False)
    pool = eng.posterior_summary(burnin=0.2, pooled=True)
    T = eng.trace_rows()
    table = eng.log_table_from(T)                          # [S, C, log columns]
    head = eng.log_head()
    eng.close()
    n = len(eng.DT)
    tabs = [table[:, :, head.index(h % 0):head.index(h % 0) + n] for h in heads]
    kind_tables = [tabs[0], tabs[1], tabs[0] - tabs[1]] + tabs[2:]          # net = l_i - m_i, one rounded subtraction
    assert per.curves.kinds[:3] == ("birth", "death", "net") and len(per.curves.kinds) == len(kind_tables)
    assert per.curves.n == 240 and pool.curves.n == 240 * T.shape[1] and pool.params.n == pool.curves.n
    moved = np.ptp(table[60:, :, head.index(param_names[3])], axis=0).max()
    print("chains %d, NaN entries in the per-bin columns %d, range of %s after burn-in %.3g" % (
        T.shape[1], int(np.isnan(np.stack(kind_tables)).sum()), param_names[3], moved))
    assert moved > 0
    for res, pooled in ((per, False), (pool, True)):
        check("curves pooled=%d" % pooled, curve_triples(res.curves),
              np.moveaxis(sr.curve_summary(kind_tables, S, 0.2, pooled), 2, -1))
        assert res.names == param_names
        cols = [head.index(p) for p in param_names]
        check("parameters pooled=%d" % pooled, col_triples(res.params), sr.col_summary(table, S, cols, 0.2, pooled))


def case_dd_engine(mb, md):
    from literate_amd.ddrate import LOG_HEAD, DDRateEngine
    ts, te, origin, present = _dd_data()
    eng = DDRateEngine(ts, te, origin, present, 16, m_birth=int(mb), m_death=int(md), seed=33, s_freq=5, n_trace_slots=300)
    _engine_case(eng, ("l_%s", "m_%s", "niche_%s", "nicheFrac_%s"), ["posterior", "likelihood", "prior"] + LOG_HEAD[6:14])


def case_trend_engine(cb, cd):
    from literate_amd.trendrate import LOG_HEAD, TrendRateEngine
    R = np.load(os.path.join(GOLDEN, "ratemaps.npz"))
    ts, te, origin, present = _dd_data()
    eng = TrendRateEngine(ts, te, origin, present, R["TREND"], 16, const_birth=bool(int(cb)), const_death=bool(int(cd)),
                          seed=35, s_freq=5, n_trace_slots=300)
    _engine_case(eng, ("l_%s", "m_%s"), ["posterior", "likelihood", "prior"] + LOG_HEAD[6:12])


# ---- 3. hand-built edges -----------------------------------------------------------------------------------------------
def _col(x, **kw):
    """one column, one chain -> (mean, lo, hi)"""
    from literate_amd import ops
    x = np.asarray(x, dtype=float)
    kw.setdefault("burnin", 0.0)
    res = ops.col_summary(x[:, None, None], len(x), [0], **kw)
    return col_triples(res)[0, 0]


def case_edges():
    import pytest
    from literate_amd import ops
    # n_in exactly 2: n = 2 -> round(1.9) = 2, the window is the whole column
    assert _col([3.0, 1.0]).tolist() == [2.0, 1.0, 3.0]
    # n = 30 -> round(28.5) = 28 (half to even): three windows
    x = np.random.default_rng(1).normal(0, 1, 30)
    check("n=30", _col(x), sr.triple(x))
    # ties in window width: n = 20, n_in = 19, [d0, d18] and [d1, d19] both 1 wide -> the first
    vals = np.random.default_rng(2).permutation(np.array([1.0] + [2.0] * 18 + [3.0]))
    t = _col(vals)
    assert t[1] == 1.0 and t[2] == 2.0
    check("ties", t, sr.triple(vals))
    # many equal minima, spread over the threads and the reduction tree: an arithmetic sequence of 5000 exact values
    seq = np.random.default_rng(3).permutation(np.arange(5000) * 0.25)
    t = _col(seq)
    assert t[1] == 0.0 and t[2] == (sr.n_in_of(5000) - 1) * 0.25
    check("equal widths", t, sr.triple(seq))
    # a constant column: its HPD is the value twice
    t = _col(np.full(50, 0.1))
    assert t[1] == 0.1 and t[2] == 0.1
    check("constant", t, sr.triple(np.full(50, 0.1)))
    # one NaN, of either sign bit (the sort leaves them at opposite ends): NaN three times; the next column is untouched
    for bad in (np.nan, np.copysign(np.nan, -1.0)):
        y = np.random.default_rng(4).normal(0, 1, 64)
        y[17] = bad
        rows = np.stack([y, np.arange(64.0)], axis=1)[:, None, :]
        res = col_triples(ops.col_summary(rows, 64, [0, 1], burnin=0.0))
        assert np.isnan(res[0, 0]).all()
        check("a NaN column and its neighbour", res[0], sr.col_summary(rows, 64, [0, 1], 0.0, True)[0])
    # infinities are values: window widths inf - inf = NaN behave as in the reference's scan (restated by sr.triple's loop)
    base = np.random.default_rng(8).normal(5, 1, 40)                    # n = 40, n_in = 38: three windows
    for name, x in (("two +inf", np.r_[base[:38], np.inf, np.inf]), ("39 +inf", np.r_[base[:1], np.full(39, np.inf)]),
                    ("39 -inf", np.r_[np.full(39, -np.inf), base[:1]]), ("38 -inf", np.r_[np.full(38, -np.inf), base[:2]]),
                    ("3 -inf", np.r_[np.full(3, -np.inf), base[:37]]), ("both signs", np.r_[-np.inf, base[:38], np.inf])):
        x = np.random.default_rng(9).permutation(x)
        with np.errstate(invalid="ignore"):
            one = sr.triple(x)
            check("infinities: " + name, _col(x), one)
            assert np.array_equal(sr.triples(x[:, None])[0], one, equal_nan=True), name
    # burn-in that leaves n_in < 2
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        _col([1.0, 2.0, 3.0], burnin=0.7)
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        ops.curve_summary(np.ones((20, 1, 12)), 20, 1, np.ones(4), 2, 2, burnin=0.95)
    ops.curve_summary(np.ones((20, 2, 12)), 20, 1, np.ones(4), 2, 2, burnin=0.95, pooled=True)       # 2 chains x 1 row
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        ops.curve_summary(np.ones((20, 2, 12)), 20, 1, np.ones(4), 2, 2, burnin=0.95, pooled=False)
    # unknown sampler, unknown DDRate model
    for sampler in (0, 3):
        with pytest.raises(ValueError, match="LR_ERR_MODEL"):
            ops.curve_summary(np.ones((20, 1, 12)), 20, sampler, np.ones(4), 2, 2)
    with pytest.raises(ValueError, match="LR_ERR_MODEL"):
        ops.curve_summary(np.ones((20, 1, 12)), 20, 1, np.ones(4), 3, 2)
    # pooled order = chain after chain, burn-in dropped from every chain: chains that differ
    rng = np.random.default_rng(5)
    S, C = 50, 3
    T = rng.normal(0, 1, (S, C, 4)) + np.array([0.0, 10.0, -5.0])[None, :, None]
    T[:10, 1] = 1e6                                        # burn-in rows of chain 1: dropped only if the order is right
    for pooled in (True, False):
        res = ops.col_summary(T, S, [0, 3], burnin=0.2, pooled=pooled)
        assert res.n == (40 * C if pooled else 40)
        check("pooled=%d order" % pooled, col_triples(res), sr.col_summary(T, S, [0, 3], 0.2, pooled))
    # constant curves: m_birth = 0, m_death = 0 -> niche and nicheFrac are the constant 1.0
    args = np.abs(rng.normal(1, 0.3, (40, 2, 8)))
    rows = np.concatenate([np.zeros((40, 2, 4)), args], axis=2)
    res = ops.curve_summary(rows, 40, 1, np.arange(1.0, 7.0), 0, 0, burnin=0.0, pooled=True)
    v = _np(res.values)[0]
    assert np.all(v[3:] == 1.0) and res.kinds[3:] == ("niche", "nicheFrac")
    l_max, m_max = args[:, :, 0].T.reshape(-1), args[:, :, 5].T.reshape(-1)
    for k, x in enumerate((l_max, m_max, l_max - m_max)):
        check("constant rates kind %d" % k, np.moveaxis(v[k], 0, -1), np.tile(sr.triple(x), (6, 1)))


# ---- 4. chunking ---------------------------------------------------------------------------------------------------------
def case_chunking():
    import pytest
    from literate_amd import _hip, ops
    _hip.require_gpu()                                   # torch opens the device before the size queries ask it
    lib = _hip.load()
    rng = np.random.default_rng(6)
    S, C, nb = 120, 6, 17
    args = np.abs(rng.normal(1, 0.3, (S, C, 8)))
    args[..., 2] = rng.uniform(0, nb, (S, C))                       # x0
    args[..., 3:5] *= 40.0                                          # div_0, L
    rows = np.concatenate([rng.normal(0, 1, (S, C, 4)), args], axis=2)
    DT = rng.uniform(5, 60, nb)

    def bits(t):
        return _np(t).view(np.int64)

    for pooled in (True, False):
        def q(k):
            return lib.lr_curve_summary_workspace_bytes(S, C, 12, 4, 1, nb, 0.2, int(pooled), k)
        full, three, one = q(0), q(3), q(1)
        print("curve workspace pooled=%d: full %d, three bins %d, one bin %d bytes" % (pooled, full, three, one))
        assert full == q(nb) and full > three > one > 0
        ref = ops.curve_summary(rows, S, 1, DT, 2, 2, burnin=0.2, pooled=pooled, workspace_bytes=full)
        for cap in (three, one, full - 1, three + 1):
            got = ops.curve_summary(rows, S, 1, DT, 2, 2, burnin=0.2, pooled=pooled, workspace_bytes=cap)
            assert np.array_equal(bits(got.values), bits(ref.values)), cap
        with pytest.raises(ValueError, match="LR_ERR_WORKSPACE"):
            ops.curve_summary(rows, S, 1, DT, 2, 2, burnin=0.2, pooled=pooled, workspace_bytes=one - 1)
        b, d, ni, nf = [_np(x).reshape(S, C, nb) for x in ops.dd_rates(args.reshape(-1, 8), DT, 2, 2)]
        check("chunked curves pooled=%d" % pooled, curve_triples(ref),
              np.moveaxis(sr.curve_summary([b, d, b - d, ni, nf], S, 0.2, pooled), 2, -1))
        cols = np.array([11, 0, 5, 5, 7, 1, 2, 9, 3, 10, 4], dtype=np.int32)      # 11 columns, one of them twice
        cp = cols.ctypes.data_as(_hip.c_vp)

        def qc(k):
            return lib.lr_col_summary_workspace_bytes(S, C, 12, cp, len(cols), 0.2, int(pooled), k)
        full, three, one = qc(0), qc(3), qc(1)
        print("column workspace pooled=%d: full %d, three columns %d, one column %d bytes" % (pooled, full, three, one))
        assert full > three > one > 0
        ref = ops.col_summary(rows, S, cols, burnin=0.2, pooled=pooled, workspace_bytes=full)
        for cap in (three, one):
            got = ops.col_summary(rows, S, cols, burnin=0.2, pooled=pooled, workspace_bytes=cap)
            for x, y in zip(got[:3], ref[:3]):
                assert np.array_equal(bits(x), bits(y)), cap
        with pytest.raises(ValueError, match="LR_ERR_WORKSPACE"):
            ops.col_summary(rows, S, cols, burnin=0.2, pooled=pooled, workspace_bytes=one - 1)
        check("chunked columns pooled=%d" % pooled, col_triples(ref), sr.col_summary(rows, S, cols, 0.2, pooled))
    # more columns than one gather launch takes (64)
    wide = rng.normal(3, 1, (40, 2, 150))                # (means away from 0: a relative bound on a mean that cancels is no bound)
    check("150 columns", col_triples(ops.col_summary(wide, 40, range(150), burnin=0.1, pooled=True)),
          sr.col_summary(wide, 40, range(150), 0.1, True))


# ---- 5. size -------------------------------------------------------------------------------------------------------------
def cfg5_rows(seed=7, S=1000, C=256, nb=128):
    """synthetic DDRate parameter rows at cfg5's shape: [S, C, 12] (4 leading columns, 8 parameters) and DT [nb]"""
    rng = np.random.default_rng(seed)
    args = np.empty((S, C, 8))
    args[..., 0] = rng.gamma(4.0, 0.05, (S, C))                     # l_max
    args[..., 1] = rng.normal(0.0, 0.3, (S, C))                     # k
    args[..., 2] = rng.uniform(0.0, nb, (S, C))                     # x0
    args[..., 3] = rng.gamma(4.0, 20.0, (S, C))                     # div_0
    args[..., 4] = rng.gamma(4.0, 60.0, (S, C))                     # L
    args[..., 5] = rng.gamma(4.0, 0.02, (S, C))                     # m_max
    args[..., 6:8] = np.abs(rng.normal(0.0, 1.0, (S, C, 2)))        # nuB, nuD
    rows = np.concatenate([rng.normal(0, 1, (S, C, 4)), args], axis=2)
    t = np.arange(nb)
    DT = 30.0 + 250.0 / (1.0 + np.exp(-(t - 50) / 10.0)) + rng.uniform(0, 5, nb)
    return rows, DT


def cfg5_restatement(rows, DT, bins, S, burnin, mb=2, md=2):
    """[1, 5, len(bins), 3]: the restatement on chosen bins of the curves lr_dd_rates gives for the kept rows, pooled"""
    from literate_amd import ops
    burn = int(burnin * S)
    A = np.ascontiguousarray(rows[burn:S, :, 4:12].transpose(1, 0, 2)).reshape(-1, 8)       # chain after chain
    cols = [[] for _ in range(4)]
    for a in range(0, len(A), 1 << 15):                  # (lr_dd_rates takes at most 65535 parameter vectors a launch)
        for k, x in enumerate(ops.dd_rates(A[a:a + (1 << 15)], DT, mb, md)):
            cols[k].append(_np(x[:, list(bins)]))
    b, d, ni, nf = [np.concatenate(c) for c in cols]
    return np.stack([sr.triples(x) for x in (b, d, b - d, ni, nf)])[None]


CFG5_BINS = [0, 18, 36, 54, 73, 91, 109, 127]


def case_cfg5():
    """256 chains x 1000 samples x 128 bins, pooled, workspace capped at 1 GiB: every kind on eight bins spread over the
    range, the first and the last among them"""
    import torch
    from literate_amd import _hip, ops
    S, C, nb = 1000, 256, 128
    rows, DT = cfg5_rows()
    full = _hip.load().lr_curve_summary_workspace_bytes(S, C, 12, 4, 1, nb, 0.2, 1, 0)
    print("full workspace %d bytes" % full)
    assert full > (1 << 30)
    dev_rows = torch.as_tensor(rows).cuda()
    res = ops.curve_summary(dev_rows, S, 1, DT, 2, 2, burnin=0.2, pooled=True, workspace_bytes=1 << 30)
    assert res.n == 204800 and tuple(res.values.shape) == (1, 5, 3, nb)
    got = curve_triples(res)[:, :, CFG5_BINS]
    check("cfg5 shape", got, cfg5_restatement(rows, DT, CFG5_BINS, S, 0.2))


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------
def check_cli_tables(stem, log_paths, per_bin, param_names, origin=None):
    """<stem>_summary.tsv / _summary_params.tsv against the restatement applied to the .log files of the same run:
    plotDD.py's procedure (combine_logs with the burn-in, then make_vec_dict) on the run's own logs."""
    from literate_amd import logs
    tabs = []
    for p in log_paths:
        head = open(p).readline().rstrip("\r\n").split("\t")
        tabs.append(np.loadtxt(p, skiprows=1, ndmin=2))
    table = np.stack(tabs, axis=1)                                   # [S, C, columns]
    S = table.shape[0]
    lines = open(stem + "_summary.tsv").read().splitlines()
    shead = lines[0].split("\t")
    tab = np.array([[float(x) for x in l.split("\t")] for l in lines[1:]])
    nb = tab.shape[0]
    assert (per_bin[0] % (nb - 1)) in head and (per_bin[0] % nb) not in head
    if origin is None:                                               # bin centres of unit bins on an integer origin
        origin = tab[0, 0] - .5
        assert origin == np.floor(origin)
    assert np.array_equal(tab[:, 0], origin + np.arange(nb) + .5)
    assert np.isnan(tab[0, 2:4]).all() and np.all(tab[:, 1] >= 0) and not np.isnan(tab[1:, 2:4]).any()
    kind_cols = {}
    for kind, h in zip(("birth", "death", "niche", "nicheFrac"), per_bin):
        kind_cols[kind] = table[:, :, head.index(h % 0):head.index(h % 0) + nb]
    kind_cols["net"] = kind_cols["birth"] - kind_cols["death"]
    seen = 4
    for kind in logs.SUMMARY_KIND_ORDER:
        if kind not in kind_cols:
            continue
        c = shead.index(logs.SUMMARY_KIND_HEAD[kind][0])
        assert shead[c:c + 3] == logs.SUMMARY_KIND_HEAD[kind]
        want = sr.curve_summary([kind_cols[kind]], S, 0.2, True)[0, 0].T          # [nb, 3]
        check("table " + kind, tab[:, c:c + 3], want)
        seen += 3
    assert seen == len(shead)
    plines = [l.split("\t") for l in open(stem + "_summary_params.tsv").read().splitlines()]
    assert plines[0] == logs.SUMMARY_PARAM_HEAD and [p[0] for p in plines[1:]] == param_names
    got = np.array([[float(x) for x in p[1:]] for p in plines[1:]])
    check("table parameters", got, sr.col_summary(table, S, [head.index(p) for p in param_names], 0.2, True)[0])
    return tab, S


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case", " ".join(sys.argv[1:]), "ok")
