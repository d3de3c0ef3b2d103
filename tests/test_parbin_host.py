"""The host side of the parametric samplers on replicate data sets (include/literate_hip_parbin.h,
literate_amd/replicates_par.py), no GPU: the header against the ctypes binding and the build; the argument errors;
load_binned_replicates through its binning seam (the oracle's create_bins); the restatement tests/helpers/parbin_ref.py pinned to
the oracles' rows exactly, and held to the tie condition in every case tests/test_hip_parbin.py uses; the pooled summary and the
<stem>_replicates.tsv table on an engine of known rows with numpy stand-ins for the kernels; the log names.
"""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

from helpers import parbin_ref as pr
from helpers import stream_cases as S
from helpers import summary_ref
from oracle import dd_mcmc_oracle as ddo
from oracle import literate_oracle as lo
from oracle import trend_mcmc_oracle as tro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ---- the header, the binding, the build ---------------------------------------------------------------------------------------
def test_the_header_the_binding_and_the_build_agree():
    from literate_amd import _hip, build, ops
    with open(os.path.join(ROOT, "include", "literate_hip_parbin.h")) as f:
        text = f.read()
    body = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = dict(re.findall(r"#define (LR_PARBIN_\w+) (\d+)", text))
    assert int(consts["LR_PARBIN_MAX_BINS"]) == _hip.LR_PARBIN_MAX_BINS == 512
    assert int(consts["LR_PARBIN_STATE_W"]) == _hip.LR_PARBIN_STATE_W == pr.STATE_W == 16
    assert {k: int(consts["LR_PARBIN_S_" + k.upper()]) for k in ops.PARBIN_STATE} == ops.PARBIN_STATE
    assert (pr.S_LIK, pr.S_PRIOR, pr.S_PROPOSED, pr.S_ACCEPTED) == tuple(ops.PARBIN_STATE[k] for k in ("lik", "prior", "proposed", "accepted"))
    assert pr.TRACE_W == _hip.LR_TRACE_W and ops.PARBIN_NPAR == pr.NPAR
    decl = {m.group(1): [" ".join(a.split()) for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(lr_parbin_\w+)\s*\(([^;{}]*?)\)\s*;", body, flags=re.S)}
    assert set(decl) == {"lr_parbin_init", "lr_parbin_steps"}
    kinds = {"const lr_parbin_problem*": C.POINTER(_hip.ParbinProblem), "int64_t": _hip.c_i64, "int32_t": _hip.c_i32, "double*": _hip.c_vp}
    for name, args in decl.items():
        res, got = _hip.SIGNATURES[name]
        assert res is _hip.c_i32 and got == [kinds[a.rsplit(" ", 1)[0]] for a in args], name
        assert "stream" not in args[-1], "the stream rides in the descriptor"
    struct = re.search(r"typedef struct lr_parbin_problem \{(.*?)\} lr_parbin_problem;", body, flags=re.S).group(1)
    fields = []
    for stmt in struct.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            typ, names = re.match(r"(.*?)\s+(\w+(?:\s*,\s*\w+)*)$", stmt).groups()
            fields += [(n.strip(), typ) for n in names.split(",")]
    want = {"int32_t": _hip.c_i32, "int64_t": _hip.c_i64, "uint64_t": C.c_uint64, "double": _hip.c_f64}
    assert [(n, want.get(t, _hip.c_vp)) for n, t in fields] == [(n, t) for n, t in _hip.ParbinProblem._fields_]
    assert fields[-1] == ("stream", "void*")
    assert "lr_parbin.hip" in build.SOURCES and "lr_par_iter.h" in build.HEADERS and any(h.endswith("literate_hip_parbin.h") for h in build.HEADERS)
    src = {}
    for name in ("lr_parbin.hip", "lr_mlik.hip", "lr_tmlik.hip", "lr_par_iter.h"):
        with open(os.path.join(ROOT, "literate_amd", "csrc", name)) as f:
            src[name] = f.read()
    # each sampler exists once: the acceptance rules stand in the shared header and nowhere else
    assert src["lr_par_iter.h"].count("> log_u") == 2
    for name in ("lr_parbin.hip", "lr_mlik.hip", "lr_tmlik.hip"):
        assert '#include "lr_par_iter.h"' in src[name] and "> log_u" not in src[name], name
    p = src["lr_parbin.hip"]
    assert "__syncthreads" not in p and "__shared__" not in p, "no barrier, no LDS"
    assert "atomic" not in p.replace("floating-point atomics", ""), "no atomics"
    # neither entry point has `void* stream` last: the counted set is what it was
    assert len(S.stream_entry_points()) == 38 and not any(n.startswith("lr_parbin") for n in S.stream_entry_points())


# ---- the arguments ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog", ["DDRate", "trend_rate"])
def test_arg_error_names_every_refused_flag(prog):
    from literate_amd import replicates, replicates_par as rp
    parser = __import__(prog).build_parser()
    ok = parser.parse_args(["--replicates", "x", "--chains", "4", "-m_birth", "1", "-rm_first_bin", "1"] if prog == "DDRate" else
                           ["--replicates", "x", "--chains", "4", "-rm_first_bin", "1", "-no_death", "1"])
    assert rp.arg_error(ok) is None and ok.replicates_name == ""
    names = [n for n, _, _ in rp.REFUSED]
    assert names == ["ppc", "ppc_age", "ade", "ade_joint", "waic", "loo", "mlik"] and rp.REFUSED[:6] == replicates.ONE_DATA_SET
    for name, off, why in rp.REFUSED:
        args = parser.parse_args(["--replicates", "x", "--%s" % name, "0.2"])
        assert getattr(args, name) != off and rp.arg_error(args) == why
        assert why.startswith("--%s " % name) and why.endswith("not with --replicates") and why.count(":") == 1
    assert "leave -d empty" in rp.arg_error(parser.parse_args(["--replicates", "x", "-d", "f.tsv"]))
    assert "runs on one GPU (WORLD_SIZE is 2)" in rp.arg_error(ok, world=2)
    assert "at least 1" in rp.arg_error(parser.parse_args(["--replicates", "x", "--chains", "0"]))
    assert rp.chains_per_replicate(6, 3) == 2 and rp.chains_per_replicate(3, 3) == 1
    for bad in ((4, 3), (2, 3), (0, 1)):
        with pytest.raises(ValueError, match="multiple of the %d files" % bad[1]):
            rp.chains_per_replicate(*bad)
    assert [rp.replicate_of(c, 2) for c in range(6)] == [0, 0, 1, 1, 2, 2] and rp.default_name(7) == "replicates7"


# ---- load_binned_replicates ---------------------------------------------------------------------------------------------------
def write_tsv(path, ts, te):
    with open(path, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, b) in enumerate(zip(ts, te)):
            f.write("%d\t%d\t%d\n" % (i, a, b))


@pytest.fixture
def cpu_binning(monkeypatch):
    """the GPU's create_bins replaced by the oracle's loops"""
    from literate_amd import replicates_par as rp
    monkeypatch.setattr(rp, "_bin", lo.create_bins)
    return rp


def files_of(tmp_path, ends=(1990, 1990, 1990), firsts=(1950, 1950, 1950)):
    rng = np.random.default_rng(4)
    files = []
    for r, (end, first) in enumerate(zip(ends, firsts)):
        ts = np.sort(rng.integers(first, first + 30, 40 + 5 * r))
        ts[0] = first
        te = np.minimum(ts + rng.integers(0, 20, ts.size), end)
        te[-1] = end
        files.append(str(tmp_path / ("rep_%d.tsv" % r)))
        write_tsv(files[-1], ts, te)
    return files


def cli_args(**kw):
    base = dict(TBP=False, first_year=-1, last_year=-1, death_jitter=.5, rm_first_bin=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_load_binned_replicates_by_the_clis_own_path(tmp_path, cpu_binning):
    rp = cpu_binning
    files = files_of(tmp_path, ends=(1990, 1992, 1990), firsts=(1950, 1952, 1950))          # 40 bins each, another window for the second
    reps = rp.load_binned_replicates(files, cli_args())
    assert (reps.R, reps.n_bins) == (3, 40) and reps.paths == files and reps.n_lineages.tolist() == [40, 45, 50]
    assert reps.origin.tolist() == [1950.0, 1952.0, 1950.0] and reps.present.tolist() == [1990.5, 1992.5, 1990.5]
    for r, path in enumerate(files):
        ts, te, present, origin = rp._parse(path, cli_args())
        o, p, ns, ne, dt, nb, _ = lo.create_bins(origin, present, np.asarray(ts, dtype=float), np.asarray(te, dtype=float), 0)
        np.testing.assert_array_equal(reps.n_spec[r], ns), np.testing.assert_array_equal(reps.n_exti[r], ne)
        np.testing.assert_array_equal(reps.DT[r], dt)
        eb, ed = reps.empirical(r)
        np.testing.assert_array_equal(eb, ns / dt), np.testing.assert_array_equal(ed, ne / dt)
    assert not np.array_equal(reps.DT[0], reps.DT[2])
    # -rm_first_bin 1 drops the bin and moves the origin
    cut = rp.load_binned_replicates(files, cli_args(rm_first_bin=1))
    assert cut.n_bins == 39 and cut.origin.tolist() == [1951.0, 1953.0, 1951.0] and cut.present.tolist() == reps.present.tolist()
    np.testing.assert_array_equal(cut.DT, reps.DT[:, 1:]), np.testing.assert_array_equal(cut.n_spec, reps.n_spec[:, 1:])
    # a covariate of the wrong length is refused
    with pytest.raises(ValueError, match="the trend has 41 entries, the replicates 40 time bins"):
        rp.load_binned_replicates(files, cli_args(), trend=np.ones(41))
    assert rp.load_binned_replicates(files, cli_args(), trend=np.ones(40)).trend.shape == (40,)


def test_a_differing_bin_count_is_refused_by_file_name(tmp_path, cpu_binning):
    rp = cpu_binning
    files = files_of(tmp_path, ends=(1990, 1990, 1993))
    with pytest.raises(ValueError) as e:
        rp.load_binned_replicates(files, cli_args())
    assert str(e.value).startswith(files[2] + ": 43 time bins, the first replicate (%s) has 40" % files[0])
    wide = files_of(tmp_path, ends=(2600,), firsts=(1950,))
    with pytest.raises(ValueError, match="650 time bins; the replicate sampler holds at most 512"):
        rp.load_binned_replicates(wide, cli_args())
    with pytest.raises(ValueError, match="no replicate given"):
        rp.load_binned_replicates([], cli_args())


# ---- the restatement ----------------------------------------------------------------------------------------------------------
MODELS = [(1, mb, md) for mb, md in pr.DD_MODELS] + [(2, cb, cd) for cb, cd in pr.TREND_MODELS]


@pytest.mark.parametrize("sampler,mb,md", MODELS, ids=["s%d_%d_%d" % m for m in MODELS])
def test_the_restatement_is_the_oracles_loop_exactly(sampler, mb, md):
    """two replicates x 2 chains, chain0 = 3: every row of chain c equals, bit for bit, what run_dd_mcmc / run_trend_mcmc returns
    on the statistics of replicate c // 2 with PhiloxDraws(seed, 3 + c) (the logged x0 + ORIGIN and L + div_0 formed here as the
    oracle forms them)"""
    D = pr.synthetic(2, 10, 31)
    n_it, s_freq, seed, chain0 = 120, 7, 91, 3
    rows, state, margin = pr.run(D, sampler, mb, md, 2, n_it, s_freq, seed, chain0)
    assert rows.shape == (18, 4, pr.TRACE_W) and margin > 0
    for c in range(4):
        r = c // 2
        if sampler == 1:
            want = ddo.run_dd_mcmc(D.n_spec[r], D.n_exti[r], D.DT[r], np.arange(10.0), D.origin[r], D.present[r], mb, md,
                                   ddo.PhiloxDraws(seed, chain0 + c), n_it, s_freq)
            want = np.array([w[:14] for w in want])
            got = rows[:, c, :12].copy()
            got[:, 6] += D.origin[r]
            got[:, 8] += got[:, 7]
            np.testing.assert_array_equal(got[:, 4:12], want[:, 6:14])
        else:
            want = tro.run_trend_mcmc(D.n_spec[r], D.n_exti[r], D.DT[r], D.trend, tro.PhiloxDraws(seed, chain0 + c), n_it, s_freq, bool(mb), bool(md))
            want = np.array([w[:12] for w in want])
            np.testing.assert_array_equal(rows[:, c, 4:10], want[:, 6:12])
        np.testing.assert_array_equal(rows[:, c, [0, 1, 2, 3]], want[:, [0, 1, 2, 5]])
        assert np.all(rows[:, c, 4 + pr.NPAR[sampler]:] == 0.0)
        assert state[c, pr.S_LIK] == rows[-1, c, 2] or n_it % s_freq != 1
        assert state[c, pr.S_PROPOSED:pr.S_PROPOSED + 2].sum() <= n_it and np.all(state[c, 14:] == 0.0)
    assert not np.array_equal(rows[:, 0], rows[:, 2]), "the replicates differ"


@pytest.mark.parametrize("case", pr.CASES, ids=[c[0] for c in pr.CASES])
def test_no_case_of_the_gpu_tests_stands_near_a_tie(case):
    """the tie condition: no acceptance margin of the restatement within 1e-6 of zero, so a device within 1e-9 decides alike"""
    D, rows, state, margin = pr.run_case(case)
    assert margin > pr.TIE, "%s: smallest margin %.3g" % (case[0], margin)
    assert np.isfinite(rows[..., :4]).all() and state[:, pr.S_ACCEPTED:pr.S_ACCEPTED + 2].sum(axis=1).min() >= 1


@pytest.mark.parametrize("sampler", [1, 2])
def test_the_lineage_cases_stand_near_no_tie(sampler):
    D, rows, state, margin = pr.run_lineage_case(sampler)
    assert (D.R, D.n_bins) == (2, 12) and margin > pr.TIE and not np.array_equal(D.n_exti[0], D.n_exti[1])
    np.testing.assert_array_equal(D.n_spec[0], D.n_spec[1])          # the births are shared, the deaths resampled


def test_the_closed_form_of_the_statistical_check():
    """under model (0, 0) the likelihood depends on l_max through N log l - l T alone, and the prior through -l / 10"""
    D = pr.synthetic(1, 12, 9)
    ch = pr.Chain(D, 0, 1, 0, 0)
    N, T = D.n_spec[0].sum(), D.DT[0].sum()
    a, b = ch.args + 0., ch.args + 0.
    a[0], b[0] = 0.1, 0.15
    np.testing.assert_allclose(ch.lik_of(b) - ch.lik_of(a), N * np.log(0.15 / 0.1) - 0.05 * T, rtol=1e-12)
    np.testing.assert_allclose(ch.prior_of(b) - ch.prior_of(a), -0.05 / 10, rtol=1e-9)
    assert pr.constant_rate_posterior_mean(N, T) == (N + 1) / (T + 0.1)


# ---- the pooled summary and the per-replicate table ---------------------------------------------------------------------------
class FakeOps:
    """numpy stand-ins for the three kernels pooled_summary and replicates_table call (tests/helpers/summary_ref.py, the
    oracle's rate maps); they return what literate_amd.ops returns, on the host"""
    CURVE_KINDS = {1: ("birth", "death", "net", "niche", "nicheFrac"), 2: ("birth", "death", "net")}

    def __init__(self):
        self.calls = []

    def col_summary(self, rows, n_samples, columns, burnin=0.2, pooled=True, workspace_bytes=None):
        self.calls.append(("col", tuple(rows.shape), pooled))
        out = summary_ref.col_summary(rows.numpy(), n_samples, columns, burnin, pooled)
        return types.SimpleNamespace(mean=out[:, :, 0], lo=out[:, :, 1], hi=out[:, :, 2])

    def dd_rates(self, args, DT, m_birth=2, m_death=2):
        import torch
        self.calls.append(("dd_rates", tuple(args.shape)))
        out = [np.array(x) for x in zip(*[lo.dd_rates(a, DT, np.arange(len(DT)).astype(float), m_birth, m_death) for a in args.numpy()])]
        return tuple(torch.as_tensor(x) for x in out)

    def curve_summary(self, rows, n_samples, sampler, aux, m_birth, m_death, arg_col=4, burnin=0.2, pooled=True, workspace_bytes=None):
        self.calls.append(("curve", tuple(rows.shape), pooled))
        R = rows.numpy()
        b, d = [np.array(x).reshape(R.shape[0], R.shape[1], -1) for x in
                zip(*[lo.trend_rates(a, aux, bool(m_birth), bool(m_death)) for a in R[..., arg_col:arg_col + 6].reshape(-1, 6)])]
        return types.SimpleNamespace(kinds=self.CURVE_KINDS[2], values=summary_ref.curve_summary([b, d, b - d], n_samples, burnin, pooled))


def fake_engine(sampler, S=40, R=3, cpr=2, nb=7):
    import torch
    from literate_amd import replicates_par as rp
    D = pr.synthetic(R, nb, 55)
    reps = rp.BinnedReplicates(["dir/rep_%d.tsv" % r for r in range(R)], D.n_spec, D.n_exti, D.DT, D.origin, D.present, trend=D.trend)
    g = np.random.default_rng(3)
    trace = np.zeros((S, R * cpr, pr.TRACE_W))
    trace[..., 0] = np.arange(S)[:, None]
    trace[..., 1:4] = g.normal(size=(S, R * cpr, 3))
    if sampler == 1:          # [l_max, k, x0, div_0, L, m_max, nuB, nuD] around the initial state, a level per replicate
        trace[..., 4:12] = np.array([0.5, 1.5, 3.0, 10.0, 200.0, 0.1, 1.0, 1.0]) * g.uniform(0.8, 1.2, (S, R * cpr, 8))
    else:
        trace[..., 4:10] = np.array([.1, .1, 0.3, -0.2, 1.0, 1.0]) * g.uniform(0.8, 1.2, (S, R * cpr, 6))
    trace[..., 4] += 0.05 * np.repeat(np.arange(R), cpr)
    eng = object.__new__(rp.ParametricReplicateEngine)
    eng.reps, eng.sampler, eng.chains_per_rep, eng.n_chains, eng.n_bins = reps, sampler, cpr, R * cpr, nb
    eng.m_birth, eng.m_death = (2, 1) if sampler == 1 else (0, 0)
    eng.trace = torch.as_tensor(trace)
    eng.chain_origin = torch.as_tensor(np.repeat(reps.origin, cpr))
    eng.samples_done = lambda: S
    return eng, D, trace


@pytest.mark.parametrize("sampler", [1, 2])
def test_the_pooled_summary_and_the_replicates_table_on_known_rows(sampler, monkeypatch, tmp_path):
    from literate_amd import replicates_par as rp
    eng, D, trace = fake_engine(sampler)
    fake = FakeOps()
    monkeypatch.setattr(rp, "_ops", lambda: fake)
    S, R, cpr, nb, burnin = 40, 3, 2, 7, 0.25
    kinds, values, names, params = rp.pooled_summary(eng, burnin)
    # the parameters: the log's values - x0 + ORIGIN of the chain's own replicate, L + div_0 - pooled over all chains
    table = trace[..., :12].copy() if sampler == 1 else trace.copy()
    if sampler == 1:
        table[..., 6] += np.repeat(D.origin, cpr)
        table[..., 8] += table[..., 7]
        assert names == ["posterior", "likelihood", "prior", "l_max", "steepness_k", "midpoint_x0", "initCarryingCap", "maxCarryingCap",
                         "m_max", "nuB", "nuD"]
    else:
        assert names == ["posterior", "likelihood", "prior", "l_min", "m_min", "alpha", "beta", "delta", "gamma"]
    cols = list(range(1, 1 + len(names)))
    np.testing.assert_array_equal(params, summary_ref.col_summary(table, S, cols, burnin, True)[0])
    # the curves: every row at the rates of its OWN replicate's DT (DDRate), the shared covariate (trend_rate)
    if sampler == 1:
        assert kinds == ("birth", "death", "net", "niche", "nicheFrac")
        tabs = [np.zeros((S, R * cpr, nb)) for _ in kinds]
        for s in range(S):
            for c in range(R * cpr):
                b, d, ni, nf = lo.dd_rates(trace[s, c, 4:12], D.DT[c // cpr], np.arange(nb).astype(float), 2, 1)
                for t, x in zip(tabs, (b, d, b - d, ni, nf)):
                    t[s, c] = x
        assert [c for c in fake.calls if c[0] == "dd_rates"] == [("dd_rates", (S * cpr, 8))] * R, "one launch per replicate's chain slice"
    else:
        assert kinds == ("birth", "death", "net")
        b, d = [np.array(x).reshape(S, R * cpr, nb) for x in zip(*[lo.trend_rates(a, D.trend, False, False) for a in trace[..., 4:10].reshape(-1, 6)])]
        tabs = [b, d, b - d]
        assert ("curve", (S, R * cpr, pr.TRACE_W), True) in fake.calls
    np.testing.assert_array_equal(values, summary_ref.curve_summary(tabs, S, burnin, True)[0])
    assert values.shape == (len(kinds), 3, nb) and all(c[2] for c in fake.calls if c[0] != "dd_rates"), "everything pooled"
    # the per-replicate table: each replicate's own chain slice, and the spread of the means
    names2, tri, sd = rp.replicates_table(eng, burnin)
    assert names2 == names and tri.shape == (R, len(names), 3)
    for r in range(R):
        np.testing.assert_array_equal(tri[r], summary_ref.col_summary(table[:, r * cpr:(r + 1) * cpr], S, cols, burnin, True)[0])
    np.testing.assert_allclose(sd, np.std(tri[:, :, 0], axis=0, ddof=1), rtol=1e-15)
    assert sd[3] > 0.03, "the level put on each replicate's first parameter shows between the replicates"
    # the files
    stem = str(tmp_path / "pooled")
    rp.write_pooled_summary(stem, eng.reps, kinds, values, names, params)
    rp.write_replicates_table(stem + "_replicates.tsv", eng.reps.paths, names2, tri, sd)
    with open(stem + "_summary.tsv") as f:
        lines = [ln.split("\t") for ln in f.read().splitlines()]
    assert lines[0][:4] == ["time", "net_diversity", "emp_birth", "emp_death"] and len(lines) == 1 + nb and len(lines[0]) == 4 + 3 * len(kinds)
    body = np.array([[float(x) for x in ln] for ln in lines[1:]])
    np.testing.assert_array_equal(body[:, 0], np.mean(D.origin) + np.arange(nb) + .5)
    np.testing.assert_array_equal(body[:, 1], D.DT.mean(axis=0))
    assert np.isnan(body[0, 2]) and np.isnan(body[0, 3])
    np.testing.assert_array_equal(body[1:, 2], (D.n_spec / D.DT).mean(axis=0)[1:])          # the empirical rates: means over replicates
    np.testing.assert_array_equal(body[1:, 3], (D.n_exti / D.DT).mean(axis=0)[1:])
    np.testing.assert_array_equal(body[:, 4:7], values[0].T)
    with open(stem + "_summary_params.tsv") as f:
        lines = f.read().splitlines()
    assert lines[0] == "parameter\tmean\tminHPD\tmaxHPD" and [ln.split("\t")[0] for ln in lines[1:]] == names
    with open(stem + "_replicates.tsv") as f:
        lines = [ln.split("\t") for ln in f.read().splitlines()]
    assert lines[0] == rp.REPLICATES_HEAD and len(lines) == 1 + R * len(names)
    assert lines[1 + len(names)][:3] == ["1", "rep_1.tsv", "posterior"]
    got = np.array([[float(x) for x in ln[3:]] for ln in lines[1:]]).reshape(R, len(names), 4)
    np.testing.assert_array_equal(got[:, :, :3], tri), np.testing.assert_array_equal(got[0, :, 3], sd)
    # one replicate: no spread to report
    one, _, _ = fake_engine(sampler, R=1)
    assert np.isnan(rp.replicates_table(one, burnin)[2]).all()


# ---- the logs -----------------------------------------------------------------------------------------------------------------
def test_the_per_replicate_log_names_and_heads():
    from literate_amd import replicates_par as rp
    suffix, tail, ptail = rp.log_names(1, 2, 2)
    assert (suffix, tail, ptail) == ("_LDDN_MDDN", ".log", "")
    assert rp.replicate_log_paths("a/b/bands_7.tsv", 8898, suffix, tail, 1) == ["a/b/bands_7_8898_LDDN_MDDN.log"]
    assert rp.replicate_log_paths("a/b/bands_7.tsv", 8898, suffix, tail, 2) == ["a/b/bands_7_8898_LDDN_MDDN_c0.log", "a/b/bands_7_8898_LDDN_MDDN_c1.log"]
    assert rp.log_names(1, 0, -1)[0] == "_LL_ML" and rp.log_names(1, 1, 1)[0] == "_LDD_MDD"
    suffix, tail, ptail = rp.log_names(2, 0, 1, no_death=True, trend_index=3)
    assert (suffix, tail, ptail) == ("_EXPB_ND", "_3.trendrate.log", "_3")
    assert rp.replicate_log_paths("x/r.tsv", 5, suffix, tail, 3)[2] == "x/r_5_EXPB_ND_c2_3.trendrate.log"
    assert rp.log_names(2, 1, 0)[0] == "_CONB_EXPD"
    # a replicate's log object carries its own statistics and writes the engines' head
    D = pr.synthetic(2, 5, 1)
    reps = rp.BinnedReplicates(["a", "b"], D.n_spec, D.n_exti, D.DT, D.origin, D.present, trend=D.trend)
    log = rp.ReplicateLog(1, reps, 1, 2, -1)
    assert log.origin == D.origin[1] and np.shares_memory(log.DT, reps.DT[1]) and (log.m_birth, log.m_death) == (2, -1)
    head = log.log_head()
    assert head[:6] == ["it", "posterior", "likelihood", "likelihood_birth", "likelihood_death", "prior"] and len(head) == 14 + 4 * 5 + 3
    tlog = rp.ReplicateLog(2, reps, 0, 1, 0)
    assert (tlog.const_birth, tlog.const_death) == (True, False) and tlog.trend is reps.trend and len(tlog.log_head()) == 12 + 2 * 5 + 3


def test_the_documents_name_the_feature():
    for path, words in (("README.md", ("DDRate.py --replicates", "trend_rate.py --replicates")),
                        ("DESIGN.md", ("lr_parbin", "lr_par_iter.h", "Parametric samplers on replicate data sets")),
                        ("INTEGRATION.md", ("literate_hip_parbin.h", "lr_parbin_init", "lr_parbin_steps")),
                        ("profiles/EXPERIMENTS.md", ("Parametric samplers on replicate data sets",))):
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for w in words:
            assert w in text, (path, w)
