"""The RJ sampler on per-chain binned statistics (include/literate_hip_rjbin.h, csrc/lr_rjbin.hip, literate_amd/replicates.py) on
the GPU, against the restatement of runMCMC: oracle.mcmc_oracle.run_mcmc on the chain's own replicate with PhiloxDraws(seed,
chain0 + c), k_max = 32.

   1. each chain on its own data: 3 replicates x 2 chains, every row of every chain;
   2. the settings matrix on the same shape;
   3. the bin edges 1, 2, 64, 65, 512 (513 refused), one chain, one replicate;
   4. the cap on the number of rates and its warning;
   5. a run cut into launches is the same run bit for bit, and slots outside the due range keep their sentinel;
   6. against ChainEngine, from lineages;
   7. exact-size guarded buffers, the error codes in the header's order, a busy side stream;
   8. the command line end to end.

The tolerance is rtol = atol = 1e-9 (what test_cfg3_synthetic_10k_lineages_256_chains holds the engines to); no row is skipped.
The seeds below were run through the oracle alone (check_oracle_rows: no nan in any row); none had to be changed for a
Metropolis decision at a tie.
"""
import ctypes as C
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import mcmc_oracle as mo          # noqa: E402

pytestmark = pytest.mark.gpu

KMAX, HEAD = 32, 13
W = HEAD + 2 * (2 * KMAX - 1)
T0 = 5


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def make_stats(R, n_bins, seed, dead=False):
    """R replicates of n_bins bins: lineage-time with a few br == 0 bins (no events there) and a few bins without events;
    start_time / end_time differ in their fractions between replicates (and stay more than 1 apart at one bin)"""
    rng = np.random.default_rng(seed)
    out = []
    for r in range(R):
        br = np.abs(15.0 + np.cumsum(rng.normal(size=n_bins) * 2.0)) + 0.5 + rng.random(n_bins)
        sp, ex = rng.poisson(0.3 * br).astype(float), rng.poisson(0.2 * br).astype(float)
        if n_bins >= 8:
            z = rng.choice(n_bins, size=3, replace=False)
            br[z[:2]], sp[z[:2]], ex[z[:2]] = 0.0, 0.0, 0.0
            sp[z[2]], ex[z[2]] = 0.0, 0.0
            e = rng.choice(n_bins, size=2, replace=False)
            sp[e[0]], ex[e[1]] = 0.0, 0.0
        st = dict(sp=sp, ex=ex, br=br)
        if dead:
            st["ex_dead"] = np.floor(ex * 0.8)
            st["br_dead"] = br * (0.55 + 0.1 * rng.random(n_bins))
        start = T0 + 0.05 + 0.11 * r + 0.3 * rng.random() * 0.1
        end = T0 + n_bins + 0.27 + 0.13 * r
        out.append((st, float(start), float(end)))
    return out


def settings(**kw):
    return mo.Settings(model_BDI=kw.get("model", 2), const_rates=kw.get("const_rates", 0), const_death_rate=kw.get("const_death_rate", 0),
                       use_rate_HP=kw.get("use_rate_HP", 1), Poisson_HP=kw.get("Poisson_prior", 0.0),
                       update_fraction=kw.get("update_fraction", 0.75))


def dev_settings(ops, **kw):
    return ops.RjbinSettings(kw.get("model", 2), kw.get("const_rates", 0), kw.get("const_death_rate", 0), kw.get("use_rate_HP", 1),
                             kw.get("Poisson_prior", 0.0), kw.get("update_fraction", 0.75))


def dev_data(ops, reps, cpr, dead=False):
    arr = lambda k: np.array([st[k] for st, _, _ in reps])
    return ops.RjbinData(arr("sp"), arr("ex"), arr("br"), [s for _, s, _ in reps], [e for _, _, e in reps], cpr,
                         arr("ex_dead") if dead else None, arr("br_dead") if dead else None)


class Overflow:
    """counts the add moves the oracle refuses at k_max (mo._rjmcmc's last return value)"""

    def __enter__(self):
        self.n, self.saved = 0, mo._rjmcmc

        def spy(*a, **k):
            res = self.saved(*a, **k)
            self.n += 1 if res[-1] else 0
            return res
        mo._rjmcmc = spy
        return self

    def __exit__(self, *exc):
        mo._rjmcmc = self.saved


@functools.lru_cache(maxsize=None)
def oracle_run(R, n_bins, data_seed, cpr, seed, chain0, n_it, s_freq, kw, init_kind=None):
    """the restatement's run of every chain, computed once per case -> (reps, [out per chain], overflows met)"""
    kw = dict(kw)
    reps = make_stats(R, n_bins, data_seed, dead=kw.get("model", 2) == 3)
    outs = []
    with Overflow() as ov:
        for c in range(R * cpr):
            st, start, end = reps[c // cpr]
            init = full_init(c, start, end, n_bins) if init_kind == "full" else None
            with np.errstate(all="ignore"):
                outs.append(mo.run_mcmc(st, start, end, settings(**kw), mo.PhiloxDraws(seed, chain0 + c), n_it, s_freq, init=init,
                                        k_max=KMAX))
    return reps, outs, ov.n


def full_init(c, start, end, n_bins):
    """K_l = K_m = LR_KMAX: 31 interior shifts, every segment longer than 1"""
    rng = np.random.default_rng(1000 + c)
    step = (n_bins - 2.0) / KMAX
    tL = np.concatenate([[start], T0 + 1.0 + step * np.arange(1, KMAX) + 0.3 * rng.random(KMAX - 1), [end]])
    tM = np.concatenate([[start], T0 + 1.0 + step * np.arange(1, KMAX) + 0.3 * rng.random(KMAX - 1), [end]])
    assert np.min(np.diff(tL)) > 1.0 and np.min(np.diff(tM)) > 1.0
    return 0.1 + 0.4 * rng.random(KMAX), 0.05 + 0.3 * rng.random(KMAX), tL, tM


def check_oracle_rows(outs):
    """on the CPU: the oracle alone runs the chosen seeds without nan rows"""
    for c, o in enumerate(outs):
        assert np.isfinite(np.array(o["mcmc"])).all(), "chain %d: the oracle's own rows hold nan / inf" % c
        assert all(np.isfinite(r).all() for r in o["sp"]) and all(np.isfinite(r).all() for r in o["ex"])


def want_rows(outs):
    """the oracle's rows in the trace layout [S, C, W] (NaN where a row holds nothing)"""
    S, Cn = len(outs[0]["mcmc"]), len(outs)
    want = np.full((S, Cn, W), np.nan)
    for c, o in enumerate(outs):
        for s in range(S):
            want[s, c, :HEAD] = o["mcmc"][s][:HEAD]
            for off, row, K in ((HEAD, o["sp"][s], int(o["mcmc"][s][6])), (HEAD + 2 * KMAX - 1, o["ex"][s], int(o["mcmc"][s][7]))):
                assert len(row) == 2 * K - 1
                want[s, c, off:off + K] = row[:K]
                want[s, c, off + KMAX:off + KMAX + K - 1] = row[K:]
    return want


def close(got, want, what):
    """every element of every row: NaN exactly where the oracle's layout has none, the rest to rtol = atol = 1e-9"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: the rows' lengths differ (NaN pattern)" % what
    fin = ~np.isnan(want)
    err = np.abs(got[fin] - want[fin]) / (1e-9 + 1e-9 * np.abs(want[fin]))
    worst = float(np.nanmax(err)) if err.size else 0.0
    print("%s: largest error %.3g of the tolerance over %d numbers" % (what, worst, err.size))
    if not (worst <= 1.0 and np.isfinite(got[fin]).all()):
        at = np.argwhere(~np.isclose(got, want, rtol=1e-9, atol=1e-9, equal_nan=True))[:3]
        raise AssertionError("%s: differs first at %s: %s against %s" % (what, at.tolist(), got[tuple(at[0])], want[tuple(at[0])]))


def device_run(reps, cpr, seed, chain0, n_it, s_freq, kw, init=None):
    from literate_amd import ops
    kw = dict(kw)
    data = dev_data(ops, reps, cpr, dead=kw.get("model", 2) == 3)
    st = dev_settings(ops, **kw)
    state = ops.rjbin_init(data, seed, st, chain0, init=init)
    rows = ops.rjbin_steps(data, state, 0, n_it, s_freq, seed, st, chain0)
    return rows.cpu().numpy(), state.cpu().numpy(), data.warnings()


def bits(ts):
    return [np.ascontiguousarray(t.cpu().numpy()).tobytes() for t in ts]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def test_1_each_chain_on_its_own_data():
    """R = 3 distinct replicates x 2 chains (C = 6: one full workgroup and one with two idle waves), 40 bins, 300 iterations,
    s_freq = 1: every row of every chain against the oracle on that chain's replicate"""
    reps, outs, _ = oracle_run(3, 40, 7, 2, 11, 0, 300, 1, ())
    check_oracle_rows(outs)
    assert len({r[0]["br"].tobytes() for r in reps}) == 3 and len({r[1] % 1 for r in reps}) == 3 and len({r[2] % 1 for r in reps}) == 3
    assert all((r[0]["br"] == 0).sum() >= 2 and ((r[0]["sp"] == 0) & (r[0]["br"] > 0)).any() for r in reps)
    got, _, warn = device_run(reps, 2, 11, 0, 300, 1, ())
    want = want_rows(outs)
    assert want.shape == (300, 6, W)
    close(got, want, "3 replicates x 2 chains")
    assert warn == 0
    assert len({got[-1, c, 2] for c in range(6)}) == 6, "six chains, six likelihoods"
    assert (got[:, :, 6:8].max(axis=0) > 1).any(), "some chain holds a rate shift at some time"


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
MATRIX = [dict(model=0), dict(model=1), dict(model=2), dict(model=3), dict(const_rates=1), dict(const_death_rate=1), dict(use_rate_HP=0),
          dict(Poisson_prior=2.5), dict(update_fraction=0.3)]


@pytest.mark.parametrize("kw", MATRIX, ids=["_".join("%s%s" % kv for kv in m.items()) for m in MATRIX])
def test_2_the_settings_matrix(kw):
    key = tuple(sorted(kw.items()))
    reps, outs, _ = oracle_run(3, 40, 7, 2, 23, 4, 200, 1, key)
    check_oracle_rows(outs)
    got, _, _ = device_run(reps, 2, 23, 4, 200, 1, key)
    close(got, want_rows(outs), str(kw))
    if kw.get("const_rates"):
        assert (got[:, :, 6:8] == 1).all()
    if kw.get("const_death_rate"):
        assert (got[:, :, 7] == 1).all()
    if kw.get("use_rate_HP") == 0:
        assert (got[:, :, 10:12] == 1).all()
    if kw.get("Poisson_prior"):
        assert (got[:, :, 12] == 2.5).all()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins,R,cpr", [(1, 5, 1), (2, 5, 1), (64, 5, 1), (65, 5, 1), (512, 5, 1), (40, 1, 1), (40, 1, 3)],
                         ids=["bins1", "bins2", "bins64", "bins65_lane_wrap", "bins512", "C1", "R1"])
def test_3_bin_edges(n_bins, R, cpr):
    n_it = 200 if n_bins < 512 else 120
    reps, outs, _ = oracle_run(R, n_bins, 30 + n_bins, cpr, 5, 0, n_it, 1, ())
    check_oracle_rows(outs)
    got, _, _ = device_run(reps, cpr, 5, 0, n_it, 1, ())
    close(got, want_rows(outs), "%d bins, R = %d, %d chains each" % (n_bins, R, cpr))
    if n_bins == 1:
        assert (got[:, :, 6:8] == 1).all(), "at one bin the guard on short segments rejects every shift"
        assert len(np.unique(got[:, 0, 4])) > 10, "the multiplier moves still run"


def test_3_513_bins_are_refused_and_nothing_is_touched():
    import torch
    from literate_amd import _hip, ops
    lib = _hip.load()
    reps = make_stats(2, 513, 3)
    data = dev_data(ops, reps, 1)
    state = torch.full((2, _hip.LR_RJBIN_STATE_W), 7.0, dtype=torch.float64, device="cuda")
    rows = torch.full((4, 2, W), 7.0, dtype=torch.float64, device="cuda")
    prob = ops.rjbin_problem(data, state, 1)
    assert _hip.launch_problem(lib.lr_rjbin_init, data.device, prob, None, None, None, None, None, None) == _hip.LR_ERR_SIZE
    assert _hip.launch_problem(lib.lr_rjbin_steps, data.device, prob, 0, 4, 1, _hip.ptr(rows), 4, 0) == _hip.LR_ERR_SIZE
    with pytest.raises(ValueError, match="lr_rjbin_init: LR_ERR_SIZE"):
        ops.rjbin_init(data, 1)
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool((rows == 7.0).all()) and data.warnings() == 0


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 4])
def test_4_the_cap_on_the_number_of_rates(seed):
    """K_l = K_m = LR_KMAX at 128 bins: the warning word has LR_WARN_KCAP set exactly when the oracle met an overflow"""
    from literate_amd import _hip
    reps, outs, overflows = oracle_run(2, 128, 9, 2, seed, 0, 200, 1, (), "full")
    check_oracle_rows(outs)
    inits = [full_init(c, reps[c // 2][1], reps[c // 2][2], 128) for c in range(4)]
    init = (np.array([i[0] for i in inits]), np.array([i[1] for i in inits]), np.array([i[2] for i in inits]),
            np.array([i[3] for i in inits]), np.full(4, KMAX), np.full(4, KMAX))
    got, _, warn = device_run(reps, 2, seed, 0, 200, 1, (), init=init)
    close(got, want_rows(outs), "from K = 32")
    assert got[0, :, 6:8].min() >= KMAX - 1
    print("overflows the oracle met: %d, warning word %d" % (overflows, warn))
    assert bool(warn & _hip.LR_WARN_KCAP) == (overflows > 0)
    # (both seeds meet the cap; the answer "not set" is test 1's, whose oracle runs meet no overflow and whose word stays 0)
    assert oracle_run(3, 40, 7, 2, 11, 0, 300, 1, ())[2] == 0


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def test_5_a_run_cut_into_launches_is_the_same_run():
    import torch
    from literate_amd import ops
    reps = make_stats(3, 40, 7)
    data = dev_data(ops, reps, 2)
    seed, s, n_it = 17, 7, 300
    cap, first = 47, 2                    # 43 rows are due: slots 2 .. 44; 0, 1, 45, 46 keep the sentinel
    one = torch.full((cap, 6, W), -7.0, dtype=torch.float64, device="cuda")
    st1 = ops.rjbin_init(data, seed)
    ops.rjbin_steps(data, st1, 0, n_it, s, seed, rows=one, slot0=first)
    cut = torch.full((cap, 6, W), -7.0, dtype=torch.float64, device="cuda")
    st2 = ops.rjbin_init(data, seed)
    it, slot = 0, first
    for n in (1, 6, 100, 193):
        ops.rjbin_steps(data, st2, it, n, s, seed, rows=cut, slot0=slot)
        slot += ops.rows_due(it, n, s)
        it += n
    assert it == n_it and slot == first + 43
    assert bits([one, st1]) == bits([cut, st2])
    host = one.cpu().numpy()
    assert (host[:first] == -7.0).all() and (host[first + 43:] == -7.0).all() and not (host[first:first + 43, :, :HEAD] == -7.0).any()
    assert host[first:first + 43, 0, 0].tolist() == [float(7 * i) for i in range(43)]
    # and the rows are the oracle's
    _, outs, _ = oracle_run(3, 40, 7, 2, seed, 0, n_it, s, ())
    close(host[first:first + 43], want_rows(outs), "s_freq 7")


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
def test_6_against_the_existing_engine_from_lineages():
    """all R = 4 replicates the same data set, 2 chains each: the trace heads are ChainEngine's chain for chain; with the
    death times of replicates 1 - 3 re-drawn, replicate 0's chains still match and the others do not"""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    from literate_amd.replicates import ReplicateEngine, Replicates
    seed, n_it = 29, 200
    ts, te, _ = synth.make_lineages(2000, n_bins=40, n_shifts=3, seed=2)
    eng = ChainEngine(ts, te, 8, seed=seed, s_freq=1, n_trace_slots=n_it)
    eng.init()
    eng.steps(n_it)
    want = eng.trace_rows()[:, :, :HEAD]
    eng.close()
    same = ReplicateEngine(Replicates.from_lineages([(ts, te)] * 4), 8, seed=seed, s_freq=1, n_trace_slots=n_it)
    assert [same.replicate_of(c) for c in range(8)] == [0, 0, 1, 1, 2, 2, 3, 3] and same.n_bins == eng.n_bins
    same.init()
    same.steps(n_it)
    got = same.trace_rows()[:, :, :HEAD]
    same.close()
    close(got, want, "four copies of one data set against ChainEngine")
    rng = np.random.default_rng(5)
    data = [(ts, te)]
    for r in range(3):
        te_r = te.copy()
        dead = te < te.max() - 1.0
        te_r[dead] = np.maximum(np.floor(ts[dead]), np.floor(te[dead]) + rng.integers(-2, 3, dead.sum())) + 0.5
        te_r = np.minimum(te_r, np.floor(te.max()) - 0.5)
        te_r[np.argmax(te)] = te.max()
        data.append((ts, te_r))
    other = ReplicateEngine(Replicates.from_lineages(data), 8, seed=seed, s_freq=1, n_trace_slots=n_it)
    other.init()
    other.steps(n_it)
    got = other.trace_rows()[:, :, :HEAD]
    other.close()
    close(got[:, :2], want[:, :2], "replicate 0 beside re-drawn replicates")
    for c in range(2, 8):
        assert not np.allclose(got[:, c, 1:4], want[:, c, 1:4], rtol=1e-6), "chain %d runs on other data" % c


# ---- 7 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins,R,cpr,model", [(1, 1, 1, 2), (65, 3, 2, 0), (512, 2, 3, 3)])
def test_7_the_buffer_contract_on_exact_size_guarded_buffers(n_bins, R, cpr, model):
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    reps = make_stats(R, n_bins, 5, dead=model == 3)
    st = ops.RjbinSettings(model=model)
    Cn = R * cpr

    def whole():
        data = dev_data(ops, reps, cpr, dead=model == 3)
        state = ops.rjbin_init(data, 9, st)
        first = ops.rjbin_steps(data, state, 0, 25, 3, 9, st)                           # rows_cap exactly the 9 rows written
        rows = ops.alloc_output((13, Cn, W), torch.float64, "cuda")
        ops.rjbin_steps(data, state, 25, 15, 3, 9, st, rows=rows)                       # iterations 27 .. 39: slots 0 .. 4
        ops.rjbin_steps(data, state, 40, 24, 3, 9, st, rows=rows, slot0=5)              # 42 .. 63: slots 5 .. 12, exactly to the end
        return first, rows, state

    out = contract(ops, torch, whole, label="rjbin bins %d" % n_bins)
    assert out[0].shape[0] == 9 and out[1][0, 0, 0] == 27 and out[1][-1, Cn - 1, 0] == 63 and out[1][5, 0, 0] == 42


def test_7_argument_errors_in_the_headers_order_leave_the_buffers_untouched():
    import torch
    from helpers.abi_cases import refuses
    from literate_amd import _hip, ops
    lib = _hip.load()
    reps, big = make_stats(2, 8, 5, dead=True), make_stats(2, 513, 5, dead=True)
    D = lambda r=reps, cpr=2, dead=True: dev_data(ops, r, cpr, dead=dead)
    S = ops.RjbinSettings
    for what, call, code in (
            ("513 bins", lambda: ops.rjbin_init(D(big), 1), "LR_ERR_SIZE"),
            ("513 bins before the model", lambda: ops.rjbin_init(D(big), 1, S(model=4)), "LR_ERR_SIZE"),
            ("model 4", lambda: ops.rjbin_init(D(), 1, S(model=4)), "LR_ERR_MODEL"),
            ("model -1", lambda: ops.rjbin_init(D(), 1, S(model=-1)), "LR_ERR_MODEL"),
            ("model 3 without the dead pair", lambda: ops.rjbin_init(D(dead=False), 1, S(model=3)), "LR_ERR_MODEL"),
            ("update_fraction 1.5", lambda: ops.rjbin_init(D(), 1, S(update_fraction=1.5)), "LR_ERR_MODEL"),
            ("update_fraction < 0", lambda: ops.rjbin_init(D(), 1, S(update_fraction=-0.1)), "LR_ERR_MODEL"),
            ("poisson_HP < 0", lambda: ops.rjbin_init(D(), 1, S(poisson_HP=-1.0)), "LR_ERR_MODEL")):
        refuses(ops, torch, call, code, label=what, entry="lr_rjbin_init")
    # the step arguments, and the order NULL < SIZE < MODEL < the step arguments: straight at the library, on buffers of a known fill
    data = D()
    state = ops.rjbin_init(data, 1)
    before = state.clone()
    rows = torch.full((9, 4, W), 7.0, dtype=torch.float64, device="cuda")
    bigd = D(big)

    def steps(d=data, st=state, s=S(), cap=10, rows_=rows, it0=0, n_it=10, sf=1, slot0=0, null=None, R=None, cpr=None):
        prob = ops.rjbin_problem(d, st, 1, s)
        if null:
            setattr(prob, null, None)
        if R is not None:
            prob.R = R
        if cpr is not None:
            prob.chains_per_rep = cpr
        return _hip.launch_problem(lib.lr_rjbin_steps, d.device, prob, it0, n_it, sf, _hip.ptr(rows_), cap, slot0)

    E = _hip
    assert steps(cap=9) == E.LR_ERR_SIZE and steps(cap=10, slot0=1) == E.LR_ERR_SIZE and steps(cap=-1) == E.LR_ERR_SIZE
    assert steps(s=S(model=4), cap=9) == E.LR_ERR_MODEL and steps(s=S(update_fraction=2.0), sf=0) == E.LR_ERR_MODEL
    assert steps(sf=0) == steps(it0=-1) == steps(n_it=-1) == steps(slot0=-1) == E.LR_ERR_SIZE
    assert steps(R=0) == steps(R=0, s=S(model=4)) == steps(cpr=0) == steps(R=2 ** 30, cpr=2) == E.LR_ERR_SIZE
    assert steps(R=2 ** 30, cpr=2, s=S(model=7)) == E.LR_ERR_SIZE
    # ... also without rows: NULL is the answer only where the step arguments are valid and a row is due
    assert steps(rows_=None, sf=0) == steps(rows_=None, it0=-1) == steps(rows_=None, n_it=-1) == E.LR_ERR_SIZE
    assert steps(rows_=None) == E.LR_ERR_NULL and steps(d=bigd, s=S(model=4)) == E.LR_ERR_SIZE
    for field in ("sp", "ex", "br", "start_time", "end_time", "state", "warn"):
        assert steps(d=bigd, s=S(model=4), null=field) == E.LR_ERR_NULL, field
    assert steps(s=S(model=3), null="ex_dead") == steps(s=S(model=3), null="br_dead") == E.LR_ERR_MODEL
    assert steps(s=S(model=2), null="ex_dead", cap=9, n_it=0) == 0, "the dead pair is required for model 3 only"
    assert lib.lr_rjbin_steps(None, 0, 10, 1, _hip.ptr(rows), 10, 0) == E.LR_ERR_NULL
    assert lib.lr_rjbin_init(None, None, None, None, None, None, None) == E.LR_ERR_NULL
    # some but not all of the six initial arrays
    prob = ops.rjbin_problem(data, state, 1)
    assert _hip.launch_problem(lib.lr_rjbin_init, data.device, prob, _hip.ptr(rows), None, None, None, None, None) == E.LR_ERR_NULL
    torch.cuda.synchronize()
    assert torch.equal(before, state) and bool((rows == 7.0).all()) and data.warnings() == 0
    for what, call in (("s_freq 0", lambda: ops.rjbin_steps(data, state, 0, 10, 0, 1)), ("it0 < 0", lambda: ops.rjbin_steps(data, state, -1, 10, 1, 1)),
                       ("n_iters < 0", lambda: ops.rjbin_steps(data, state, 0, -1, 1, 1))):
        with pytest.raises(ValueError, match="lr_rjbin_steps: LR_ERR_SIZE"):
            call()
    # where no row is due rows may be NULL; n_iters = 0 launches nothing
    assert steps(rows_=None, it0=1, n_it=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, state)
    assert steps(rows_=None, it0=1, n_it=2, sf=5) == 0 and steps(cap=9, it0=3, n_it=9) == 0
    torch.cuda.synchronize()
    assert not torch.equal(before, state) and rows[:, :, 0].unique().tolist() == [float(i) for i in range(3, 12)]


def test_7_the_stream_contract_on_a_busy_side_stream():
    """lr_rjbin_init and lr_rjbin_steps take the stream in their descriptor, so they are not among the functions
    helpers/stream_cases finds by their last parameter: the library handed to TorchRuntime here is a pair of adapters with the
    stream last, which put it into the descriptor and call the entry point.  8 bins, 2 replicates x 2 chains, 60 iterations in
    two launches; the statistics and the times are the inputs copied behind the delay."""
    import torch
    from helpers import stream_cases as S
    from literate_amd import _hip, ops
    lib = _hip.load()
    nb, R, cpr = 8, 2, 2

    def init(prob, stream):
        prob.stream = stream
        return lib.lr_rjbin_init(C.byref(prob), None, None, None, None, None, None)

    def steps(prob, it0, n, s, rows, cap, slot0, stream):
        prob.stream = stream
        return lib.lr_rjbin_steps(C.byref(prob), it0, n, s, rows, cap, slot0)
    adapters = types.SimpleNamespace(lr_rjbin_init=init, lr_rjbin_steps=steps)
    rt = S.TorchRuntime(library=(adapters, ["lr_rjbin_init", "lr_rjbin_steps"]))

    def make(seed):
        reps = make_stats(R, nb, 40 + seed)
        arr = lambda k: np.array([st[k] for st, _, _ in reps])
        return arr("sp"), arr("ex"), arr("br"), np.array([s for _, s, _ in reps]), np.array([e for _, _, e in reps])

    def call(sp, ex, br, start, end):
        data = ops.RjbinData(sp, ex, br, start, end, cpr)
        assert data.sp.data_ptr() == sp.data_ptr() and data.end_time.data_ptr() == end.data_ptr()          # used as they are: no copy
        state = ops.alloc_output((R * cpr, _hip.LR_RJBIN_STATE_W), torch.float64, "cuda")
        rows = ops.alloc_output((20, R * cpr, W), torch.float64, "cuda")
        prob = ops.rjbin_problem(data, state, 9)
        here = rt.current_stream_arg
        assert adapters.lr_rjbin_init(prob, here()) == 0
        assert adapters.lr_rjbin_steps(prob, 0, 25, 3, _hip.ptr(rows), 20, 0, here()) == 0          # rows of iterations 0 .. 24: slots 0 .. 8
        assert adapters.lr_rjbin_steps(prob, 25, 35, 3, _hip.ptr(rows), 20, 9, here()) == 0         # 27 .. 57: slots 9 .. 19
        return dict(state=state, rows=rows)
    a, b = [S.dev(torch, x) for x in make(0)], [S.dev(torch, x) for x in make(1)]
    bufs = [torch.empty_like(x) for x in a]
    want, table = S.ordered(rt, lambda: call(*bufs), a, b, bufs, "rjbin")
    assert table["lr_rjbin_init"]["calls"] == 1 and table["lr_rjbin_steps"]["calls"] == 2
    rows = np.frombuffer(want["rows"]).reshape(20, R * cpr, W)
    assert rows[-1, 0, 0] == 57.0 and rows[9, 3, 0] == 27.0


# ---- 8 ----------------------------------------------------------------------------------------------------------------------
def write_tsv(path, ts, te):
    with open(path, "w") as f:
        f.write("id\tts\tte\n")
        for i, (a, b) in enumerate(zip(ts, te)):
            f.write("%d\t%d\t%d\n" % (i, a, b))


def cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "LiteRateForward.py")] + args, cwd=cwd, env=env, capture_output=True,
                          text=True, timeout=600)


def test_8_the_command_line_end_to_end(tmp_path):
    import LiteRateForward as LRF
    from literate_amd import logs, ops, replicates
    from literate_amd.engine import split_trace_row
    rng = np.random.default_rng(8)
    ts = np.sort(rng.integers(1950, 1985, 200))
    ts[0], files = 1950, []
    for r in range(3):
        te = np.minimum(ts + rng.integers(0, 25, 200), 1990)
        te[-1] = 1990
        d = tmp_path / ("rep%d" % r)
        d.mkdir()
        files.append(str(d / ("bands_%d.tsv" % r)))
        write_tsv(files[-1], ts, te)
    flags = ["--chains", "6", "-n", "2000", "-s", "100", "-seed", "3", "--rtt", "0.2", "--ess", "0.2", "--combine", "0.2"]
    res = cli(["--replicates", str(tmp_path / "rep*" / "bands_*.tsv")] + flags, str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    # the same run through the engine
    args = LRF.build_parser().parse_args(["--replicates", "x"] + flags)
    reps = replicates.load_replicates(files, args, LRF.parse_data)
    eng = replicates.ReplicateEngine(reps, 6, model=0, seed=3, s_freq=100, n_trace_slots=20)
    eng.init()
    eng.steps(2000)
    trace = eng.trace_rows()
    assert trace.shape == (20, 6, W)
    head = "\t".join(logs.MCMC_HEAD + logs.ADEQUACY_HEAD) + "\n"
    for r, path in enumerate(files):
        for k in range(2):
            p = logs.log_paths(path, 0, "", k)[1]
            assert os.path.dirname(p["mcmc"]) == os.path.join(os.path.dirname(path), "literate_mcmc_logs")
            assert os.path.basename(p["mcmc"]) == "bands_%d_BD_c%d_mcmc.log" % (r, k)
            with open(p["mcmc"]) as f:
                lines = f.readlines()
            assert lines[0] == head and len(lines) == 21
            h, sp_row, ex_row = split_trace_row(trace[0, 2 * r + k])
            got = np.array([float(x) for x in lines[1].split("\t")[:HEAD]])
            np.testing.assert_allclose(got, h, rtol=1e-12)
            with open(p["sp_rates"]) as f:
                np.testing.assert_allclose([float(x) for x in f.readline().split("\t")], sp_row, rtol=1e-12)
            with open(p["ex_rates"]) as f:
                np.testing.assert_allclose([float(x) for x in f.readline().split("\t")], ex_row, rtol=1e-12)
        div = np.loadtxt(logs.log_paths(path, 0, "")[1]["div"], skiprows=1)
        assert np.array_equal(div[:, 0], reps.sp[r]) and np.array_equal(div[:, 2], reps.br[r])
    stem = os.path.join(os.path.dirname(files[0]), "literate_mcmc_logs", "replicates3")
    S, burn = 20, 4
    want = ops.rtt_summary(eng.trace[burn:S], S - burn, eng.start_time, eng.end_time, burnin=0.0, pooled=True)
    logs.write_rtt_tables(str(tmp_path / "want"), want.time, want.rates[0].cpu().numpy(), want.shift_freq[0].cpu().numpy(),
                          want.k_counts[0].cpu().numpy())
    for tail in ("_RTT.tsv", "_RTT_K.tsv"):
        with open(stem + tail) as f, open(str(tmp_path / "want") + tail) as g:
            assert f.read() == g.read(), tail
    with open(stem + "_ESS.tsv") as f:
        first = f.readline()
    assert first.startswith("#") and "between-imputation variance" in first
    assert os.path.exists(stem + "_ESS_chains.tsv")
    for kind in ("mcmc", "sp_rates", "ex_rates", "div"):
        assert os.path.exists("%s_COMBINED_%s.log" % (stem, kind)), kind
    with open(stem + "_COMBINED_mcmc.log") as f:
        assert len(f.readlines()) == 1 + 6 * 16
    tab = np.loadtxt(stem + "_div_replicates.tsv", skiprows=1)
    with np.errstate(all="ignore"):
        eb, ed = reps.sp / reps.br, reps.ex / reps.br
    np.testing.assert_array_equal(tab[:, 0], np.arange(reps.n_bins))
    for j, x in enumerate((eb, ed, reps.br)):
        np.testing.assert_allclose(tab[:, 1 + 3 * j], x.mean(axis=0), rtol=1e-15, equal_nan=True)
        np.testing.assert_allclose(tab[:, 2 + 3 * j], x.min(axis=0), rtol=1e-15, equal_nan=True)
        np.testing.assert_allclose(tab[:, 3 + 3 * j], x.max(axis=0), rtol=1e-15, equal_nan=True)
    eng.close()


def test_8_every_refused_flag_combination_exits_with_its_sentence(tmp_path):
    from literate_amd import replicates
    rng = np.random.default_rng(8)
    files = []
    for r in range(2):
        ts = np.sort(rng.integers(1950, 1985, 50))
        ts[0] = 1950
        te = np.minimum(ts + rng.integers(0, 25, 50), 1990 + (5 if r else 0))
        te[-1] = 1990 + (5 if r else 0)
        files.append(str(tmp_path / ("r%d.tsv" % r)))
        write_tsv(files[-1], ts, te)
    one = ["--replicates", files[0], "-n", "200", "-s", "100"]
    sentences = dict((n, why) for n, _, why in replicates.ONE_DATA_SET)
    for flag, want in ([("--%s" % n, sentences[n]) for n in ("ppc", "ppc_age", "ade", "ade_joint", "waic", "loo")]):
        res = cli(one + [flag, "0.2"], str(tmp_path))
        assert res.returncode != 0 and want in res.stderr, (flag, res.stderr[-500:])
    for extra, want in ((["--checkpoint", "ck"], "--checkpoint saves one engine's workspace"), (["--init_shifts", "2"], "--init_shifts spaces its shifts"),
                        (["-rm_first_bin", "1"], "-rm_first_bin 1 makes the reference's own sampler fail"),
                        (["-d", files[0]], "leave -d empty"), (["--chains", "3"], None)):
        res = cli((["--replicates", ",".join(files)] if want is None else one) + extra, str(tmp_path))
        assert res.returncode != 0, extra
        if want is not None:
            assert want in res.stderr, (extra, res.stderr[-500:])
    env = dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE="2")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "LiteRateForward.py")] + one, cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode != 0 and "runs on one GPU (WORLD_SIZE is 2)" in res.stderr
    # --chains 3 over two files, then two files whose windows differ: the second one is named
    res = cli(["--replicates", ",".join(files), "--chains", "3", "-n", "200", "-s", "100"], str(tmp_path))
    assert res.returncode != 0 and "must be a multiple of the 2 files" in res.stderr
    res = cli(["--replicates", ",".join(files), "--chains", "2", "-n", "200", "-s", "100"], str(tmp_path))
    assert res.returncode != 0 and "r1.tsv" in res.stderr and "differs from the first replicate's" in res.stderr
