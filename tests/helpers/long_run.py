"""Every sampler across iterations 2^31 and 2^32, and the Philox key across 2^32: TEST INFRASTRUCTURE shared by
tests/test_long_run_host.py (the references alone: margins, power, the host-side arithmetic) and tests/test_hip_long_run.py.

The draws are addressed by (seed, chain key, iteration, purpose, index) and "the state holds everything a launch starts
from", so a run is STARTED 24 iterations short of a boundary (OFFSETS) and taken 60 iterations on, in the launches of CUTS:
they end 4 short of the boundary, exactly on it, one past it, and run on.

The stepping samplers (lr_rjbin, lr_rjmc3, lr_tmlik, lr_mlik, lr_adej) take it0: their restatements loop over the true
iteration from their initial state.

The chain engines take no it0: N is written into (LR_I_IT_LO, LR_I_IT_HI) and (LR_I_NEXT_LO, LR_I_NEXT_HI) of the state that
lr_mcmc_init left, and lr_mcmc_restore follows (start_engine_at).  What such a run must be is read off the code, not off a
run:
  - lr_mcmc_init "prepares the proposal of iteration 0" (include/literate_hip.h): mode 1 of lr_chain_step_core / lr_dd_step_core
    (csrc/lr_step.h) stores it = 0 and proposes at address 0 - the move selectors, the multipliers, the RJ and Gibbs variates
    and the acceptance uniform, whose logarithm waits in LR_S_LOG_U;
  - a step decides the pending proposal, writes the row when it == next_sample, adds one to `it` and proposes at the new
    `it`; the four-chain kernel's draws ahead (csrc/lr_mcmc.hip, draw_duty) and the speculative kernel's (csrc/lr_spec.h,
    ctx.it0 + 1 ...) are made from the state's counter within the launch and carry nothing else over.
So iteration N consumes the proposal drawn at address 0 and every later iteration N + k draws at N + k: the reference is
the oracle loop over the local k = 0 .. 59 with its draws remapped by engine_map (0 -> 0, k -> N + k) and N added to the
iteration column (N is a multiple of s_freq, so the oracle's k % s_freq is the engine's condition).
  - One thing more rides on the counter under the parametric samplers: lr_dd_accept (csrc/lr_step.h) accepts "|| it == 0", as
    DDRate.py and trend_rate.py do.  At it = N the pending proposal of address 0 goes through the Metropolis rule like any
    other, where the oracle loops would accept their local iteration 0 whatever it is.  The oracle loops are therefore run one
    iteration longer with PendingFirst: their local iteration 0 proposes the state itself (accepted, changing nothing), local
    j >= 1 is the engine's iteration N + j - 1 on the draws of engine_map(j - 1), and the first row is dropped.
"""
import collections
import functools

import numpy as np

from helpers import chain_edges as CE
from helpers import edges as E

OFFSETS = (2 ** 31 - 24, 2 ** 32 - 24)          # both multiples of 8
CUTS = (20, 4, 1, 35)
N_IT = sum(CUTS)
MARGIN = 1e-6                                    # tests/test_hip_mc3.py's: no decision of a restatement closer to a tie
KMAX = 32
assert N_IT == 60 and all(n % 8 == 0 for n in OFFSETS)


def boundary(N):
    """the power of two the run started at N crosses"""
    b = 2 ** 31 if N < 2 ** 31 else 2 ** 32
    assert N < b <= N + N_IT
    return b


# ---- 32-bit words -----------------------------------------------------------------------------------------------------------
def as_i32(word):
    """the int32 with the bits of an unsigned 32-bit word"""
    word = int(word)
    assert 0 <= word < 2 ** 32
    return word - 2 ** 32 if word >= 2 ** 31 else word


def as_u32(i32):
    """the unsigned word with the bits of an int32"""
    i32 = int(i32)
    assert -2 ** 31 <= i32 < 2 ** 31
    return i32 & 0xFFFFFFFF


def split64(n):
    """(low, high) int32 lanes of a 64-bit counter, as the engines' integer state holds it"""
    n = int(n)
    assert 0 <= n < 2 ** 64
    return as_i32(n & 0xFFFFFFFF), as_i32(n >> 32)


def join64(lo, hi):
    return as_u32(lo) | (as_u32(hi) << 32)


# ---- what a broken counter would draw from: the faults the tests must notice ------------------------------------------------
def drop_high(it):
    """a counter that lost its high word"""
    return it & 0xFFFFFFFF


def sign_extend(it):
    """a counter whose low word went through a signed int on its way to 64 bits"""
    return (it | 0xFFFFFFFF00000000) if (it < 2 ** 32 and it & 0x80000000) else it


def fault_of(N):
    """the fault that shows at the boundary a run started at N crosses"""
    return sign_extend if boundary(N) == 2 ** 31 else drop_high


# ---- the draws shim ---------------------------------------------------------------------------------------------------------
ADDRESSED = frozenset(("move", "multiplier", "times_move", "rj_select", "rj_add", "rj_remove", "gibbs_poi", "gibbs_rate", "accept",
                       "slide", "normal", "normal_vec", "shape"))          # their first argument is the iteration
UNADDRESSED = frozenset(("init_rates", "init"))                            # drawn at the fixed address of the initial state


class RemappedDraws:
    """An oracle draws object (mcmc_oracle / dd_mcmc_oracle / trend_mcmc_oracle / adej_ref .PhiloxDraws) with the iteration
    argument of every draw method passed through f; a method it does not know is an AttributeError, not a guess."""

    def __init__(self, draws, f):
        self._draws, self._f = draws, f

    def __getattr__(self, name):
        if name.startswith("_") or name not in ADDRESSED | UNADDRESSED:
            raise AttributeError("RemappedDraws does not know the draw method %r" % name)
        method = getattr(self._draws, name)
        if name in UNADDRESSED:
            return method
        f = self._f
        return lambda it, *a, **kw: method(f(it), *a, **kw)


def engine_map(N):
    """local iteration k of a chain engine started at N -> the address it draws at (module docstring)"""
    return lambda k: 0 if k == 0 else N + k


def compose(outer, inner):
    return inner if outer is None else (lambda k: outer(inner(k)))


class PendingFirst:
    """The draws of a parametric oracle loop (kind "dd" / "trend") run one iteration longer: local iteration 0 proposes the
    state itself - the multiplier move with no parameter selected - and local j >= 1 draws at f(j - 1) (module docstring)."""

    def __init__(self, draws, kind, f):
        self._draws, self._kind, self._f = draws, kind, f

    def __getattr__(self, name):
        if name.startswith("_") or name not in ADDRESSED:
            raise AttributeError("PendingFirst does not know the draw method %r" % name)
        method = getattr(self._draws, name)
        f, kind = self._f, self._kind

        def draw(j, *a, **kw):
            if j > 0:
                return method(f(j - 1), *a, **kw)
            if name == "move":                                   # the multiplier branch: DD rr1 >= 0.1, trend rr >= .33
                return (0.0, 1.0) if kind == "dd" else 1.0
            if name == "multiplier":                             # no parameter selected: every factor is 1
                n = len(a[0])
                return np.zeros(n, dtype=int), np.full(n, 0.5)
            if name == "accept":
                return 0.5
            raise AssertionError("local iteration 0 draws %r" % name)
        return draw


# ---- the chain engines ------------------------------------------------------------------------------------------------------
N_CHAINS, ORACLE_CHAINS = 6, (0, 3, 5)          # a full quad and a half-empty one, three pairs
PIPELINED_CHAINS = 32                           # unit tables, cb 16: the launches' pipelined halves (lr_fused_iter_kernel)
FORCED = tuple(e for e in E.ENGINES if e not in ("auto", "persistent"))
PERSISTENT_FAMILIES = ("persistent4", "persistent2", "spec")
# (configuration, engine) pairs a forced engine does not run as that engine (E.engine_runs) and that are therefore no case:
# lr_persist_kernel has no general-time form
EXCLUDED = (("B", "persistent2"), ("F", "persistent2"))
EngineCase = collections.namedtuple("EngineCase", "config engine chains s_freq generic")


def runs(engine, name):
    """E.engine_runs for a configuration of CE.CONFIGS; the streaming kernel runs the launches' plan (lr_stream_eligible)"""
    cfg = CE.CONFIGS[name]
    return E.engine_runs("launch" if engine == "stream" else engine, cfg.model, cfg.sampler, not cfg.general, cfg.n_bins)


def engine_cases():
    out = []
    for name in "AB":
        out += [EngineCase(name, e, N_CHAINS, 1, False) for e in FORCED if runs(e, name)]
    out.append(EngineCase("A", "persistent4", N_CHAINS, 1, True))                # under LR_P4_GENERIC=1
    out += [EngineCase("C", e, N_CHAINS, 1, False) for e in ("launch", "persistent4")]
    for name in "EF":
        out += [EngineCase(name, e, N_CHAINS, 1, False) for e in ("launch",) + PERSISTENT_FAMILIES if runs(e, name)]
    out += [EngineCase("A", e, N_CHAINS, 8, False) for e in FORCED]              # a family each: rows at N, N + 8, ...
    out.append(EngineCase("A", "launch", PIPELINED_CHAINS, 1, False))
    return out


N_ENGINE_CASES = 28          # A 6, B 5, A generic 1, C 2, E 4, F 3, s_freq 8: 6, pipelined 1 - each at both offsets
KERNELS = ("lr_fused_iter_kernel", "lr_packscan_kernel", "lr_stream_kernel", "lr_persist_kernel", "lr_persist4_kernel",
           "lr_spec_kernel")


def engine_case_id(case):
    tag = case.engine + ("-generic" if case.generic else "") + ("-s%d" % case.s_freq if case.s_freq != 1 else "")
    return "%s-%s-%d" % (case.config, tag, case.chains)


def followed(case):
    return ORACLE_CHAINS if case.chains == N_CHAINS else (0, case.chains // 2, case.chains - 1)


def make_engine(case, chain_offset=0):
    from literate_amd.engine import ChainEngine
    cfg = CE.CONFIGS[case.config]
    slots = N_IT // case.s_freq + (1 if N_IT % case.s_freq else 0)
    if cfg.sampler == 0:
        ts, te = CE.data(case.config)
        return ChainEngine(ts, te, case.chains, model=cfg.model, seed=CE.SEED, s_freq=case.s_freq, n_trace_slots=slots,
                           engine=case.engine, chain_offset=chain_offset)
    ts, te, _, trend = CE.param_data(case.config)
    return E.param_engine(CE.KIND[cfg.sampler], ts, te, trend, case.chains, case.engine, CE.SEED, case.s_freq, slots, chain_offset)


def start_engine_at(eng, N):
    """eng.init(), then N into the iteration counter and the next sampled iteration of every chain (the low word as the
    int32 with the same bits; the slot stays 0), then lr_mcmc_restore: the header's rule for state written from outside."""
    from literate_amd import _hip
    eng.init()
    lo, hi = split64(N)
    sc = eng.state_i32[:, _hip.IROW_SCALARS]
    assert int(sc[:, _hip.I_SLOT].abs().max()) == 0 and int(sc[:, _hip.I_IT_LO].abs().max()) == 0
    for col, v in ((_hip.I_IT_LO, lo), (_hip.I_IT_HI, hi), (_hip.I_NEXT_LO, lo), (_hip.I_NEXT_HI, hi)):
        sc[:, col] = v
    _hip.check(_hip.launch(eng.lib.lr_mcmc_restore, eng.device, eng.handle), "lr_mcmc_restore")


@functools.lru_cache(maxsize=None)
def rj_engine_rows(name, key, N, s_freq, fault=None):
    """the oracle's sampled rows of the chain with Philox key `key` (taken modulo 2^32) of an RJ engine started at N"""
    from oracle import mcmc_oracle as mo
    cfg = CE.CONFIGS[name]
    ts, te = CE.data(name)
    draws = RemappedDraws(mo.PhiloxDraws(CE.SEED, key % 2 ** 32), compose(fault, engine_map(N)))
    with np.errstate(all="ignore"):
        rows = mo.run_mcmc(CE.rj_stats(name), ts.min(), te.max(), mo.Settings(model_BDI=cfg.model), draws, N_IT, s_freq, k_max=KMAX)["mcmc"]
    rows = [r.copy() for r in rows]
    for r in rows:
        r[0] += N
    return rows


@functools.lru_cache(maxsize=None)
def param_engine_rows(name, key, N, fault=None):
    """the oracle's log rows (s_freq 1) of the chain with Philox key `key` of a DDRate / trend_rate engine started at N"""
    from oracle import dd_mcmc_oracle as ddo
    from oracle import trend_mcmc_oracle as tro
    kind = CE.KIND[CE.CONFIGS[name].sampler]
    _, _, bins, trend = CE.param_data(name)
    o, p, nsp, nex, dt, t_range = bins
    emp, f = CE.param_emp(name), compose(fault, engine_map(N))
    with np.errstate(all="ignore"):
        if kind == "dd":
            draws = PendingFirst(ddo.PhiloxDraws(CE.SEED, key % 2 ** 32), kind, f)
            rows = ddo.run_dd_mcmc(nsp, nex, dt, t_range, o, p, 2, 2, draws, N_IT + 1, 1, emp=emp)
        else:
            draws = PendingFirst(tro.PhiloxDraws(CE.SEED, key % 2 ** 32), kind, f)
            rows = tro.run_trend_mcmc(nsp, nex, dt, trend, draws, N_IT + 1, 1, False, False, emp=emp)
    rows = [r.copy() for r in rows[1:]]
    for j, r in enumerate(rows):
        assert r[0] == j + 1
        r[0] = N + j
    return rows


def engine_rows(case, c, N, fault=None, chain_offset=0):
    if CE.CONFIGS[case.config].sampler == 0:
        return rj_engine_rows(case.config, chain_offset + c, N, case.s_freq, fault)
    assert case.s_freq == 1
    return param_engine_rows(case.config, chain_offset + c, N, fault)


# ---- the stepping samplers --------------------------------------------------------------------------------------------------
# lr_rjbin: (bins, model, s_freq): 2 replicates x 2 chains; 512 bins: 8 bins per lane; s_freq 8: the rows at N, N + 8, ...
RJBIN_CASES = {"bins40-m0": (40, 0, 1), "bins40-m2": (40, 2, 1), "bins512": (512, 2, 1), "bins40-s8": (40, 2, 8)}
RJBIN_SEED, RJBIN_CHAIN0, RJBIN_DATA_SEED = 11, 4, 7
# lr_rjmc3: (T, swap_every): NW = 4 and NW = 8; a swap round behind every iteration, every fifth and every third.  At
# swap_every 1 and 5 the first round's number (N + until_swap + 1) // swap_every is odd at both offsets; at 3 it is odd at
# 2^31 - 24 and even at 2^32 - 24, so that both start values of lr_rjmc3's `par` occur (asserted in the tests).
RJMC3_CASES = tuple((T, every) for T in (4, 5) for every in (1, 5, 3))
RJMC3_SEED, RJMC3_CHAIN0 = 23, 4


def first_round(N, every):
    """number of the first swap round of a launch at it0 = N: lr_rjmc3's until_swap and the round it reaches"""
    until_swap = every - 1 - N % every
    return (N + until_swap + 1) // every


def rjbin_reps(n_bins, model=2):
    from test_hip_replicates import make_stats
    return make_stats(2, n_bins, RJBIN_DATA_SEED, dead=model == 3)


@functools.lru_cache(maxsize=None)
def rjbin_reference(case, N, seed=RJBIN_SEED, chain0=RJBIN_CHAIN0, fault=None, per_rep=2):
    """the restatement of four chains (per_rep per replicate, keys chain0 + c modulo 2^32) started at it0 = N -> (the
    replicates in use, outs, the smallest margin of a decision)"""
    from helpers import rjmc3_ref as ref
    from test_hip_replicates import settings
    n_bins, model, s = RJBIN_CASES[case]
    reps = rjbin_reps(n_bins, model)[:4 // per_rep]
    outs = []
    for c in range(4):
        st, start, end = reps[c // per_rep]
        outs.append(ref.run_chain_from(st, start, end, settings(model=model), seed, (chain0 + c) % 2 ** 32, N, N_IT, s, KMAX, remap=fault))
    return reps, outs, min(o["margin"] for o in outs)


@functools.lru_cache(maxsize=None)
def rjmc3_reference(T, every, N, seed=RJMC3_SEED, chain0=RJMC3_CHAIN0, fault=None):
    """the restatement of 2 replicates x 1 ladder of T temperatures (40 bins, betas 1 / (1 + 0.5 j)) started at it0 = N; the
    keys chain0 + g T + w and the swap stream's key chain0 + g T are taken modulo 2^32 -> (reps, outs, smallest margin)"""
    from helpers import rjmc3_ref as ref
    from test_hip_replicates import settings
    reps = rjbin_reps(40)
    betas = ref.ladder_betas(T, 0.5)
    outs = [ref.run_ladder(reps[g][0], reps[g][1], reps[g][2], settings(), seed, chain0 + g * T, betas, every, N_IT, 1, k_max=KMAX,
                           it0=N, remap=fault) for g in range(2)]
    return reps, outs, min(o["margin"] for o in outs)


# the key wraps at 2^32: (uint32) (chain0 + c), (uint32) seed
WRAP_CHAIN0 = 2 ** 32 - 2


TMLIK = dict(bins=65, cols=3, data_seed=9, T=3, R=5, s=1, seed=21, col=(0, 1, 1, 2, 0), flags=(0, 1, 2, 3, 0))


def tmlik_problem():
    """the shape of tests/test_hip_tmlik.py's "cut into launches" case -> (problem, grid arguments, wins)"""
    import test_hip_tmlik as t
    c = TMLIK
    P = t.synthetic(c["bins"], c["cols"], c["data_seed"])
    betas, scales = t.ladder(c["T"])
    M = len(c["col"])
    key0 = [3 + m * c["R"] for m in range(M)]
    return P, (list(c["col"]), list(c["flags"]), key0, betas, scales, c["R"]), t.win_table(M, c["T"])


@functools.lru_cache(maxsize=None)
def tmlik_reference(N, fault=None):
    """tmlik_ref.run from it0 = N -> (rows [M, n, R, T, ROW_W], state [M, R, T, STATE_W], smallest margin)"""
    from helpers import tmlik_ref as ref
    P, (col, flags, key0, betas, scales, R), wins = tmlik_problem()
    M, T, s, seed = len(col), len(betas), TMLIK["s"], TMLIK["seed"]
    rows, state, margin = np.zeros((M, N_IT // s, R, T, ref.ROW_W)), np.zeros((M, R, T, ref.STATE_W)), np.inf
    for m in range(M):
        for r in range(R):
            for j in range(T):
                ch = ref.Chain(P, col[m], flags[m], betas[j], scales[j], wins[m, j], m)
                draws = ref.PhiloxDraws(seed, (key0[m] + r) * T + j)
                rows[m, :, r, j] = ref.run_chain(ch, draws if fault is None else RemappedDraws(draws, fault), N_IT, s, it0=N)
                state[m, r, j] = ch.state()
                margin = min(margin, ch.margin)
    return rows, state, margin


MLIK = dict(bins=65, data_seed=9, model=(2, 2), T=3, R=5, s=1, seed=21)


def mlik_problem():
    """the shape of tests/test_hip_mlik.py's "cut into launches" case -> (model, betas, scales)"""
    import test_hip_mlik as t
    M = t.synthetic(MLIK["bins"], MLIK["data_seed"], *MLIK["model"])
    return (M,) + tuple(t.ladder(MLIK["T"]))


@functools.lru_cache(maxsize=None)
def mlik_reference(N, fault=None):
    """mlik_ref.run from it0 = N -> (rows [n, R, T, ROW_W], state [R, T, STATE_W]); the restatement reports no margins"""
    from helpers import mlik_ref as ref
    M, betas, scales = mlik_problem()
    T, R, s, seed = len(betas), MLIK["R"], MLIK["s"], MLIK["seed"]
    rows, state = np.zeros((N_IT // s, R, T, ref.ROW_W)), np.zeros((R, T, ref.STATE_W))
    for r in range(R):
        for j in range(T):
            draws = ref.PhiloxDraws(seed, r * T + j)
            rows[:, r, j], ch = ref.run_chain(M, betas[j], scales[j], draws if fault is None else RemappedDraws(draws, fault), N_IT, s, it0=N)
            state[r, j] = ch.state()
    return rows, state


ADEJ = dict(table="a12", chains=130, compared=(0, 64, 129), s=1, seed=3)


@functools.lru_cache(maxsize=None)
def adej_reference(N, fault=None):
    """adej_ref.run of the compared chains from it0 = N -> ({chain: run dict}, smallest margin)"""
    from helpers import adej_cases as cases
    from helpers import adej_ref as ref
    data, st = ref.Data(*cases.table(ADEJ["table"])), ref.Settings()
    out = {}
    for c in ADEJ["compared"]:
        draws = ref.PhiloxDraws(ADEJ["seed"], c)
        out[c] = ref.run(data, 0.0, st, draws if fault is None else RemappedDraws(draws, fault), N_IT, ADEJ["s"], it0=N)
    return out, min(float(r["margin"].min()) for r in out.values())


def differs_from(N, it_col, rows, broken):
    """The power of a case: rows and broken are the same restatement on the true counter and on fault_of(N)'s - equal below
    the boundary, different in the last row and in more than half of the rows from the boundary on.  it_col: the rows'
    iterations; rows, broken: [rows, ...] arrays with that leading axis."""
    it_col, rows, broken = np.asarray(it_col), np.asarray(rows, dtype=float), np.asarray(broken, dtype=float)
    assert rows.shape == broken.shape and len(it_col) == len(rows)
    same = np.array([np.array_equal(a, b, equal_nan=True) for a, b in zip(rows, broken)])
    after = it_col >= boundary(N)
    assert same[~after].all(), "the fault shows below the boundary"
    assert after.sum() >= 4 and not same[-1] and (~same[after]).sum() * 2 > after.sum(), (int(after.sum()), same[after].tolist())
