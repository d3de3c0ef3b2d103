"""Cases of the many-shift tests: chains whose rate and shift-time vectors reach past DPP row 0 (lanes 16..63 of the wave
that owns the chain, csrc/lr_chain.h), shared by tests/test_hip_many_shifts.py (the device against the oracle) and
tests/test_many_shifts_host.py (the oracle alone: that the inputs exercise what they claim).

Part A: records for the explicit-draw kernels (lr_rj_propose_score, lr_log_priors, lr_expand_rates, lr_binned_keiding),
exhaustive over K and the edited lane.  Part B: data sets, many-shift initial states and oracle trajectories of the
engine tests.  Everything is drawn from seeded generators: both modules see identical inputs."""
import functools

import numpy as np

from helpers import edges as E

# ------------------------------------------------------------------------------------------------------------------
# part A
# ------------------------------------------------------------------------------------------------------------------
SCORER_KMAX = (2, 16, 17, 33, 63)
MULT_MASKS = ("on", "off", "alternating", "last")
PRIOR_KMAX_FULL = (1, 16, 17, 33)
PRIOR_SHAPES = (2.0, 1.37)
PRIOR_POISSON = (None, 0.5, 3.0, 27.5, 200.0)
EXPAND_BINS = (1, 2, 127, 128, 129, 1000)
EXPAND_KMAX = 63
KEIDING_BINS = (1, 63, 64, 65, 256, 1000)


def _state(rng, K):
    """K pairwise distinct rates and K + 1 strictly increasing, pairwise distinct times."""
    rates = np.exp(rng.uniform(np.log(0.01), np.log(5.0), K))
    times = rng.uniform(-20.0, 20.0) + np.concatenate([[0.0], np.cumsum(rng.uniform(1.5, 4.0, K))])
    return rates, times


def _beta_u(rng, i):
    """Beta(10, 10), every seventh record near an end of (0, 1)."""
    if i % 7 == 3:
        return 0.02 + 1e-3 * rng.random()
    if i % 7 == 5:
        return 0.98 - 1e-3 * rng.random()
    return float(rng.beta(10.0, 10.0))


@functools.lru_cache(maxsize=None)
def add_records(kmax):
    """Every K in 1..kmax-1 x every interval ind in 0..K-1: dict(rates, times, K, ind, delta, u)."""
    rng = np.random.default_rng(1000 + kmax)
    out = []
    for K in range(1, kmax):
        for ind in range(K):
            rates, times = _state(rng, K)
            delta = rng.uniform(0.05, 0.95) * (times[ind + 1] - times[ind])
            out.append(dict(rates=rates, times=times, K=K, ind=ind, delta=float(delta), u=_beta_u(rng, len(out))))
    return out


@functools.lru_cache(maxsize=None)
def remove_records(kmax):
    """Every K in 2..kmax x every removed shift idx in 1..K-1: dict(rates, times, K, idx)."""
    rng = np.random.default_rng(2000 + kmax)
    out = []
    for K in range(2, kmax + 1):
        for idx in range(1, K):
            rates, times = _state(rng, K)
            out.append(dict(rates=rates, times=times, K=K, idx=idx))
    return out


@functools.lru_cache(maxsize=None)
def mult_records(kmax):
    """Every K in 1..kmax x the four update masks: dict(rates, times, K, ff, u, mask)."""
    rng = np.random.default_rng(3000 + kmax)
    out = []
    for K in range(1, kmax + 1):
        for mask in MULT_MASKS:
            rates, times = _state(rng, K)
            ff = {"on": np.ones(K, int), "off": np.zeros(K, int), "alternating": np.arange(K) % 2,
                  "last": (np.arange(K) == K - 1).astype(int)}[mask]
            out.append(dict(rates=rates, times=times, K=K, ff=ff, u=rng.random(K), mask=mask))
    return out


def pack_scorer(recs, kmax, move):
    """The arguments of ops.rj_propose_score for `recs` (move 0 multiplier, 1 add, 2 remove), zero padded."""
    C = len(recs)
    rates = np.zeros((C, kmax)); times = np.zeros((C, kmax + 1)); K = np.zeros(C, np.int32)
    index = np.zeros(C, np.int32); draws = np.zeros((C, 2 * kmax))
    for i, r in enumerate(recs):
        k = K[i] = r["K"]
        rates[i, :k], times[i, :k + 1] = r["rates"], r["times"]
        if move == 1:
            index[i], draws[i, 0], draws[i, 1] = r["ind"], r["delta"], r["u"]
        elif move == 2:
            index[i] = r["idx"]
        else:
            draws[i, :k], draws[i, kmax:kmax + k] = r["ff"], r["u"]
    return rates, times, K, np.full(C, move, np.int32), index, draws


def check_state_invariants(recs):
    """What the delete-by-value reference needs: pairwise distinct rates and times, times strictly increasing."""
    for r in recs:
        assert len(r["rates"]) == r["K"] and len(r["times"]) == r["K"] + 1
        assert len(np.unique(r["rates"])) == r["K"] and np.all(r["rates"] > 0)
        assert np.all(np.diff(r["times"]) > 0) and len(np.unique(r["times"])) == r["K"] + 1


@functools.lru_cache(maxsize=None)
def prior_records():
    """(kmax, K) of the prior cases with rates log-uniform over 1e-3..1e2 and a Gamma rate per record: every K in
    1..63 at kmax 63, K = kmax at the smaller paddings.  Returns {kmax: dict(rates [C, kmax], K, b)}."""
    rng = np.random.default_rng(4000)
    out = {}
    for kmax, Ks in [(63, list(range(1, 64)))] + [(k, [k]) for k in PRIOR_KMAX_FULL]:
        Ks = [k for k in Ks for _ in range(3)]
        rates = np.ones((len(Ks), kmax))
        for i, k in enumerate(Ks):
            rates[i, :k] = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), k))
        out[kmax] = dict(rates=rates, K=np.array(Ks, np.int32), b=rng.uniform(0.3, 4.0, len(Ks)))
    return out


@functools.lru_cache(maxsize=None)
def expand_case(n_bins, mode, n_chains):
    """Shift times for lr_expand_rates: chain c has K = 1 + c % 63 rates (n_chains == 1: K = 63) on a window of
    n_bins bins whose ends lie on integers or (round mode) on x.5; the K - 1 interior shifts are sorted draws from the
    window, with pairs and triples moved into one bin (zero-width segments) and every fifth on an integer / every
    seventh on x.5 (round mode rounds half to even, upwards and downwards).  dict(rates, times, K, kmax, n_bins, mode)."""
    rng = np.random.default_rng(5000 + 10 * n_bins + mode + 7 * n_chains)
    kmax = EXPAND_KMAX
    rates = np.zeros((n_chains, kmax)); times = np.zeros((n_chains, kmax + 1)); Ks = np.zeros(n_chains, np.int32)
    for c in range(n_chains):
        K = kmax if n_chains == 1 else 1 + c % kmax
        t0i = int(rng.integers(-3, 20)) * 2                  # an even origin
        inner = np.sort(rng.uniform(0.0, float(n_bins), K - 1))
        for j in range(K - 1):
            if j % 5 == 1:
                inner[j] = np.floor(inner[j])
            elif j % 7 == 2:
                inner[j] = np.floor(inner[j]) + 0.5
        for j in range(2, K - 1, 9):                         # three shifts inside one bin
            inner[j - 2:j + 1] = np.floor(inner[j]) + np.array([0.1, 0.3, 0.45])
        for j in range(5, K - 1, 9):                         # two shifts inside one bin
            inner[j - 1:j + 1] = np.floor(inner[j]) + np.array([0.2, 0.25])
        t0, end = float(t0i), float(t0i + n_bins)
        if mode == 1 and c % 4 == 1:
            # the window's own ends on x.5 in round mode: t0i + .5 rounds down to the even t0i; the end rounds to
            # t0i + n_bins from either side when that is even
            t0 = t0i + 0.5
            if n_bins % 2 == 0:
                end += 0.5 if c % 8 == 1 else -0.5
        Ks[c] = K
        rates[c, :K] = np.exp(rng.uniform(np.log(0.01), np.log(5.0), K))
        times[c, :K + 1] = np.concatenate([[t0], np.clip(np.sort(t0i + inner), t0, end), [end]])
    return dict(rates=rates, times=times, K=Ks, kmax=kmax, n_bins=n_bins, mode=mode)


def expand_reference(case):
    """rates[get_rate_index(...)] of every chain (the oracle rounds; floor mode floors first, as runMCMC does), with the
    assertion that the oracle's index has n_bins entries."""
    from oracle import literate_oracle as lo
    out = np.zeros((len(case["K"]), case["n_bins"]))
    for c, K in enumerate(case["K"]):
        t = case["times"][c, :K + 1]
        assert np.all(np.diff(t) >= 0)
        ind = lo.get_rate_index(t if case["mode"] else np.floor(t), case["n_bins"])
        assert len(ind) == case["n_bins"], (c, K, len(ind))
        out[c] = case["rates"][c, :K][ind]
    return out


@functools.lru_cache(maxsize=None)
def keiding_case(n_bins):
    rng = np.random.default_rng(6000 + n_bins)
    C = 5
    return dict(birth=np.exp(rng.uniform(np.log(.02), np.log(.6), (C, n_bins))),
                death=np.exp(rng.uniform(np.log(.02), np.log(.6), (C, n_bins))),
                n_spec=rng.integers(0, 400, n_bins), n_exti=rng.integers(0, 400, n_bins),
                DT=rng.uniform(0.5, 900.0, n_bins))


# ------------------------------------------------------------------------------------------------------------------
# part B
# ------------------------------------------------------------------------------------------------------------------
N_IT, C, SEED, POISSON_HP = 400, 37, 9090, 200.0
START_K = ((31, 32), (24, 28), (17, 16))          # (KL, KM) of chain c: START_K[c % 3]
ORACLE_CHAINS = (0, 1, 2, 18, 34, 36)
RJ_ENGINES = ("launch", "packed", "persistent2", "persistent4", "spec", "auto")
# name -> (lineages, n_bins asked of synth.make_lineages, its seed, the window's bins, the table class H of models 0-2)
DATASETS = {"h72": (2000, 66, 5, None, 72), "h264": (3000, 200, 2, 193, 264), "h520": (3000, 310, 3, None, 520)}


def _grid(x):
    return np.round(x * 2.0 ** 32) / 2.0 ** 32


@functools.lru_cache(maxsize=None)
def lineages(name, general):
    """Synthetic lineages at unit resolution (integer births, deaths at .5); on general times births and deaths move
    inside their bins on the 2^-32 grid (the first births and the extant lineages stay, so the window does)."""
    from literate_amd import synth
    n, bins, seed, _, _ = DATASETS[name]
    ts, te, _ = synth.make_lineages(n, n_bins=bins, n_shifts=4, seed=seed)
    if general:
        rng = np.random.default_rng(seed + 77)
        keep_s, keep_e = ts == ts.min(), te >= te.max()
        ts = np.where(keep_s, ts, ts + _grid(rng.uniform(0.0, 0.45, len(ts))))
        te = np.where(keep_e, te, te + _grid(rng.uniform(0.0, 0.45, len(te))))
    assert np.all(te > ts)
    return ts, te


def window(name):
    ts, te = lineages(name, False)
    return float(ts.min()), float(te.max()), int(te.max()) - int(ts.min())


@functools.lru_cache(maxsize=None)
def initial_states(name):
    """(L, M, tL, tM) lists over the C chains: K rates within +-5 % of 0.3 / 0.1 and K - 1 shifts on a jittered grid -
    in distinct bins, more than MIN_ALLOWED_T apart, with fractional parts in (0.1, 0.45).  runMCMC indexes its INITIAL
    state by rounded shift times and every later one by floored times (LRF:225 against LRF:262), and the engines follow
    it; with fractions below .5 the two agree, so a chain's final state can be re-scored without knowing whether its
    shift times were ever re-indexed."""
    start, end, _ = window(name)
    L, M, tL, tM = [], [], [], []
    for c in range(C):
        rng = np.random.default_rng([SEED, c])
        kl, km = START_K[c % 3]
        for k, base, R, T in ((kl, 0.3, L, tL), (km, 0.1, M, tM)):
            step = (end - start) / k
            R.append(base * (1.0 + rng.uniform(-0.05, 0.05, k)))
            T.append(np.concatenate([[start], np.floor(start + step * np.arange(1, k)) + rng.uniform(0.1, 0.45, k - 1), [end]]))
    return L, M, tL, tM


def check_initial_states(name):
    from oracle import literate_oracle as lo
    L, M, tL, tM = initial_states(name)
    for c in range(C):
        assert (len(L[c]), len(M[c])) == START_K[c % 3]
        for R, T, base in ((L[c], tL[c], 0.3), (M[c], tM[c], 0.1)):
            assert len(T) == len(R) + 1 and np.all(np.abs(R / base - 1.0) <= 0.05)
            assert np.all(np.diff(T) > lo.MIN_ALLOWED_T) and len(np.unique(np.floor(T[1:-1]))) == len(R) - 1
            assert np.all(T[1:-1] != np.floor(T[1:-1])) and np.array_equal(np.round(T), np.floor(T))


def _recording_draws(seed, chain):
    from oracle import mcmc_oracle as mo

    class Recording(mo.PhiloxDraws):
        """The device's stream, keeping what the reversible-jump dispatcher drew: select[it] = (r0, r1),
        add[it] = (ind, K), remove[it] = (idx, K)."""

        def __init__(self, seed, chain):
            super().__init__(seed, chain)
            self.select, self.add, self.remove = {}, {}, {}

        def rj_select(self, it):
            r = super().rj_select(it)
            self.select[it] = r
            return r

        def rj_add(self, it, times):
            r = super().rj_add(it, times)
            self.add[it] = (int(r[0]), len(times) - 1)
            return r

        def rj_remove(self, it, K):
            r = super().rj_remove(it, K)
            self.remove[it] = (int(r), int(K))
            return r

    return Recording(seed, chain)


@functools.lru_cache(maxsize=None)
def stats_of(name, general, model):
    from oracle import literate_oracle as lo
    ts, te = lineages(name, general)
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    assert len(sp) == window(name)[2]
    stats = dict(sp=sp, ex=ex, br=br)
    if model == 3:
        stats["ex_dead"], stats["br_dead"] = lo.bin_events_dead(ts, te, te.max())
    return stats


@functools.lru_cache(maxsize=None)
def oracle_runs(name, general, model):
    """{chain: (run_mcmc result, the recording draw source)} of ORACLE_CHAINS from the many-shift initial states."""
    from oracle import mcmc_oracle as mo
    ts, te = lineages(name, general)
    stats = stats_of(name, general, model)
    L, M, tL, tM = initial_states(name)
    out = {}
    for c in ORACLE_CHAINS:
        draws = _recording_draws(SEED, c)
        with np.errstate(all="ignore"):
            ref = mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=model, Poisson_HP=POISSON_HP), draws, N_IT, 1,
                              init=(L[c], M[c], tL[c], tM[c]), k_max=32)
        out[c] = (ref, draws)
    return out


def coverage(name, general, model):
    """What the oracle-checked chains of one configuration went through, from the trace rows (s_freq = 1: row it holds
    the state after iteration it) and the recorded draws."""
    cov = dict(adds_from_16=0, removes_from_17=0, refused_at_cap=0, chains_crossing_down=0, adds_low_lane=0,
               removes_low_lane=0, finite=True, k_min=99, k_max=0, refused_chains=[])
    for c, (ref, draws) in oracle_runs(name, general, model).items():
        rows = np.array([r[:13] for r in ref["mcmc"]])
        cov["finite"] = cov["finite"] and bool(np.all(np.isfinite(rows[:, 1:4])))
        k0 = START_K[c % 3]
        K = np.vstack([[k0], rows[:, 6:8].astype(int)])              # K[it] = (KL, KM) before iteration it
        cov["k_min"], cov["k_max"] = min(cov["k_min"], K.min()), max(cov["k_max"], K.max())
        for side in (0, 1):
            k = K[:, side]
            seen_high = np.maximum.accumulate(k >= 17)
            if np.any(seen_high & (k <= 15)):
                cov["chains_crossing_down"] += 1
        refused = False
        for it, (r0, r1) in draws.select.items():
            side = 0 if r0 > 0.5 else 1
            before, after = K[it, side], K[it + 1, side]
            if r1 > 0.5 and before >= 32:
                assert it not in draws.add
                cov["refused_at_cap"] += 1
                refused = True
            if it in draws.add and after == before + 1:
                ind, k = draws.add[it]
                assert k == before
                cov["adds_from_16"] += k >= 16
                cov["adds_low_lane"] += (k >= 17 and ind + 1 <= 15)
            if it in draws.remove and after == before - 1:
                idx, k = draws.remove[it]
                assert k == before
                cov["removes_from_17"] += k >= 17
                cov["removes_low_lane"] += (k >= 17 and idx <= 15)
        if refused:
            cov["refused_chains"].append(c)
    return cov


def engine_cases():
    """(data set, general, model, engine) of the engine tests: model 0 on every family that runs the data set's class,
    unit and general times; model 3 on one family per table mode; model 2 on the four-chain kernel."""
    out = []
    for name in DATASETS:
        n_bins = window(name)[2]
        for general in (False, True):
            for engine in RJ_ENGINES:
                if E.engine_runs(engine, 0, 0, not general, n_bins):
                    out.append((name, general, 0, engine))
    out += [("h72", False, 3, "persistent4"), ("h72", True, 3, "packed"), ("h72", True, 3, "launch")]
    out += [("h264", False, 2, "persistent4"), ("h264", True, 2, "persistent4")]
    return out


def oracle_configs():
    """The (data set, general, model) the engine cases need oracle trajectories for."""
    return sorted(set(c[:3] for c in engine_cases()))
