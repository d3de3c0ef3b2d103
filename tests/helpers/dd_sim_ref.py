"""Numpy restatement of lr_simulate_dd_batch, written from its definition (include/literate_hip.h):

replicate r is lr_simulate_bd_batch's replicate - living lineages hold slot numbers, at step t every living slot draws
u = uniform_a(t, P_SIM, 0, key (seed + r) & MASK, slot); u < lt spawns a lineage, otherwise not (u < lt + mt) survives;
the newborns of a step take the next unused slot numbers - with the thresholds of step t recomputed from the count n_t
living at its start: (br, dr) = DDRate's rate map (DDRate.py:55-100, transcribed below with np.power) of params[r] at
x = x_bins[r, t // steps_per_bin] with float(n_t) in the place of DT[b]; lt = br / steps_per_bin, mt = dr / steps_per_bin.

It runs its own step loop on oracle.philox and shares no code with oracle/sim_oracle.py.  Besides the counts it returns
the smallest absolute distance between any draw and either threshold over the run: the device forms x ** nu as
exp(nu * lr_log x), so its thresholds differ from these in the last bits, and a comparison of the integer outputs is
meaningful only when no draw came that close to a threshold."""
import numpy as np

from oracle import philox as px

SMALL_NUMBER = 0.000000000000001      # DDRate.py:47


def dd_rates_at(par, x, d, m_birth, m_death):
    """(birth rate, death rate) of DDRate.py:71-100 for one bin: x its TIME_RANGE value, d what stands for DT"""
    l_max, k, x0, div_0, L, m_max, nuB, nuD = [np.float64(v) for v in par]
    x, d = np.float64(x), np.float64(d)

    def get_logistic(nu=1):                                              # DD:55-56
        return div_0 + L / ((1 + np.exp(-k * (x - x0))) ** (1 / nu))

    def get_const_K():                                                   # DD:58-59
        return np.float64(1.0) * (L + div_0)

    def floored(rate):                                                   # DD:63, 68
        return np.float64(SMALL_NUMBER) if rate <= 0 else rate

    with np.errstate(all="ignore"):
        if m_birth == 0:
            birth = np.float64(1.0) * l_max
        else:
            niche = get_const_K() if m_birth == 1 else get_logistic()
            niche_frac = d / niche
            birth = floored(l_max - l_max * np.power(niche_frac, nuB))   # DD:61-62, 81, 85
        if m_death <= 0:
            death = np.float64(1.0) * m_max
        else:
            niche = get_const_K() if m_death == 1 else get_logistic()
            niche_frac = d / niche
            death = floored(m_max + m_max * np.power(niche_frac, nuD))   # DD:66-67, 96, 100
    return birth, death


def simulate_one(par, x_bins, spb, n_start, seed, m_birth, m_death, capacity):
    """(counts [4, n_bins], totals [4], smallest |u - threshold|) of one replicate under `seed`"""
    nb = len(x_bins)
    counts, totals = np.zeros((4, nb), dtype=np.int64), np.zeros(4, dtype=np.int64)
    n0 = int(n_start)
    if n0 < 1 or n0 > capacity:
        totals[:] = (0, 0, 1, -1)
        return counts, totals, np.inf
    alive = np.arange(n0, dtype=np.uint64)
    created, first_empty, closest = n0, -1, np.inf
    key = int(seed) & px.MASK
    for t in range(nb * spb):
        b = t // spb
        n = len(alive)
        if t % spb == 0:
            counts[2, b] = n
        if n == 0:
            if first_empty < 0:
                first_empty = t
            continue
        br, dr = dd_rates_at(par, x_bins[b], float(n), m_birth, m_death)
        lt, mt = br / np.float64(spb), dr / np.float64(spb)
        u = px.uniform_a_np(t, px.P_SIM, 0, key, alive)
        gap = np.concatenate([np.abs(u - lt), np.abs(u - (lt + mt))])
        gap = gap[np.isfinite(gap)]
        if len(gap):
            closest = min(closest, float(gap.min()))
        birth = u < lt
        keep = birth | ~(u < lt + mt)
        born = int(birth.sum())
        if created + born > capacity:
            totals[:] = (created, 0, 1, first_empty)
            return counts, totals, closest
        counts[0, b] += born
        counts[1, b] += n - int(keep.sum())
        counts[3, b] += n
        alive = np.concatenate([alive[keep], np.arange(created, created + born, dtype=np.uint64)])
        created += born
    totals[:] = (created, len(alive), 0, first_empty)
    return counts, totals, closest


def simulate(params, x_bins, spb, n_start, seed, m_birth=2, m_death=2, capacity=None):
    """lr_simulate_dd_batch's layout: (counts [n, 4, n_bins], totals [n, 4], closest [n]); replicate r runs under
    seed + r.  x_bins [n_bins] or [n, n_bins]; n_start an int or [n]; capacity defaults as ops.simulate_dd_batch's."""
    params = np.atleast_2d(np.asarray(params, dtype=np.float64))
    n = len(params)
    x = np.asarray(x_bins, dtype=np.float64)
    if x.ndim == 1:
        x = np.tile(x, (n, 1))
    n0 = np.full(n, n_start, dtype=np.int64) if np.ndim(n_start) == 0 else np.asarray(n_start, dtype=np.int64)
    cap = int(capacity) if capacity else max(64 * int(n0.max()), 1 << 20)
    out = [simulate_one(params[r], x[r], int(spb), n0[r], int(seed) + r, m_birth, m_death, cap) for r in range(n)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])
