"""Numpy restatement of the multi-trait extinction sampler (include/literate_hip_mte.h): the specification the device is held to
(tests/test_hip_mte.py) and that tests/test_mte_host.py checks without a GPU.

Chain c runs MTEmodel.py's loop (MTE:287-366) on the statistics of problem c // chains_per_problem with the draws of
oracle/philox.py's Stream(seed, chain0 + c), addressed as the header lists them: the grouped likelihood, the prior, the moves
with their thresholds, `>=` in the acceptance test, the unconditional acceptance of iteration 0 and of a Gibbs step, a NaN
likelihood counted as -inf.  Every accept decision's margin |lhs - log u| is recorded (iteration 0, Gibbs steps and non-finite
sides apart): where none is within TIE of zero, a device that agrees to 1e-9 takes the same decisions.

loglik_lineages is the likelihood as MTEmodel.py:336-354 computes it - a plain loop over the lineages - and the reference of
the grouped form here and on the device.

The cases of tests/test_hip_mte.py stand here too (CASES), so the host test can hold every one of them to the tie condition
without a GPU.
"""
import functools
import math
import os

import numpy as np

from oracle.philox import Stream

STATE_W, ROW_W = 176, 192
S_M, S_BETA, S_LIK, S_PRIOR, S_PROPOSED, S_ACCEPTED, S_I, S_SD, S_Y = 0, 1, 2, 3, 4, 7, 16, 32, 48
P_MOVE, P_YMASK, P_YNORM, P_ACCEPT, P_GIBBS_BETA, P_GIBBS_TAU, P_INIT_Y, P_INIT_HP = range(64, 72)
INIT_BETA_BASE = 1024
TIE = 1e-6
LGAMMA_1_5 = math.lgamma(1.5)
FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "mte_example.tsv")

# settings: (bvs, constant, bvs_from, pI)
BVS, NO_BVS, CONSTANT = (1, 0, 10, 0.05), (0, 0, 10, 0.05), (1, 1, 10, 0.05)


def thresholds(bvs, constant):
    """the selector's thresholds (MTE:287-300): below the first a Y move, the second the multiplier on m, the third a flip"""
    if constant:
        return 0.0, 1.0, 1.0
    return (0.45, 0.46, 0.91) if bvs else (0.90, 0.95, 0.95)


class Data:
    """code [G, T], n_states [T]; n, E, B [P, G]"""

    def __init__(self, code, n_states, n, E, B):
        self.code, self.n_states = np.asarray(code, dtype=np.int64), np.asarray(n_states, dtype=np.int64)
        self.n, self.E, self.B = [np.atleast_2d(np.asarray(x, dtype=float)) for x in (n, E, B)]
        self.G, self.T = self.code.shape
        self.P = self.n.shape[0]
        self.off = np.concatenate([[0], np.cumsum(self.n_states)]).astype(np.int64)
        self.n_cats = int(self.off[-1])

    def take(self, problems):
        p = list(problems)
        return Data(self.code, self.n_states, self.n[p], self.E[p], self.B[p])


# ---- the likelihood ------------------------------------------------------------------------------------------------------
def softmax_cats(Y, off):
    """softmax(Y_t) of every trait, concatenated; a trait's sum runs over its states in ascending order"""
    out = np.zeros(len(Y))
    for t in range(len(off) - 1):
        e = np.exp(Y[off[t]:off[t + 1]])
        s = 0.0
        for v in e:
            s += v
        out[off[t]:off[t + 1]] = e / s
    return out


def q_cats(Y, I, n_states, off):
    q = softmax_cats(np.asarray(Y, dtype=float), off)
    for t, S in enumerate(n_states):
        if not I[t]:
            q[off[t]:off[t + 1]] = 1.0 / S
    return q


def loglik_grouped(D, p, m, Y, I):
    """lik = E_tot log(m / Z) + sum_g E_g log w_g - (m / Z) sum_g B_g w_g, Z = sum_g n_g w_g / N (combinations with E_g = 0 leave
    the second sum alone)"""
    q = q_cats(Y, I, D.n_states, D.off)
    w = np.zeros(D.G)
    for t in range(D.T):
        w = w + q[D.off[t] + D.code[:, t]]
    n, E, B = D.n[p], D.E[p], D.B[p]
    with np.errstate(all="ignore"):
        r = m / (np.sum(n * w) / np.sum(n))
        lik = np.sum(E) * np.log(r) + np.sum(np.where(E != 0, E * np.log(w), 0.0)) - r * np.sum(B * w)
    return -np.inf if np.isnan(lik) else float(lik)


def loglik_lineages(bl, ex, tr, n_states, m, Y, I):
    """MTE:336-354, a plain loop over the lineages: rate_i = m s_i / mean(s), s_i = sum_t q_t[tr[i, t]]; sum_i ex_i log rate_i -
    bl_i rate_i.  -> (lik, the sum of the absolute terms)"""
    off = np.concatenate([[0], np.cumsum(n_states)]).astype(np.int64)
    q = q_cats(Y, I, n_states, off)
    s = [0.0] * len(bl)
    for i in range(len(bl)):
        for t in range(len(n_states)):
            s[i] += q[off[t] + tr[i, t]]
    total = 0.0
    for v in s:
        total += v
    lik, mag = 0.0, 0.0
    for i in range(len(bl)):
        rate = m * (s[i] / total * len(bl))
        a, b = (ex[i] * math.log(rate) if ex[i] else 0.0), bl[i] * rate
        lik += a - b
        mag += abs(a) + abs(b)
    return lik, mag


def log_prior(D, m, Y, I, sd, beta, pI):
    """MTE:347-356: Normal(0, sd_t) on every Y_t[s]; Gamma(1.5, rate beta) on 1 / sd_t^2; Gamma(1, rate 0.1) on beta; Gamma(1, rate
    1) on m; log(pI) sum I"""
    with np.errstate(all="ignore"):
        pY = 0.0
        for t in range(D.T):
            y = np.asarray(Y[D.off[t]:D.off[t + 1]], dtype=float)
            pY += np.sum(-0.5 * math.log(2.0 * math.pi) - np.log(sd[t]) - 0.5 * (y / sd[t]) ** 2)
        tau = 1.0 / np.asarray(sd, dtype=float) ** 2
        pT = np.sum(1.5 * np.log(beta) - LGAMMA_1_5 + 0.5 * np.log(tau) - beta * tau)
        return float(pY + pT + (math.log(0.1) - 0.1 * beta) - m + math.log(pI) * np.sum(I))


# ---- the chain -----------------------------------------------------------------------------------------------------------
class Chain:
    def __init__(self, D, p, settings, stream, given=None):
        self.D, self.p, self.u = D, p, stream
        self.bvs, self.constant, self.bvs_from, self.pI = settings
        self.th = thresholds(self.bvs, self.constant)
        T, off = D.T, D.off
        if given is None:
            self.m = float(np.sum(D.E[p]) / np.sum(D.B[p]))
            self.I = np.full(T, 0 if (self.bvs or self.constant) else 1, dtype=np.int64)
            self.Y = np.zeros(D.n_cats)
            for t in range(T):
                for k in range(off[t] + 1, off[t + 1]):          # state 0 stays 0
                    self.Y[k] = 0.1 * stream.normal(0, P_INIT_Y, k)
            self.sd = self.draw_sd(0, P_INIT_HP, 1.0)
            self.beta = self.draw_beta(0, P_INIT_HP, INIT_BETA_BASE)
        else:
            self.m, self.Y, self.I, self.sd, self.beta = given
            self.Y, self.I, self.sd = np.array(self.Y, dtype=float), np.array(self.I, dtype=np.int64), np.array(self.sd, dtype=float)
        self.lik = loglik_grouped(D, p, self.m, self.Y, self.I)
        self.prior = log_prior(D, self.m, self.Y, self.I, self.sd, self.beta, self.pI)
        self.proposed, self.accepted = [0, 0, 0], [0, 0, 0]
        self.margin = np.inf

    def draw_sd(self, it, purpose, rate0):
        D, sd = self.D, np.zeros(self.D.T)
        for t in range(D.T):
            a = 0.0
            for y in self.Y[D.off[t]:D.off[t + 1]]:
                a += y * y
            tau = self.u.gamma(it, purpose, 64 * t, 1.5 + 0.5 * D.n_states[t]) / (rate0 + 0.5 * a)
            sd[t] = 1.0 / math.sqrt(tau)
        return sd

    def draw_beta(self, it, purpose, base):
        return self.u.gamma(it, purpose, base, 1.0 + 1.5 * self.D.T) / (0.1 + float(np.sum(1.0 / self.sd ** 2)))

    def step(self, it):
        D, T = self.D, self.D.T
        ua, _ = self.u.pair(it, P_ACCEPT, 0)
        r, pick = self.u.pair(it, P_MOVE, 0)
        coin, um = self.u.pair(it, P_MOVE, 1)
        t = min(int(pick * T), T - 1)
        Y, I, m, hasting = self.Y.copy(), self.I.copy(), self.m, 0.0
        if r < self.th[0]:
            kind = 0
            for k in range(D.off[t] + 1, D.off[t + 1]):
                if self.u.pair(it, P_YMASK, k)[0] < 0.5:
                    Y[k] += 0.5 * self.u.normal(it, P_YNORM, k)
        elif r < self.th[1]:
            kind = 1
            hasting = 2.0 * math.log(1.1) * (um - .5)
            m = self.m * math.exp(hasting)
        elif r < self.th[2] and it >= self.bvs_from:
            kind = 2
            I[t] = 1 - I[t]
        else:
            kind = 3
            if coin > 0.5:
                self.beta = self.draw_beta(it, P_GIBBS_BETA, 0)
            else:
                self.sd = self.draw_sd(it, P_GIBBS_TAU, self.beta)
        prior = log_prior(D, m, Y, I, self.sd, self.beta, self.pI)
        lik = self.lik if kind == 3 else loglik_grouped(D, self.p, m, Y, I)
        with np.errstate(all="ignore"):
            lhs, log_u = (lik - self.lik) + (prior - self.prior) + hasting, (math.log(ua) if ua > 0 else -np.inf)
        ok = kind == 3 or it == 0 or bool(lhs >= log_u)
        if kind != 3 and it != 0 and np.isfinite(lhs) and np.isfinite(log_u):
            self.margin = min(self.margin, abs(lhs - log_u))
        if kind != 3:
            self.proposed[kind] += 1
        if ok:
            self.Y, self.I, self.m, self.lik, self.prior = Y, I, m, lik, prior
            if kind != 3:
                self.accepted[kind] += 1

    def state(self):
        D, s = self.D, np.zeros(STATE_W)
        s[S_M], s[S_BETA], s[S_LIK], s[S_PRIOR] = self.m, self.beta, self.lik, self.prior
        s[S_PROPOSED:S_PROPOSED + 3], s[S_ACCEPTED:S_ACCEPTED + 3] = self.proposed, self.accepted
        s[S_I:S_I + D.T], s[S_SD:S_SD + D.T], s[S_Y:S_Y + D.n_cats] = self.I, self.sd, self.Y
        return s

    def row(self, it):
        D, row = self.D, np.zeros(ROW_W)
        row[:5] = it, self.lik + self.prior, self.lik, self.prior, self.m
        o = 5
        row[o:o + D.T] = self.I
        row[o + D.T:o + D.T + D.n_cats] = softmax_cats(self.Y, D.off)          # whatever I is (MTE:392)
        row[o + D.T + D.n_cats:o + 2 * D.T + D.n_cats] = self.sd
        row[o + 2 * D.T + D.n_cats] = self.beta
        return row


def run(D, settings, cpp, n_iter, s_freq, seed, chain0=0):
    """every chain -> (rows [ceil(n_iter / s_freq), C, ROW_W], state [C, STATE_W], the smallest margin)"""
    C = D.P * cpp
    n = (n_iter + s_freq - 1) // s_freq
    rows, state, margin = np.zeros((n, C, ROW_W)), np.zeros((C, STATE_W)), np.inf
    for c in range(C):
        ch, k = Chain(D, c // cpp, settings, Stream(seed, chain0 + c)), 0
        for it in range(n_iter):
            ch.step(it)
            if it % s_freq == 0:
                rows[k, c] = ch.row(it)
                k += 1
        state[c], margin = ch.state(), min(margin, ch.margin)
    return rows, state, margin


# ---- data ----------------------------------------------------------------------------------------------------------------
def group(code, n_states, combo, bl, ex, keep):
    """n, E, B [P, G] of lineages with combination combo[i], P = len(keep) masks"""
    G = len(code)
    n = [np.bincount(combo[k], minlength=G) for k in keep]
    E = [np.bincount(combo[k], weights=ex[k], minlength=G) for k in keep]
    B = [np.bincount(combo[k], weights=bl[k], minlength=G) for k in keep]
    return Data(code, n_states, n, E, B)


@functools.lru_cache(maxsize=None)
def synthetic(P, G, n_states, seed, n_lin=None):
    """A random table of G combinations (rows need not differ) of traits with n_states states and n_lin lineages with exponential
    durations, extinct with probability 0.6; problem p keeps a random 70 % of them, and every problem but the first leaves the
    upper half of the combinations empty (n_g = 0) -> (Data, (combo, bl, ex, tr, keep)): grouped and per lineage"""
    g = np.random.default_rng(seed)
    n_states = np.asarray(n_states, dtype=np.int64)
    code = np.stack([g.integers(0, S, G) for S in n_states], axis=1)
    n_lin = n_lin or max(3 * G, 200)
    combo = g.integers(0, G, n_lin)
    bl = g.exponential(4.0, n_lin) + 0.01
    ex = (g.uniform(size=n_lin) < 0.6).astype(float)
    keep = []
    for p in range(P):
        k = g.uniform(size=n_lin) < 0.7
        if p > 0 and G > 1:
            k &= combo < (G + 1) // 2
        k[np.argmax(ex > 0)] = True          # (a problem holds an extinction)
        keep.append(k)
    return group(code, n_states, combo, bl, ex, keep), (combo, bl, ex, code[combo], keep)


def random_params(D, C, seed, I="mixed", m=None):
    """m [C], Y [C, n_cats], I [C, T] for C chains"""
    g = np.random.default_rng(seed)
    Y = g.normal(0.0, 1.0, (C, D.n_cats))
    ind = {"zeros": np.zeros((C, D.T), dtype=np.int64), "ones": np.ones((C, D.T), dtype=np.int64)}.get(I)
    if ind is None:
        ind = g.integers(0, 2, (C, D.T))
    mm = g.uniform(0.05, 0.5, C) if m is None else np.full(C, float(m))
    return mm, Y, ind


def read_example(path=FIXTURE):
    """the fixture -> (ts, te, traits [n, 6] int, the traits' names): the columns behind ts, te, the last one included, as the
    reference's default picks them (MTE:137-141)"""
    with open(path) as f:
        head = f.readline().split()
    tab = np.loadtxt(path, delimiter="\t", skiprows=1, usecols=range(1, len(head)))
    return tab[:, 0], tab[:, 1], tab[:, 2:].astype(np.int64), head[3:]


EXAMPLE_SLICES = [(np.inf, 0.0), (23.0, 8.0), (8.0, 0.0), (np.inf, 23.0)]          # whole, then three slices


# ---- the cases of tests/test_hip_mte.py ----------------------------------------------------------------------------------
G_EDGES = [1, 63, 64, 65, 128, 129, 1024]          # every instantiation (1, 2, 4, 16 combinations a lane; 8: G_MID8) and its edges
G_MID8 = 300
T1, T16 = (16,), (16,) * 7 + (2,) * 7 + (1,) * 2          # one trait; 16 traits mixing 1, 2 and 16 states: 128 categories
T3 = (3, 1, 5)
SHAPES = [(1, 1), (3, 5), (2, 3)]          # (P, chains_per_problem): five and three chains a problem straddle the four-wave blocks
MODES = [("bvs", BVS), ("nobvs", NO_BVS), ("const", CONSTANT)]
N_ITER = 300


def _cases():
    """(name, (P, G, n_states, data seed), settings, chains_per_problem, n_iter, s_freq, seed, chain0).
    Every G edge with T = 1 and T = 16, the factors (P, chains_per_problem), mode and s_freq cycling through them so that each
    value of each meets every instantiation's edge at least once over the table; then the full cross of the three factors at
    G = 65 with three mixed traits and at G = 300 (eight combinations a lane)."""
    out, i = [], 0
    for G in G_EDGES + [G_MID8]:
        for ns in (T1, T16):
            (P, cpp), (mname, st), sf = SHAPES[i % 3], MODES[(i + i // 3) % 3], (1, 7)[i % 2]
            out.append(("G%d_T%d_P%dx%d_%s_s%d" % (G, len(ns), P, cpp, mname, sf), (P, G, ns, 100 + i), st, cpp, N_ITER, sf, 9000 + i, i % 4))
            i += 1
    for (P, cpp) in SHAPES:
        for mname, st in MODES:
            for sf in (1, 7):
                out.append(("G65_T3_P%dx%d_%s_s%d" % (P, cpp, mname, sf), (P, 65, T3, 200 + i), st, cpp, N_ITER, sf, 9000 + i, 2))
                i += 1
    return out


CASES = _cases()
# the cut and independence tests of tests/test_hip_mte.py run on the device alone (bit for bit against itself); the tie condition
# does not bear on them


@functools.lru_cache(maxsize=None)
def run_case(case):
    """(data, rows, state, margin) of a case; computed once per process and shared - leave the arrays unchanged"""
    name, key, settings, cpp, n_iter, s_freq, seed, chain0 = case
    D = synthetic(*key)[0]
    return (D,) + run(D, settings, cpp, n_iter, s_freq, seed, chain0)


# ---- the laws of the statistical checks ----------------------------------------------------------------------------------
def constant_posterior(E_tot, B_tot):
    """With constant = 1 only m moves and every I_t = 0: w_g is the same for all g, Z = w, r_g = m, so the likelihood of m is
    m^E_tot exp(-m B_tot); the prior Gamma(1, rate 1) adds exp(-m), the other terms of the posterior do not involve m (the Gibbs
    steps move sd and beta_hp alone), and the multiplier move with its Hastings term leaves it invariant on m > 0.  Hence m | data ~
    Gamma(E_tot + 1, rate B_tot + 1) -> (mean, variance)"""
    a, b = E_tot + 1.0, B_tot + 1.0
    return a / b, a / b ** 2


def relation_lineages(n=3000, seed=5):
    """trait A: 3 states with extinction rates 0.05, 0.10, 0.20 (1 : 2 : 4); trait B: 3 states assigned at random; every lineage
    observed for at most 8 time units: bl = min(Exp(rate), 8), extinct where the death came first -> (ts, te, traits)"""
    g = np.random.default_rng(seed)
    A, Bt = g.integers(0, 3, n), g.integers(0, 3, n)
    life = g.exponential(1.0 / np.array([0.05, 0.10, 0.20])[A])
    ts = np.full(n, 8.0)
    te = np.where(life < 8.0, 8.0 - life, 0.0)
    return ts, te, np.stack([A, Bt], axis=1)
