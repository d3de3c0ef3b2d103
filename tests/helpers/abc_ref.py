"""Numpy restatement of include/literate_hip_abc.h, written from the header: the binomial draw on given uniforms, the
count-level simulation on oracle.philox, the distance, and - from literate_amd/abc.py's docstrings - the rounds of the ABC
driver.  The specification the device and the module are held to.

Everything is elementwise IEEE double arithmetic, every operation rounded on its own, so the functions work on arrays (one
entry per draw or simulation): a masked array operation gives each entry the bits a scalar loop would.  per_lineage() is the
scheme the binomials replace - one uniform per living lineage and step - for the statistical comparison."""
import math

import numpy as np

from oracle import philox as P

NPAR, MAX_LIVING, SEARCH_CAP, P_ABC = 6, 1 << 24, 200, 56
FLAG_OVERFLOW, FLAG_EXTINCT, FLAG_REFUSED = 1, 2, 4


def powi(w, m):
    """w^m by binary powering, elementwise: f = 1, b = w, e = m; while e > 0 { if (e & 1) f = f b; e >>= 1; if (e > 0) b = b b }"""
    f, b, e = np.ones_like(w), w.copy(), m.copy()
    while (e > 0).any():
        f = np.where((e & 1) == 1, f * b, f)
        e = e >> 1
        b = np.where(e > 0, b * b, b)
    return f


def chunk_len(n, q):
    """M = 16 / q >= n ? n : (int) (16 / q)"""
    ln = 16.0 / q
    return np.where(ln >= n, n, np.floor(np.minimum(ln, 2.0 ** 40)).astype(np.int64))


def binomial(n, p, draw):
    """Bin(n, p) elementwise; draw(c) -> the uniforms of chunk c, one per entry (only the entries that have a chunk c use
    theirs).  Returns (x, used), int64."""
    n, p = np.asarray(n, dtype=np.int64), np.asarray(p, dtype=np.float64)
    x_out, used = np.zeros(n.shape, dtype=np.int64), np.zeros(n.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        whole = (n > 0) & (p >= 1.0)
        act = (n > 0) & (p > 0.0) & (p < 1.0)
    x_out[whole] = n[whole]
    if not act.any():
        return x_out, used
    flip = act & (p > 0.5)
    q = np.where(act, np.where(flip, 1.0 - p, p), 0.5)
    w = 1.0 - q
    r = q / w
    M = chunk_len(np.maximum(n, 1), q)
    y = np.zeros(n.shape, dtype=np.int64)
    left = np.where(act, n, 0)
    c = 0
    while (left > 0).any():
        on = left > 0
        m = np.where(on, np.minimum(left, M), 1)
        f = powi(w, m)
        cap = np.minimum(m, SEARCH_CAP)
        u = np.asarray(draw(c), dtype=np.float64).copy()
        x = np.zeros(n.shape, dtype=np.int64)
        go = on & (u >= f) & (x < cap)
        while go.any():
            u = np.where(go, u - f, u)
            x = x + go
            xs = np.where(go, x, 1)
            f = np.where(go, f * (r * ((m - xs + 1).astype(np.float64) / xs.astype(np.float64))), f)
            go = go & (u >= f) & (x < cap)
        y += np.where(on, x, 0)
        used += on
        left = np.where(on, left - M, left)
        c += 1
    x_out[act] = np.where(flip, n - y, y)[act]
    return x_out, used


def binomial_given(n, p, u):
    """lr_abc_binomial: n [N], p [N], u [N, n_u] -> (x, used) int32"""
    n, p, u = np.asarray(n, dtype=np.int64), np.asarray(p, dtype=np.float64), np.asarray(u, dtype=np.float64)
    N, n_u = u.shape
    x, used = np.full(N, -1, dtype=np.int64), np.zeros(N, dtype=np.int64)
    ok = (n >= 0) & (n <= MAX_LIVING) & ~np.isnan(p)
    act = ok & (n > 0) & (p > 0.0) & (p < 1.0)
    q = np.where(act, np.where(p > 0.5, 1.0 - p, p), 0.5)
    M = chunk_len(np.maximum(n, 1), q)
    need = np.where(act, (n + M - 1) // M, 0)
    short = ok & (need > n_u)
    used[short] = need[short]
    run = ok & ~short
    if run.any():
        padded = np.concatenate([u, np.zeros((N, 1))], axis=1)
        bx, bu = binomial(np.where(run, n, 0), np.where(run, p, 0.0), lambda c: padded[:, min(c, n_u)])
        x[run], used[run] = bx[run], bu[run]
    return x.astype(np.int32), used.astype(np.int32)


def _max(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(b > a, b, a)


def _min(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(b < a, b, a)


def philox_draw(seed, ids, t, odd):
    """chunk c -> member a of Stream(seed, id).pair(t | (seed >> 32) << 32, P_ABC, 2 c + odd) for every id"""
    it = np.uint64(int(t) | ((int(seed) >> 32) & P.MASK) << 32)
    k0, k1 = np.uint64(int(seed) & P.MASK), np.asarray(ids, dtype=np.int64).astype(np.uint64) & np.uint64(P.MASK)
    return lambda c: P.uniform_a_np(it, P_ABC, 2 * c + odd, k0, k1)


def step_probabilities(theta, n, K, n0d, spb):
    """steps 1 and 2 and the probabilities of step 3 of the header: -> (K, pb, pd)"""
    l0, m0, Kmax, g, h = theta[:, 0], theta[:, 1], theta[:, 3], theta[:, 4], theta[:, 5]
    nd = n.astype(np.float64)
    with np.errstate(all="ignore"):
        grow = g * (nd / Kmax) + h
        room = 1.0 - K / Kmax
        K = _max(n0d, K + ((grow * room) * Kmax) / spb)
        x = ((l0 - m0) * nd) / K
        lt = _max(0.0, l0 - x) / spb
        mt = _max(0.0, m0 + x) / spb
        pb = _min(1.0, lt)
        pd = _min(1.0, lt + mt) - pb
    return K, pb, pd


def simulate(seed, ids, theta, n_start, n_bins, spb, max_living, obs, weight, per_lineage_rng=None):
    """lr_abc_simulate for every id -> (dist [N], flags int32 [N], counts int64 [N, 4, n_bins], k_end [N]).
    per_lineage_rng: a numpy Generator - then B and D are counted from one uniform per living lineage (u < lt spawns, lt <= u <
    lt + mt kills) instead of drawn as binomials on Philox: the scheme of the script, for the statistical comparison."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, NPAR)
    N = len(theta)
    ids = np.asarray(ids, dtype=np.int64).reshape(N)
    n0 = np.broadcast_to(np.asarray(n_start, dtype=np.int64), (N,)).copy()
    obs, weight = np.asarray(obs, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        refused = (n0 < 1) | (n0 > max_living) | ~(theta[:, 3] > 0.0) | (ids < 0) | (ids > 0xFFFFFFFF) | ~np.isfinite(theta).all(1)
    flags = np.where(refused, FLAG_REFUSED, 0).astype(np.int32)
    alive = ~refused
    n = np.where(alive, n0, 0)
    K = np.where(alive, theta[:, 2], 0.0)
    n0d, spbd = n0.astype(np.float64), float(spb)
    counts = np.zeros((N, 4, n_bins), dtype=np.int64)
    d = np.zeros((3, N))
    last = n_bins * spb - 1
    for b in range(n_bins):
        nB, nD, ls = [np.zeros(N, dtype=np.int64) for _ in range(3)]
        at_start = n.copy()
        for s in range(spb):
            if not alive.any():
                break
            t = b * spb + s
            Kn, pb, pd = step_probabilities(theta, n, K, n0d, spbd)
            K = np.where(alive, Kn, K)
            na = np.where(alive, n, 0)
            with np.errstate(all="ignore"):
                pc = pd / (1.0 - pb)
            if per_lineage_rng is None:
                B, _ = binomial(na, pb, philox_draw(seed, ids, t, 0))
                D, _ = binomial(np.where(pb < 1.0, na - B, 0), pc, philox_draw(seed, ids, t, 1))
            else:
                u = per_lineage_rng.random((N, max(int(na.max()), 1)))
                mine = np.arange(u.shape[1])[None, :] < na[:, None]
                B = (mine & (u < pb[:, None])).sum(1)
                D = (mine & (u >= pb[:, None]) & (u < (pb + pd)[:, None])).sum(1)
            nB, nD, ls = nB + B, nD + D, ls + na
            n = np.where(alive, n + B - D, n)
            over = alive & (n > max_living)
            gone = alive & ~over & (n == 0) & (t < last)
            flags[over] |= FLAG_OVERFLOW
            flags[gone] |= FLAG_EXTINCT
            alive = alive & ~over & ~gone
        whole = flags == 0
        for q, v in enumerate((nB, nD, at_start, ls)):
            counts[:, q, b] = np.where(whole, v, 0)
        with np.errstate(all="ignore"):
            time = ls.astype(np.float64) / spbd
            sim = (nB.astype(np.float64) / time, nD.astype(np.float64) / time, at_start.astype(np.float64))
            for k in range(3):
                if weight[k, b] != 0.0:
                    d[k] = np.where(whole, d[k] + weight[k, b] * np.abs(sim[k] - obs[k, b]), d[k])
    dist = np.where(flags != 0, np.inf, (d[0] + d[1]) + d[2])
    return dist, flags, counts, K


def simulate_one(seed, sim_id, theta, n_start, n_bins, spb, max_living, obs, weight):
    dist, flags, counts, K = simulate(seed, [sim_id], [theta], n_start, n_bins, spb, max_living, obs, weight)
    return float(dist[0]), int(flags[0]), counts[0], float(K[0])


def mean_relative_weights(obs, rows=(0, 1)):
    """weight = 1 / (obs x the number of counted entries) over the positive entries of the given rows, 0 elsewhere"""
    obs = np.asarray(obs, dtype=np.float64)
    counted = np.zeros(obs.shape, dtype=bool)
    counted[list(rows)] = np.isfinite(obs[list(rows)]) & (obs[list(rows)] > 0)
    with np.errstate(all="ignore"):
        return np.where(counted, 1.0 / (obs * counted.sum()), 0.0)


def statistics(counts, spb):
    """counts [4, n_bins] -> obs [3, n_bins]"""
    t = counts[3].astype(np.float64) / float(spb)
    return np.stack([counts[0] / t, counts[1] / t, counts[2].astype(np.float64)])


# ---- the rounds of the driver (literate_amd/abc.py) ---------------------------------------------------------------------------
def prior_transform(priors, u):
    th = np.empty_like(u)
    for d, (dist, a, b) in enumerate(priors):
        for i in range(len(u)):
            th[i, d] = a if dist == "fixed" else (a + (b - a) * u[i, d] if dist == "uniform"
                                                  else np.exp(np.log(a) + (np.log(b) - np.log(a)) * u[i, d]))
    return th


def log_prior_one(priors, th):
    lp = 0.0
    for d, (dist, a, b) in enumerate(priors):
        if dist == "uniform":
            lp -= math.log(b - a)
        elif dist == "loguniform":
            lp -= np.log(th[d]) + math.log(math.log(b / a))
    return lp


def keep_smallest(dist, n_keep, eps=np.inf):
    order = [i for i in np.argsort(dist, kind="stable") if np.isfinite(dist[i]) and dist[i] <= eps]
    return np.array(order[:n_keep], dtype=np.int64)


def log_weights(new, priors, old, old_w, var2, moved):
    """log w_i = log prior(theta_i) - log sum_j w_j N(theta_i | theta_j, diag var2) over the moved coordinates, normalised"""
    mv = np.nonzero(moved)[0]
    const = -0.5 * np.sum(np.log(2.0 * np.pi * var2[mv]))
    out = np.empty(len(new))
    for i in range(len(new)):
        d = new[i, mv][None, :] - old[:, mv]
        terms = np.log(old_w) - 0.5 * (d * d / var2[mv]).sum(1) + const
        top = terms.max()
        out[i] = log_prior_one(priors, new[i]) - (top + math.log(np.exp(terms - top).sum()))
    top = out.max()
    return out - (top + math.log(np.exp(out - top).sum()))


def run_rounds(simulate_fn, priors, n_sims, keep, rounds, seed):
    """-> dict(theta, weights, log_weights, dist, ids, eps [one per round run], kept [...], stopped)"""
    rng = np.random.Generator(np.random.Philox(int(seed)))
    free = np.array([p[0] != "fixed" for p in priors])
    n_keep = int(math.ceil(keep * n_sims))
    theta = prior_transform(priors, rng.random((n_sims, NPAR)))
    ids = np.arange(n_sims, dtype=np.int64)
    dist, flags = simulate_fn(theta, ids)
    sel = keep_smallest(dist, n_keep)
    assert len(sel)
    pt, pd, pi = theta[sel], dist[sel], ids[sel]
    pw = np.full(len(sel), 1.0 / len(sel))
    lw = np.log(pw)
    eps, kept, stopped = [float(pd[-1])], [len(sel)], None
    for r in range(1, rounds):
        mean = (pw[:, None] * pt).sum(0)
        var2 = 2.0 * (pw[:, None] * (pt - mean) ** 2).sum(0)
        moved = free & (var2 > 0.0)
        cw = np.cumsum(pw)
        anc = np.minimum(np.searchsorted(cw, rng.random(n_sims) * cw[-1], side="right"), len(pw) - 1)
        z = rng.standard_normal((n_sims, NPAR))
        theta = pt[anc] + np.where(moved, np.sqrt(var2), 0.0) * z
        inside = np.ones(n_sims, dtype=bool)
        for d, (kind, a, b) in enumerate(priors):
            if kind != "fixed":
                inside &= (theta[:, d] >= a) & (theta[:, d] <= b)
        at = np.nonzero(inside)[0]
        ids = r * np.int64(n_sims) + at
        dist, flags = simulate_fn(theta[at], ids)
        sel = keep_smallest(dist, n_keep, eps[-1])
        kept.append(len(sel))
        if len(sel) < 2:
            stopped = r
            break
        new = theta[at][sel]
        lw = log_weights(new, priors, pt, pw, var2, moved)
        pt, pd, pi, pw = new, dist[sel], ids[sel], np.exp(lw)
        eps.append(float(pd[-1]))
    return dict(theta=pt, weights=pw, log_weights=lw, dist=pd, ids=pi, eps=eps, kept=kept, stopped=stopped)
