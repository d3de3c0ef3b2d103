"""Numpy restatement of the scoring of a simulation study (include/literate_hip_score.h's covered and score, and
literate_amd/simstudy.py's shift, power, false-positive and K arithmetic): the specification the device and the module are
held to.  Written with plain loops over replicates, kinds and bins, from rates [G, 3, 3, n_bins], shift_freq [G, 2, n_bins],
k_counts [G, 2, KMAX], the truth [2, n_bins] (or [G, 2, n_bins]) and a prior frequency vector [n_bins]."""
import math

import numpy as np


def truth3(truth):
    """[..., 2, n_bins] -> [..., 3, n_bins]: birth, death, net = birth - death"""
    t = np.asarray(truth, dtype=np.float64)
    return np.concatenate([t, (t[..., 0, :] - t[..., 1, :])[..., None, :]], axis=-2)


def covered(rates, truth):
    """int32 [G, 3, n_bins]: HPD low <= truth <= HPD high, ends included"""
    rates = np.asarray(rates, dtype=np.float64)
    G, _, _, nb = rates.shape
    t = np.broadcast_to(truth3(truth), (G, 3, nb))
    out = np.zeros((G, 3, nb), dtype=np.int32)
    for g in range(G):
        for k in range(3):
            for i in range(nb):
                out[g, k, i] = 1 if rates[g, k, 1, i] <= t[g, k, i] <= rates[g, k, 2, i] else 0
    return out


def score(rates, truth):
    """[3, n_bins, 6]: groups, coverage, bias, mean absolute error, root mean squared error, mean HPD width; and the sums of
    |terms| / G of the four real-valued columns [3, n_bins, 4] (what the bound of a reordered sum is stated in)"""
    rates = np.asarray(rates, dtype=np.float64)
    G, _, _, nb = rates.shape
    t = np.broadcast_to(truth3(truth), (G, 3, nb))
    cov = covered(rates, truth)
    out, mag = np.zeros((3, nb, 6)), np.zeros((3, nb, 4))
    for k in range(3):
        for i in range(nb):
            err = rates[:, k, 0, i] - t[:, k, i]
            width = rates[:, k, 2, i] - rates[:, k, 1, i]
            out[k, i] = [G, cov[:, k, i].sum() / G, math.fsum(err) / G, math.fsum(np.abs(err)) / G,
                         math.sqrt(math.fsum(err * err) / G), math.fsum(width) / G]
            mag[k, i] = [math.fsum(np.abs(err)) / G, math.fsum(np.abs(err)) / G, math.fsum(err * err) / G, math.fsum(np.abs(width)) / G]
    return out, mag


def empirical(sp, ex, br, truth):
    """[3, n_bins, 6] for the raw estimates sp / br, ex / br and their difference: no band, coverage and width NaN"""
    sp, ex, br = [np.asarray(x, dtype=np.float64) for x in (sp, ex, br)]
    R, nb = sp.shape
    t = truth3(truth)
    out = np.full((3, nb, 6), np.nan)
    for i in range(nb):
        est = [sp[:, i] / br[:, i], ex[:, i] / br[:, i]]
        est.append(est[0] - est[1])
        for k in range(3):
            err = est[k] - t[k, i]
            out[k, i, 0] = R
            out[k, i, 2], out[k, i, 3], out[k, i, 4] = err.sum() / R, np.abs(err).sum() / R, math.sqrt((err * err).sum() / R)
    return out


def two_ln_bf(f, pi):
    """2 ln [(f / (1 - f)) / (pi / (1 - pi))]; -inf at f = 0, +inf at f = 1, NaN where the prior frequency is 0"""
    if not pi > 0:
        return float("nan")
    if f <= 0:
        return -math.inf
    if f >= 1:
        return math.inf
    return 2.0 * math.log((f / (1.0 - f)) / (pi / (1.0 - pi)))


def reported(shift_freq, prior, bf=6.0):
    """bool [G, 2, n_bins]: the replicate reports a shift of the kind in the bin"""
    f = np.asarray(shift_freq, dtype=np.float64)
    G, _, nb = f.shape
    prior = np.broadcast_to(np.asarray(prior, dtype=np.float64), (nb,))
    out = np.zeros((G, 2, nb), dtype=bool)
    for g in range(G):
        for k in range(2):
            for i in range(nb):
                out[g, k, i] = two_ln_bf(f[g, k, i], prior[i]) > bf
    return out


def true_shifts(truth, k):
    t = np.asarray(truth, dtype=np.float64)[k]
    return [i for i in range(1, len(t)) if t[i] != t[i - 1]]


def shifts(shift_freq, k_counts, truth, prior, bf=6.0, tol=2):
    """dict per kind name ("birth", "death"): true_bins, ratio, power (lists beside each other), false_positive, k_true,
    k_mode_share, k_mean; and k_mode [G, 2]"""
    rep = reported(shift_freq, prior, bf)
    G, _, nb = rep.shape
    truth = np.asarray(truth, dtype=np.float64)
    kc = np.asarray(k_counts)
    out = {"k_mode": np.zeros((G, 2), dtype=np.int64)}
    for k, kind in enumerate(("birth", "death")):
        tb = true_shifts(truth, k)
        power = []
        for i in tb:
            hits = sum(1 for g in range(G) if any(rep[g, k, j] for j in range(max(0, i - tol), min(nb, i + tol + 1))))
            power.append(hits / G)
        far = [j for j in range(nb) if all(abs(j - i) > tol for i in tb)]
        fp = sum(1 for g in range(G) if any(rep[g, k, j] for j in far)) / G
        modes, means = [], []
        for g in range(G):
            c = [int(v) for v in kc[g, k]]
            modes.append(c.index(max(c)) + 1)
            means.append(sum((j + 1) * v for j, v in enumerate(c)) / sum(c))
        out["k_mode"][:, k] = modes
        out[kind] = dict(true_bins=tb, ratio=[truth[k, i] / truth[k, i - 1] for i in tb], power=power, false_positive=fp,
                         k_true=len(tb) + 1, k_mode_share=sum(1 for m in modes if m == len(tb) + 1) / G, k_mean=sum(means) / G)
    return out
