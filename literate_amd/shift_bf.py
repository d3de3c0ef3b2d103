"""Bayes factors for rate shifts from the Monte Carlo prior on shift times (host only, numpy).

ops.shift_prior counts, over replicates of the prior, the shift times that fall in each unit bin; the functions here turn
those counts into what plotRJforward.v3.py derives from its own loop: the prior frequency of a shift in a bin (get_prior_shift
:86), the sampled frequencies that amount to 2 ln BF = 2 and = 6 against it (calcBF :54-56, the two dashed lines of the
shift-frequency plot) and the birth_BF2 / birth_BF6 / death_BF2 / death_BF6 vectors (get_r_plot :188-195).  The arithmetic
mirrors the script's expressions.  Nothing raises on an empty prior (a span shorter than 2 accepts no shift): the
thresholds are then 0 and the Bayes factors NaN."""
import numpy as np


def prior_s(hist, accepted):
    """The prior frequency of a shift in a bin, np.mean(histogram / accepted replicates) (:86); 0 without replicates."""
    hist = np.asarray(hist, dtype=np.float64)
    if not accepted or hist.size == 0:
        return 0.0
    return float(np.mean(hist / float(accepted)))


def calc_bf(threshold, prior):
    """calcBF (:54-56): the sampled frequency at which 2 ln BF against the prior frequency reaches `threshold`."""
    prior = np.float64(prior)                   # (numpy's division: a prior of 1 gives NaN, it does not raise)
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.exp(threshold / 2) * prior / (1 - prior)
        return float(A / (A + 1))


def thresholds(prior):
    """(bf2, bf6): the frequencies of positive and of strong evidence for a shift (:87-88)."""
    return calc_bf(2, prior), calc_bf(6, prior)


def two_ln_bf(freq, prior):
    """2 ln [(f / (1 - f)) / (pi / (1 - pi))] of sampled frequencies f against the prior frequency pi - the quantity
    calcBF inverts.  -inf at f = 0, +inf at f = 1, NaN where the prior frequency is 0 (or NaN)."""
    f = np.asarray(freq, dtype=np.float64)
    pi = np.asarray(prior, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 2.0 * np.log((f / (1.0 - f)) / (pi / (1.0 - pi)))
    out = np.where(pi > 0, out, np.nan)
    return out if out.ndim else float(out)


def flags(freq, mean_rate, bf2, bf6):
    """(BF2, BF6) vectors of get_r_plot (:188-195): the mean rate where bf2 <= f < bf6 (positive evidence of a shift in the
    bin) resp. where f >= bf6 (strong evidence), NaN elsewhere."""
    f = np.asarray(freq, dtype=np.float64)
    rate = np.asarray(mean_rate, dtype=np.float64)
    return np.where((f >= bf2) & (f < bf6), rate, np.nan), np.where(f >= bf6, rate, np.nan)


def k_bayes_factor(k_counts_row, k_accepted):
    """2 ln BF of 'at least one shift' (K > 1) against a constant rate (K = 1): the posterior odds from one row of
    rtt_summary's k_counts over the prior odds from the accepted replicates' K histogram.  NaN where either odds is 0 / 0
    or the prior saw only one side."""
    post = np.asarray(k_counts_row, dtype=np.float64).ravel()
    pri = np.asarray(k_accepted, dtype=np.float64).ravel()
    if post.size == 0 or pri.size == 0 or pri[0] == 0 or pri[1:].sum() == 0:
        return float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(2.0 * np.log((post[1:].sum() / post[0]) / (pri[1:].sum() / pri[0])))
