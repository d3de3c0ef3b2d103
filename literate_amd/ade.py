"""Age-dependent extinction of a finished run: how strongly does a lineage's chance of dying depend on its age?

--ppc_age tells whether it does; this module puts a number on it, the Weibull shape k of the reference's ADE_discrete/
scripts: k < 1 a liability of newness, k > 1 ageing, k = 1 what the three samplers assume.  The reference fits k against a
CONSTANT baseline death rate, and on data with rate shifts that estimate is confounded with the shifts (rates rising 0.05 ->
0.15 -> 0.3 without any age effect give k = 1.07 and a likelihood ratio of 6 against k = 1).  Here the age effect is fitted
conditional on the time pattern the run has sampled, and the reference's constant-baseline Weibull is reported beside it.

Model, at the resolution of the bins (include/literate_hip_ade.h): a lineage is born at the start of its birth bin; at age a
(in bins) its hazard in bin b is c mu[b] k a^(k - 1), mu one posterior draw of the per-bin death rates, c a free multiplier.
A death is known to its bin only, so the likelihood is interval-censored.  Year-resolution input is represented exactly;
continuous times are coarsened to their bins (a birth to the start of its bin, a death to its bin).

1. The lineages are counted per class (birth bin, age at death) once (ops.ade_classes).
2. For every draw and every shape of a grid the multiplier is profiled out on the device (ops.ade_profile): one workgroup
   per (draw, shape), whatever the number of lineages.  Coarse pass: 65 shapes 2^((j - 32) 3 / 32), 1/8 .. 8, node 32 exactly
   1; per draw a parabola in log shape through the maximum and its neighbours gives m_s and se_s.  Fine pass: 129 shapes
   equally spaced in log shape over [min_s (m_s - 6 se_s), max_s (m_s + 6 se_s)], clipped to the coarse range.
3. Per draw p_s(g) ~ exp(profile log-likelihood) over the fine nodes (a flat prior on log shape), shape_ml_s the
   parabola-refined argmax, lr_s = 2 (max over all nodes - value at k = 1).  Over the draws p(g) = mean_s p_s(g): its mean,
   median and 95 % interval (each quantile the smallest node whose CDF reaches it), the mass below 1, the mass on the two
   edge nodes, the fine step over the median se_s; mean and 95 % HPD of shape_ml_s and lr_s (ops.col_summary).
4. The same two passes with one draw mu = 1: the reference's constant-baseline Weibull (const_*), with its scale
   c^(-1/k) and mean longevity scale Gamma(1 + 1/k), in bins.
5. <stem>_ADE.tsv (one row) and <stem>_ADE_shape.tsv (one row per coarse and fine node).

What this is not: the sampled rates were fitted under k = 1, so the result is an estimate CONDITIONAL on the run's time
pattern, not a joint posterior of shape and rates; the joint sampler of both is literate_amd/ade_joint.py (--ade_joint).

Refused where --ppc_age is refused (-model_BDI 3, -pyrate_output, -rm_first_bin 1), and with more than LR_ADE_MAX_BINS bins."""
import math
from collections import namedtuple

import numpy as np

N_COARSE, N_FINE, ONE = 65, 129, 32
MAX_BINS = 512                      # LR_ADE_MAX_BINS
FIT_INTS = ["draws", "draws_flagged", "lineages", "lineages_used", "lineages_unused", "bins", "deaths", "censored", "classes"]
FIT_FLOATS = ["shape_mean", "shape_median", "shape_q025", "shape_q975", "p_shape_lt_1", "edge_mass", "grid_step_over_se",
              "shape_ml_mean", "shape_ml_hpd_low", "shape_ml_hpd_high", "lr_mean", "lr_hpd_low", "lr_hpd_high",
              "const_shape_ml", "const_shape_q025", "const_shape_q975", "const_lr", "const_scale", "const_mean_longevity"]
FIT_HEAD = FIT_INTS + FIT_FLOATS
SHAPE_HEAD = ["grid", "shape", "weight", "loglik_mean", "loglik_min", "loglik_max"]

Passes = namedtuple("Passes", "coarse_ll fine_shapes fine_ll m se p shape_ml lr")
Passes.__doc__ = """two_passes' results over the draws it was given: coarse_ll [S, 65], fine_shapes [129], fine_ll [S, 129], m, se [S]: the
coarse parabola's vertex (log shape) and width, p [S, 129]: the normalised weights of the fine nodes, shape_ml, lr [S]."""

AdeResult = namedtuple("AdeResult", "draw_rows dead cens totals flag kept coarse_shapes fine_shapes cond const weight "
                                    "weight_coarse shape_ml lr fit")
AdeResult.__doc__ = """fit_rates' results (host arrays).  draw_rows [S]: the trace rows the draws came from (None when rates were given
directly); dead [A, A], cens [A], totals [2]: the classes; flag [S], kept [S]: the draws left out and used; coarse_shapes
[65], fine_shapes [129]; cond, const: Passes over the kept draws and over the one draw mu = 1; weight [129], weight_coarse
[65]: p(g) on the fine nodes and its like on the coarse ones; shape_ml, lr [3]: (mean, HPD low, HPD high) over the draws;
fit: dict of <stem>_ADE.tsv (FIT_HEAD)."""


class DeviceProfile:
    """The device path of fit_rates: the classes, the profile and the column summary by literate_amd.ops.  The tests put the
    numpy restatement in its place (three methods, host arrays in and out).  classes() keeps its device tensors, and
    profile() runs on those: the host copies it is handed are the same counts."""

    def classes(self, ts, te, t0, n_bins):
        from . import ops
        self._dead, self._cens, tot = ops.ade_classes(ts, te, t0, n_bins)
        return self._dead.cpu().numpy(), self._cens.cpu().numpy(), tot.cpu().numpy()

    def profile(self, dead, cens, mu_bins, shapes):
        from . import ops
        import torch
        dev = self._dead.device
        ll, c, flag = ops.ade_profile(self._dead, self._cens, torch.as_tensor(mu_bins, dtype=torch.float64, device=dev),
                                      np.asarray(shapes, dtype=np.float64))
        return ll.cpu().numpy(), c.cpu().numpy(), flag.cpu().numpy()

    def summary(self, vals):
        from . import ops
        import torch
        vals = torch.as_tensor(np.ascontiguousarray(vals), dtype=torch.float64, device=self._dead.device)
        n = int(vals.shape[0])
        res = ops.col_summary(vals.reshape(n, 1, -1).contiguous(), n, range(vals.shape[1]), burnin=0.0, pooled=True)
        return np.stack([x[0].cpu().numpy() for x in (res.mean, res.lo, res.hi)], axis=1)


def arg_error(burnin, n_draws, model=2, pyrate_output=False, rm_first_bin=False):
    """Why a CLI's --ade BURNIN cannot run (None when it can): what --ppc_age refuses, for the same reasons."""
    if not (0.0 <= burnin < 1.0):
        return "--ade takes a burn-in fraction in [0, 1)"
    if n_draws < 1:
        return "--ade_draws must be at least 1"
    return shared_refusal("--ade", "trace", model, pyrate_output, rm_first_bin)


def shared_refusal(flag, reads, model, pyrate_output, rm_first_bin):
    """What --ade and --ade_joint both refuse (None when nothing): flag - the option's name, reads - where it takes the
    times from ("trace", "run")."""
    if pyrate_output:
        return "%s reads the AD / TBP times of the %s; -pyrate_output flips them in the logs: not supported together" % (flag, reads)
    if rm_first_bin:
        return ("%s fits the age effect on every lineage of the data; under -rm_first_bin 1 the lineages of the removed bin "
                "were born outside the window the model was fitted on: not supported together" % flag)
    if model == 3:
        return ("%s censors the extant lineages; under -model_BDI 3 the death rates were fitted to the extinct lineages "
                "only, so the extant ones were never in that likelihood: not supported together" % flag)
    return None


def class_counts(dead, cens, totals):
    """The count fields of a fit row (--ade's and --ade_joint's) from ade_classes' host arrays; a class is a cell with
    jb + a < A and a count > 0, as the device reads the table."""
    dead, cens, totals = (np.asarray(x) for x in (dead, cens, totals))
    A = len(cens)
    is_class = (dead > 0) & (np.add.outer(np.arange(A), np.arange(A)) < A)
    return dict(lineages=int(totals[0] + totals[1]), lineages_used=int(totals[0]), lineages_unused=int(totals[1]),
                deaths=int(dead[is_class].sum()), censored=int(cens.sum()), classes=int(is_class.sum()))


def coarse_shapes():
    """the 65 shapes 2^((j - 32) 3 / 32): 1/8 .. 8, node 32 exactly 1"""
    return 2.0 ** ((np.arange(N_COARSE) - ONE) * 3.0 / 32.0)


def refine(logk, ll):
    """logk [G] equally spaced, ll [S, G] -> (vertex [S], se [S]): per row the parabola through the maximum and its two
    neighbours (the index clamped to 1 .. G - 2), its vertex clipped to the neighbours, se = 1 / sqrt(-curvature) - the grid
    step where the curvature is >= 0 (the vertex is then the middle node)"""
    logk, ll = np.asarray(logk, dtype=np.float64), np.asarray(ll, dtype=np.float64)
    G = len(logk)
    h = (logk[-1] - logk[0]) / (G - 1)
    i = np.clip(np.argmax(ll, axis=1), 1, G - 2)
    r = np.arange(ll.shape[0])
    y0, y1, y2 = ll[r, i - 1], ll[r, i], ll[r, i + 1]
    curv = (y0 - 2.0 * y1 + y2) / (h * h)
    ok = curv < 0.0
    safe = np.where(ok, curv, -1.0)
    vertex = np.where(ok, logk[i] - (y2 - y0) / (2.0 * h) / safe, logk[i])
    vertex = np.clip(vertex, logk[i - 1], logk[i + 1])
    return vertex, np.where(ok, 1.0 / np.sqrt(-safe), h)


def fine_shapes(m, se):
    """the 129 shapes of the fine pass, equally spaced in log shape over [min (m - 6 se), max (m + 6 se)] clipped to the
    coarse range"""
    edge = ONE * 3.0 / 32.0 * math.log(2.0)
    lo, hi = max(float(np.min(m - 6.0 * se)), -edge), min(float(np.max(m + 6.0 * se)), edge)
    return np.exp(np.linspace(lo, hi, N_FINE))


def node_weights(ll):
    """ll [S, G] -> p [S, G] ~ exp(ll), each row normalised"""
    w = np.exp(ll - np.max(ll, axis=1, keepdims=True))
    return w / np.sum(w, axis=1, keepdims=True)


def quantile_node(shapes, p, q):
    """the smallest node whose CDF reaches q"""
    cdf = np.cumsum(p)
    return float(shapes[min(int(np.searchsorted(cdf, q, side="left")), len(shapes) - 1)])


def mixture(shapes, p):
    """p(g) on the nodes `shapes` -> dict(shape_mean, shape_median, shape_q025, shape_q975, p_shape_lt_1, edge_mass)"""
    shapes, p = np.asarray(shapes, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return dict(shape_mean=float(np.sum(p * shapes)), shape_median=quantile_node(shapes, p, 0.5),
                shape_q025=quantile_node(shapes, p, 0.025), shape_q975=quantile_node(shapes, p, 0.975),
                p_shape_lt_1=float(np.sum(p[shapes < 1.0])), edge_mass=float(p[0] + p[-1]))


def two_passes(profile_of, n_draws, coarse_ll=None):
    """profile_of(shapes) -> (ll [S, G], c, flag) of the kept draws -> Passes.  coarse_ll: the coarse pass, where it has run"""
    ks = coarse_shapes()
    cll = np.asarray(profile_of(ks)[0] if coarse_ll is None else coarse_ll, dtype=np.float64).reshape(n_draws, N_COARSE)
    m, se = refine(np.log(ks), cll)
    fs = fine_shapes(m, se)
    fll = np.asarray(profile_of(fs)[0], dtype=np.float64).reshape(n_draws, N_FINE)
    vertex, _ = refine(np.log(fs), fll)
    lr = 2.0 * (np.maximum(fll.max(axis=1), cll.max(axis=1)) - cll[:, ONE])
    return Passes(cll, fs, fll, m, se, node_weights(fll), np.exp(vertex), lr)


def fit_rates(ts, te, t0, mu_bins, profile=None, draw_rows=None):
    """The fit of the module docstring on S draws of per-bin death rates mu_bins [S, n_bins] -> AdeResult.  profile: where the
    classes, the profile and the column summary are computed (DeviceProfile by default).  ValueError when fewer unflagged
    draws are left than a 95 % HPD takes (round(0.95 n) >= 2), or with more than LR_ADE_MAX_BINS bins."""
    be = profile if profile is not None else DeviceProfile()
    if hasattr(mu_bins, "detach"):
        mu_bins = mu_bins.detach().cpu().numpy()
    mu = np.ascontiguousarray(np.asarray(mu_bins, dtype=np.float64))
    if mu.ndim != 2:
        raise ValueError("mu_bins must be [draws, n_bins]")
    S, A = mu.shape
    if A > MAX_BINS:
        raise ValueError(too_many_bins(A))
    dead, cens, tot = (np.asarray(x) for x in be.classes(ts, te, t0, A))
    ks = coarse_shapes()
    first = be.profile(dead, cens, mu, ks)
    flag = np.asarray(first[2]).astype(bool)
    kept = ~flag
    n_k = int(kept.sum())
    if int(round(0.95 * n_k)) < 2:
        raise ValueError("age-dependent extinction: %d of the %d draws hold a death rate that is not finite, negative, or zero "
                         "in a bin with an observed death, and the %d left are fewer than a 95 %% HPD takes (round(0.95 n) >= 2)"
                         % (S - n_k, S, n_k))
    mu_k = np.ascontiguousarray(mu[kept])
    cond = two_passes(lambda shapes: be.profile(dead, cens, mu_k, shapes), n_k, coarse_ll=np.asarray(first[0])[kept])
    ones = np.ones((1, A))
    const = two_passes(lambda shapes: be.profile(dead, cens, ones, shapes), 1)
    k_hat = float(const.shape_ml[0])
    c_hat = float(np.asarray(be.profile(dead, cens, ones, np.array([k_hat]))[1]).reshape(-1)[0])
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        scale = float(np.float64(c_hat) ** (-1.0 / k_hat))
    weight = cond.p.mean(axis=0)
    st = np.asarray(be.summary(np.stack([cond.shape_ml, cond.lr], axis=1)), dtype=np.float64)
    fit = dict(draws=S, draws_flagged=S - n_k, bins=A, **class_counts(dead, cens, tot))
    fit.update(mixture(cond.fine_shapes, weight))
    logf = np.log(cond.fine_shapes)
    fit["grid_step_over_se"] = float((logf[-1] - logf[0]) / (N_FINE - 1) / np.median(cond.se))
    for name, row in zip(("shape_ml", "lr"), st):
        fit[name + "_mean"], fit[name + "_hpd_low"], fit[name + "_hpd_high"] = (float(v) for v in row)
    cm = mixture(const.fine_shapes, const.p[0])
    fit.update(const_shape_ml=k_hat, const_shape_q025=cm["shape_q025"], const_shape_q975=cm["shape_q975"],
               const_lr=float(const.lr[0]), const_scale=scale, const_mean_longevity=scale * math.gamma(1.0 + 1.0 / k_hat))
    idx = None if draw_rows is None else np.asarray(draw_rows, dtype=np.int64)
    return AdeResult(idx, dead, cens, tot, flag, kept, ks, cond.fine_shapes, cond, const, weight,
                     node_weights(cond.coarse_ll).mean(axis=0), st[0], st[1], fit)


def too_many_bins(n_bins):
    return ("--ade: the run has %d time bins, and the age-dependent extinction fit takes at most %d (LR_ADE_MAX_BINS): its "
            "classes are a table of bins x bins" % (n_bins, MAX_BINS))


def write_tables(stem, res):
    """<stem>_ADE.tsv (FIT_HEAD, one row) and <stem>_ADE_shape.tsv (SHAPE_HEAD, one row per coarse and per fine node: the
    node's weight and the mean, minimum and maximum of the profile log-likelihood over the kept draws).  Numbers as
    str(float), counts as integers, as the other summary writers write them."""
    with open(stem + "_ADE.tsv", "w") as f:
        f.write("\t".join(FIT_HEAD) + "\n")
        f.write("\t".join("%d" % res.fit[k] if k in FIT_INTS else str(float(res.fit[k])) for k in FIT_HEAD) + "\n")
    with open(stem + "_ADE_shape.tsv", "w") as f:
        f.write("\t".join(SHAPE_HEAD) + "\n")
        for grid, shapes, w, ll in (("coarse", res.coarse_shapes, res.weight_coarse, res.cond.coarse_ll),
                                    ("fine", res.fine_shapes, res.weight, res.cond.fine_ll)):
            for g in range(len(shapes)):
                f.write("\t".join([grid] + [str(float(v)) for v in (shapes[g], w[g], ll[:, g].mean(), ll[:, g].min(),
                                                                    ll[:, g].max())]) + "\n")


def read_tables(stem):
    """what write_tables wrote -> (fit dict, shape rows as a list of (grid, shape, weight, mean, min, max))"""
    with open(stem + "_ADE.tsv") as f:
        head, vals = [l.rstrip("\n").split("\t") for l in f]
    fit = {k: int(v) if k in FIT_INTS else float(v) for k, v in zip(head, vals)}
    with open(stem + "_ADE_shape.tsv") as f:
        rows = [l.rstrip("\n").split("\t") for l in f][1:]
    return fit, [(r[0],) + tuple(float(v) for v in r[1:]) for r in rows]


def _say(stem, res):
    f = res.fit
    return ("ADE: %s_ADE.tsv, %s_ADE_shape.tsv (%d draws, %d flagged; %d of %d lineages used, %d deaths in %d classes; Weibull "
            "shape given the sampled rates %.4f (95 %% %.4f - %.4f), P(shape < 1) %.3f, likelihood ratio against 1 %.2f; "
            "constant baseline %.4f (%.4f - %.4f), ratio %.2f; edge_mass %.2g)"
            % (stem, stem, f["draws"], f["draws_flagged"], f["lineages_used"], f["lineages"], f["deaths"], f["classes"],
               f["shape_median"], f["shape_q025"], f["shape_q975"], f["p_shape_lt_1"], f["lr_mean"], f["const_shape_ml"],
               f["const_shape_q025"], f["const_shape_q975"], f["const_lr"], f["edge_mass"]))


def write_run(eng, n_local, total_chains, world, rank, burnin, n_draws, stem):
    """The three CLIs' --ade, on the path of ppc_age.write_run: the rows the run sampled, int(burnin * S) dropped per chain,
    gathered to rank 0; there n_draws of them chosen as --ppc chooses them, their per-bin death rates by the engine's own
    draw_rates, and fit_rates on the engine's lineages and window -> the two files and one line on stdout."""
    from . import ppc
    from ._hip import LR_TRACE_W
    if int(eng.n_bins) > MAX_BINS:                                           # (every rank, before the collective)
        raise ValueError(too_many_bins(int(eng.n_bins)))
    rows = ppc._gathered_rows(eng, n_local, total_chains, world, burnin)     # (every rank calls: a collective)
    if rank != 0:
        return None
    if rows.dim() != 3 or rows.shape[2] != LR_TRACE_W:
        raise ValueError("rows must be [samples, chains, LR_TRACE_W]")
    flat = rows.reshape(-1, LR_TRACE_W)
    idx = ppc.draw_indices(flat.shape[0], n_draws)
    _, mu = eng.draw_rates(flat, idx)
    if int(mu.shape[1]) != int(eng.n_bins):
        raise ValueError("draw_rates gave %d bins, the engine has %d" % (mu.shape[1], eng.n_bins))
    res = fit_rates(eng.ts, eng.te, eng.t0, mu, draw_rows=idx)
    write_tables(stem, res)
    print(_say(stem, res))
    return res
