"""Approximate Bayesian computation around the count-level simulator (csrc/lr_abc.hip, include/literate_hip_abc.h): fit
the niche-construction model, which has no likelihood, by simulating it.

    python -m literate_amd.abc -d data.tsv [-TBP] --model niche|fixed [--prior priors.tsv] --sims 1048576 --keep 0.01
           --rounds 4 [--steps_per_bin 100] [--start_bin B] [--max_living M] [--stats rates|rates+div] [--seed S] --out STEM

What the reference set out to do in the ABCMachine of simulateRateABC.v2.py (:346-452, dead code there): draw parameters from
the prior, simulate, keep the draws whose per-bin statistics lie nearest the observed ones.  Here every round is one launch
of lr_abc_simulate.  Round 0 is rejection ABC; rounds 1 .. R - 1 are population Monte Carlo (Beaumont, Cornuet, Marin &
Robert 2009, Biometrika 96:983) in batch form: ancestors drawn by weight, every free coordinate perturbed by a normal of
twice the weighted variance of the previous population, the tolerance the largest distance kept before, the weights
prior / mixture of kernels.  Parameters and their small-array arithmetic live on the host in numpy; the simulations and the
N x n_kept kernel sums run on the device.

What comes out is a sample from the posterior GIVEN THAT the simulated statistics lie within eps of the observed ones, eps >
0, under per-bin rates (and diversities) that are not sufficient statistics: wider than the posterior given the data.  K0, g
and h are weakly identified on short series.
"""
import argparse
import math
import sys
import time

import numpy as np

PARAMS = ["l0", "m0", "K0", "Kmax", "g", "h"]
DISTS = ("fixed", "uniform", "loguniform")
CHUNK = 1024          # proposals per block of the kernel-mixture sum (1024 x 10486 kept x 6 doubles: 0.5 GB)


# ---- priors -----------------------------------------------------------------------------------------------------------------
def default_priors(n_start, max_div, model="niche"):
    """[(dist, a, b)] per parameter of PARAMS.  l0, m0 loguniform(0.01, 5); K0 uniform(n_start, largest observed diversity);
    Kmax loguniform(that, 20 x that); g, h uniform(0, 1) (simulateRateABC.v2.py:382-383), fixed at 0 under --model fixed."""
    if model not in ("niche", "fixed"):
        raise ValueError("model must be niche or fixed, not %r" % (model,))
    n_start, max_div = float(n_start), float(max_div)
    gh = ("uniform", 0.0, 1.0) if model == "niche" else ("fixed", 0.0, 0.0)
    k0 = ("uniform", n_start, max_div) if max_div > n_start else ("fixed", n_start, n_start)
    return [("loguniform", 0.01, 5.0), ("loguniform", 0.01, 5.0), k0, ("loguniform", max_div, 20.0 * max_div), gh, gh]


def check_prior(name, dist, a, b):
    if dist not in DISTS:
        raise ValueError("prior of %s: unknown distribution %r (one of %s)" % (name, dist, ", ".join(DISTS)))
    if not (np.isfinite(a) and np.isfinite(b)):
        raise ValueError("prior of %s: bounds %r, %r are not finite" % (name, a, b))
    if dist == "fixed":
        return (dist, float(a), float(a))
    if not a < b:
        raise ValueError("prior of %s: the support [%r, %r] is empty" % (name, a, b))
    if dist == "loguniform" and not a > 0:
        raise ValueError("prior of %s: a loguniform prior needs a positive lower bound, not %r" % (name, a))
    return (dist, float(a), float(b))


def read_priors(path, priors):
    """Rows `param dist a b` (tab or blank separated, `#` comments, an optional header line `param ...`) replace the entries
    of `priors`; a `fixed` row may leave b out."""
    out = list(priors)
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            cells = line.split("#")[0].split()
            if not cells or cells[0] == "param":
                continue
            if cells[0] not in PARAMS:
                raise ValueError("%s line %d: unknown parameter %r (one of %s)" % (path, ln, cells[0], ", ".join(PARAMS)))
            if len(cells) < 3 or (len(cells) < 4 and cells[1] != "fixed"):
                raise ValueError("%s line %d: expected `param dist a b`" % (path, ln))
            try:
                a = float(cells[2])
                b = float(cells[3]) if len(cells) > 3 else a
            except ValueError:
                raise ValueError("%s line %d: bounds that are not numbers" % (path, ln))
            out[PARAMS.index(cells[0])] = check_prior(cells[0], cells[1], a, b)
    return out


def free_of(priors):
    return np.array([p[0] != "fixed" for p in priors])


def prior_transform(priors, u):
    """u [N, 6] uniforms -> theta [N, 6]"""
    th = np.empty_like(u)
    for d, (dist, a, b) in enumerate(priors):
        if dist == "fixed":
            th[:, d] = a
        elif dist == "uniform":
            th[:, d] = a + (b - a) * u[:, d]
        else:
            th[:, d] = np.exp(np.log(a) + (np.log(b) - np.log(a)) * u[:, d])
    return th


def prior_mean(priors):
    return np.array([a if dist == "fixed" else (0.5 * (a + b) if dist == "uniform" else (b - a) / math.log(b / a))
                     for dist, a, b in priors])


def in_support(priors, theta):
    ok = np.ones(len(theta), dtype=bool)
    for d, (dist, a, b) in enumerate(priors):
        if dist != "fixed":
            ok &= (theta[:, d] >= a) & (theta[:, d] <= b)
    return ok


def log_prior(priors, theta):
    """log density over the free coordinates, for theta inside the support"""
    lp = np.zeros(len(theta))
    for d, (dist, a, b) in enumerate(priors):
        if dist == "uniform":
            lp -= math.log(b - a)
        elif dist == "loguniform":
            lp -= np.log(theta[:, d]) + math.log(math.log(b / a))
    return lp


# ---- the pieces of a round --------------------------------------------------------------------------------------------------
def n_keep_of(keep, n_sims):
    return int(math.ceil(keep * n_sims))


def smallest(dist, n_keep, eps=np.inf):
    """positions of the n_keep smallest finite distances <= eps, ascending, ties to the lower position (a stable sort)"""
    order = np.argsort(dist, kind="stable")
    order = order[np.isfinite(dist[order]) & (dist[order] <= eps)]
    return order[:n_keep]


def weighted_var(theta, w):
    mean = (w[:, None] * theta).sum(0)
    return (w[:, None] * (theta - mean) ** 2).sum(0)


def ancestors(w, u):
    cw = np.cumsum(w)
    return np.minimum(np.searchsorted(cw, u * cw[-1], side="right"), len(w) - 1)


def weighted_quantiles(x, w, qs=(0.025, 0.5, 0.975)):
    """the first sorted value at which the cumulated weight reaches q"""
    order = np.argsort(x, kind="stable")
    cw = np.cumsum(w[order])
    return np.array([x[order[min(int(np.searchsorted(cw, q * cw[-1], side="left")), len(x) - 1)]] for q in qs])


def log_weights_device(theta, lp, prev_theta, prev_w, var2, moved, device=None):
    """log w_i = log prior(theta_i) - log sum_j w_j N(theta_i | theta_j, diag var2) over the moved coordinates, normalised to
    sum to one: a chunked log-sum-exp in float64 with torch on the device."""
    import torch
    dev = device or "cuda"
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    new, old, lw, v = t(theta[:, moved]), t(prev_theta[:, moved]), torch.log(t(prev_w)), t(var2[moved])
    const = -0.5 * float(np.sum(np.log(2.0 * np.pi * var2[moved])))
    mix = torch.empty(len(theta), dtype=torch.float64, device=dev)
    for a in range(0, len(theta), CHUNK):
        d = new[a:a + CHUNK, None, :] - old[None, :, :]
        mix[a:a + CHUNK] = torch.logsumexp(lw[None, :] - 0.5 * (d * d / v).sum(-1) + const, dim=1)
    out = t(lp) - mix
    return (out - torch.logsumexp(out, dim=0)).cpu().numpy()


class AbcResult:
    """theta [n, 6], weights [n], dist [n], ids [n]: the last population; rounds: one dict per round run; stopped: the round
    that kept fewer than 2 particles (the population is then the round before's), or None"""

    def __init__(self, priors, theta, weights, dist, ids, rounds, stopped):
        self.priors, self.theta, self.weights, self.dist, self.ids = priors, theta, weights, dist, ids
        self.rounds, self.stopped = rounds, stopped


def _round_row(r, n_sims, inside, dist, flags, kept, eps, w):
    return dict(round=r, simulations=n_sims, in_support=int(inside), finite=int(np.isfinite(dist).sum()),
                overflowed=int(((flags & 1) != 0).sum()), extinct=int(((flags & 2) != 0).sum()), kept=int(kept), eps=float(eps),
                ess=float(1.0 / np.sum(w * w)) if len(w) else 0.0)


def fit(simulate, priors, n_sims, keep, rounds, seed, log_weights=log_weights_device, verbose=False):
    """simulate(theta [M, 6], ids int64 [M]) -> (dist [M], flags [M]) host arrays.  Proposal j of round r has the id r n_sims +
    j, whether or not it is simulated.  Host draws: numpy Generator(Philox(seed)) - round 0 takes random((N, 6)), every later
    round random(N) for the ancestors, then standard_normal((N, 6))."""
    if n_sims < 2 or not (0.0 < keep <= 1.0) or rounds < 1:
        raise ValueError("abc: at least 2 simulations, 0 < keep <= 1 and at least one round")
    if rounds * n_sims > 1 << 32:
        raise ValueError("abc: %d rounds of %d simulations need more than the 2^32 simulation ids there are" % (rounds, n_sims))
    rng = np.random.Generator(np.random.Philox(int(seed)))
    free, n_keep = free_of(priors), n_keep_of(keep, n_sims)
    theta = prior_transform(priors, rng.random((n_sims, len(PARAMS))))
    ids = np.arange(n_sims, dtype=np.int64)
    dist, flags = simulate(theta, ids)
    sel = smallest(dist, n_keep)
    if not len(sel):
        raise ValueError("abc: no simulation of round 0 has a finite distance (%d overflowed max_living, %d went extinct, %d "
                         "were refused): widen max_living or change the priors" %
                         (((flags & 1) != 0).sum(), ((flags & 2) != 0).sum(), ((flags & 4) != 0).sum()))
    pop_t, pop_d, pop_i = theta[sel], dist[sel], ids[sel]
    pop_w = np.full(len(sel), 1.0 / len(sel))
    eps = float(pop_d[-1])
    table = [_round_row(0, n_sims, n_sims, dist, flags, len(sel), eps, pop_w)]
    stopped = None
    for r in range(1, rounds):
        if verbose:
            print("round %d: kept %d, eps %.6g, ESS %.1f" % (r - 1, table[-1]["kept"], eps, table[-1]["ess"]))
        var2 = 2.0 * weighted_var(pop_t, pop_w)
        moved = free & (var2 > 0.0)
        anc = ancestors(pop_w, rng.random(n_sims))
        z = rng.standard_normal((n_sims, len(PARAMS)))
        theta = pop_t[anc] + np.where(moved, np.sqrt(var2), 0.0) * z
        inside = in_support(priors, theta)
        at = np.nonzero(inside)[0]
        ids = r * np.int64(n_sims) + at.astype(np.int64)
        dist, flags = simulate(theta[at], ids)
        sel = smallest(dist, n_keep, eps)
        if len(sel) < 2:
            table.append(_round_row(r, n_sims, len(at), dist, flags, len(sel), eps, pop_w[:0]))
            stopped = r
            break
        new_t = theta[at][sel]
        lw = log_weights(new_t, log_prior(priors, new_t), pop_t, pop_w, var2, moved)
        pop_t, pop_d, pop_i, pop_w = new_t, dist[sel], ids[sel], np.exp(lw)
        eps = float(pop_d[-1])
        table.append(_round_row(r, n_sims, len(at), dist, flags, len(sel), eps, pop_w))
    return AbcResult(priors, pop_t, pop_w, pop_d, pop_i, table, stopped)


# ---- the observed statistics ------------------------------------------------------------------------------------------------
class Observed:
    """What the simulations are scored against.  n_spec, n_exti, DT: create_bins' per-bin statistics; the simulation starts at
    the left edge of bin b0 with the lineages observed living there and covers bins b0 .. n_bins - 1."""

    def __init__(self, n_spec, n_exti, DT, start_bin=None, stats="rates"):
        from .ppc import observed_diversity, pick_start_bin
        if stats not in ("rates", "rates+div"):
            raise ValueError("--stats must be rates or rates+div, not %r" % (stats,))
        n_spec, n_exti, DT = np.asarray(n_spec), np.asarray(n_exti), np.asarray(DT, dtype=float)
        div = observed_diversity(n_spec, n_exti)
        self.b0 = b0 = pick_start_bin(div, start_bin)
        nb = len(DT) - b0
        if nb < 2:
            raise ValueError("abc: %d bin after the start bin %d: at least 2 are needed" % (nb, b0))
        self.n_bins, self.n_start, self.max_div = nb, int(div[b0]), int(div[b0:].max())
        with np.errstate(all="ignore"):
            self.obs = np.stack([n_spec[b0:] / DT[b0:], n_exti[b0:] / DT[b0:], div[b0:-1].astype(float)])
        # the mean relative deviation over the counted entries (simulateRateABC.v2.py:426-430); an entry whose observed value
        # is 0 (or not finite: a bin without lineage-time) has no relative deviation and does not count
        counted = np.isfinite(self.obs) & (self.obs > 0)
        if stats == "rates":
            counted[2] = False
        if not counted.any():
            raise ValueError("abc: no bin with a positive observed rate to score against")
        with np.errstate(all="ignore"):
            self.weight = np.where(counted, 1.0 / (self.obs * counted.sum()), 0.0)
        self.obs = np.where(counted, self.obs, 0.0)

    def default_max_living(self):
        return int(min(1 << 20, 16 * self.max_div))


def device_simulator(observed, steps_per_bin, max_living, seed, device=None):
    from . import ops
    import torch
    dev = device or "cuda"
    obs, weight = [torch.as_tensor(a, dtype=torch.float64, device=dev) for a in (observed.obs, observed.weight)]

    def simulate(theta, ids, counts=False):
        if not len(theta):
            return (np.zeros(0), np.zeros(0, dtype=np.int32)) + ((np.zeros((0, 4, observed.n_bins), dtype=np.int64),) if counts else ())
        res = ops.abc_simulate(theta, observed.n_start, obs, weight, steps_per_bin, max_living, seed, sim_id=ids, counts=counts,
                               device=dev)
        out = (res.dist.cpu().numpy(), res.flags.cpu().numpy())
        return out + (res.counts.cpu().numpy(),) if counts else out
    return simulate


# ---- files ------------------------------------------------------------------------------------------------------------------
def _num(v):
    return str(float(v))


def params_table(res):
    """STEM_ABC.tsv: per parameter the prior mean, the weighted posterior mean, the weighted 2.5 %, 50 % and 97.5 % quantiles, and
    whether it was fixed"""
    pm = prior_mean(res.priors)
    lines = ["param\tprior_mean\tmean\tq2.5\tq50\tq97.5\tfixed"]
    for d, name in enumerate(PARAMS):
        q = weighted_quantiles(res.theta[:, d], res.weights)
        lines.append("\t".join([name, _num(pm[d]), _num(np.sum(res.weights * res.theta[:, d]))] + [_num(v) for v in q] +
                               [str(int(res.priors[d][0] == "fixed"))]))
    return "\n".join(lines) + "\n"


ROUND_COLS = ["round", "simulations", "in_support", "finite", "overflowed", "extinct", "kept", "eps", "ess"]


def rounds_table(res):
    lines = ["\t".join(ROUND_COLS)]
    for row in res.rounds:
        lines.append("\t".join(_num(row[c]) if c in ("eps", "ess") else str(row[c]) for c in ROUND_COLS))
    if res.stopped is not None:
        lines.append("# round %d kept fewer than 2 particles: the population of round %d stands" % (res.stopped, res.stopped - 1))
    return "\n".join(lines) + "\n"


def fit_stats(counts, steps_per_bin):
    """counts [n, 4, n_bins] -> [n, 3, n_bins]: birth rate, death rate, diversity at the start of the bin"""
    t = counts[:, 3].astype(float) / float(steps_per_bin)
    return np.stack([counts[:, 0] / t, counts[:, 1] / t, counts[:, 2].astype(float)], axis=1)


FIT_KINDS = ["birth_rate", "death_rate", "diversity"]


def fit_table(observed, res, sims):
    """STEM_ABC_fit.tsv: per kind and bin the observed value beside the kept simulations' weighted mean and 95 % band"""
    lines = ["kind\tbin\tobserved\tmean\tq2.5\tq97.5"]
    for k, kind in enumerate(FIT_KINDS):
        for b in range(observed.n_bins):
            q = weighted_quantiles(sims[:, k, b], res.weights, (0.025, 0.975))
            lines.append("\t".join([kind, str(observed.b0 + b), _num(observed.obs[k, b]), _num(np.sum(res.weights * sims[:, k, b])),
                                    _num(q[0]), _num(q[1])]))
    return "\n".join(lines) + "\n"


def write_files(stem, observed, res, sims, settings):
    paths = []
    for suffix, text in (("_ABC.tsv", params_table(res)), ("_ABC_rounds.tsv", rounds_table(res)),
                         ("_ABC_fit.tsv", fit_table(observed, res, sims))):
        with open(stem + suffix, "w") as f:
            f.write(text)
        paths.append(stem + suffix)
    np.savez(stem + "_ABC.npz", theta=res.theta, weights=res.weights, dist=res.dist, ids=res.ids, params=np.array(PARAMS),
             prior_dist=np.array([p[0] for p in res.priors]), prior_bounds=np.array([p[1:] for p in res.priors]),
             obs=observed.obs, weight=observed.weight, start_bin=observed.b0, n_start=observed.n_start, sims=sims,
             stopped=-1 if res.stopped is None else res.stopped, **settings)
    return paths + [stem + "_ABC.npz"]


def run(n_spec, n_exti, DT, model="niche", prior_file=None, n_sims=1 << 20, keep=0.01, rounds=4, steps_per_bin=100, start_bin=None,
        max_living=None, stats="rates", seed=1, out=None, device=None, verbose=False):
    """The whole fit on create_bins' statistics -> (Observed, AbcResult, sims [n_kept, 3, n_bins]); with `out`, the four files."""
    observed = Observed(n_spec, n_exti, DT, start_bin, stats)
    priors = default_priors(observed.n_start, observed.max_div, model)
    if prior_file:
        priors = read_priors(prior_file, priors)
    max_living = int(max_living or observed.default_max_living())
    simulate = device_simulator(observed, steps_per_bin, max_living, seed, device)
    res = fit(simulate, priors, n_sims, keep, rounds, seed, verbose=verbose)
    # the kept ids alone, once more, with their counts: what the id rule is for
    dist, _, counts = simulate(res.theta, res.ids, counts=True)
    if not np.array_equal(dist, res.dist):
        raise RuntimeError("abc: the kept simulations did not reproduce their distances")
    sims = fit_stats(counts, steps_per_bin)
    if out:
        write_files(out, observed, res, sims, dict(model=model, n_sims=n_sims, keep=keep, rounds=rounds, steps_per_bin=steps_per_bin,
                                                   max_living=max_living, stats=stats, seed=seed))
    return observed, res, sims


def parser():
    p = argparse.ArgumentParser(prog="python -m literate_amd.abc", description="Fit the niche-construction model, which has no "
                                "likelihood, by approximate Bayesian computation on the GPU")
    p.add_argument("-d", required=True, help="data file, as DDRate.py -d")
    p.add_argument("-TBP", action="store_true", default=False)
    p.add_argument("-first_year", type=int, default=-1)
    p.add_argument("-last_year", type=int, default=-1)
    p.add_argument("-death_jitter", type=float, default=.5)
    p.add_argument("--model", default="niche", choices=["niche", "fixed"], help="fixed: g = h = 0, the fixed niche")
    p.add_argument("--prior", default="", help="TSV `param dist a b` (fixed, uniform, loguniform) replacing default priors")
    p.add_argument("--sims", type=int, default=1 << 20, help="simulations per round")
    p.add_argument("--keep", type=float, default=0.01, help="share of a round's simulations kept")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--steps_per_bin", type=int, default=100)
    p.add_argument("--start_bin", type=int, default=-1)
    p.add_argument("--max_living", type=int, default=0, help="default min(2^20, 16 x the largest observed diversity)")
    p.add_argument("--stats", default="rates", choices=["rates", "rates+div"])
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--out", required=True, metavar="STEM")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    from .literate_library import create_bins, parse_ts_te
    t = time.time()
    try:
        ts, te, present, origin = parse_ts_te(args.d, args.TBP, args.first_year, args.last_year, args.death_jitter)
        _, _, n_spec, n_exti, DT, _, _ = create_bins(origin, present, np.asarray(ts, dtype=float), np.asarray(te, dtype=float), 0)
        observed, res, _ = run(n_spec, n_exti, DT, args.model, args.prior or None, args.sims, args.keep, args.rounds, args.steps_per_bin,
                               None if args.start_bin < 0 else args.start_bin, args.max_living or None, args.stats, args.seed, args.out,
                               verbose=True)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e))
    if res.stopped is not None:
        print("round %d kept fewer than 2 particles: the population of round %d stands" % (res.stopped, res.stopped - 1), file=sys.stderr)
    print(rounds_table(res), end="")
    print(params_table(res), end="")
    print("%d bins from bin %d, %d lineages at the start; %.2f s" % (observed.n_bins, observed.b0, observed.n_start, time.time() - t))


if __name__ == "__main__":
    main()
