"""Simulation study: score the RJ sampler against known rates, the whole study on the GPU.

Before trusting a run a user asks whether, at this data size, the sampler can recover a rate history like this one: how often
the 95 % HPD band holds the true rate, how large a shift is found and how often, how often one is reported that is not
there.  The reference answers with simulated data (simulateRateABC.v2.py, the rate generators of its notebook 4), one run
per data set.  Here:

    read_scenario / scenario_from_rtt   the true rates per unit bin, from a TSV or from a finished run's RTT table
    simulate                            ops.simulate_bd_batch: every replicate of the scenario in one launch
    keep_replicates                     which of them reach the sampler (and why the others do not)
    statistics                          the per-bin statistics of the kept ones -> replicates.Replicates.from_counts
    run                                 ... -> ReplicateEngine (one launch for all chains) -> ops.rtt_score (one launch for all
                                        replicates) -> shifts(): power, false positives, K recovery -> Result
    main                                python -m literate_amd.simstudy SCENARIO --replicates R ... --out STEM: the four files

Everything after the sampler is arithmetic on small arrays, [G, 2, n_bins] at most: it runs on the host in numpy."""
import argparse
import sys
import time

import numpy as np

MIN_BINS, MAX_BINS = 2, 512
KINDS = ("birth", "death", "net")
SCORE_HEAD = ["n", "coverage", "bias", "mae", "rmse", "hpd_width"]
EMP_HEAD = ["emp_n", "emp_bias", "emp_mae", "emp_rmse"]
REASONS = ("kept", "overflow", "extinct", "empty_bin", "lineages")


# ---- the scenario -----------------------------------------------------------------------------------------------------------
def check_scenario(birth, death, what="scenario"):
    """[2, n_bins] float64 of the true birth and death rates per unit bin, or ValueError with the reason in a sentence"""
    birth, death = np.asarray(birth, dtype=np.float64).ravel(), np.asarray(death, dtype=np.float64).ravel()
    if birth.size != death.size:
        raise ValueError("%s: %d birth rates but %d death rates" % (what, birth.size, death.size))
    if birth.size < MIN_BINS:
        raise ValueError("%s: %d bins; a scenario needs at least %d unit bins" % (what, birth.size, MIN_BINS))
    if birth.size > MAX_BINS:
        raise ValueError("%s: %d bins; the replicate sampler holds at most %d" % (what, birth.size, MAX_BINS))
    sc = np.stack([birth, death])
    if not np.all(np.isfinite(sc)):
        raise ValueError("%s: a rate is not a finite number" % what)
    if (sc < 0).any():
        raise ValueError("%s: a rate is negative" % what)
    return sc


def _table(path):
    """(header, rows) of a tab- or blank-separated table; lines that start with # and empty lines are skipped"""
    with open(path) as f:
        lines = [ln.strip() for ln in f]
    lines = [ln for ln in lines if ln and not ln.startswith("#")]
    if not lines:
        raise ValueError("%s: no header line" % path)
    return lines[0].split(), [ln.split() for ln in lines[1:]]


def read_scenario(path):
    """A TSV with the header `bin birth death` and one row per unit bin (bin 0, 1, ...) -> [2, n_bins]"""
    head, rows = _table(path)
    if head != ["bin", "birth", "death"]:
        raise ValueError("%s: the header must be `bin birth death`, not `%s`" % (path, " ".join(head)))
    birth, death = [], []
    for i, r in enumerate(rows):
        try:
            if len(r) != 3:
                raise ValueError
            b, lam, mu = int(r[0]), float(r[1]), float(r[2])
        except ValueError:
            raise ValueError("%s: row %d is not `bin birth death` (an integer and two numbers)" % (path, i)) from None
        if b != i:
            raise ValueError("%s: row %d names bin %d; the rows are the unit bins 0, 1, ... in order" % (path, i, b))
        birth.append(lam), death.append(mu)
    return check_scenario(birth, death, path)


def scenario_from_rtt(path):
    """The posterior mean birth and death rates of a finished run's <stem>_RTT.tsv as the scenario -> [2, n_bins]"""
    head, rows = _table(path)
    if "birth_rate" not in head or "death_rate" not in head:
        raise ValueError("%s: no birth_rate and death_rate columns; --from_rtt takes a <stem>_RTT.tsv" % path)
    ib, idd = head.index("birth_rate"), head.index("death_rate")
    try:
        birth, death = [float(r[ib]) for r in rows], [float(r[idd]) for r in rows]
    except (ValueError, IndexError):
        raise ValueError("%s: a row does not hold a number in its birth_rate or death_rate column" % path) from None
    return check_scenario(birth, death, path)


# ---- simulated replicates -----------------------------------------------------------------------------------------------------
def simulate(scenario, n_reps, steps_per_bin=100, n_start=100, seed=0, capacity=None):
    """n_reps simulations of the scenario in one launch -> (counts [n_reps, 4, n_bins], totals [n_reps, 4]) as host int64
    (ops.simulate_bd_batch: replicate r is the stream seed + r)"""
    from . import ops
    lam = np.repeat(scenario[0][None], int(n_reps), axis=0)
    mu = np.repeat(scenario[1][None], int(n_reps), axis=0)
    counts, totals = ops.simulate_bd_batch(lam, mu, int(steps_per_bin), int(n_start), int(seed), capacity)
    return counts.cpu().numpy(), totals.cpu().numpy()


def keep_replicates(counts, totals, min_lineages=0, max_lineages=None):
    """Which simulated replicates reach the sampler -> reason int [n_reps], an index into REASONS (0 = kept).  Dropped, by
    the first rule that applies: its overflow flag is set; it went extinct (totals[:, 3] != -1); a bin without lineage-steps;
    its created lineages outside [min_lineages, max_lineages]."""
    counts, totals = np.asarray(counts), np.asarray(totals)
    reason = np.zeros(totals.shape[0], dtype=np.int64)
    rules = [(totals[:, 2] != 0, 1), (totals[:, 3] != -1, 2), ((counts[:, 3] <= 0).any(axis=1), 3),
             ((totals[:, 0] < min_lineages) | ((totals[:, 0] > max_lineages) if max_lineages is not None else False), 4)]
    for hit, code in rules:
        reason[(reason == 0) & hit] = code
    return reason


def statistics(counts, steps_per_bin):
    """(sp, ex, br) [R, n_bins] float64 of simulated counts: births (founders are not births), deaths, and the lineage-steps
    in time units"""
    counts = np.asarray(counts)
    return counts[:, 0].astype(np.float64), counts[:, 1].astype(np.float64), counts[:, 3].astype(np.float64) / float(steps_per_bin)


def end_time(n_bins):
    """where the command line's death jitter leaves a real data set: a span that is not integer valued, as the summary
    requires, so the RTT bins are exactly the scenario's unit bins"""
    return float(n_bins) + 0.5


# ---- the score's host side ------------------------------------------------------------------------------------------------------
def truth_kinds(scenario):
    """[3, n_bins]: birth, death, net = birth - death"""
    return np.stack([scenario[0], scenario[1], scenario[0] - scenario[1]])


def empirical_score(sp, ex, br, scenario):
    """[3, n_bins, 6]: lr_rtt_score's columns for the raw estimates sp / br, ex / br and their difference; no band, so
    coverage and width are NaN"""
    with np.errstate(all="ignore"):
        est = np.stack([sp / br, ex / br, sp / br - ex / br], axis=1)          # [R, 3, n_bins]
    err = est - truth_kinds(scenario)[None]
    out = np.full((3, scenario.shape[1], 6), np.nan)
    out[:, :, 0] = est.shape[0]
    out[:, :, 2], out[:, :, 3], out[:, :, 4] = err.mean(axis=0), np.abs(err).mean(axis=0), np.sqrt((err * err).mean(axis=0))
    return out


def true_shifts(scenario):
    """[per kind (birth, death)] the bins i >= 1 whose rate differs from bin i - 1's"""
    return [np.flatnonzero(scenario[k][1:] != scenario[k][:-1]) + 1 for k in range(2)]


def shifts(shift_freq, k_counts, scenario, prior, bf=6.0, tol=2):
    """Power, false positives and K recovery from shift_freq [G, 2, n_bins], k_counts [G, 2, LR_KMAX] and the prior frequency
    of a shift in a bin (a number, or [n_bins]) -> dict:
      reported [G, 2, n_bins] bool: 2 ln BF of the replicate's frequency against the prior exceeds bf;
      true_bins [2] arrays; ratio, power [2] arrays beside them: the rate ratio at a true shift and the share of replicates
        that report a shift of its kind within tol bins of it;
      false_positive [2]: the share of replicates that report a shift farther than tol from every true one;
      k_true, k_mode_share, k_mean [2]: the true number of rates, the share of replicates whose posterior mode of K equals
        it, the mean over replicates of the posterior mean of K;  k_mode [G, 2]."""
    from . import shift_bf
    f = np.asarray(shift_freq, dtype=np.float64)
    G, _, nb = f.shape
    two = shift_bf.two_ln_bf(f, np.broadcast_to(np.asarray(prior, dtype=np.float64), (nb,))[None, None, :])
    with np.errstate(invalid="ignore"):
        reported = two > bf
    bins = np.arange(nb)
    tb = true_shifts(scenario)
    ratio, power, fp = [], [], np.zeros(2)
    for k in range(2):
        with np.errstate(all="ignore"):
            ratio.append(scenario[k][tb[k]] / scenario[k][tb[k] - 1])
        power.append(np.array([reported[:, k, np.abs(bins - i) <= tol].any(axis=1).mean() for i in tb[k]]))
        far = np.ones(nb, dtype=bool)
        for i in tb[k]:
            far &= np.abs(bins - i) > tol
        fp[k] = reported[:, k, far].any(axis=1).mean() if far.any() else 0.0
    kc = np.asarray(k_counts, dtype=np.float64)
    k_mode = kc.argmax(axis=2) + 1
    k_true = np.array([len(tb[0]) + 1, len(tb[1]) + 1])
    k_post_mean = (kc * np.arange(1, kc.shape[2] + 1)).sum(axis=2) / kc.sum(axis=2)
    return dict(reported=reported, two_ln_bf=two, true_bins=tb, ratio=ratio, power=power, false_positive=fp, k_true=k_true,
                k_mode=k_mode, k_mode_share=(k_mode == k_true[None]).mean(axis=0), k_mean=k_post_mean.mean(axis=0))


class Result:
    """What run() returns: the scenario [2, n_bins] and settings (a dict); counts, totals, reason, seeds of every simulated
    replicate; kept (their indices); sp, ex, br of the kept ones; time; rates [G, 3, 3, n_bins], shift_freq, k_counts, covered
    and score [3, n_bins, 6] (host copies of ops.rtt_score's; G = the kept replicates); empirical [3, n_bins, 6]; prior_s and
    shifts (shifts()'s dict); seconds per step; trace (the device tensor, while keep_trace) and n_samples."""

    def arrays(self):
        """every array of the study, by name (what STEM_SIM.npz holds)"""
        s = self.shifts
        out = dict(scenario=self.scenario, counts=self.counts, totals=self.totals, reason=self.reason, seeds=self.seeds,
                   kept=self.kept, sp=self.sp, ex=self.ex, br=self.br, time=self.time, rates=self.rates, shift_freq=self.shift_freq,
                   k_counts=self.k_counts, covered=self.covered, score=self.score, empirical=self.empirical,
                   prior_s=np.float64(self.prior_s), reported=s["reported"], false_positive=s["false_positive"], k_true=s["k_true"],
                   k_mode=s["k_mode"], k_mode_share=s["k_mode_share"], k_mean=s["k_mean"])
        for k in range(2):
            for name in ("true_bins", "ratio", "power"):
                out["%s_%s" % (KINDS[k], name)] = np.asarray(s[name][k])
        for key, v in self.settings.items():
            out["setting_" + key] = np.asarray(-1 if v is None else v)
        return out


def run(scenario, n_reps, chains_per_rep=1, n_iter=200000, s_freq=200, seed=1, steps_per_bin=100, n_start=100, capacity=None,
        min_lineages=0, max_lineages=None, use_rate_HP=1, poisson_prior=0.0, update_fraction=0.75, block=0, burnin=0.2, bf=6.0,
        bf_reps=1 << 20, tol=2, keep_trace=False, verbose=False):
    """The whole study (the module's docstring) -> Result.  scenario: [2, n_bins] or a path read_scenario takes."""
    import torch
    from . import _hip, ops, shift_bf
    from .replicates import ReplicateEngine, Replicates
    sc = read_scenario(scenario) if isinstance(scenario, str) else check_scenario(scenario[0], scenario[1])
    nb = sc.shape[1]
    n_reps, cpr, n_iter, s_freq = int(n_reps), int(chains_per_rep), int(n_iter), int(s_freq)
    if n_reps < 2 or cpr < 1 or n_iter < 1 or s_freq < 1:
        raise ValueError("a study needs at least 2 replicates, 1 chain each, 1 iteration and a sampling frequency of 1")
    S = (n_iter + s_freq - 1) // s_freq
    n_group = cpr * (S - int(burnin * S))
    if not 0.0 <= burnin < 1.0 or n_group > _hip.LR_SCORE_MAX_SAMPLES or n_group < 2:
        raise ValueError("%d chains x %d samples after a burn-in of %g: a replicate is scored on 2 to %d samples (the study's "
                         "chains are short on purpose: raise -s)" % (cpr, S - int(burnin * S) if 0.0 <= burnin < 1.0 else 0, burnin,
                                                                      _hip.LR_SCORE_MAX_SAMPLES))
    res = Result()
    res.scenario, res.seconds = sc, {}
    res.settings = dict(n_reps=n_reps, chains_per_rep=cpr, n_iter=n_iter, s_freq=s_freq, seed=int(seed), steps_per_bin=int(steps_per_bin),
                        n_start=int(n_start), capacity=capacity, min_lineages=int(min_lineages), max_lineages=max_lineages,
                        use_rate_HP=int(use_rate_HP), poisson_prior=float(poisson_prior), update_fraction=float(update_fraction),
                        burnin=float(burnin), bf=float(bf), bf_reps=int(bf_reps), tol=int(tol))

    def lap(name, t):
        torch.cuda.synchronize()
        res.seconds[name] = time.time() - t
        if verbose:
            print("%-9s %.3f s" % (name, res.seconds[name]))
        return time.time()

    t = time.time()
    res.counts, res.totals = simulate(sc, n_reps, steps_per_bin, n_start, seed, capacity)
    res.seeds = int(seed) + np.arange(n_reps, dtype=np.int64)
    res.reason = keep_replicates(res.counts, res.totals, min_lineages, max_lineages)
    res.kept = np.flatnonzero(res.reason == 0)
    if res.kept.size < 2:
        raise ValueError("%d of %d simulated replicates can be sampled (%s): a study needs 2; raise --n_start or the rates" %
                         (res.kept.size, n_reps, ", ".join("%d %s" % ((res.reason == c).sum(), REASONS[c]) for c in range(1, 5))))
    res.sp, res.ex, res.br = statistics(res.counts[res.kept], steps_per_bin)
    t = lap("simulate", t)

    G, end = int(res.kept.size), end_time(nb)
    reps = Replicates.from_counts(res.sp, res.ex, res.br, 0.0, end, paths=["replicate%d" % r for r in res.kept])
    eng = ReplicateEngine(reps, G * cpr, model=0, seed=int(seed), use_rate_HP=int(use_rate_HP), poisson_HP=float(poisson_prior),
                          update_fraction=float(update_fraction), s_freq=s_freq, n_trace_slots=S)
    eng.init()
    done, block = 0, int(block) if int(block) > 0 else n_iter
    while done < n_iter:
        eng.steps(min(block, n_iter - done))
        done += min(block, n_iter - done)
    eng.check_status()
    res.warning = eng.warning_text()
    t = lap("sample", t)

    truth = torch.as_tensor(sc, device=eng.trace.device)
    out = ops.rtt_score(eng.trace, S, cpr, 0.0, end, truth=truth, burnin=burnin)
    res.time, res.n_samples = out.time, out.n_samples
    res.rates, res.shift_freq, res.k_counts, res.covered, res.score = [x.cpu().numpy() for x in
                                                                        (out.rates, out.shift_freq, out.k_counts, out.covered, out.score)]
    res.empirical = empirical_score(res.sp, res.ex, res.br, sc)
    t = lap("score", t)

    lam = float(poisson_prior) if poisson_prior > 0 else None
    prior = ops.shift_prior(0.0, end, n_reps=int(bf_reps), seed=int(seed), poi_lambda=lam)
    res.prior_s = shift_bf.prior_s(prior.shift_hist.cpu().numpy(), int(prior.totals[0].item()))
    res.shifts = shifts(res.shift_freq, res.k_counts, sc, res.prior_s, bf, tol)
    lap("shifts", t)
    res.trace = eng.trace if keep_trace else None
    if not keep_trace:
        eng.close()
    return res


# ---- files ----------------------------------------------------------------------------------------------------------------------
def _num(v):
    return str(float(v))


def rates_table(res):
    """STEM_SIM_rates.tsv as text: kind, bin, truth, the six score columns, the four empirical ones"""
    tk = truth_kinds(res.scenario)
    lines = ["\t".join(["kind", "bin", "truth"] + SCORE_HEAD + EMP_HEAD)]
    for k in range(3):
        for i in range(res.scenario.shape[1]):
            emp = res.empirical[k, i]
            lines.append("\t".join([KINDS[k], str(i), _num(tk[k, i])] + [_num(v) for v in res.score[k, i]] +
                                   [_num(emp[0]), _num(emp[2]), _num(emp[3]), _num(emp[4])]))
    return "\n".join(lines) + "\n"


def shifts_table(res):
    """STEM_SIM_shifts.tsv as text, one table in long format, `kind bin quantity value`: per true shift (its kind and bin) the
    rate ratio and the power; then per kind, bin NA, the false-positive rate and the K rows (k_true, k_mode_share, k_mean)"""
    s = res.shifts
    lines = ["kind\tbin\tquantity\tvalue"]
    for k in range(2):
        for i, r, p in zip(s["true_bins"][k], s["ratio"][k], s["power"][k]):
            lines.append("%s\t%d\tratio\t%s" % (KINDS[k], i, _num(r)))
            lines.append("%s\t%d\tpower\t%s" % (KINDS[k], i, _num(p)))
    for k in range(2):
        for name, v in (("false_positive", s["false_positive"][k]), ("k_true", s["k_true"][k]), ("k_mode_share", s["k_mode_share"][k]),
                        ("k_mean", s["k_mean"][k])):
            lines.append("%s\tNA\t%s\t%s" % (KINDS[k], name, _num(v)))
    return "\n".join(lines) + "\n"


def replicates_table(res):
    """STEM_SIM_replicates.tsv as text: per simulated replicate its seed, lineages created, living at the end, kept or the
    reason it was dropped, and its modes of K_l and K_m (NA when dropped)"""
    where = {int(r): g for g, r in enumerate(res.kept)}
    lines = ["replicate\tseed\tlineages\tliving\tstatus\tK_l_mode\tK_m_mode"]
    for r in range(res.totals.shape[0]):
        g = where.get(r)
        km = ["NA", "NA"] if g is None else [str(int(v)) for v in res.shifts["k_mode"][g]]
        lines.append("\t".join([str(r), str(int(res.seeds[r])), str(int(res.totals[r, 0])), str(int(res.totals[r, 1])),
                                REASONS[int(res.reason[r])]] + km))
    return "\n".join(lines) + "\n"


def write_files(res, stem):
    for suffix, text in (("_SIM_rates.tsv", rates_table(res)), ("_SIM_shifts.tsv", shifts_table(res)),
                         ("_SIM_replicates.tsv", replicates_table(res))):
        with open(stem + suffix, "w") as f:
            f.write(text)
    np.savez(stem + "_SIM.npz", **res.arrays())
    return [stem + s for s in ("_SIM_rates.tsv", "_SIM_shifts.tsv", "_SIM_replicates.tsv", "_SIM.npz")]


def parser():
    p = argparse.ArgumentParser(prog="python -m literate_amd.simstudy", description="Simulate many data sets under known rates, "
                                "run the RJ sampler on all of them in one launch and score what it recovers")
    p.add_argument("scenario", nargs="?", default="", help="TSV `bin birth death`, one row per unit bin (2 to 512)")
    p.add_argument("--from_rtt", default="", metavar="RTT", help="take the scenario from a finished run's <stem>_RTT.tsv")
    p.add_argument("--replicates", type=int, default=256)
    p.add_argument("--chains_per_rep", type=int, default=1)
    p.add_argument("-n", type=int, default=200000, help="MCMC iterations")
    p.add_argument("-s", type=int, default=200, help="sampling frequency")
    p.add_argument("-seed", type=int, default=1)
    p.add_argument("-use_rate_HP", type=int, default=1)
    p.add_argument("-Poisson_prior", type=float, default=0.0)
    p.add_argument("-update_fraction", type=float, default=0.75)
    p.add_argument("--block", type=int, default=0, help="iterations per launch (0: all in one)")
    p.add_argument("--steps_per_bin", type=int, default=100)
    p.add_argument("--n_start", type=int, default=100)
    p.add_argument("--capacity", type=int, default=0, help="most lineages a replicate may create (0: the simulator's default)")
    p.add_argument("--min_lineages", type=int, default=0)
    p.add_argument("--max_lineages", type=int, default=0, help="0: the capacity")
    p.add_argument("--burnin", type=float, default=0.2)
    p.add_argument("--bf", type=float, default=6.0, help="2 ln BF above which a replicate reports a shift")
    p.add_argument("--bf_reps", type=int, default=1 << 20)
    p.add_argument("--tol", type=int, default=2, help="bins between a reported and a true shift that still count as found")
    p.add_argument("--out", default="study", metavar="STEM")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    if bool(args.scenario) == bool(args.from_rtt):
        raise SystemExit("name the scenario: a TSV file, or --from_rtt <stem>_RTT.tsv (not both)")
    try:
        sc = scenario_from_rtt(args.from_rtt) if args.from_rtt else read_scenario(args.scenario)
        res = run(sc, args.replicates, args.chains_per_rep, args.n, args.s, args.seed, args.steps_per_bin, args.n_start,
                  args.capacity or None, args.min_lineages, args.max_lineages or None, args.use_rate_HP, args.Poisson_prior,
                  args.update_fraction, args.block, args.burnin, args.bf, args.bf_reps, args.tol, verbose=True)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e))
    if res.warning:
        print(res.warning, file=sys.stderr)
    t = time.time()
    files = write_files(res, args.out)
    print("%-9s %.3f s" % ("files", time.time() - t))
    print("%d of %d replicates sampled, %d chains each, %d samples per replicate; birth coverage %.3f, death coverage %.3f" %
          (res.kept.size, args.replicates, args.chains_per_rep, res.n_samples, res.score[0, :, 1].mean(), res.score[1, :, 1].mean()))
    print("\n".join(files))


if __name__ == "__main__":
    main()
