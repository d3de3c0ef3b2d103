"""Trait-dependent rates: the host side of LiteTraitRate.py (the reference's other/LiteTraitRate.py, rebuilt on the GPU).

Every lineage carries one static real trait x; its birth rate is the RJ skyline's lambda(t) times s^L(x) = 1 / (1 + exp(-kappa_l
(x - x0_l))), its death rate mu(t) s^M(x) (transform_rate_logistic).  ops.TraitEngine alternates lr_rjbin's iteration on the
trait-weighted bin statistics with a trait move every --trait_every iterations (include/literate_hip_trait.h); this module
reads and matches the trait file, tunes the trait windows during the burn-in, writes the reference's three logs and
summarises the effect of the trait from the rows resident on the device.

The windows of the trait move are tuned per side between blocks of the first --trait_tune of the run, on the acceptance pooled
over the chains: win <- clip(win exp(4 (rate - 0.3) / sqrt(b)), win / 1000, 1000 win) after block b (trend_mlik's rule, towards
30 %); both windows of a side take the same factor.  Afterwards they are frozen, and only rows sampled after the tuning phase
enter the summary.

The mcmc log has the reference's header (LiteTraitRate.py:637).  The reference keeps one Gamma rate for both processes, this
sampler one each, as runMCMC does: the column gamma_rate_hp holds the birth process's.
"""
import math
import os
import sys

import numpy as np

TRAIT_MCMC_HEAD = ["it", "posterior", "likelihood", "prior", "lambda_avg", "mu_avg", "K_l", "K_m", "x0_l", "kappa_l", "x0_m", "kappa_m",
                   "root_age", "death_age", "gamma_rate_hp", "poisson_rate_hp"]
EFFECT_HEAD = ["parameter", "mean", "minHPD", "maxHPD", "ess_pooled", "ess_min", "rhat", "P_gt_0", "accept_rate", "win_final"]
CURVE_HEAD = ["trait", "trait_raw", "sL_mean", "sL_minHPD", "sL_maxHPD", "sM_mean", "sM_minHPD", "sM_maxHPD"]
PARAMS = ("x0_l", "kappa_l", "x0_m", "kappa_m")
TUNE_TARGET, TUNE_GAIN, TUNE_BLOCKS = 0.3, 4.0, 20
REFUSED = {"replicates": "--replicates: one data set per launch - every replicate would need its own trait-weighted statistics",
           "mc3": "--mc3: the heated chains would need a tempered trait move, which is not built",
           "ppc": "--ppc: the predictive simulator draws lineages without traits",
           "ppc_age": "--ppc_age: the lifespan check assumes one death rate for all lineages of a bin",
           "ade": "--ade: the age-dependent fit assumes one death rate for all lineages of a bin",
           "ade_joint": "--ade_joint: the joint sampler has no trait multiplier",
           "waic": "--waic: the pointwise scorer has no trait multiplier",
           "loo": "--loo: the pointwise scorer has no trait multiplier"}


def read_traits(path):
    """-trait_data FILE: tab-separated, a header row, then `lineage_name value` rows -> {name: value}.  A duplicate name or a
    value that is not a finite number is refused by name."""
    out = {}
    with open(path) as f:
        lines = f.read().splitlines()
    for ln, line in enumerate(lines[1:], start=2):
        if not line.strip():
            continue
        cells = line.split("\t")
        if len(cells) < 2:
            raise ValueError("%s line %d: expected `lineage_name<TAB>value`" % (path, ln))
        name = cells[0].strip()
        try:
            v = float(cells[1])
        except ValueError:
            v = float("nan")
        if not math.isfinite(v):
            raise ValueError("%s: the trait of lineage %r is not a finite number (%r)" % (path, name, cells[1].strip()))
        if name in out:
            raise ValueError("%s: lineage %r has more than one trait value" % (path, name))
        out[name] = v
    return out


def kept_names(input_file, TBP, first_year, last_year):
    """The names (first column) of the lineages parse_ts_te keeps, in its order: the same window filters on the same table."""
    import pandas as pd
    table = pd.read_csv(input_file, delimiter='\t').to_numpy()
    names = np.array([str(v) for v in table[:, 0]])
    born = table[:, 2] if table.shape[1] == 4 else table[:, 1]
    not_later = (lambda a, b: a >= b) if TBP else (lambda a, b: a <= b)
    if first_year != -1:
        inside = not_later(first_year, born)
        names, born = names[inside], born[inside]
    if last_year != -1:
        inside = not_later(born, last_year)
        names, born = names[inside], born[inside]
    return [str(n) for n in names]


def match_traits(names, traits):
    """the trait of every kept lineage, in the data's order; a lineage without a value is refused by name (values of lineages
    the data do not hold - those parse_ts_te dropped among them - are ignored)"""
    missing = [n for n in names if n not in traits]
    if missing:
        raise ValueError("no trait value for lineage %r%s" % (missing[0], " (and %d more)" % (len(missing) - 1) if len(missing) > 1 else ""))
    return np.array([traits[n] for n in names], dtype=float)


def standardise(x, raw=False):
    """-> (x', mean, sd): mean 0 and sd 1 unless raw (then x, 0, 1); a constant trait is refused"""
    x = np.asarray(x, dtype=float)
    if raw:
        return x, 0.0, 1.0
    m, sd = float(x.mean()), float(x.std())
    if not sd > 0.0:
        raise ValueError("the trait is the same for every lineage: nothing to estimate")
    return (x - m) / sd, m, sd


def x0_range(x):
    """the support of the uniform prior on x0: the observed range widened by a tenth of its span on each side"""
    lo, hi = float(np.min(x)), float(np.max(x))
    return lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo)


def arg_error(args, world=1):
    """Why LiteTraitRate.py cannot run these flags (None when it can); every refusal names its flag and its reason."""
    if args.model_BDI != 2:
        return ("-model_BDI %d: only the Keiding likelihood (-model_BDI 2) is built with trait-dependent rates - the trait-weighted "
                "exposures WL, WM replace its br_length, which the other likelihoods use as a count of lineages" % args.model_BDI)
    if world > 1:
        return "several ranks: the trait sampler runs all its chains on one device"
    for flag, why in REFUSED.items():
        v = getattr(args, flag)
        if (flag == "replicates" and v) or (flag == "mc3" and v != 1) or (flag not in ("replicates", "mc3") and v != -1.0):
            return why
    if not args.trait_data:
        return "-trait_data FILE is required: a tab-separated file with a header row and `lineage_name value` rows"
    if args.chains < 1 or args.trait_every < 0 or args.trait_win_x0 <= 0 or args.trait_win_kappa <= 0:
        return "--chains must be at least 1, --trait_every at least 0 and the trait windows positive"
    if not (0.0 <= args.trait_tune < 1.0):
        return "--trait_tune takes a fraction of -n in [0, 1)"
    for flag in ("rtt", "ess"):
        v = getattr(args, flag)
        if v != -1.0 and not (0.0 <= v < 1.0):
            return "--%s takes a burn-in fraction in [0, 1)" % flag
    return None


def tuned(win, rate, b):
    """the window after tuning block b (1-based) at acceptance `rate` (nan: no proposal in the block - unchanged)"""
    if not math.isfinite(rate):
        return win
    return win * math.exp(TUNE_GAIN * (rate - TUNE_TARGET) / math.sqrt(b))


def log_paths(data_file, out="", chain=None):
    out_dir = "%s/literate_mcmc_logs" % (os.path.dirname(data_file) or os.getcwd())
    stem = os.path.splitext(os.path.basename(data_file))[0] + out
    if chain is not None:
        stem += "_c%d" % chain
    return out_dir, {k: "%s/%s_trait_%s.log" % (out_dir, stem, k) for k in ("mcmc", "sp_rates", "ex_rates")}, "%s/%s" % (out_dir, stem)


def header_lines(mean, sd, raw, n, x_lo, x_hi):
    return ["# trait: %d lineages, %s; mean %r, sd %r; x0 uniform on [%r, %r]" %
            (n, "as given (-trait_raw)" if raw else "standardised", mean, sd, x_lo, x_hi)]


class TraitLogWriter:
    """The three logs of every chain in the reference's format (LiteTraitRate.py:635-641), appended and flushed per block."""

    def __init__(self, data_file, out, n_chains, comments=()):
        self.paths = [log_paths(data_file, out, None if n_chains == 1 else c)[1] for c in range(n_chains)]
        for p in self.paths:
            with open(p["mcmc"], "w") as f:
                for c in comments:
                    f.write(c + "\n")
                f.write("\t".join(TRAIT_MCMC_HEAD) + "\n")
            open(p["sp_rates"], "w").close()
            open(p["ex_rates"], "w").close()

    def append(self, rows):
        """rows [samples, chains, LR_TRAIT_ROW_W] (host)"""
        from . import _hip
        from .logs import split_row
        TW = _hip.LR_TRACE_W
        for c, p in enumerate(self.paths):
            lm, ls, le = [], [], []
            for r in rows[:, c]:
                head, sp_row, ex_row = split_row(r[:TW])
                vals = [str(int(head[0]))] + [str(float(v)) for v in head[1:6]] + [str(int(head[6])), str(int(head[7]))]
                vals += [str(float(v)) for v in r[TW:TW + 4]] + [str(float(head[8])), str(float(head[9])), str(float(head[10])), str(float(head[12]))]
                lm.append("\t".join(vals) + "\n")
                ls.append("\t".join(str(float(v)) for v in sp_row) + "\n")
                le.append("\t".join(str(float(v)) for v in ex_row) + "\n")
            for key, lines in (("mcmc", lm), ("sp_rates", ls), ("ex_rates", le)):
                with open(p[key], "a") as f:
                    f.writelines(lines)


def hpd(v, level=0.95):
    """calcHPD: the shortest interval holding `level` of the sample"""
    v = np.sort(np.asarray(v, dtype=float))
    n_in = int(round(level * len(v)))
    if n_in < 2:
        return float("nan"), float("nan")
    w = v[n_in - 1:] - v[:len(v) - n_in + 1]
    i = int(np.argmin(w))
    return float(v[i]), float(v[i + n_in - 1])


def write_effect(stem, eng, first_row, accept, wins, x_mean, x_sd, x_std):
    """<stem>_trait_effect.tsv and <stem>_trait_curves.tsv from the rows resident on the device, those before `first_row` (the
    tuning phase) left out: lr_col_summary pooled (mean, 95 % HPD) and lr_ess_summary (ESS, split R-hat) of the four
    parameters, P(kappa > 0), the acceptance of the trait moves after tuning and the final windows per side; then the
    multiplier curves s^L(x), s^M(x) on 101 points over the observed trait range (mean and 95 % band over the pooled draws; host)."""
    from . import _hip, ops
    S = eng.samples_done()
    rows = eng.trace[first_row:S]
    n = S - first_row
    cols = [_hip.LR_TRACE_W + j for j in range(4)]
    cs = ops.col_summary(rows, n, cols, burnin=0.0, pooled=True)
    mean, lo, hi = [t[0].cpu().numpy() for t in (cs.mean, cs.lo, cs.hi)]
    if n >= 4:
        es = ops.ess_summary(rows, n, cols, burnin=0.0)
        ess_p, ess_min, rhat = es.pooled_ess.cpu().numpy(), np.nanmin(es.ess.cpu().numpy(), axis=0), es.rhat.cpu().numpy()
    else:
        ess_p = ess_min = rhat = np.full(4, np.nan)
    draws = rows[:, :, _hip.LR_TRACE_W:_hip.LR_TRACE_W + 4].reshape(-1, 4).cpu().numpy()
    with open(stem + "_trait_effect.tsv", "w") as f:
        f.write("\t".join(EFFECT_HEAD) + "\n")
        for j, name in enumerate(PARAMS):
            side = j // 2
            p_gt = str(float((draws[:, j] > 0).mean())) if j & 1 else "nan"
            win = wins[0][side] if j % 2 == 0 else wins[1][side]
            f.write("\t".join([name] + [str(float(v)) for v in (mean[j], lo[j], hi[j], ess_p[j], ess_min[j], rhat[j])] +
                              [p_gt, str(float(accept[side])), str(float(win))]) + "\n")
    grid = np.linspace(float(np.min(x_std)), float(np.max(x_std)), 101)
    with np.errstate(over="ignore"):
        sL = 1.0 / (1.0 + np.exp(-draws[:, 1][:, None] * (grid[None, :] - draws[:, 0][:, None])))
        sM = 1.0 / (1.0 + np.exp(-draws[:, 3][:, None] * (grid[None, :] - draws[:, 2][:, None])))
    with open(stem + "_trait_curves.tsv", "w") as f:
        f.write("\t".join(CURVE_HEAD) + "\n")
        for i, g in enumerate(grid):
            (l0, l1), (m0, m1) = hpd(sL[:, i]), hpd(sM[:, i])
            f.write("\t".join(str(float(v)) for v in (g, g * x_sd + x_mean, sL[:, i].mean(), l0, l1, sM[:, i].mean(), m0, m1)) + "\n")
    return dict(zip(PARAMS, mean))


def run(args):
    """LiteTraitRate.py after its argument checks"""
    import time
    import torch
    from . import _hip, logs, ops
    from .literate_library import parse_ts_te
    rseed = np.random.randint(0, 9999) if args.seed == -1 else args.seed
    ts, te, _, _ = parse_ts_te(args.d, args.TBP, args.first_year, args.last_year, args.death_jitter)
    ts, te = np.asarray(ts, dtype=float), np.asarray(te, dtype=float)
    names = kept_names(args.d, args.TBP, args.first_year, args.last_year)
    if len(names) != len(ts):
        raise SystemExit("the names of %s do not line up with its lineages (%d names, %d lineages)" % (args.d, len(names), len(ts)))
    try:
        x_raw = match_traits(names, read_traits(args.trait_data))
        x, x_mean, x_sd = standardise(x_raw, args.trait_raw)
    except ValueError as e:
        raise SystemExit("-trait_data: %s" % e)
    lo, hi = x0_range(x)
    n_samples = (args.n + args.s - 1) // args.s if args.n > 0 else 0
    wins = [[args.trait_win_x0] * 2, [args.trait_win_kappa] * 2]
    settings = ops.TraitSettings(args.const_rates, args.const_death_rate, args.use_rate_HP, args.Poisson_prior, args.update_fraction,
                                 args.trait_every, tuple(wins[0]), tuple(wins[1]), lo, hi)
    n_bins = int(np.ceil(te.max()) - np.floor(ts.min()))          # TraitEngine's own window, checked before anything is uploaded
    if n_bins < 1 or n_bins > _hip.LR_RJBIN_MAX_BINS:
        raise SystemExit("%d unit time bins: the trait sampler holds 1 to %d" % (n_bins, _hip.LR_RJBIN_MAX_BINS))
    eng = ops.TraitEngine(ts, te, x, args.chains, seed=rseed, settings=settings, s_freq=args.s, n_trace_slots=n_samples)
    out_dir, _, stem = log_paths(args.d, args.out)
    os.makedirs(out_dir, exist_ok=True)
    comments = header_lines(x_mean, x_sd, args.trait_raw, len(x), lo, hi)
    print(comments[0][2:])
    writer = TraitLogWriter(args.d, args.out, args.chains, comments) if n_samples else None
    eng.init()
    block = args.block if args.block > 0 else args.p * max(1, 50000 // max(args.p, 1))
    tune_end = int(args.trait_tune * args.n) if args.trait_every > 0 else 0
    tune_block = max(-(-tune_end // TUNE_BLOCKS), 1)
    done, b, written = 0, 0, 0
    prop0, acc0 = eng.trait_counts()
    t_start = time.time()
    while done < args.n:
        # the tuning phase runs in (at most) TUNE_BLOCKS shorter blocks, one window update after each
        n = min(tune_block, tune_end - done) if done < tune_end else min(block, args.n - done)
        eng.steps(n)
        done += n
        S = eng.samples_done()
        if writer is not None and S > written:
            writer.append(eng.trace[written:S].cpu().numpy())
            written = S
        prop, acc = eng.trait_counts()
        if done <= tune_end:
            b += 1
            dp, da = (prop - prop0).sum(axis=0), (acc - acc0).sum(axis=0)
            for side in range(2):
                f = tuned(1.0, da[side] / dp[side] if dp[side] > 0 else float("nan"), b)
                f = min(max(f, 1e-3 * args.trait_win_x0 / wins[0][side]), 1e3 * args.trait_win_x0 / wins[0][side])
                wins[0][side], wins[1][side] = wins[0][side] * f, wins[1][side] * f
            eng.set_windows(wins[0], wins[1])
            prop0, acc0 = prop, acc                      # (after the last tuning block: the counts the acceptance is taken from)
        print(done, "windows x0 %s kappa %s" % (wins[0], wins[1]))
        sys.stdout.flush()
    torch.cuda.synchronize()
    el = time.time() - t_start
    if args.n > 0:
        print("%d iterations x %d chains in %.2f s (%.0f iterations/s/chain)" % (args.n, args.chains, el, args.n / max(el, 1e-9)))
    if eng.warnings() & _hip.LR_WARN_KCAP:
        print("warning: an add-shift move was proposed from %d rates and rejected (the device's cap)" % _hip.LR_KMAX, file=sys.stderr)
    if n_samples:
        first = min((tune_end + args.s - 1) // args.s, n_samples)
        if n_samples - first >= 2:
            prop, acc = eng.trait_counts()
            dp, da = (prop - prop0).sum(axis=0), (acc - acc0).sum(axis=0)
            with np.errstate(all="ignore"):
                rate = np.where(dp > 0, da / np.maximum(dp, 1), np.nan)
            means = write_effect(stem, eng, first, rate, wins, x_mean, x_sd, x)
            print("trait effect: %s_trait_effect.tsv, %s_trait_curves.tsv (%d samples per chain after the tuning phase): %s" %
                  (stem, stem, n_samples - first, ", ".join("%s %.4g" % kv for kv in means.items())))
        base = eng.trace[:, :, :_hip.LR_TRACE_W].contiguous()
        if args.rtt != -1.0:
            burn = max(int(args.rtt * n_samples), first)
            res = ops.rtt_summary(base[burn:], n_samples - burn, eng.start_time, eng.end_time, burnin=0.0, pooled=True)
            logs.write_rtt_tables(stem + "_trait", res.time, res.rates[0].cpu().numpy(), res.shift_freq[0].cpu().numpy(),
                                  res.k_counts[0].cpu().numpy())
            print("baseline rates through time - the rates of a lineage at multiplier s = 1, i.e. the skylines lambda(t), mu(t) "
                  "themselves, not the rates of an average lineage: %s_trait_RTT.tsv, %s_trait_RTT_K.tsv" % (stem, stem))
        if args.ess != -1.0:
            head = logs.MCMC_HEAD[:_hip.LR_TRACE_HEAD] + [""] * (_hip.LR_TRACE_W - _hip.LR_TRACE_HEAD) + list(PARAMS)
            cols = [1, 2, 3, 4, 5, 6, 7, 10, 11, 12] + [_hip.LR_TRACE_W + j for j in range(4)]
            burn = max(int(args.ess * n_samples), first)          # as --rtt: the tuning phase changes the windows and is left out
            if n_samples - burn < 4:
                print("--ess: %d samples per chain after the burn-in and the tuning phase; the summary needs at least 4" % (n_samples - burn))
            else:
                res = ops.ess_summary(eng.trace[burn:].contiguous(), n_samples - burn, cols, burnin=0.0)
                host = res._replace(**{k: getattr(res, k).cpu().numpy() for k in res._fields if k != "n"})
                print(logs.write_ess_tables(stem + "_trait", [head[c] for c in cols], host, args.s))
    eng.close()
