"""The joint covariate model: the host side of MultiTrendRate.py.

trend_rate.py asks of one column of the trend file at a time whether it drives the rates.  Here every rate is log-linear in
all chosen columns at once - rate_b = base exp(sum_j I_j coef_j X[j, b]) on each side - with an indicator per covariate and
side (Bayesian variable selection, Kuo-Mallick), so that "which of these matter once the others are in the model?" has an
answer: P(I = 1) per (side, covariate) and the posterior frequency of the indicator patterns.  The data are create_bins'
per-bin statistics, as trend_rate.py -d computes them; every chain runs as one wave of one kernel
(include/literate_hip_mtrend.h).  This module reads and standardises the covariates, tunes the two coefficient windows during
the first --tune share of the run, names and writes the logs block by block and summarises the run.

The tuning is trend_mlik.tuned's rule towards 30 % acceptance, per side, on the counts of the moves of INCLUDED coefficients
pooled over the chains (a move of an excluded coefficient is judged by its prior alone); the windows start at 0.1 and are
frozen from the end of the tuning, where the indicators start to flip unless --bvs_from says otherwise.  So that there are
included coefficients to tune on, a run with selection starts from the full model: lr_mtrend_init's initial coefficients with
every free indicator set to 1 (given = 1).

What the result is and is not is said in DESIGN.md ("Joint covariate model").
"""
import math
import os
import sys

import numpy as np

MAX_BINS, MAX_COVS = 512, 16          # include/literate_hip_mtrend.h
WIN0 = 0.1
MT_HEAD = ["side", "covariate", "P_I", "2lnBF", "coef_mean", "coef_minHPD", "coef_maxHPD", "n_included", "avg_mean", "avg_ess", "avg_rhat",
           "accept_coef", "accept_coef_included", "accept_flip", "accept_multiplier", "window"]
MODELS_HEAD = ["rank", "frequency", "n", "birth", "death"]
RATES_HEAD = ["bin", "l_mean", "l_minHPD", "l_maxHPD", "l_empirical", "m_mean", "m_minHPD", "m_maxHPD", "m_empirical"]
N_MODELS = 20
# flags of trend_rate.py this command refuses, each with its reason
REFUSED = {"replicates": "the joint model runs all chains on one data set (replicate data sets are out of its scope)",
           "mlik": "marginal likelihoods of the joint model are not built (no power-posterior ladder for this sampler)",
           "ppc": "the posterior predictive checks simulate under trend_rate.py's one-covariate rate map, not under the joint model",
           "ppc_age": "the lifespan check simulates under trend_rate.py's one-covariate rate map, not under the joint model",
           "ade": "age-dependent extinction conditions on trend_rate.py's death rates, not on the joint model's",
           "ade_joint": "age-dependent extinction conditions on trend_rate.py's death rates, not on the joint model's",
           "waic": "WAIC scores lineages under trend_rate.py's one-covariate rate map, not under the joint model",
           "loo": "PSIS-LOO scores lineages under trend_rate.py's one-covariate rate map, not under the joint model",
           "mc3": "heated chains that swap belong to the RJ sampler; the joint model's chains are independent"}


def arg_error(args, world=1):
    """Why MultiTrendRate.py cannot run these flags (None when it can); every refusal names its flag and its reason."""
    for flag, why in REFUSED.items():
        if getattr(args, flag, None) not in (None, "", -1.0, 0):
            return "--%s: %s" % (flag, why)
    if world > 1:
        return "several ranks (WORLD_SIZE is %d): the joint model runs all its chains in one launch on one GPU" % world
    if not args.d:
        return "-d FILE is required: the lineages, as trend_rate.py takes them"
    if not args.trend_data:
        return "-trend_data FILE is required: a tab-separated table of covariates with a header row, one row per time bin"
    if args.chains < 1 or args.n < 0 or args.s < 1:
        return "--chains and -s must be at least 1, -n at least 0"
    if args.bvs not in (0, 1):
        return "-bvs takes 0 or 1"
    if not (0.0 < args.pI < 1.0):
        return "-pI takes a probability inside (0, 1)"
    if not (args.slab_sd > 0.0 and math.isfinite(args.slab_sd)):
        return "-slab_sd takes a positive standard deviation"
    if not (0.0 <= args.tune < 1.0):
        return "--tune takes the share of the run the windows are tuned in, in [0, 1)"
    if args.bvs_from < -1:
        return "--bvs_from takes an iteration (default: the end of the tuning)"
    for flag in ("ess", "summary"):
        v = getattr(args, flag)
        if v != -1.0 and not (0.0 <= v < 1.0):
            return "--%s takes a burn-in fraction in [0, 1)" % flag
    return None


def parse_columns(spec, n_cols):
    """--columns all | i,j,k -> the column indices; an index outside the file is refused by name"""
    if spec.strip() == "all":
        return list(range(n_cols))
    try:
        cols = [int(x) for x in spec.split(",")]
    except ValueError:
        raise ValueError("--columns takes all or a comma-separated list of column indices, not %r" % spec)
    for c in cols:
        if c < 0 or c >= n_cols:
            raise ValueError("--columns: column %d lies outside the trend file (it holds columns 0 .. %d)" % (c, n_cols - 1))
    if len(set(cols)) != len(cols):
        raise ValueError("--columns names a column twice")
    return cols


def standardise(x):
    """mean 0 and population sd 1 over the bins in use"""
    x = np.asarray(x, dtype=float)
    return (x - np.mean(x)) / np.std(x)


def check_column(x, name):
    if not np.all(np.isfinite(x)):
        raise ValueError("column %s holds a value that is not finite" % name)
    if np.max(x) == np.min(x):
        raise ValueError("column %s is constant over the run's bins: it cannot be standardised" % name)


def design_matrix(table, names, columns, rm_first_bin, n_bins, diversity=None):
    """table [rows, columns of the file] -> (X [P, n_bins] standardised, the covariates' names).  The rows are cut as
    parse_trend_data cuts them: the last one is dropped, and the first with -rm_first_bin 1; diversity: DT, appended as the column
    `diversity`"""
    table = np.asarray(table, dtype=float)
    cols = parse_columns(columns, table.shape[1]) if isinstance(columns, str) else list(columns)
    for c in cols:
        if c < 0 or c >= table.shape[1]:
            raise ValueError("--columns: column %d lies outside the trend file (it holds columns 0 .. %d)" % (c, table.shape[1] - 1))
    kept = table[:-1][1:] if rm_first_bin else table[:-1]
    if kept.shape[0] != n_bins:
        raise ValueError("the trend file holds %d rows, %d in use: the data have %d time bins" % (table.shape[0], kept.shape[0], n_bins))
    if n_bins > MAX_BINS:
        raise ValueError("%d time bins: the joint model holds at most %d" % (n_bins, MAX_BINS))
    out, used = [], []
    for c in cols:
        check_column(kept[:, c], "%d (%s)" % (c, names[c]))
        out.append(standardise(kept[:, c]))
        used.append(str(names[c]))
    if diversity is not None:
        check_column(np.asarray(diversity, dtype=float), "diversity")
        out.append(standardise(diversity))
        used.append("diversity")
    if len(out) < 1:
        raise ValueError("no covariate chosen")
    if len(out) > MAX_COVS:
        raise ValueError("%d covariates: the joint model holds at most %d" % (len(out), MAX_COVS))
    return np.stack(out), used


def read_design(path, columns, rm_first_bin, n_bins, diversity=None):
    import pandas as pd
    df = pd.read_csv(path, sep="\t")
    return design_matrix(df.to_numpy().astype(float), [str(c) for c in df.columns], columns, rm_first_bin, n_bins, diversity)


def log_name(data_file, seed, const_b, const_d, no_death, chain=None):
    from .trendrate import model_suffix
    return "%s_%s%s_joint%s.multitrend.log" % (os.path.splitext(data_file)[0], seed, model_suffix(const_b, const_d, no_death),
                                                 "" if chain is None else "_c%d" % chain)


def summary_stem(data_file):
    return os.path.splitext(data_file)[0] + "_joint_MT"


def header(names, n_bins):
    head = ["it", "posterior", "likelihood", "likelihood_birth", "likelihood_death", "prior", "l0", "m0"]
    head += ["I_l_%s" % n for n in names] + ["a_%s" % n for n in names] + ["I_m_%s" % n for n in names] + ["b_%s" % n for n in names]
    return head + ["l_%d" % b for b in range(n_bins)] + ["m_%d" % b for b in range(n_bins)]


def bin_rates(rows, X):
    """rows [n, >= 8 + 4 P] -> (l [n, n_bins], m [n, n_bins]): base exp(sum_j I_j coef_j X[j])"""
    P = X.shape[0]
    eta_l = (rows[:, 8:8 + P] * rows[:, 8 + P:8 + 2 * P]) @ X
    eta_m = (rows[:, 8 + 2 * P:8 + 3 * P] * rows[:, 8 + 3 * P:8 + 4 * P]) @ X
    return rows[:, 6:7] * np.exp(eta_l), rows[:, 7:8] * np.exp(eta_m)


def tune_windows(win, accepted, proposed, b):
    """trend_mlik.tuned's rule after block b on the two windows: accepted, proposed [2] of the block, pooled over the chains"""
    from .trend_mlik import tuned
    w = tuned(np.asarray(win, dtype=float).reshape(2, 1), np.asarray(accepted, dtype=float).reshape(2, 1),
              np.asarray(proposed, dtype=float).reshape(2, 1), b, [True, True])
    return (float(w[0, 0]), float(w[1, 0]))


def two_ln_bf(P, pI, n):
    """2 ln of the Bayes factor of I = 1 at posterior frequency P against the prior odds, P clipped to [1 / (2 n), 1 - 1 / (2 n)]"""
    P = min(max(float(P), 1.0 / (2 * n)), 1.0 - 1.0 / (2 * n))
    return 2.0 * math.log((P / (1.0 - P)) / (pI / (1.0 - pI)))


def model_table(I, top=N_MODELS):
    """I [n, 2 P] of 0 / 1 -> [(frequency, count, pattern)] of the `top` most visited patterns, the most visited first (ties:
    the smaller pattern read as a binary number first)"""
    I = (np.asarray(I) != 0).astype(np.int64)
    keys = I @ (1 << np.arange(I.shape[1], dtype=np.int64))
    u, first, cnt = np.unique(keys, return_index=True, return_counts=True)
    order = sorted(range(len(u)), key=lambda i: (-cnt[i], u[i]))[:top]
    return [(cnt[i] / float(len(keys)), int(cnt[i]), I[first[i]]) for i in order]


def conditional_coef(I, coef):
    """mean and 95 % HPD of a coefficient over the rows that include it -> (mean, lo, hi, n)"""
    from .traitrate import hpd
    v = np.asarray(coef)[np.asarray(I) != 0]
    if len(v) == 0:
        return float("nan"), float("nan"), float("nan"), 0
    lo, hi = hpd(v)
    return float(v.mean()), lo, hi, len(v)


def acceptance(counters):
    """counters [C, 2, 6] (proposed, accepted) -> the rate per kind, pooled over the chains (NaN: never proposed)"""
    c = np.asarray(counters, dtype=float).sum(axis=0)
    with np.errstate(all="ignore"):
        return np.where(c[0] > 0, c[1] / c[0], np.nan)


def write_mt(path, names, sides, P_I, coef, avg, acc, wins, pI, n):
    """<stem>_joint_MT.tsv.  sides: the free sides; P_I [2, P]; coef [2][P] = (mean, lo, hi, n); avg [2][P] = (mean, ess, rhat)"""
    f64 = lambda v: str(float(v))
    with open(path, "w") as f:
        f.write("\t".join(MT_HEAD) + "\n")
        for s in sides:
            for j, name in enumerate(names):
                line = [("birth", "death")[s], name, f64(P_I[s][j]), f64(two_ln_bf(P_I[s][j], pI, n))]
                line += [f64(coef[s][j][0]), f64(coef[s][j][1]), f64(coef[s][j][2]), str(int(coef[s][j][3]))]
                line += [f64(v) for v in avg[s][j]]
                line += [f64(acc[1 + s]), f64(acc[4 + s]), f64(acc[3]), f64(acc[0]), f64(wins[s])]
                f.write("\t".join(line) + "\n")


def read_tsv(path):
    with open(path) as f:
        lines = f.read().splitlines()
    head = lines[0].split("\t")
    return head, [dict(zip(head, ln.split("\t"))) for ln in lines[1:]]


def write_models(path, table, P):
    with open(path, "w") as f:
        f.write("\t".join(MODELS_HEAD) + "\n")
        for k, (freq, cnt, pat) in enumerate(table):
            f.write("\t".join([str(k + 1), str(float(freq)), str(cnt), "".join(str(int(v)) for v in pat[:P]),
                               "".join(str(int(v)) for v in pat[P:])]) + "\n")


def write_rates(path, l, m, emp):
    """l, m = (mean, lo, hi) [n_bins] each"""
    with open(path, "w") as f:
        f.write("\t".join(RATES_HEAD) + "\n")
        for b in range(len(l[0])):
            f.write("\t".join([str(b)] + [str(float(v[b])) for v in (l[0], l[1], l[2], emp[0], m[0], m[1], m[2], emp[1])]) + "\n")


def summarise(stem, kept, X, names, sides, counters, wins, pI, emp):
    """The three summary files from kept [n, C, width] rows after the burn-in, chains pooled.  The model-averaged I x coef (mean,
    ESS, split R-hat: ops.ess_summary) and the rates per bin (mean, 95 % HPD: ops.col_summary) are computed on the device from
    columns derived there; the coefficient given inclusion is a selection of rows of varying length and stays on the host."""
    import torch
    from . import ops
    P, nb = X.shape
    n, C, _ = kept.shape
    dev = torch.as_tensor(kept, device="cuda")
    Xd = torch.as_tensor(X, device="cuda")
    Ia_l, Ia_m = dev[:, :, 8:8 + P] * dev[:, :, 8 + P:8 + 2 * P], dev[:, :, 8 + 2 * P:8 + 3 * P] * dev[:, :, 8 + 3 * P:8 + 4 * P]
    derived = torch.cat([Ia_l, Ia_m, dev[:, :, 6:7] * torch.exp(Ia_l @ Xd), dev[:, :, 7:8] * torch.exp(Ia_m @ Xd)], dim=2).contiguous()
    ess = ops.ess_summary(derived, n, list(range(2 * P)), burnin=0.0)
    avg_mean, avg_ess, avg_rhat = [v.cpu().numpy() for v in (ess.pooled_mean, ess.pooled_ess, ess.rhat)]
    col = ops.col_summary(derived, n, list(range(2 * P, 2 * P + 2 * nb)), burnin=0.0)
    cm, clo, chi = [v.cpu().numpy().reshape(-1) for v in (col.mean, col.lo, col.hi)]
    flat = kept.reshape(n * C, -1)
    I = [flat[:, 8:8 + P], flat[:, 8 + 2 * P:8 + 3 * P]]
    coef = [flat[:, 8 + P:8 + 2 * P], flat[:, 8 + 3 * P:8 + 4 * P]]
    P_I = [I[0].mean(axis=0), I[1].mean(axis=0)]
    cc = [[conditional_coef(I[s][:, j], coef[s][:, j]) for j in range(P)] for s in (0, 1)]
    avg = [[(avg_mean[s * P + j], avg_ess[s * P + j], avg_rhat[s * P + j]) for j in range(P)] for s in (0, 1)]
    write_mt(stem + ".tsv", names, sides, P_I, cc, avg, acceptance(counters), wins, pI, n * C)
    write_models(stem + "_models.tsv", model_table(np.concatenate(I, axis=1)), P)
    write_rates(stem + "_rates.tsv", (cm[:nb], clo[:nb], chi[:nb]), (cm[nb:], clo[nb:], chi[nb:]), emp)


def run(args):
    """MultiTrendRate.py after its argument checks"""
    import time
    import torch
    from . import logs, ops
    from .literate_library import create_bins, parse_ts_te, set_seed
    from .trend_mlik import TUNE_BLOCKS, tune_blocks
    seed = set_seed(args.seed)
    no_death = bool(args.no_death)
    const_b, const_d = bool(args.const_B), True if no_death else bool(args.const_D)
    TS, TE, PRESENT, ORIGIN = parse_ts_te(args.d, args.TBP, args.first_year, args.last_year, args.death_jitter)
    _, _, n_spec, n_exti, DT, n_bins, _ = create_bins(ORIGIN, PRESENT, np.asarray(TS, dtype=float), np.asarray(TE, dtype=float),
                                                      int(args.rm_first_bin))
    try:
        X, names = read_design(args.trend_data, args.columns, int(args.rm_first_bin), n_bins, DT if args.with_diversity else None)
    except (ValueError, OSError) as e:
        raise SystemExit("%s: %s" % (args.trend_data, e))
    P, C = X.shape[0], args.chains
    data = ops.MtrendData(n_spec, n_exti, DT, X, C, names)
    tune_end = int(args.tune * args.n)
    bvs_from = tune_end if args.bvs_from < 0 else args.bvs_from
    wins = (WIN0, WIN0)

    def settings():
        return ops.MtrendSettings(int(const_b), int(const_d), int(no_death), args.bvs, bvs_from, args.pI, args.slab_sd, wins)

    print("%d time bins, %d covariates (%s), %d chains; windows tuned until iteration %d, indicators flip from %d" %
          (n_bins, P, " ".join(names), C, tune_end, bvs_from) if args.bvs else
          "%d time bins, %d covariates (%s), %d chains; windows tuned until iteration %d, every covariate included" %
          (n_bins, P, " ".join(names), C, tune_end))
    with np.errstate(all="ignore"):
        emp = (n_spec / DT, n_exti / DT)
    paths = [log_name(args.d, seed, const_b, const_d, no_death, None if C == 1 else k) for k in range(C)]
    for path in paths:
        with open(path, "w", newline="") as f:
            f.write("\t".join(header(names, n_bins)) + "\r\n")
    state = ops.mtrend_init(data, seed, settings())
    if args.bvs:
        # the run starts from the full model - the initial coefficients, every free indicator 1 (those of a constant side read as
        # 0) -, so that the windows are tuned on included coefficients before the indicators start to flip
        full = state.cpu().numpy()
        S0 = ops.MTREND_STATE
        full[:, S0["I_l"]:S0["I_l"] + P], full[:, S0["I_m"]:S0["I_m"] + P] = 1.0, 1.0
        state = ops.mtrend_init(data, seed, settings(), given=full)
    W = ops.mtrend_row_columns(P)["width"]
    S = ops.MTREND_STATE
    block = args.block if args.block > 0 else max(args.p, 1) * max(1, 50000 // max(args.p, 1))
    # the launches end at the tuning blocks' ends and at the log blocks' ends
    ends = sorted(set([e for e in tune_blocks(tune_end)[1:] if 0 < e <= args.n] + list(range(block, args.n, block)) + [args.n]))
    tune_at = {e: b for b, e in enumerate(tune_blocks(tune_end)) if b >= 1 and e > 0}

    def counts():
        st = state.cpu().numpy()
        return np.stack([st[:, S["proposed"]:S["proposed"] + 6], st[:, S["accepted"]:S["accepted"] + 6]], axis=1)

    done, kept, pending, cnt0 = 0, [], [], counts()
    t_start = time.time()

    def flush():
        if not pending:
            return
        h = np.concatenate(pending, axis=0)
        del pending[:]
        tables = []
        for c in range(C):
            l, m = bin_rates(h[:, c], X)
            tables.append(np.concatenate([h[:, c, :W], l, m], axis=1))
        logs.append_table_logs(paths, tables)

    for end in ends if args.n > 0 else []:
        rows = ops.mtrend_steps(data, state, done, end - done, args.s, seed, settings())
        done = end
        if rows.shape[0]:
            h = rows[:, :, :W].cpu().numpy()
            kept.append(h)
            pending.append(h)
        if done in tune_at:
            cnt = counts()
            d = (cnt - cnt0).sum(axis=0)
            wins = tune_windows(wins, d[1, 4:6], d[0, 4:6], tune_at[done])
            cnt0 = cnt
        if done % block == 0 or done == args.n:
            flush()
            st = state.cpu().numpy()
            print(done, "likelihood %.3f" % (st[0, S["lik_b"]] + st[0, S["lik_d"]]), "windows %.4g %.4g" % wins)
            sys.stdout.flush()
    torch.cuda.synchronize()
    el = time.time() - t_start
    if args.n > 0:
        print("%d iterations x %d chains in %.2f s" % (args.n, C, el))
    all_rows = np.concatenate(kept, axis=0) if kept else np.zeros((0, C, W))
    n_s = all_rows.shape[0]
    stem = summary_stem(args.d)
    sides = [s for s, const in ((0, const_b), (1, const_d)) if not const]
    if args.summary != -1.0 and n_s - int(args.summary * n_s) >= 2:
        summarise(stem, np.ascontiguousarray(all_rows[int(args.summary * n_s):]), X, names, sides, counts(), wins, args.pI, emp)
        print("summary: %s.tsv, _models.tsv, _rates.tsv (%d samples per chain)" % (stem, n_s - int(args.summary * n_s)))
    if args.ess != -1.0 and n_s:
        head = header(names, n_bins)
        ecols = [2, 6, 7] + list(range(8 + P, 8 + 2 * P)) + list(range(8 + 3 * P, 8 + 4 * P))
        res = ops.ess_summary(np.ascontiguousarray(all_rows), n_s, ecols, burnin=args.ess)
        host = res._replace(**{k: getattr(res, k).cpu().numpy() for k in res._fields if k != "n"})
        print(logs.write_ess_tables(stem, [head[c] for c in ecols], host, args.s))
    return 0
