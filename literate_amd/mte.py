"""Multi-trait extinction: the host side of MTEmodel.py (the reference's other/MTEmodel.py, rebuilt on the GPU).

Every lineage carries several categorical traits; its extinction rate is a mean rate m times the sum of one softmax multiplier
per trait, normalised to mean 1 over the lineages, and an indicator per trait - Bayesian variable selection - says whether the
trait's multipliers differ at all.  The likelihood depends on a lineage only through its combination of states, so the data
of a time slice are three numbers per combination (ops.mte_tables), every slice is a problem of its own on the one table of
combinations, and every chain of every slice runs as one wave of one kernel (include/literate_hip_mte.h).  This module reads
and checks the table, names the logs as the reference does, writes them block by block and summarises the run.

Departures from the reference are listed in DESIGN.md ("Multi-trait extinction").
"""
import math
import os
import sys

import numpy as np

SUMMARY_HEAD = ["t0", "t1", "parameter", "mean", "minHPD", "maxHPD", "P_I", "2lnBF"]
MAX_COMBOS, MAX_TRAITS, MAX_STATES, MAX_CATS = 1024, 16, 16, 128          # include/literate_hip_mte.h


def arg_error(args, world=1):
    """Why MTEmodel.py cannot run these flags (None when it can); every refusal names its flag and its reason."""
    if args.A != 0:
        return "-A %d: marginal likelihoods of this model are not built (no power-posterior ladder for the multi-trait sampler)" % args.A
    if world > 1:
        return "several ranks (WORLD_SIZE is %d): the multi-trait sampler runs all chains of all slices in one launch on one GPU" % world
    if not args.d:
        return "-d FILE is required: a tab-separated table `name ts te trait ...` with a header row"
    if args.chains < 1 or args.n < 0 or args.s < 1 or args.bvs_from < 0:
        return "--chains and -s must be at least 1, -n and --bvs_from at least 0"
    if args.bvs not in (0, 1) or args.const not in (0, 1) or args.mu_species not in (0, 1):
        return "-bvs, -const and -mu_species take 0 or 1"
    if not (0.0 < args.pI < 1.0):
        return "-pI takes a probability inside (0, 1)"
    if args.slices and args.slice_edges:
        return "--slices and --slice_edges both name the slices: give one"
    for flag in ("ess", "summary"):
        v = getattr(args, flag)
        if v != -1.0 and not (0.0 <= v < 1.0):
            return "--%s takes a burn-in fraction in [0, 1)" % flag
    return None


def parse_slices(args):
    """[(t0, t1)] with t0 > t1, ages before the present: --slices 'a-b,c-d', or --slice_edges e0,e1,... (consecutive slices), or
    the one slice of -t0 / -t1"""
    try:
        if args.slices:
            out = []
            for part in args.slices.split(","):
                a, b = part.split("-")
                out.append((float(a), float(b)))
        elif args.slice_edges:
            e = sorted((float(x) for x in args.slice_edges.split(",")), reverse=True)
            if len(e) < 2:
                raise ValueError
            out = list(zip(e[:-1], e[1:]))
        else:
            out = [(float(args.t0), float(args.t1))]
    except ValueError:
        raise ValueError("--slices takes 'a-b,c-d,...' and --slice_edges 'e0,e1,...' (ages, at least two)")
    for t0, t1 in out:
        if not t0 > t1 or t1 < 0:
            raise ValueError("slice %s-%s: the older age comes first and no age is negative" % (t0, t1))
    return out


def read_table(path, traits=()):
    """-d FILE -> (ts, te, trait values [n, T] float, names [T]).  -traits i ...: 1-based among the columns behind ts and te;
    default: all of them, the last one included, as the reference computes it (MTE:137-141)."""
    with open(path) as f:
        head = f.readline().split()
    tab = np.loadtxt(path, delimiter="\t", skiprows=1, usecols=range(1, len(head)), ndmin=2)
    n_tr = tab.shape[1] - 2
    cols = [int(i) + 1 for i in traits] if len(traits) else list(range(2, 2 + n_tr))
    if n_tr < 1 or any(c < 2 or c >= tab.shape[1] for c in cols):
        raise ValueError("-traits: the table holds %d trait columns, numbered from 1" % max(n_tr, 0))
    return tab[:, 0], tab[:, 1], tab[:, cols], [head[3:][c - 2] for c in cols]


def check_traits(values, names):
    """the refusals that need the table alone -> the traits as integers"""
    if values.shape[1] > MAX_TRAITS:
        raise ValueError("%d traits: the sampler holds at most %d" % (values.shape[1], MAX_TRAITS))
    for t, name in enumerate(names):
        v = values[:, t]
        if not np.all(np.isfinite(v)) or np.any(v != np.floor(v)) or np.any(v < 0):
            bad = v[~(np.isfinite(v) & (v == np.floor(v)) & (v >= 0))][0]
            raise ValueError("trait %s: state %r is not a non-negative integer" % (name, float(bad)))
        S = len(np.unique(v))
        if S < 2:
            raise ValueError("trait %s has the same state in every lineage: nothing to select" % name)
        if S > MAX_STATES:
            raise ValueError("trait %s has %d states: the sampler holds at most %d per trait" % (name, S, MAX_STATES))
    return values.astype(np.int64)


def check_tables(tab, slices):
    """the refusals that need the grouped statistics"""
    G = tab["code"].shape[0]
    if G > MAX_COMBOS:
        raise ValueError("%d combinations of trait states: the sampler holds at most %d" % (G, MAX_COMBOS))
    if int(tab["n_states"].sum()) > MAX_CATS:
        raise ValueError("%d states over all traits: the sampler holds at most %d" % (int(tab["n_states"].sum()), MAX_CATS))
    for p, (t0, t1) in enumerate(slices):
        if tab["n"][p].sum() == 0:
            raise ValueError("slice %s-%s holds no lineage" % (t0, t1))
        if tab["E"][p].sum() == 0:
            raise ValueError("slice %s-%s holds no extinction: its mean rate has no estimate" % (t0, t1))


def log_name(data_file, const, out, t0, t1, chain=None):
    """the reference's file name (MTE:163-173); chain: `_c<k>` before the extension"""
    wd = os.path.dirname(data_file) or os.getcwd()
    name = os.path.splitext(os.path.basename(data_file))[0]
    tag = "_const_" if const == 1 else ""
    if out != "":
        tag = "%s_%s_" % (tag, out)
    stem = "%s/%s%s" % (wd, name, tag)
    if t0 < np.inf or t1 > 0:
        stem += "%s-%s" % (float(t0), float(t1))
    return stem + ("" if chain is None else "_c%d" % chain) + ".log"


def summary_stem(data_file, const, out):
    return os.path.splitext(log_name(data_file, const, out, np.inf, 0.0))[0]


def combo_names(tab, p):
    """`m<states>_<count>` of the combinations slice p holds (MTE:200-228), in the table's order -> (names, their indices)"""
    keep = np.nonzero(tab["n"][p] > 0)[0]
    names = []
    for g in keep:
        vals = [tab["states"][t][tab["code"][g, t]] for t in range(tab["code"].shape[1])]
        names.append("m" + "".join("%d" % int(v) for v in vals) + "_%d" % int(tab["n"][p, g]))
    return names, keep


def header(names, n_states, combos=()):
    """the reference's header (MTE:254-269)"""
    head = ["it", "posterior", "likelihood", "prior", "mean_r"] + ["I_%s" % n for n in names]
    head += ["m_%s_%d" % (n, j) for n, S in zip(names, n_states) for j in range(int(S))]
    return head + ["sd_%s" % n for n in names] + ["beta_hp"] + list(combos)


def combo_rates(rows, tab, p, keep):
    """rows [n, width] of slice p's chains -> r_g = m w_g / Z of the combinations `keep`, from each row's m, I and softmax columns"""
    from .ops import mte_row_columns
    cols, ns = mte_row_columns(tab["n_states"]), tab["n_states"]
    off = np.concatenate([[0], np.cumsum(ns)])
    q = rows[:, cols["q"]].copy()
    I = rows[:, cols["I"]]
    for t, S in enumerate(ns):
        q[:, off[t]:off[t + 1]] = np.where(I[:, t:t + 1] != 0, q[:, off[t]:off[t + 1]], 1.0 / S)
    w = np.zeros((rows.shape[0], tab["code"].shape[0]))
    for t in range(len(ns)):
        w += q[:, off[t] + tab["code"][:, t].astype(np.int64)]
    Z = (w * tab["n"][p][None, :]).sum(axis=1) / tab["n"][p].sum()
    return rows[:, 4:5] * w[:, keep] / Z[:, None]


def two_ln_bf(P, pI, n):
    """2 ln of the Bayes factor of I = 1 at posterior frequency P and prior pI, P clipped to [1 / (2 n), 1 - 1 / (2 n)] for n rows"""
    P = min(max(float(P), 1.0 / (2 * n)), 1.0 - 1.0 / (2 * n))
    return 2.0 * math.log((P / (1.0 - P)) / (pI / (1.0 - pI)))


def write_summary(path, kept, counters, data_names, n_states, slices, cpp, pI):
    """<stem>_MTE.tsv: kept [n, C, width] rows after the burn-in, chains of a slice pooled; counters [C, 2, 3] (proposed, accepted)"""
    from .ops import MTE_MOVES, mte_row_columns
    from .traitrate import hpd
    cols = mte_row_columns(n_states)
    head = header(data_names, n_states)
    f64 = lambda v: str(float(v))
    with open(path, "w") as f:
        f.write("\t".join(SUMMARY_HEAD) + "\n")
        for p, (t0, t1) in enumerate(slices):
            x = kept[:, p * cpp:(p + 1) * cpp].reshape(-1, kept.shape[2])
            n = x.shape[0]
            for c in range(4, cols["width"]):
                v = x[:, c]
                if cols["I"].start <= c < cols["I"].stop:
                    P = v.mean()
                    line = [f64(P), "nan", "nan", f64(P), f64(two_ln_bf(P, pI, n))]
                else:
                    lo, hi = hpd(v)
                    line = [f64(v.mean()), f64(lo), f64(hi), "nan", "nan"]
                f.write("\t".join([f64(t0), f64(t1), head[c]] + line) + "\n")
            cnt = counters[p * cpp:(p + 1) * cpp].sum(axis=0)
            for k, move in enumerate(MTE_MOVES):
                rate = cnt[1, k] / cnt[0, k] if cnt[0, k] > 0 else float("nan")
                f.write("\t".join([f64(t0), f64(t1), "accept_%s" % move, f64(rate), "nan", "nan", "nan", "nan"]) + "\n")


def read_summary(path):
    """<stem>_MTE.tsv -> {(t0, t1, parameter): {column: value}}"""
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].split("\t") == SUMMARY_HEAD
    out = {}
    for ln in lines[1:]:
        c = ln.split("\t")
        out[float(c[0]), float(c[1]), c[2]] = dict(zip(SUMMARY_HEAD[3:], (float(v) for v in c[3:])))
    return out


def run(args):
    """MTEmodel.py after its argument checks"""
    import time
    import torch
    from . import _hip, logs, ops
    rseed = np.random.randint(0, 9999) if args.seed < 0 else args.seed
    try:
        slices = parse_slices(args)
        ts, te, values, names = read_table(args.d, args.traits)
        traits = check_traits(values, names)
        tab = ops.mte_tables(ts, te, traits, slices)
        check_tables(tab, slices)
    except ValueError as e:
        raise SystemExit("%s: %s" % (args.d, e))
    cpp, P = args.chains, len(slices)
    data = ops.MteData(tab["code"], tab["n_states"], tab["n"], tab["E"], tab["B"], cpp, names, slices)
    settings = ops.MteSettings(args.bvs, args.const, args.bvs_from, args.pI)
    cols = ops.mte_row_columns(tab["n_states"])
    W = cols["width"]
    print("%d lineages, %d traits (%s states), %d combinations; %d slices x %d chains" %
          (len(ts), data.T, " ".join(str(int(s)) for s in tab["n_states"]), data.G, P, cpp))
    for p, (t0, t1) in enumerate(slices):
        print("slice %s-%s: %d lineages, %d extinct, extinction rate (mle) %s" %
              (t0, t1, tab["n"][p].sum(), tab["E"][p].sum(), tab["E"][p].sum() / tab["B"][p].sum()))
    combos = [combo_names(tab, p) if args.mu_species == 1 else ([], np.zeros(0, dtype=np.int64)) for p in range(P)]
    paths = [log_name(args.d, args.const, args.out, t0, t1, None if cpp == 1 else k) for (t0, t1) in slices for k in range(cpp)]
    for c, path in enumerate(paths):
        with open(path, "w", newline="") as f:
            f.write("\t".join(header(names, tab["n_states"], combos[c // cpp][0])) + "\r\n")
    state = ops.mte_init(data, rseed, settings)
    block = args.block if args.block > 0 else max(args.p, 1) * max(1, 50000 // max(args.p, 1))
    done, kept = 0, []
    t_start = time.time()
    while done < args.n:
        n = min(block, args.n - done)
        rows = ops.mte_steps(data, state, done, n, args.s, rseed, settings)
        done += n
        if rows.shape[0]:
            h = rows[:, :, :W].cpu().numpy()
            kept.append(h)
            tables = []
            for c in range(data.n_chains):
                p = c // cpp
                tables.append(np.concatenate([h[:, c], combo_rates(h[:, c], tab, p, combos[p][1])], axis=1) if args.mu_species == 1 else h[:, c])
            logs.append_table_logs(paths, tables)
        st = state.cpu().numpy()
        print(done, "likelihood %s" % " ".join("%.3f" % v for v in st[::cpp, ops.MTE_STATE["lik"]]))
        sys.stdout.flush()
    torch.cuda.synchronize()
    el = time.time() - t_start
    if args.n > 0:
        print("%d iterations x %d chains in %.2f s" % (args.n, data.n_chains, el))
    all_rows = np.concatenate(kept, axis=0) if kept else np.zeros((0, data.n_chains, W))
    S = all_rows.shape[0]
    stem = summary_stem(args.d, args.const, args.out)
    if args.summary != -1.0 and S - int(args.summary * S) >= 2:
        st = state.cpu().numpy()
        o = ops.MTE_STATE
        counters = np.stack([st[:, o["proposed"]:o["proposed"] + 3], st[:, o["accepted"]:o["accepted"] + 3]], axis=1)
        write_summary(stem + "_MTE.tsv", all_rows[int(args.summary * S):], counters, names, tab["n_states"], slices, cpp, args.pI)
        print("summary: %s_MTE.tsv (%d samples per chain)" % (stem, S - int(args.summary * S)))
    if args.ess != -1.0:
        head = header(names, tab["n_states"])
        ecols = [4, 2] + list(range(cols["q"].start, cols["q"].stop))
        for p, (t0, t1) in enumerate(slices):
            sub = np.ascontiguousarray(all_rows[:, p * cpp:(p + 1) * cpp])
            res = ops.ess_summary(sub, S, ecols, burnin=args.ess)
            host = res._replace(**{k: getattr(res, k).cpu().numpy() for k in res._fields if k != "n"})
            sstem = stem + ("_%s-%s" % (float(t0), float(t1)) if P > 1 or t0 < np.inf or t1 > 0 else "")
            print(logs.write_ess_tables(sstem, [head[c] for c in ecols], host, args.s))
    return 0
