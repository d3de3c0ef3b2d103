"""Numpy restatement of literate_amd/ppc.py's posterior predictive check, written from its definition (the module docstring
there, steps 1 - 5), with the simulator passed in:

    simulator(lam_bins [n, nb], mu_bins [n, nb], steps_per_bin, n_start [n], seed, capacity) -> (counts [n, 4, nb], totals [n, 4])

in the layout of lr_simulate_bd_batch (replicate r runs under seed + r; totals[:, 2] the overflow flag).  Rates per bin
come from logs.rates_per_bin on the rows as the logs hold them; HPD from tests/helpers/summary_ref.py."""
import numpy as np

from helpers import summary_ref as sr

H, KMAX = 13, 32
STATS = ("obs", "mean", "hpd_low", "hpd_high", "p_ge")
PPC_HEAD = ["time"] + ["%s_%s" % (k, s) for k in ("sp_events", "ex_events", "diversity") for s in STATS]
FIT_INTS = ["draws", "steps_per_bin", "start_bin", "n_start", "free_kept", "free_overflowed", "free_extinct", "step_kept",
            "step_overflowed", "step_extinct"]
FIT_HEAD = (FIT_INTS + ["%s_%s" % (k, s) for k in ("end_diversity", "total_births", "total_deaths") for s in STATS]
            + ["coverage_sp_events", "coverage_ex_events", "coverage_diversity"])


def draw_indices(M, n_draws):
    R = min(int(n_draws), int(M))
    return np.array([(i * M) // R for i in range(R)], dtype=np.int64)


def div_obs_of(sp, ex):
    d = [0]
    for a, b in zip(sp, ex):
        d.append(d[-1] + int(a) - int(b))
    return np.array(d, dtype=np.int64)


def start_bin_of(div_obs, start_bin=None):
    n_bins = len(div_obs) - 1
    if start_bin is not None:
        if not (0 <= start_bin < n_bins) or div_obs[start_bin] < 1:
            raise ValueError("start_bin without lineages")
        return int(start_bin)
    for b in range(1, n_bins):
        if div_obs[b] >= 1:
            return b
    raise ValueError("nothing to start from")


def row_rates(row, n_bins):
    """(lam [n_bins], mu [n_bins]) of one trace row by logs.rates_per_bin"""
    from literate_amd import logs
    head, sp_row, ex_row = logs.split_row(np.asarray(row, dtype=float))
    kl, km = int(head[6]), int(head[7])
    return (logs.rates_per_bin(sp_row[:kl], sp_row[kl:], head[8], n_bins),
            logs.rates_per_bin(ex_row[:km], ex_row[km:], head[8], n_bins))


def stats_of(vals, obs):
    """vals [n, K], obs [K] -> [K, 5]"""
    vals = np.asarray(vals, dtype=np.float64)
    if sr.n_in_of(len(vals)) < 2:
        raise ValueError("too few kept draws")
    out = np.empty((vals.shape[1], 5))
    out[:, 0] = obs
    out[:, 1:4] = sr.triples(vals)
    out[:, 4] = np.array([np.sum(vals[:, k] >= obs[k]) for k in range(vals.shape[1])]) / float(len(vals))
    return out


def coverage(stats):
    rep = [r for r in stats if np.isfinite(r[1])]
    if not rep:
        return float("nan")
    return sum(1 for r in rep if r[2] <= r[0] <= r[3]) / float(len(rep))


def check(lam, mu, sp, ex, steps_per_bin, seed, simulator, start_bin=None, capacity=None, start_time=0.0):
    """steps 2 - 4 on the draws' per-bin rates lam, mu [R, n_bins] -> dict(div_obs, start_bin, capacity, free, step, table,
    fit)"""
    sp, ex = np.asarray(sp, dtype=np.int64), np.asarray(ex, dtype=np.int64)
    lam, mu = np.asarray(lam, dtype=float), np.asarray(mu, dtype=float)
    R, n_bins = lam.shape
    div_obs = div_obs_of(sp, ex)
    b0 = start_bin_of(div_obs, start_bin)
    cap = int(capacity) if capacity else max(8 * int(sp.sum()), 1 << 16)
    nf = n_bins - b0
    # free-running: replicate i, seed + i
    fc, ft = simulator(lam[:, b0:], mu[:, b0:], steps_per_bin, np.full(R, div_obs[b0]), seed, cap)
    keep_f = ft[:, 2] == 0
    vals = np.array([list(fc[i, 2, 1:]) + [ft[i, 1], fc[i, 0].sum(), fc[i, 1].sum()] for i in range(R) if keep_f[i]], dtype=float)
    vals = vals.reshape(int(keep_f.sum()), nf + 2)
    fs = stats_of(vals, np.concatenate([div_obs[b0 + 1:], [sp[b0:].sum(), ex[b0:].sum()]]))
    # one step ahead: replicate (b - b0) * R + i, seed + R + that index; a bin nobody lived in is not simulated
    lam1, mu1, n1 = [], [], []
    for b in range(b0, n_bins):
        for i in range(R):
            lam1.append([lam[i, b]]), mu1.append([mu[i, b]]), n1.append(div_obs[b])
    sc, st = simulator(np.array(lam1), np.array(mu1), steps_per_bin, np.array(n1), seed + R, cap)
    sc, st = sc.reshape(nf, R, 4), st.reshape(nf, R, 4)
    real = np.array([div_obs[b] >= 1 for b in range(b0, n_bins)])
    keep_s = np.array([not any(st[j, i, 2] != 0 for j in range(nf) if real[j]) for i in range(R)])
    vals = np.array([[sc[j, i, 0] for j in range(nf)] + [sc[j, i, 1] for j in range(nf)] for i in range(R) if keep_s[i]],
                    dtype=float).reshape(int(keep_s.sum()), 2 * nf)
    ss = stats_of(vals, np.concatenate([sp[b0:], ex[b0:]]))
    for j in range(nf):
        if not real[j]:
            ss[j, 1:] = np.nan
            ss[nf + j, 1:] = np.nan
    table = np.full((n_bins, 16), np.nan)
    for b in range(n_bins):
        table[b, 0] = start_time + b
        table[b, 1], table[b, 6], table[b, 11] = sp[b], ex[b], div_obs[b]
        if b >= b0:
            table[b, 1:6], table[b, 6:11] = ss[b - b0], ss[nf + b - b0]
        if b > b0:
            table[b, 11:16] = fs[b - b0 - 1]
    fit = dict(draws=R, steps_per_bin=steps_per_bin, start_bin=b0, n_start=int(div_obs[b0]), free_kept=int(keep_f.sum()),
               free_overflowed=int(R - keep_f.sum()), free_extinct=int(sum(1 for i in range(R) if keep_f[i] and ft[i, 1] == 0)),
               step_kept=int(keep_s.sum()), step_overflowed=int(R - keep_s.sum()),
               step_extinct=int(sum(1 for j in range(nf) for i in range(R) if real[j] and keep_s[i] and st[j, i, 1] == 0)))
    for name, row in zip(("end_diversity", "total_births", "total_deaths"), fs[nf - 1:]):
        for s, v in zip(STATS, row):
            fit["%s_%s" % (name, s)] = float(v)
    fit["coverage_sp_events"], fit["coverage_ex_events"] = coverage(table[:, 1:6]), coverage(table[:, 6:11])
    fit["coverage_diversity"] = coverage(table[:, 11:16])
    return dict(div_obs=div_obs, start_bin=b0, capacity=cap, free=dict(counts=fc, totals=ft, kept=keep_f),
                step=dict(counts=sc, totals=st, kept=keep_s, simulated=real), table=table, fit=fit)


def posterior_predictive(rows, sp, ex, n_draws, steps_per_bin, seed, simulator, start_bin=None, capacity=None, start_time=0.0):
    """steps 1 - 4 on rows [S', C, W] (host)"""
    rows = np.asarray(rows, dtype=float)
    flat = rows.reshape(-1, rows.shape[-1])
    idx = draw_indices(len(flat), n_draws)
    n_bins = len(sp)
    rates = [row_rates(flat[k], n_bins) for k in idx]
    lam, mu = np.array([r[0] for r in rates]), np.array([r[1] for r in rates])
    out = check(lam, mu, sp, ex, steps_per_bin, seed, simulator, start_bin, capacity, start_time)
    out.update(draw_rows=idx, lam_bins=lam, mu_bins=mu)
    return out


def file_text(table, fit):
    """the text of <stem>_PPC.tsv and <stem>_PPC_fit.tsv"""
    a = "\t".join(PPC_HEAD) + "\n" + "".join("\t".join(str(float(v)) for v in row) + "\n" for row in table)
    b = "\t".join(FIT_HEAD) + "\n" + "\t".join([str(int(fit[k])) for k in FIT_INTS] + [str(float(fit[k])) for k in FIT_HEAD[len(FIT_INTS):]]) + "\n"
    return a, b


def oracle_simulator(lam, mu, spb, n_start, seed, capacity):
    """oracle/sim_oracle.py, one run per replicate, in lr_simulate_bd_batch's output layout"""
    from oracle import sim_oracle
    from helpers.sim_batch_cases import counts_from_run, steps
    n, nb = np.shape(lam)
    counts, totals = np.zeros((n, 4, nb), dtype=np.int64), np.zeros((n, 4), dtype=np.int64)
    for r in range(n):
        n0 = int(n_start[r])
        if n0 < 1 or n0 > capacity:
            totals[r] = (0, 0, 1, -1)
            continue
        try:
            ts, te, trace = sim_oracle.simulate_bd(n0, nb * spb, seed + r, steps(lam[r], spb), steps(mu[r], spb), capacity=capacity)
        except OverflowError:
            totals[r] = (0, 0, 1, -1)
            continue
        counts[r], totals[r] = counts_from_run(ts, te, trace, n0, nb, spb)
    return counts, totals
