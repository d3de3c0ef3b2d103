"""Posterior predictive check of a finished LiteRateForward run: do the sampled rates reproduce the data?

Lineages are simulated forward under posterior draws of the per-bin rates with the reference's discrete-time scheme
(simulateRateABC.v2.py:103-234; ops.simulate_bd_batch, one workgroup per replicate) and the outcome is set beside what the
data show.  Everything stays on the device until the small result tables.

1. Draws.  The post-burn-in trace rows [S', C, LR_TRACE_W] are M = S' * C rows, sample-major; R = min(n_draws, M) of them
   are used, draw i = row floor(i * M / R).  Their per-bin rates are ops.expand_rates(mode 0) of the row's rates and
   [root_age, interior shift times, death_age]: the floor-to-bin rule of logs.rates_per_bin.
2. Observed.  div_obs[b] = sum_{w < b} (sp_events[w] - ex_events[w]), b = 0 .. n_bins: the diversity at the left edge of
   bin b (at the end for b = n_bins).  The simulations start at the left edge of bin b0 = start_bin, or the smallest
   b >= 1 with div_obs[b] >= 1: a birth-death process cannot start from nobody.  Earlier bins are reported as observed.
3. Two sets of replicates, one launch each:
   free-running - replicate i runs bins b0 .. n_bins - 1 under draw i from div_obs[b0] lineages (seed + i): the predictive
   diversity trajectory.  From a single founder this band is wide by nature; start_bin moves the start;
   one step ahead - for every bin b >= b0 and every draw i a ONE-bin replicate from the OBSERVED div_obs[b] under draw i's
   rates of that bin, replicate (b - b0) * R + i (seed + R + that index): the births and deaths the rates predict given the
   diversity the data had.  A bin with div_obs[b] = 0 keeps its indices - so no other bin's seeds depend on it - but is
   not simulated (the simulator refuses a start of 0 at no cost) and is reported nan.
4. Summary over the kept draws: a free-running replicate that overflowed `capacity` drops its draw from the free-running
   tables; a draw ANY of whose one-bin replicates overflowed is dropped from the one-step tables as a whole, so every
   column of a table is over the same draws.  Extinct replicates are kept.  Per statistic: mean and 95 % HPD
   (ops.col_summary on the counts as doubles), p_ge = the share of kept replicates >= the observed value, and the
   coverage = the share of reported bins whose observed value lies inside the HPD.
5. <stem>_PPC.tsv (one row per bin) and <stem>_PPC_fit.tsv (one row).

Time mapping: a bin's simulated births / deaths are the events during its steps - what sp_events / ex_events count on
year-resolution input (ts = y, te = y + death_jitter).  Branch length is deliberately not compared: on such data the
observed br_length carries the jitter convention (a full year in the birth bin, death_jitter in the death bin), the
simulated one does not; diversity at bin edges and event counts have no such ambiguity.

The other two samplers.  trend_rate.py's rates are fixed per bin (the covariate is data): posterior_predictive_rates is the
same check started at step 2 from per-bin rates given directly.  DDRate.py's rates are a function of the diversity itself,
and the check must keep that feedback: posterior_predictive_dd runs both sets through ops.simulate_dd_batch, which
recomputes the rates of every step from the count living at that step."""
from collections import namedtuple

import numpy as np

from ._hip import LR_KMAX, LR_TRACE_HEAD, LR_TRACE_W

STATS = ("obs", "mean", "hpd_low", "hpd_high", "p_ge")
PPC_HEAD = ["time"] + ["%s_%s" % (k, s) for k in ("sp_events", "ex_events", "diversity") for s in STATS]
FIT_HEAD = (["draws", "steps_per_bin", "start_bin", "n_start", "free_kept", "free_overflowed", "free_extinct", "step_kept",
             "step_overflowed", "step_extinct"]
            + ["%s_%s" % (k, s) for k in ("end_diversity", "total_births", "total_deaths") for s in STATS]
            + ["coverage_sp_events", "coverage_ex_events", "coverage_diversity"])
N_FIT_INTS = 10

PpcResult = namedtuple("PpcResult", "draw_rows lam_bins mu_bins div_obs start_bin n_start capacity seeds free step "
                                    "table fit")
PpcResult.__doc__ = """posterior_predictive's results (host arrays).  draw_rows [R]: the trace rows drawn; lam_bins, mu_bins [R, n_bins];
div_obs [n_bins + 1]; seeds: the base seeds of the two sets; free, step: dicts with the raw counts / totals of the two
simulator calls and the kept-draw masks; table [n_bins, 16] = the rows of <stem>_PPC.tsv (PPC_HEAD); fit: dict of
<stem>_PPC_fit.tsv (FIT_HEAD)."""


def draw_indices(n_rows, n_draws):
    """the trace rows of the R = min(n_draws, M) draws: floor(i * M / R)"""
    M = int(n_rows)
    R = min(int(n_draws), M)
    if R < 1:
        raise ValueError("posterior predictive check: no draws (%d rows, n_draws %d)" % (M, n_draws))
    return (np.arange(R, dtype=np.int64) * M) // R


def observed_diversity(sp_events, ex_events):
    sp, ex = np.asarray(sp_events, dtype=np.int64), np.asarray(ex_events, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(sp - ex)]).astype(np.int64)


def pick_start_bin(div_obs, start_bin=None):
    n_bins = len(div_obs) - 1
    if start_bin is not None:
        b0 = int(start_bin)
        if not (0 <= b0 < n_bins) or div_obs[b0] < 1:
            raise ValueError("start_bin %d: no observed lineages at its left edge to start from" % b0)
        return b0
    alive = np.nonzero(div_obs[1:n_bins] >= 1)[0]
    if not len(alive):
        raise ValueError("no bin after the first starts with an observed lineage: nothing to simulate from")
    return int(alive[0]) + 1


def default_capacity(sp_events):
    return max(8 * int(np.sum(sp_events)), 1 << 16)


def _too_few(what, kept, total, capacity):
    return ValueError("posterior predictive check: %d of the %d %s draws overflowed capacity %d, and the %d left are "
                      "fewer than a 95 %% HPD takes (round(0.95 n) >= 2); pass a larger capacity"
                      % (total - kept, total, what, capacity, kept))


def _summarise(vals, obs):
    """vals [n, K] device doubles, obs [K] host -> [K, 5] host (obs, mean, hpd_low, hpd_high, p_ge)"""
    from . import ops
    import torch
    n = int(vals.shape[0])
    res = ops.col_summary(vals.reshape(n, 1, -1).contiguous(), n, range(vals.shape[1]), burnin=0.0, pooled=True)
    ge = (vals >= torch.as_tensor(np.asarray(obs, dtype=np.float64), device=vals.device)[None, :]).sum(0)
    out = np.empty((vals.shape[1], 5))
    out[:, 0] = obs
    out[:, 1], out[:, 2], out[:, 3] = (x[0].cpu().numpy() for x in (res.mean, res.lo, res.hi))
    out[:, 4] = ge.cpu().numpy() / float(n)
    return out


def coverage(stats):
    """share of the reported rows (finite mean) of stats [K, 5] whose observed value lies inside the HPD"""
    rep = np.isfinite(stats[:, 1])
    if not rep.any():
        return float("nan")
    s = stats[rep]
    return float(np.mean((s[:, 0] >= s[:, 2]) & (s[:, 0] <= s[:, 3])))


def draw_rates(flat_rows, idx, n_bins):
    """per-bin rates [R, n_bins] of the drawn rows (device): (lam_bins, mu_bins)"""
    from . import ops
    import torch
    rows = flat_rows[torch.as_tensor(idx, device=flat_rows.device)]
    H, K = LR_TRACE_HEAD, LR_KMAX
    out = []
    for k_col, base in ((6, H), (7, H + 2 * K - 1)):
        times = torch.cat([rows[:, 8:9], rows[:, base + K:base + 2 * K - 1], rows[:, 9:10]], dim=1).contiguous()
        rates = rows[:, base:base + K].contiguous()
        Kc = rows[:, k_col].to(torch.int32)
        # (lr_expand_rates takes at most 65535 rows a call)
        out.append(torch.cat([ops.expand_rates(rates[a:a + 65535], times[a:a + 65535], Kc[a:a + 65535], n_bins, mode=0)
                              for a in range(0, rows.shape[0], 65535)]))
    return out[0], out[1]


def chunked_rates(rates_of, par):
    """(lam_bins, mu_bins) of the parameter vectors par [R, W] (device): rates_of on at most 65535 of them a launch (what
    lr_dd_rates and lr_trend_rates take), its first two results"""
    import torch
    parts = [rates_of(par[a:a + 65535])[:2] for a in range(0, par.shape[0], 65535)]
    return torch.cat([q[0] for q in parts]), torch.cat([q[1] for q in parts])


def _check(R, sp, ex, spb, seed, free_sim, step_sim, start_bin, capacity, start_time):
    """Steps 2 - 4 around two simulator calls -> (div_obs, b0, cap, free, step, table, fit).  free_sim(b0, n_start, seed, cap)
    runs R replicates over bins b0 .. n_bins - 1; step_sim(b0, n1, seed, cap) runs the (n_bins - b0) * R one-bin replicates
    from n1 (device, replicate (b - b0) * R + i); both return (counts, totals) on the device."""
    import torch
    n_bins = len(sp)
    div_obs = observed_diversity(sp, ex)
    b0 = pick_start_bin(div_obs, start_bin)
    cap = int(capacity) if capacity else default_capacity(sp)
    nf = n_bins - b0                                                    # bins simulated

    # free-running
    fc, ft = free_sim(b0, int(div_obs[b0]), seed, cap)
    dev = fc.device
    keep_f = ft[:, 2] == 0
    n_f = int(keep_f.sum())
    if int(round(0.95 * n_f)) < 2:
        raise _too_few("free-running", n_f, R, cap)
    fk, tk = fc[keep_f], ft[keep_f]
    vals = torch.cat([fk[:, 2, 1:], tk[:, 1:2], fk[:, 0].sum(1, keepdim=True), fk[:, 1].sum(1, keepdim=True)], dim=1).double()
    obs = np.concatenate([div_obs[b0 + 1:], [sp[b0:].sum(), ex[b0:].sum()]])
    fs = _summarise(vals, obs)                                          # [nf + 2, 5]: diversity at b0 + 1 .. n_bins, births, deaths

    # one step ahead: replicate (b - b0) * R + i
    real = div_obs[b0:n_bins] >= 1
    n1 = torch.as_tensor(np.repeat(div_obs[b0:n_bins], R), device=dev)
    sc, st = step_sim(b0, n1, seed + R, cap)
    sc, st = sc.reshape(nf, R, 4), st.reshape(nf, R, 4)
    real_d = torch.as_tensor(real, device=dev)
    keep_s = ~((st[:, :, 2] != 0) & real_d[:, None]).any(0)
    n_s = int(keep_s.sum())
    if int(round(0.95 * n_s)) < 2:
        raise _too_few("one-step", n_s, R, cap)
    sk = sc[:, keep_s]                                                  # [nf, n_s, 4]
    vals = torch.cat([sk[:, :, 0].t(), sk[:, :, 1].t()], dim=1).double()
    ss = _summarise(vals, np.concatenate([sp[b0:], ex[b0:]]))           # [2 nf, 5]
    ss[np.concatenate([~real, ~real]), 1:] = np.nan

    table = np.full((n_bins, 16), np.nan)
    table[:, 0] = float(start_time) + np.arange(n_bins)
    table[:, 1], table[:, 6], table[:, 11] = sp, ex, div_obs[:n_bins]
    table[b0:, 1:6], table[b0:, 6:11] = ss[:nf], ss[nf:]
    table[b0 + 1:, 11:16] = fs[:nf - 1]
    fit = dict(draws=R, steps_per_bin=spb, start_bin=b0, n_start=int(div_obs[b0]), free_kept=n_f, free_overflowed=R - n_f,
               free_extinct=int((tk[:, 1] == 0).sum()), step_kept=n_s, step_overflowed=R - n_s,
               step_extinct=int((st[:, keep_s][:, :, 1] == 0)[real_d].sum()))
    for name, row in zip(("end_diversity", "total_births", "total_deaths"), fs[nf - 1:]):
        for s, v in zip(STATS, row):
            fit["%s_%s" % (name, s)] = float(v)
    fit["coverage_sp_events"], fit["coverage_ex_events"] = coverage(table[:, 1:6]), coverage(table[:, 6:11])
    fit["coverage_diversity"] = coverage(table[:, 11:16])
    host = lambda t: t.cpu().numpy()
    return (div_obs, b0, cap, dict(counts=host(fc), totals=host(ft), kept=host(keep_f)),
            dict(counts=host(sc), totals=host(st), kept=host(keep_s), simulated=real), table, fit)


def posterior_predictive_rates(lam_bins, mu_bins, sp_events, ex_events, steps_per_bin, seed, start_bin=None, capacity=None,
                               start_time=0.0, draw_rows=None):
    """Steps 2 - 5 of the module docstring on per-bin rates given directly: lam_bins, mu_bins [R, n_bins], one row per
    draw (what trend_rate.py's check passes: ops.trend_rates of the drawn rows) -> PpcResult.  draw_rows: the trace rows
    the draws came from, for the result (default 0 .. R - 1)."""
    from . import ops
    import torch
    sp, ex = np.asarray(sp_events, dtype=np.int64), np.asarray(ex_events, dtype=np.int64)
    shape = tuple(np.shape(lam_bins))
    if len(shape) != 2 or tuple(np.shape(mu_bins)) != shape or shape[1] != len(sp) or len(ex) != len(sp):
        raise ValueError("lam_bins and mu_bins must both be [draws, n_bins], with one bin per entry of sp_events / ex_events")
    if shape[0] < 1:
        raise ValueError("posterior predictive check: no draws")
    pick_start_bin(observed_diversity(sp, ex), start_bin)               # (refused before anything is launched)
    lam = ops._dev(lam_bins, torch.float64)
    mu = ops._dev(mu_bins, torch.float64, lam.device)
    R, dev = int(lam.shape[0]), lam.device
    spb, seed = int(steps_per_bin), int(seed)

    def free_sim(b0, n_start, seed_, cap):
        return ops.simulate_bd_batch(lam[:, b0:], mu[:, b0:], spb, n_start, seed_, capacity=cap, device=dev)

    def step_sim(b0, n1, seed_, cap):
        lam1 = lam[:, b0:].t().reshape(-1, 1).contiguous()
        mu1 = mu[:, b0:].t().reshape(-1, 1).contiguous()
        return ops.simulate_bd_batch(lam1, mu1, spb, n1, seed_, capacity=cap, device=dev)

    div_obs, b0, cap, free, step, table, fit = _check(R, sp, ex, spb, seed, free_sim, step_sim, start_bin, capacity, start_time)
    idx = np.arange(R, dtype=np.int64) if draw_rows is None else np.asarray(draw_rows, dtype=np.int64)
    return PpcResult(idx, lam.cpu().numpy(), mu.cpu().numpy(), div_obs, b0, int(div_obs[b0]), cap, (seed, seed + R), free,
                     step, table, fit)


def posterior_predictive(rows, sp_events, ex_events, n_draws, steps_per_bin, seed, start_bin=None, capacity=None,
                         start_time=0.0):
    """The check described in the module docstring on post-burn-in trace rows [S', C, LR_TRACE_W] -> PpcResult.
    start_time: the time of the left edge of bin 0 (only labels the table's rows)."""
    if rows.dim() != 3 or rows.shape[2] != LR_TRACE_W:
        raise ValueError("rows must be [samples, chains, LR_TRACE_W]")
    sp = np.asarray(sp_events, dtype=np.int64)
    div_obs = observed_diversity(sp, ex_events)
    pick_start_bin(div_obs, start_bin)                                  # (refused before anything is launched)
    flat = rows.reshape(-1, LR_TRACE_W)
    idx = draw_indices(flat.shape[0], n_draws)
    lam, mu = draw_rates(flat, idx, len(sp))
    return posterior_predictive_rates(lam, mu, sp, ex_events, steps_per_bin, seed, start_bin, capacity, start_time,
                                      draw_rows=idx)


def dd_arg_error(burnin, rm_first_bin, n_draws=1, steps_per_bin=1):
    """Why DDRate.py's / trend_rate.py's --ppc BURNIN cannot run (None when it can)."""
    if not (0.0 <= burnin < 1.0):
        return "--ppc takes a burn-in fraction in [0, 1)"
    if rm_first_bin:
        return ("--ppc starts its simulations from the observed diversity, counted up from the first bin; under "
                "-rm_first_bin 1 the lineages born in the removed bin are missing from that count: not supported together")
    if n_draws < 1 or steps_per_bin < 1:
        return "--ppc_draws and --ppc_scale must be at least 1"
    return None


def posterior_predictive_dd(rows, sp_events, ex_events, DT, time_range, m_birth, m_death, n_draws, steps_per_bin, seed,
                            start_bin=None, capacity=None, start_time=0.0):
    """DDRate.py's check: steps 1 - 5 of the module docstring with the diversity-dependent simulator
    (ops.simulate_dd_batch) in both sets of replicates -> PpcResult.  rows: post-burn-in trace rows [S', C, LR_TRACE_W]
    of a DDRate engine; a draw's parameters are its columns 4:12 (l_max, k, x0, div_0, L, m_max, nuB, nuD).  The rates of
    every simulated step follow the count living at that step, in the place the model gives to DT[b] (the lineage-time
    lived in bin b is not known before the bin is over; the reference's simulators feed back the count too):
    free-running - draw i runs from div_obs[b0] with x = time_range[b0:] (seed + i);
    one step ahead - replicate (b - b0) * R + i is ONE bin from div_obs[b] with x = time_range[b] (seed + R + that
    index): the feedback acts inside the bin.
    lam_bins / mu_bins of the result are ops.dd_rates of the draws at the OBSERVED DT (the log's l_i / m_i columns), for
    the reader: they do not enter the simulation."""
    from . import ops
    import torch
    if rows.dim() != 3 or rows.shape[2] != LR_TRACE_W:
        raise ValueError("rows must be [samples, chains, LR_TRACE_W]")
    sp, ex = np.asarray(sp_events, dtype=np.int64), np.asarray(ex_events, dtype=np.int64)
    n_bins = len(sp)
    DT, x = np.asarray(DT, dtype=np.float64), np.asarray(time_range, dtype=np.float64)
    if len(ex) != n_bins or len(DT) != n_bins or len(x) != n_bins:
        raise ValueError("sp_events, ex_events, DT and time_range must hold one entry per bin")
    div_obs = observed_diversity(sp, ex)
    pick_start_bin(div_obs, start_bin)                                  # (refused before anything is launched)
    flat = rows.reshape(-1, LR_TRACE_W)
    idx = draw_indices(flat.shape[0], n_draws)
    R = len(idx)
    par = flat[torch.as_tensor(idx, device=flat.device)][:, 4:12].contiguous()
    dev = par.device
    spb, seed, mb, md = int(steps_per_bin), int(seed), int(m_birth), int(m_death)
    lam, mu = chunked_rates(lambda q: ops.dd_rates(q, DT, mb, md), par)
    xd = torch.as_tensor(x, device=dev)

    def free_sim(b0, n_start, seed_, cap):
        return ops.simulate_dd_batch(par, xd[b0:], spb, n_start, seed_, mb, md, capacity=cap, device=dev)

    def step_sim(b0, n1, seed_, cap):
        nf = n_bins - b0
        return ops.simulate_dd_batch(par.repeat(nf, 1), xd[b0:].repeat_interleave(R)[:, None], spb, n1, seed_, mb, md,
                                     capacity=cap, device=dev)

    div_obs, b0, cap, free, step, table, fit = _check(R, sp, ex, spb, seed, free_sim, step_sim, start_bin, capacity, start_time)
    return PpcResult(idx, lam.cpu().numpy(), mu.cpu().numpy(), div_obs, b0, int(div_obs[b0]), cap, (seed, seed + R), free,
                     step, table, fit)


def write_tables(stem, table, fit):
    """<stem>_PPC.tsv (PPC_HEAD, one row per bin: time = the bin's left edge; sp_events / ex_events one step ahead,
    diversity at the left edge free-running; nan where nothing was simulated) and <stem>_PPC_fit.tsv (FIT_HEAD, one row).
    Numbers as str(float), counts as integers, as the other summary writers write them."""
    with open(stem + "_PPC.tsv", "w") as f:
        f.write("\t".join(PPC_HEAD) + "\n")
        for row in np.asarray(table, dtype=float):
            f.write("\t".join(str(float(v)) for v in row) + "\n")
    with open(stem + "_PPC_fit.tsv", "w") as f:
        f.write("\t".join(FIT_HEAD) + "\n")
        f.write("\t".join(["%d" % fit[k] for k in FIT_HEAD[:N_FIT_INTS]] + [str(float(fit[k])) for k in FIT_HEAD[N_FIT_INTS:]]) + "\n")


def arg_error(burnin, model, pyrate_output):
    """Why LiteRateForward.py's --ppc BURNIN cannot run (None when it can)."""
    if not (0.0 <= burnin < 1.0):
        return "--ppc takes a burn-in fraction in [0, 1)"
    if model == 1:
        return ("--ppc simulates births as per-lineage events; under -model_BDI 1 (immigration-death) new lineages do not "
                "come from living ones, so the scheme does not apply: not supported together")
    if pyrate_output:
        return ("--ppc bins the AD / TBP times of the trace; -pyrate_output flips them in the logs: not supported "
                "together")
    return None


def write_run_ppc(eng, sp_events, ex_events, n_local, total_chains, world, rank, burnin, n_draws, steps_per_bin, seed, stem,
                  start_bin=None):
    """LiteRateForward.py's --ppc: the check on the rows the run sampled, int(burnin * S) dropped per chain, on rank 0
    (the rows are gathered to its device once when the chains are sharded) -> the two files and one line on stdout."""
    rows = _gathered_rows(eng, n_local, total_chains, world, burnin)
    if rank != 0:
        return None
    res = posterior_predictive(rows, sp_events, ex_events, n_draws, steps_per_bin, seed, start_bin=start_bin,
                               start_time=np.floor(eng.start_time))
    return _write_and_say(stem, res)


def _write_and_say(stem, res):
    write_tables(stem, res.table, res.fit)
    print("posterior predictive check: %s_PPC.tsv, %s_PPC_fit.tsv (%d draws from bin %d; overflowed: %d free-running, "
          "%d one-step)" % (stem, stem, res.fit["draws"], res.start_bin, res.fit["free_overflowed"],
                            res.fit["step_overflowed"]))
    return res


def _gathered_rows(eng, n_local, total_chains, world, burnin):
    """the post-burn-in rows of all chains, [S', total_chains, LR_TRACE_W], on this rank's device (every rank calls)"""
    from . import dist as lrd
    S = eng.samples_done()
    local = eng.trace[int(burnin * S):S][:, :n_local]
    return lrd.gather_traces(local.contiguous(), total_chains) if world > 1 else local


def write_run_ppc_dd(eng, n_local, total_chains, world, rank, burnin, n_draws, steps_per_bin, seed, stem, start_bin=None):
    """DDRate.py's --ppc: posterior_predictive_dd on the rows the run sampled, int(burnin * S) dropped per chain, against
    create_bins' event counts, on rank 0 -> the two files and one line on stdout."""
    rows = _gathered_rows(eng, n_local, total_chains, world, burnin)
    if rank != 0:
        return None
    res = posterior_predictive_dd(rows, eng.n_spec, eng.n_exti, eng.DT, eng.time_range, eng.m_birth, eng.m_death, n_draws,
                                  steps_per_bin, seed, start_bin=start_bin, start_time=float(eng.origin))
    return _write_and_say(stem, res)


def write_run_ppc_trend(eng, n_local, total_chains, world, rank, burnin, n_draws, steps_per_bin, seed, stem, start_bin=None):
    """trend_rate.py's --ppc: the rates of the drawn rows by the engine's draw_rates (fixed per bin: the covariate is data),
    then posterior_predictive_rates, on rank 0 -> the two files and one line on stdout."""
    rows = _gathered_rows(eng, n_local, total_chains, world, burnin)
    if rank != 0:
        return None
    flat = rows.reshape(-1, LR_TRACE_W)
    idx = draw_indices(flat.shape[0], n_draws)
    lam, mu = eng.draw_rates(flat, idx)
    res = posterior_predictive_rates(lam, mu, eng.n_spec, eng.n_exti, steps_per_bin, seed, start_bin=start_bin,
                                     start_time=float(eng.origin), draw_rows=idx)
    return _write_and_say(stem, res)
