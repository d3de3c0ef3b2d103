"""The Metropolis-coupled RJ sampler (include/literate_hip_rjmc3.h) restated in numpy: TEST INFRASTRUCTURE.

    start, step      one replica: oracle.mcmc_oracle.run_mcmc's head and its loop body, statement for statement, as functions of
                     a state - with the one change that the likelihood difference of the acceptance test is times beta
    row_of           run_mcmc's row of a state
    swap_round       round n of a ladder: the pairs (j, j + 1), j = n % 2, n % 2 + 2, ...
    run_chain_from   one chain at beta 1 from iteration it0 on (tests/helpers/long_run.py)
    run_ladder       T replicas, the swap rounds among their iterations, the rows of the replica at position 0, the ladder
                     buffer, the swap counts, the final states

All draws are PhiloxDraws' (purposes 0 .. 10); the swap uniform is the first of oracle.philox's Stream(seed, key of replica
0).pair(it, P_SWAP, j), P_SWAP = 11.  Every acceptance decision's margin - how far its left side is from log u - is recorded,
the swaps' too: a test asserts on the CPU that none is so small that the device's last bits could decide otherwise.
"""
import numpy as np

from oracle import literate_oracle as lo
from oracle import mcmc_oracle as mo
from oracle import philox as px

P_SWAP = 11


def ladder_betas(T, dt):
    return [1.0 / (1.0 + dt * j) for j in range(T)]


def start(stats, start_time, end_time, st, draws, init=None):
    """run_mcmc's lines before the loop -> the state of a replica"""
    n_bins = len(stats["sp"])
    if init is None:
        L, M = draws.init_rates()
        tL = np.array([start_time, end_time], dtype=float)
        tM = np.array([start_time, end_time], dtype=float)
    else:
        L, M, tL, tM = [np.array(x, dtype=float) for x in init]
    S = dict(L=L, M=M, tL=tL, tM=tM, Poi=1 if st.Poisson_HP == 0 else st.Poisson_HP, Gamma_rate=[1., 1.], accepted=0)
    S["indL"], S["indM"] = lo.get_rate_index(tL, n_bins), lo.get_rate_index(tM, n_bins)
    S["likA"] = lo.calc_likelihood(st.model_BDI, L[S["indL"]], M[S["indM"]], stats)
    priorA = lo.prior_gamma(L) + lo.prior_gamma(M)
    priorA += -np.log(end_time - start_time) * (len(L) - 1 + len(M) - 1)
    S["priorPoiA"] = lo.Poisson_prior(len(L), S["Poi"]) + lo.Poisson_prior(len(M), S["Poi"])
    S["priorA"] = priorA + S["priorPoiA"]
    return S


def step(S, stats, start_time, end_time, st, draws, it, beta=1.0, k_max=None, margins=None):
    """run_mcmc's loop body on state S (changed in place); accepts iff beta (lik - likA) + prior - priorA + hasting >= log u.
    Returns True when an add move met k_max.  margins: a list the decision's margin is appended to (not for Gibbs steps and
    invalid proposals, which no last bit decides)."""
    n_bins = len(stats["sp"])
    L_acc, M_acc, timesLA, timesMA = S["L"], S["M"], S["tL"], S["tM"]
    r0, r1 = draws.move(it)
    L, timesL = L_acc + 0, timesLA + 0
    M, timesM = M_acc + 0, timesMA + 0
    indL, indM = S["indL"], S["indM"]
    hasting, gibbs, priorPoi, forced_reject = 0, 0, 0, False
    if st.const_death_rate:
        sample_shift_mu, b_freq, d_freq = 0, 0.7, 0.8
        fL, fM = st.update_fraction, 1
    else:
        sample_shift_mu, b_freq, d_freq = 0.5, 0.4, 0.8
        fL, fM = st.update_fraction, st.update_fraction
    if r0 < b_freq:
        if r1 < .5 or len(L_acc) == 1:
            L, hasting = lo.update_multiplier_freq(L_acc, *draws.multiplier(it, len(L_acc), fL))
        else:
            draws.times_move(it, len(L_acc))
            timesL = np.sort(timesLA + 0.)
            indL = lo.get_rate_index(np.floor(timesL), n_bins)
    elif r0 < d_freq:
        if r1 < .5 or len(M_acc) == 1:
            M, hasting = lo.update_multiplier_freq(M_acc, *draws.multiplier(it, len(M_acc), fM))
        else:
            draws.times_move(it, len(M_acc))
            timesM = np.sort(timesMA + 0.)
            indM = lo.get_rate_index(np.floor(timesM), n_bins)
    elif r0 < 0.999 and st.const_rates == 0:
        L, timesL, M, timesM, hasting, update_L, forced_reject = mo._rjmcmc(draws, it, L_acc, M_acc, timesLA, timesMA,
                                                                          sample_shift_mu, k_max)
        if update_L == 1:
            indL = lo.get_rate_index(np.floor(timesL), n_bins)
        else:
            indM = lo.get_rate_index(np.floor(timesM), n_bins)
        priorPoi = lo.Poisson_prior(len(L), S["Poi"]) + lo.Poisson_prior(len(M), S["Poi"])
    else:
        if st.Poisson_HP == 0:
            S["Poi"] = draws.gibbs_poi(it, *lo.rj_hp_posterior_params(len(L_acc), len(M_acc)))
        if st.use_rate_HP:
            S["Gamma_rate"] = [draws.gibbs_rate(it, 0, *lo.rate_hp_posterior_params(L_acc)),
                               draws.gibbs_rate(it, 1, *lo.rate_hp_posterior_params(M_acc))]
        gibbs = 1
    invalid = (min(abs(np.diff(timesL))) <= lo.MIN_ALLOWED_T or min(abs(np.diff(timesM))) <= lo.MIN_ALLOWED_T or forced_reject)
    if invalid:
        prior, lik = -np.inf, -np.inf
    else:
        prior = lo.prior_gamma(L, lo.GAMMA_SHAPE, S["Gamma_rate"][0]) + lo.prior_gamma(M, lo.GAMMA_SHAPE, S["Gamma_rate"][1])
        prior += -np.log(end_time - start_time) * (len(L) - 1 + len(M) - 1)
        if priorPoi != 0:
            prior += priorPoi
        else:
            prior += S["priorPoiA"]
            priorPoi = S["priorPoiA"]
        lik = lo.calc_likelihood(st.model_BDI, L[indL], M[indM], stats) if gibbs == 0 else S["likA"]
    u = draws.accept(it)
    with np.errstate(divide="ignore", invalid="ignore"):
        # (invalid proposals are rejected before the multiply: no 0 * inf)
        lhs = -np.inf if invalid else beta * (lik - S["likA"]) + prior - S["priorA"] + hasting
        ok = (lhs >= np.log(u)) or gibbs == 1
        if margins is not None and gibbs == 0 and not invalid:
            margins.append(abs(lhs - np.log(u)))
    if ok:
        S["L"], S["M"], S["tL"], S["tM"] = L, M, timesL, timesM
        S["likA"], S["priorA"], S["indL"], S["indM"], S["priorPoiA"] = lik, prior, indL, indM, priorPoi
        S["accepted"] += 1
    return bool(forced_reject)


def row_of(S, it, start_time, end_time):
    """(mcmc row, sp row, ex row) of run_mcmc for the state"""
    head = np.array([it, S["likA"] + S["priorA"], S["likA"], S["priorA"], np.mean(S["L"]), np.mean(S["M"]), len(S["L"]), len(S["M"]),
                     start_time, end_time, S["Gamma_rate"][0], S["Gamma_rate"][1], S["Poi"]], dtype=float)
    return (head, np.concatenate([S["L"], S["tL"][1:len(S["tL"]) - 1]]), np.concatenate([S["M"], S["tM"][1:len(S["tM"]) - 1]]))


def swap_round(n, pos, lik, betas, uniform, counts=None, margins=None):
    """Round n on a ladder: pos[r] the position of replica r (a permutation of 0 .. T - 1), lik[r] its likA, uniform(j) the
    u of the pair of positions (j, j + 1).  Returns the new pos; counts [T - 1][2] += (proposed, accepted)."""
    T = len(pos)
    pos = list(pos)
    for j in range(n % 2, T - 1, 2):
        a, b = pos.index(j), pos.index(j + 1)
        with np.errstate(divide="ignore"):
            d, lu = (betas[j] - betas[j + 1]) * (lik[b] - lik[a]), np.log(uniform(j))
        if margins is not None:
            margins.append(abs(d - lu))
        if counts is not None:
            counts[j][0] += 1
        if d >= lu:
            pos[a], pos[b] = j + 1, j
            if counts is not None:
                counts[j][1] += 1
    return pos


def run_chain_from(stats, start_time, end_time, st, seed, key, it0, n_it, s_freq, k_max=32, remap=None):
    """One chain (beta 1) from its initial state through iterations it0 .. it0 + n_it - 1, as lr_rjbin_steps runs them when it is
    given it0: draws, rows (it % s_freq == 0) and the iteration column by the true iteration.  remap: iteration -> the address
    the draws are made at instead (a broken counter, for the tests' power).  -> dict(mcmc, sp, ex: run_mcmc's rows; state: the
    final one; margin: the smallest of the decisions; overflows)"""
    at = remap or (lambda it: it)
    draws = mo.PhiloxDraws(seed, key)
    S = start(stats, start_time, end_time, st, draws)
    out = dict(mcmc=[], sp=[], ex=[], overflows=0)
    margins = []
    for it in range(it0, it0 + n_it):
        with np.errstate(all="ignore"):
            out["overflows"] += step(S, stats, start_time, end_time, st, draws, at(it), 1.0, k_max, margins)
        if it % s_freq == 0:
            head, sp, ex = row_of(S, it, start_time, end_time)
            out["mcmc"].append(head), out["sp"].append(sp), out["ex"].append(ex)
    out["state"], out["margin"] = S, (min(margins) if margins else np.inf)
    return out


def run_ladder(stats, start_time, end_time, st, seed, key0, betas, swap_every, n_it, s_freq, k_max=32, inits=None, it0=0,
               remap=None):
    """One ladder: replica w draws from PhiloxDraws(seed, key0 + w) and starts at position w (the keys, the swap stream's key0
    too, modulo 2^32); iterations it0 .. it0 + n_it - 1 from the initial states (lr_rjmc3_steps given it0: the swap rounds'
    numbers and the rows follow the true iteration; remap: as run_chain_from's, the swap uniforms' address included).  ->
    dict(mcmc, sp, ex: the rows of the replica at position 0, as run_mcmc's; ladder [S, T, 4]; swaps [T - 1, 2]; states, pos: the
    final ones; margin: the smallest of all decisions; overflows)"""
    T = len(betas)
    at = remap or (lambda it: it)
    draws = [mo.PhiloxDraws(seed, (key0 + w) % 2 ** 32) for w in range(T)]
    swap_stream = px.Stream(seed, key0 % 2 ** 32)
    states = [start(stats, start_time, end_time, st, draws[w], None if inits is None else inits[w]) for w in range(T)]
    pos = list(range(T))
    out = dict(mcmc=[], sp=[], ex=[], ladder=[], swaps=[[0, 0] for _ in range(T - 1)], overflows=0)
    margins = []
    for it in range(it0, it0 + n_it):
        for w in range(T):
            with np.errstate(all="ignore"):
                out["overflows"] += step(states[w], stats, start_time, end_time, st, draws[w], at(it), betas[pos[w]], k_max, margins)
        if it % s_freq == 0:
            head, sp, ex = row_of(states[pos.index(0)], it, start_time, end_time)
            out["mcmc"].append(head), out["sp"].append(sp), out["ex"].append(ex)
            out["ladder"].append([[float(pos.index(j)), states[pos.index(j)]["likA"], float(len(states[pos.index(j)]["L"])),
                                   float(len(states[pos.index(j)]["M"]))] for j in range(T)])
        if swap_every > 0 and (it + 1) % swap_every == 0:
            pos = swap_round((it + 1) // swap_every, pos, [s["likA"] for s in states], betas,
                             lambda j: swap_stream.pair(at(it), P_SWAP, j)[0], out["swaps"], margins)
    out["ladder"], out["swaps"] = np.array(out["ladder"], dtype=float).reshape(-1, T, 4), np.array(out["swaps"], dtype=np.int64).reshape(T - 1, 2)
    out["states"], out["pos"], out["margin"] = states, pos, (min(margins) if margins else np.inf)
    return out
