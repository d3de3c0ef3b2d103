// lr_rjbin_iter.h - one chain of runMCMC (LRF:216-373) on per-bin statistics, held by one wave: the device code and the host
// checks that lr_rjbin.hip (one wave per chain, no wave waits for another) and lr_rjmc3.hip (the waves of a workgroup are the
// rungs of a temperature ladder and exchange their positions) share.  The iteration exists once, here:
//
//   lr_rjbin_bins<BPL>       a lane's bins of the replicate's statistics, in registers for the whole launch
//   lr_rjbin_chain           the accepted state of a chain between two iterations (lane j: rate j, shift time j)
//   lr_rjbin_start           the initial state (lr_rjbin_init)
//   lr_rjbin_load / _store   the state buffer's rows (include/literate_hip_rjbin.h)
//   lr_rjbin_iterate<BPL, TEMPERED>   one iteration; TEMPERED: the likelihood difference of the acceptance test times beta
//   lr_rjbin_trace_row       the engines' trace row of the accepted state
//   lr_rjbin_args            the argument checks of both entry points, in the header's order
#pragma once
#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_rjbin.h"
#include "lr_chain.h"
#include "lr_internal.h"

#define LR_RJBIN_UD_LANE 32   /* first of the four lanes holding the wave-uniform draws of an iteration's one Philox call */

static_assert(LR_RJBIN_MAX_BINS == 8 * LR_WAVE, "a lane holds at most 8 bins");
static_assert(LR_RJBIN_STATE_W == (LR_RJBIN_ROW_SCALARS + 1) * LR_ROW && LR_ROW == LR_WAVE, "state layout: rows of one wave");
static_assert(LR_KMAX <= LR_RJBIN_UD_LANE && LR_RJBIN_UD_LANE + 4 <= LR_WAVE, "one lane per rate below the wave-uniform draws");

struct lr_rjbin_cfg {
    double poisson_HP, update_fraction, mult_l;
    long long rows_cap, slot0, chain0;
    int n_bins, n_chains, chains_per_rep, model, const_rates, const_death_rate, use_rate_HP, s_freq;
    uint32_t seed;
};

// a lane's bins: b = lane + 64 i.  d_ex, d_br: the death half's statistics (model 3: the _dead pair); lk = log br
template <int BPL>
struct lr_rjbin_bins {
    double sp[BPL], br[BPL], d_ex[BPL], d_br[BPL], lk[BPL];
};

// the accepted state; lg0, lg1, lpoi: the logarithms of g0, g1, poi (kept by lr_rjbin_load and lr_rjbin_iterate)
struct lr_rjbin_chain {
    double L, M, tL, tM, likA, priorA, priorPoiA, g0, g1, poi, n_acc, lg0, lg1, lpoi;
    int eL, eM, KL, KM;
};

// what an iteration reads beside the state and does not change: the replicate's times and the move frequencies
struct lr_rjbin_run {
    double t_start, t_end, log_T, sample_shift_mu, b_freq, d_freq, fL, fM;
};

__device__ __forceinline__ lr_rjbin_run lr_rjbin_run_of(const lr_rjbin_cfg& cfg, double t_start, double t_end) {
    lr_rjbin_run r;
    r.t_start = t_start, r.t_end = t_end, r.log_T = lr_log(t_end - t_start);
    r.sample_shift_mu = cfg.const_death_rate ? 0.0 : 0.5;
    r.b_freq = cfg.const_death_rate ? 0.7 : 0.4, r.d_freq = 0.8;
    r.fL = cfg.update_fraction, r.fM = cfg.const_death_rate ? 1.0 : cfg.update_fraction;
    return r;
}

template <int BPL>
__device__ __forceinline__ void lr_rjbin_load_bins(lr_rjbin_bins<BPL>& B, const double* __restrict__ sp, const double* __restrict__ ex,
                                                   const double* __restrict__ br, const double* __restrict__ ex_dead,
                                                   const double* __restrict__ br_dead, int rep, int model, int n_bins, int lane) {
    const size_t o = (size_t)rep * n_bins;
    const double* dex = model == LR_MODEL_KEIDING_DEAD ? ex_dead : ex;
    const double* dbr = model == LR_MODEL_KEIDING_DEAD ? br_dead : br;
#pragma unroll
    for (int i = 0; i < BPL; ++i) {
        const int b = lane + LR_WAVE * i;
        const bool in = b < n_bins;
        B.sp[i] = in ? sp[o + b] : 0.0, B.br[i] = in ? br[o + b] : 0.0;
        B.d_ex[i] = in ? dex[o + b] : 0.0, B.d_br[i] = in ? dbr[o + b] : 0.0;
        B.lk[i] = (model < 2 && B.br[i] > 0.0) ? lr_log(B.br[i]) : 0.0;
    }
}

// the rate and its logarithm of every bin of the lane: segment j holds for edge[j] <= b (the last such j wins)
template <int BPL>
__device__ __forceinline__ void lr_rjbin_expand(double R, double logR, int E, int K, int lane, double (&r)[BPL], double (&lr)[BPL]) {
    const double r0 = lr_bcast(R, 0), l0 = lr_bcast(logR, 0);
#pragma unroll
    for (int i = 0; i < BPL; ++i) r[i] = r0, lr[i] = l0;
    for (int j = 1; j < K; ++j) {
        const double rj = lr_bcast(R, j), lj = lr_bcast(logR, j);
        const int ej = lr_bcast_i(E, j);
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const bool in = lane + LR_WAVE * i >= ej;
            r[i] = in ? rj : r[i], lr[i] = in ? lj : lr[i];
        }
    }
}

// calc_likelihood (LRF:137-162) of rates L (lane j, K_l of them; logL their logarithms) on edges eL, and M likewise
template <int BPL>
__device__ __forceinline__ double lr_rjbin_loglik(const lr_rjbin_bins<BPL>& B, int model, int n_bins, double L, double logL, int eL,
                                                  int KL, double M, double logM, int eM, int KM, int lane) {
    double lam[BPL], llam[BPL], mu[BPL], lmu[BPL];
    lr_rjbin_expand<BPL>(L, logL, eL, KL, lane, lam, llam);
    lr_rjbin_expand<BPL>(M, logM, eM, KM, lane, mu, lmu);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < BPL; ++i) {
        const int b = lane + LR_WAVE * i;
        double t;
        if (model >= 2) {
            t = (llam[i] * B.sp[i] - lam[i] * B.br[i]) + (lmu[i] * B.d_ex[i] - mu[i] * B.d_br[i]);
        } else {
            const double k = B.br[i];
            const double ev = B.sp[i] * (model == 0 ? B.lk[i] + llam[i] : llam[i]) + B.d_ex[i] * (lmu[i] + B.lk[i]);
            const double xp = model == 0 ? k * (lam[i] + mu[i]) : k * mu[i] + lam[i];
            t = k > 0.0 ? ev - xp : 0.0;
        }
        acc += b < n_bins ? t : 0.0;
    }
    return lr_wave_sum(acc);
}

// log of the rates of both processes in one call: lanes 0-31 the birth rates, lanes 32-63 the death rates
__device__ __forceinline__ void lr_rjbin_log_rates(double L, double M, int lane, double* logL, double* logM) {
    const double Mhi = lr_half_lo(M);          // lane 32 + j <- M[j]
    const double lx = lr_log(lane < 32 ? L : Mhi);
    *logL = lx, *logM = lr_half_hi(lx);        // lane j <- lx[32 + j] (j < 32; the lanes above hold no rate)
}

// the initial state of chain c: the six arrays' (all or none), or the CLI's start (LRF:580-583)
template <int BPL>
__device__ __forceinline__ void lr_rjbin_start(lr_rjbin_chain& S, const lr_rjbin_bins<BPL>& B, const lr_rjbin_cfg& cfg,
                                               const lr_rjbin_run& run, const lr_stream& rng, size_t c, const double* __restrict__ L0,
                                               const double* __restrict__ M0, const double* __restrict__ tL0,
                                               const double* __restrict__ tM0, const int* __restrict__ KL0,
                                               const int* __restrict__ KM0, int lane) {
    double L, M, tL, tM;
    int KL, KM;
    L = M = tL = tM = 0.0, KL = KM = 1;
    if (L0) {
        KL = min(max(KL0[c], 1), LR_KMAX), KM = min(max(KM0[c], 1), LR_KMAX);
        if (lane < KL) L = L0[c * LR_KMAX + lane];
        if (lane < KM) M = M0[c * LR_KMAX + lane];
        if (lane <= KL) tL = tL0[c * (LR_KMAX + 1) + lane];
        if (lane <= KM) tM = tM0[c * (LR_KMAX + 1) + lane];
    } else {
        const double l0 = lr_gamma(rng, 0, LR_P_INIT, 0, 2.0) * 2.0;   // np.random.gamma(2,2,1), LRF:580
        const double m0 = lr_gamma(rng, 0, LR_P_INIT, 64, 2.0) * 2.0;  // LRF:581
        if (lane == 0) L = l0, M = m0, tL = tM = run.t_start;
        if (lane == 1) tL = tM = run.t_end;
    }
    // the initial index comes from get_rate_index on the RAW times: round, not floor (LRF:224-225, 129)
    const int eL = lr_wave_edges(tL, 1), eM = lr_wave_edges(tM, 1);
    double logL, logM;
    lr_rjbin_log_rates(L, M, lane, &logL, &logM);
    S.likA = lr_rjbin_loglik<BPL>(B, cfg.model, cfg.n_bins, L, logL, eL, KL, M, logM, eM, KM, lane);
    S.poi = cfg.poisson_HP == 0.0 ? 1.0 : cfg.poisson_HP, S.g0 = S.g1 = 1.0;          // LRF:220-222
    // the initial prior uses prior_gamma's default rate b = 2 (LRF:201, 227)
    double priorA = lr_wave_prior_gamma(L, KL, LR_GAMMA_SHAPE, 2.0, lane) + lr_wave_prior_gamma(M, KM, LR_GAMMA_SHAPE, 2.0, lane);
    priorA += -run.log_T * (KL - 1 + KM - 1);
    const double lpoi = lr_log(S.poi);
    S.priorPoiA = lr_poisson_prior(KL, S.poi, lpoi) + lr_poisson_prior(KM, S.poi, lpoi);
    priorA += S.priorPoiA;
    S.priorA = priorA, S.n_acc = 0.0;
    S.L = L, S.M = M, S.tL = tL, S.tM = tM, S.eL = eL, S.eM = eM, S.KL = KL, S.KM = KM;
    S.lg0 = S.lg1 = 0.0, S.lpoi = lpoi;
}

__device__ __forceinline__ void lr_rjbin_load(lr_rjbin_chain& S, const double* __restrict__ st, int lane) {
    S.L = st[LR_RJBIN_ROW_L * LR_ROW + lane], S.M = st[LR_RJBIN_ROW_M * LR_ROW + lane];
    S.tL = st[LR_RJBIN_ROW_TL * LR_ROW + lane], S.tM = st[LR_RJBIN_ROW_TM * LR_ROW + lane];
    S.eL = (int)st[LR_RJBIN_ROW_EL * LR_ROW + lane], S.eM = (int)st[LR_RJBIN_ROW_EM * LR_ROW + lane];
    const double sc = st[LR_RJBIN_ROW_SCALARS * LR_ROW + lane];
    S.likA = lr_bcast(sc, LR_RJBIN_S_LIKA), S.priorA = lr_bcast(sc, LR_RJBIN_S_PRIORA), S.priorPoiA = lr_bcast(sc, LR_RJBIN_S_PRIORPOIA);
    S.g0 = lr_bcast(sc, LR_RJBIN_S_GRATE_L), S.g1 = lr_bcast(sc, LR_RJBIN_S_GRATE_M), S.poi = lr_bcast(sc, LR_RJBIN_S_POI);
    S.KL = min(max((int)lr_bcast(sc, LR_RJBIN_S_KL), 1), LR_KMAX), S.KM = min(max((int)lr_bcast(sc, LR_RJBIN_S_KM), 1), LR_KMAX);
    S.n_acc = lr_bcast(sc, LR_RJBIN_S_ACCEPTED);
    const double lx = lr_log(lane == 0 ? S.g0 : (lane == 1 ? S.g1 : (lane == 2 ? S.poi : 1.0)));
    S.lg0 = lr_bcast(lx, 0), S.lg1 = lr_bcast(lx, 1), S.lpoi = lr_bcast(lx, 2);
}

// the state: elements behind a row's length are written as 0, so that a state is a function of the chain alone
__device__ __forceinline__ void lr_rjbin_store(const lr_rjbin_chain& S, double* __restrict__ st, int lane) {
    st[LR_RJBIN_ROW_L * LR_ROW + lane] = lane < S.KL ? S.L : 0.0, st[LR_RJBIN_ROW_M * LR_ROW + lane] = lane < S.KM ? S.M : 0.0;
    st[LR_RJBIN_ROW_TL * LR_ROW + lane] = lane <= S.KL ? S.tL : 0.0, st[LR_RJBIN_ROW_TM * LR_ROW + lane] = lane <= S.KM ? S.tM : 0.0;
    st[LR_RJBIN_ROW_EL * LR_ROW + lane] = lane <= S.KL ? (double)S.eL : 0.0;
    st[LR_RJBIN_ROW_EM * LR_ROW + lane] = lane <= S.KM ? (double)S.eM : 0.0;
    double so = 0.0;
    so = (lane == LR_RJBIN_S_LIKA) ? S.likA : so;
    so = (lane == LR_RJBIN_S_PRIORA) ? S.priorA : so;
    so = (lane == LR_RJBIN_S_PRIORPOIA) ? S.priorPoiA : so;
    so = (lane == LR_RJBIN_S_GRATE_L) ? S.g0 : so;
    so = (lane == LR_RJBIN_S_GRATE_M) ? S.g1 : so;
    so = (lane == LR_RJBIN_S_POI) ? S.poi : so;
    so = (lane == LR_RJBIN_S_KL) ? (double)S.KL : so;
    so = (lane == LR_RJBIN_S_KM) ? (double)S.KM : so;
    so = (lane == LR_RJBIN_S_ACCEPTED) ? S.n_acc : so;
    st[LR_RJBIN_ROW_SCALARS * LR_ROW + lane] = so;
}

// Iteration `it` of the chain.  TEMPERED: the chain samples L^beta * prior - the likelihood difference of the acceptance test
// is multiplied by beta (> 0); a proposal that is invalid is rejected before the multiply, and the Gibbs steps do not see the
// likelihood.
template <int BPL, bool TEMPERED>
__device__ __forceinline__ void lr_rjbin_iterate(lr_rjbin_chain& S, const lr_rjbin_bins<BPL>& B, const lr_rjbin_cfg& cfg,
                                                 const lr_rjbin_run& run, const lr_stream& rng, long long it, double beta,
                                                 unsigned int* __restrict__ warn, int lane) {
    const int model = cfg.model, n_bins = cfg.n_bins;
    // The draws of the iteration in ONE Philox call, at the engines' addresses (lr_propose_rj): lanes 0..31 the
    // multiplier pairs of their rates, lane 32 the acceptance uniform, lane 33 the move selector, lanes 34, 35 the
    // two RJ pairs.
    const int ul = lane - LR_RJBIN_UD_LANE;
    const uint32_t purpose = (ul < 0) ? LR_P_MULT : ((ul == 0) ? LR_P_ACCEPT : (ul == 1 ? LR_P_MOVE : LR_P_RJ));
    const lr_u2 ud = lr_pair(rng, (uint64_t)it, purpose, ul < 0 ? (uint32_t)lane : (ul == 3 ? 1u : 0u));
    const double log_u = lr_bcast(lr_log(ul == 0 ? ud.a : 1.0), LR_RJBIN_UD_LANE);
    const lr_u2 r{lr_bcast(ud.a, LR_RJBIN_UD_LANE + 1), lr_bcast(ud.b, LR_RJBIN_UD_LANE + 1)};

    double pL = S.L, pM = S.M, ptL = S.tL, ptM = S.tM, pg0 = S.g0, pg1 = S.g1, ppoi = S.poi, plg0 = S.lg0, plg1 = S.lg1, plpoi = S.lpoi;
    int peL = S.eL, peM = S.eM, PKL = S.KL, PKM = S.KM;
    double hasting = 0.0, priorPoi = 0.0;
    bool gibbs = false, invalid = false, kcap = false;
    if (r.a < run.b_freq) {
        if (r.b < .5 || S.KL == 1) hasting = lr_wave_multiplier(pL, S.KL, ud.a < run.fL, ud.b, cfg.mult_l, lane);
        else peL = lr_wave_edges(S.tL, 0);          // update_times leaves the times unchanged (LRF:178-195); its draws are not needed
    } else if (r.a < run.d_freq) {
        if (r.b < .5 || S.KM == 1) hasting = lr_wave_multiplier(pM, S.KM, ud.a < run.fM, ud.b, cfg.mult_l, lane);
        else peM = lr_wave_edges(S.tM, 0);
    } else if (r.a < 0.999 && cfg.const_rates == 0) {
        // RJMCMC (LRF:71-97)
        const lr_u2 q{lr_bcast(ud.a, LR_RJBIN_UD_LANE + 2), lr_bcast(ud.b, LR_RJBIN_UD_LANE + 2)};
        const lr_u2 q2{lr_bcast(ud.a, LR_RJBIN_UD_LANE + 3), lr_bcast(ud.b, LR_RJBIN_UD_LANE + 3)};
        const bool sideL = q.a > run.sample_shift_mu;
        double R = sideL ? S.L : S.M, T = sideL ? S.tL : S.tM;
        int K = sideL ? S.KL : S.KM;
        if (q.b > 0.5) {
            if (K >= LR_KMAX) {
                kcap = true;          // the device's cap on the number of rates; the reference has none
            } else {
                const int ind = min((int)(q2.a * K), K - 1);
                const double delta = q2.b * (lr_bcast(T, ind + 1) - lr_bcast(T, ind));
                double ga, gb;
                lr_wave_gamma2(rng, (uint64_t)it, LR_P_BETA_A, LR_SHAPE_BETA_RJ, LR_P_BETA_B, LR_SHAPE_BETA_RJ, lane, &ga, &gb);
                hasting = lr_wave_add_shift(R, T, K, ind, delta, ga / (ga + gb), lane);
            }
        } else if (K > 1) {
            const int idx = 1 + min((int)(q2.a * (K - 1)), K - 2);
            hasting = lr_wave_remove_shift(R, T, K, idx, lane);
        }
        const int E = lr_wave_edges(T, 0);
        if (sideL) pL = R, ptL = T, PKL = K, peL = E;
        else pM = R, ptM = T, PKM = K, peM = E;
        priorPoi = lr_poisson_prior(PKL, S.poi, S.lpoi) + lr_poisson_prior(PKM, S.poi, S.lpoi);
    } else {
        // Gibbs draws of the hyper-parameters (LRF:283-287, 99-108, 210-213)
        double gl = 0.0, gm = 0.0, gp = 0.0, dummy;
        if (cfg.use_rate_HP)
            lr_wave_gamma2(rng, (uint64_t)it, LR_P_GIBBS_L, LR_HP_GAMMA_SHAPE + LR_GAMMA_SHAPE * S.KL, LR_P_GIBBS_M,
                           LR_HP_GAMMA_SHAPE + LR_GAMMA_SHAPE * S.KM, lane, &gl, &gm);
        if (cfg.poisson_HP == 0.0) {
            lr_wave_gamma2(rng, (uint64_t)it, LR_P_GIBBS_POI, LR_RJHP_SHAPE + S.KL + S.KM, LR_P_GIBBS_POI, LR_RJHP_SHAPE + S.KL + S.KM,
                           lane, &gp, &dummy);
            ppoi = gp * (1. / (LR_RJHP_RATE + 2));
        }
        if (cfg.use_rate_HP) {
            const double sL = lr_wave_sum(lane < S.KL ? S.L : 0.0), sM = lr_wave_sum(lane < S.KM ? S.M : 0.0);
            pg0 = gl * (1. / (LR_HP_GAMMA_RATE + sL));
            pg1 = gm * (1. / (LR_HP_GAMMA_RATE + sM));
        }
        const double lx = lr_log(lane == 0 ? pg0 : (lane == 1 ? pg1 : (lane == 2 ? ppoi : 1.0)));
        plg0 = lr_bcast(lx, 0), plg1 = lr_bcast(lx, 1), plpoi = lr_bcast(lx, 2);
        gibbs = true;
    }

    // guard against tiny time frames (LRF:290-292), then the prior (LRF:296-304) and the likelihood of the proposal
    {
        const double nL = lr_dpp_zero<0x130 /* wave_shl:1 */, 0xf, 0xf>(ptL);   // lane l <- element l + 1
        const double nM = lr_dpp_zero<0x130, 0xf, 0xf>(ptM);
        const double dmin = fmin(lane < PKL ? fabs(nL - ptL) : 1e300, lane < PKM ? fabs(nM - ptM) : 1e300);
        invalid = kcap || __ballot(dmin <= LR_MIN_ALLOWED_T) != 0ull;
    }
    double priorP = -INFINITY, lik = -INFINITY;
    if (!invalid) {
        double logpL, logpM;
        lr_rjbin_log_rates(pL, pM, lane, &logpL, &logpM);
        // Gamma(2, g) log-densities of all rates of both processes in one reduction (LRF:296)
        const double vL = (lane < PKL) ? (logpL + plg0) - pL * pg0 + plg0 : 0.0;
        const double vM = (lane < PKM) ? (logpM + plg1) - pM * pg1 + plg1 : 0.0;
        priorP = lr_wave_sum(vL + vM);
        priorP += -run.log_T * (PKL - 1 + PKM - 1);
        if (priorPoi != 0.0) priorP += priorPoi;
        else priorP += S.priorPoiA, priorPoi = S.priorPoiA;
        lik = gibbs ? S.likA : lr_rjbin_loglik<BPL>(B, model, n_bins, pL, logpL, peL, PKL, pM, logpM, peM, PKM, lane);
    }
    if (kcap && lane == 0) __hip_atomic_fetch_or(warn, (unsigned int)LR_WARN_KCAP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the Gibbs draws replace the hyper-parameters whether or not the state is adopted (LRF:283-287 assign them)
    S.g0 = pg0, S.g1 = pg1, S.poi = ppoi, S.lg0 = plg0, S.lg1 = plg1, S.lpoi = plpoi;
    const double dlik = TEMPERED ? beta * (lik - S.likA) : lik - S.likA;
    const bool ok = gibbs || (!invalid && (dlik + priorP - S.priorA + hasting >= log_u));      // LRF:305-313
    if (ok) {
        S.L = pL, S.M = pM, S.tL = ptL, S.tM = ptM, S.eL = peL, S.eM = peM, S.KL = PKL, S.KM = PKM;
        S.likA = lik, S.priorA = priorP, S.priorPoiA = priorPoi, S.n_acc += 1.0;
    }
}

// one trace row (LRF:321-359), the engines' layout (lr_write_trace_row); column 2 is the likelihood itself, untempered
__device__ __forceinline__ void lr_rjbin_trace_row(const lr_rjbin_chain& S, const lr_rjbin_run& run, long long it, double* __restrict__ row,
                                                   int lane) {
    const double meanL = lr_wave_sum(lane < S.KL ? S.L : 0.0) / S.KL;
    const double meanM = lr_wave_sum(lane < S.KM ? S.M : 0.0) / S.KM;
    double h = 0.0;
    h = (lane == 0) ? (double)it : h;
    h = (lane == 1) ? S.likA + S.priorA : h;
    h = (lane == 2) ? S.likA : h;
    h = (lane == 3) ? S.priorA : h;
    h = (lane == 4) ? meanL : h;
    h = (lane == 5) ? meanM : h;
    h = (lane == 6) ? (double)S.KL : h;
    h = (lane == 7) ? (double)S.KM : h;
    h = (lane == 8) ? run.t_start : h;
    h = (lane == 9) ? run.t_end : h;
    h = (lane == 10) ? S.g0 : h;
    h = (lane == 11) ? S.g1 : h;
    h = (lane == 12) ? S.poi : h;
    if (lane < LR_TRACE_HEAD) row[lane] = h;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double* rl = row + LR_TRACE_HEAD;
    double* rm = rl + (2 * LR_KMAX - 1);
    if (lane < LR_KMAX) rl[lane] = lane < S.KL ? S.L : nan, rm[lane] = lane < S.KM ? S.M : nan;
    if (lane >= 1 && lane < LR_KMAX) {
        rl[LR_KMAX + lane - 1] = lane < S.KL ? S.tL : nan;
        rm[LR_KMAX + lane - 1] = lane < S.KM ? S.tM : nan;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------
// the checks of lr_rjbin_init (steps = false, init6 = the six arrays) and lr_rjbin_steps, in the header's order -> cfg
static inline int lr_rjbin_args(const lr_rjbin_problem* p, bool steps, const void* const* init6, int64_t it0, int64_t n_iters,
                                int32_t s_freq, const double* rows, int64_t rows_cap, int64_t slot0, lr_rjbin_cfg* cfg) {
    // (rows may be NULL where no row is due)
    int64_t need = 0;
    const bool counts_ok = !steps || lr_rows_due(it0, n_iters, s_freq, &need);
    if (!p) return LR_ERR_NULL;
    if (!p->sp || !p->ex || !p->br || !p->start_time || !p->end_time || !p->state || !p->warn ||
        (steps && !rows && counts_ok && need > 0))
        return LR_ERR_NULL;
    if (init6) {
        int given = 0;
        for (int i = 0; i < 6; ++i) given += init6[i] ? 1 : 0;
        if (given != 0 && given != 6) return LR_ERR_NULL;
    }
    if (p->n_bins < 1 || p->n_bins > LR_RJBIN_MAX_BINS || p->R < 1 || p->chains_per_rep < 1) return LR_ERR_SIZE;
    if ((int64_t)p->R * p->chains_per_rep > INT32_MAX) return LR_ERR_SIZE;
    if (p->model < 0 || p->model > 3 || (p->model == LR_MODEL_KEIDING_DEAD && (!p->ex_dead || !p->br_dead))) return LR_ERR_MODEL;
    if (!(p->update_fraction >= 0.0 && p->update_fraction <= 1.0) || !(p->poisson_HP >= 0.0)) return LR_ERR_MODEL;
    if (steps && (!counts_ok || slot0 < 0 || rows_cap < 0 || rows_cap - slot0 < need)) return LR_ERR_SIZE;
    cfg->poisson_HP = p->poisson_HP, cfg->update_fraction = p->update_fraction, cfg->mult_l = 2.0 * std::log(LR_MULT_D);
    cfg->rows_cap = steps ? rows_cap : 0, cfg->slot0 = steps ? slot0 : 0, cfg->chain0 = p->chain0;
    cfg->n_bins = p->n_bins, cfg->n_chains = p->R * p->chains_per_rep, cfg->chains_per_rep = p->chains_per_rep;
    cfg->model = p->model, cfg->const_rates = p->const_rates ? 1 : 0, cfg->const_death_rate = p->const_death_rate ? 1 : 0;
    cfg->use_rate_HP = p->use_rate_HP ? 1 : 0, cfg->s_freq = steps ? s_freq : 1, cfg->seed = (uint32_t)p->seed;
    return LR_OK;
}
