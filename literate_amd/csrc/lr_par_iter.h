// lr_par_iter.h - one chain of DDRate.py's (DD:124-241) and of trend_rate.py's (trend_rate.py:102-196) Metropolis-Hastings
// sampler on per-bin statistics, held by one wave: the device code that lr_mlik.hip / lr_tmlik.hip (one data set, a ladder of
// temperatures) and lr_parbin.hip (a data set per replicate, beta = 1) share, so each sampler exists once.
//
//   lr_par_bins<BPL, TREND>      a lane's bins in registers: b = lane + 64 i, i < nb <= BPL; TREND: the covariate's log beside
//   lr_par_load_bins             ... loaded from one data set's arrays; returns the lane's largest DT
//   lr_ddi_loglik / lr_tri_loglik    likelihood_function's sum under the parameters in lanes 0-7 / 0-5; NaN -> -inf
//   lr_ddi_start / lr_tri_start      the initial state (DD:151-161 / trend_rate.py:137)
//   lr_ddi_iterate / lr_tri_iterate  one iteration: draws, proposal, prior, likelihood, the acceptance test at L^beta
//
// The parameters sit one per lane; the proposal, prior and rate map are lr_dd.h's - the expressions the engines evaluate.
// Every sum: a lane's bins in ascending order, then lr_wave_sum.  Nothing here touches memory but lr_par_load_bins.
#ifndef LR_PAR_ITER_H
#define LR_PAR_ITER_H

#include <hip/hip_runtime.h>

#include "lr_dd.h"
#include "lr_internal.h"

template <int BPL, bool TREND>
struct lr_par_bins {
    double ns[BPL], ne[BPL], dt[BPL], lt[TREND ? BPL : 1];
    int nb;
};

// the accepted parameters (lane i: parameter i), their likelihood and prior, proposals made / accepted per move kind
struct lr_par_chain {
    double A, likA, priorA, prop0, prop1, acc0, acc1;
};

// what an iteration needs beside the chain: the model, the temperature and the window widths
struct lr_ddi_run {
    double origin, present, k0, log_k0, beta, mult_l, slide_d, norm_d, f;
    int n_bins, m_birth, m_death;
    bool niche;
};
struct lr_tri_run {
    double beta, mult_l, win, f_mult, f_norm;
    int n_bins, const_b, const_d;
};

template <int BPL, bool TREND>
__device__ __forceinline__ double lr_par_load_bins(lr_par_bins<BPL, TREND>& B, const double* __restrict__ n_spec,
                                                   const double* __restrict__ n_exti, const double* __restrict__ DT,
                                                   const double* __restrict__ trend, int n_bins, int lane) {
    B.nb = (n_bins + LR_WAVE - 1) / LR_WAVE;
    double dt_max = -INFINITY;
#pragma unroll
    for (int i = 0; i < BPL; ++i) {
        const int b = lane + LR_WAVE * i;
        const bool in = i < B.nb && b < n_bins;
        B.ns[i] = in ? n_spec[b] : 0.0, B.ne[i] = in ? n_exti[b] : 0.0, B.dt[i] = in ? DT[b] : 1.0;
        if (TREND) B.lt[i] = lr_log(in ? trend[b] : 1.0);
        if (in) dt_max = fmax(dt_max, B.dt[i]);
    }
    return dt_max;
}

// ---- DDRate ------------------------------------------------------------------------------------------------------------
// likelihood_function's sum (DD:101-107) under the parameters in lanes 0-7 of P; NaN -> -inf
template <int BPL>
__device__ __forceinline__ double lr_ddi_loglik(double P, const lr_par_bins<BPL, false>& B, int n_bins, int m_birth, int m_death,
                                                int lane) {
    const lr_dd_params p = lr_dd_unpack(P);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < BPL; ++i) {
        const int b = lane + LR_WAVE * i;
        if (i < B.nb && b < n_bins) {
            double br, dr, niche, frac;
            lr_dd_bin_rates(p, (double)b, B.dt[i], m_birth, m_death, &br, &dr, &niche, &frac);
            acc += (lr_log(br) * B.ns[i] - br * B.dt[i]) + (lr_log(dr) * B.ne[i] - dr * B.dt[i]);
        }
    }
    const double s = lr_wave_sum(acc);
    return s != s ? -INFINITY : s;
}

// run: origin, present, beta, n_bins and the model are the caller's; dt_max: the lane's (lr_par_load_bins); scale: of the windows
__device__ __forceinline__ void lr_ddi_run_of(lr_ddi_run& run, double dt_max, double scale, double mult_l, int lane) {
    run.k0 = -lr_wave_min(-dt_max), run.log_k0 = lr_log(run.k0);        // PRIOR_K0_L = np.max(DT) (DD:45)
    run.niche = run.m_birth == 2 || run.m_death == 2;
    run.f = lr_dd_update_freq(run.m_birth, run.m_death, lane);
    run.mult_l = scale * mult_l, run.slide_d = 1.5 * scale, run.norm_d = 0.2 * scale;
}

template <int BPL>
__device__ __forceinline__ void lr_ddi_start(lr_par_chain& S, const lr_par_bins<BPL, false>& B, const lr_ddi_run& run,
                                             double init_death, int lane) {
    const double x0 = run.present - (run.origin + run.present) / 2.0;       // PRESENT - np.mean([ORIGIN, PRESENT])
    const double init[LR_DD_NPAR] = {0.5, 1.5, x0, 10.0, 20000.0, init_death, 1.0, 1.0};
    S.A = 0.0;
#pragma unroll
    for (int i = 0; i < LR_DD_NPAR; ++i) S.A = (lane == i) ? init[i] : S.A;
    S.likA = lr_ddi_loglik<BPL>(S.A, B, run.n_bins, run.m_birth, run.m_death, lane);
    S.priorA = lr_dd_prior(S.A, run.origin, run.present, run.k0, run.log_k0, lane);
    S.prop0 = S.prop1 = S.acc0 = S.acc1 = 0.0;
}

template <int BPL>
__device__ __forceinline__ void lr_ddi_iterate(lr_par_chain& S, const lr_par_bins<BPL, false>& B, const lr_ddi_run& run,
                                               const lr_stream& rng, long long it, int lane) {
    // the wave-uniform draws in one Philox call: lane 0 the acceptance uniform, lane 1 the move selector, lane 2 the
    // sliding-window uniform (as lr_propose_dd takes them)
    const uint32_t purpose = lane == 0 ? LR_P_DD_ACCEPT : (lane == 1 ? LR_P_DD_MOVE : LR_P_DD_SLIDE);
    const lr_u2 ud = lr_pair(rng, (uint64_t)it, purpose, 0u);
    const double log_u = lr_bcast(lr_log(lane == 0 ? ud.a : 1.0), 0);
    double P = S.A, hasting = 0.0;
    int move;
    if (lr_bcast(ud.b, 1) < 0.1 && run.niche) {
        // update_sliding_win(x0, m = 0, M = PRESENT, d = 1.5 s) (lib:124-128)
        double ii = lr_bcast(S.A, 2) + (lr_bcast(ud.a, 2) - .5) * run.slide_d;
        if (ii > run.present) ii = run.present - (ii - run.present);
        ii = fabs(ii);
        if (lane == 2) P = ii;
        if (run.m_death == -1) {
            const double z = lr_normal(rng, (uint64_t)it, LR_P_DD_SLIDE, 1);   // update_normal_nobound(k, d = 0.2 s) (lib:136-138)
            if (lane == 1) P = S.A + z * run.norm_d;
        }
        move = 1;
    } else {
        const lr_u2 d = lr_pair(rng, (uint64_t)it, LR_P_DD_MULT, lane);
        hasting = lr_wave_multiplier(P, LR_DD_NPAR, d.a < run.f, d.b, run.mult_l, lane);   // lib:156-165
        move = 0;
    }
    const double prior = lr_dd_prior(P, run.origin, run.present, run.k0, run.log_k0, lane);
    const double lik = lr_ddi_loglik<BPL>(P, B, run.n_bins, run.m_birth, run.m_death, lane);
    const double dl = run.beta == 0.0 ? 0.0 : run.beta * (lik - S.likA);
    const bool ok = (dl + (prior - S.priorA) + hasting > log_u) || it == 0;      // DD:211
    S.prop0 += move ? 0.0 : 1.0, S.prop1 += move ? 1.0 : 0.0;
    if (ok) S.A = P, S.likA = lik, S.priorA = prior, S.acc0 += move ? 0.0 : 1.0, S.acc1 += move ? 1.0 : 0.0;
}

// ---- trend_rate --------------------------------------------------------------------------------------------------------
// likelihood_function's sum (trend_rate.py:89-91) under the parameters in lanes 0-5 of P; NaN -> -inf
template <int BPL>
__device__ __forceinline__ double lr_tri_loglik(double P, const lr_par_bins<BPL, true>& B, int n_bins, int const_b, int const_d,
                                                int lane) {
    const lr_trend_params p = lr_trend_unpack(P);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < BPL; ++i) {
        const int b = lane + LR_WAVE * i;
        if (i < B.nb && b < n_bins) {
            double br, dr;
            lr_trend_bin_rates_log(p, B.lt[i], const_b, const_d, &br, &dr);
            acc += (lr_log(br) * B.ns[i] - br * B.dt[i]) + (lr_log(dr) * B.ne[i] - dr * B.dt[i]);
        }
    }
    const double s = lr_wave_sum(acc);
    return s != s ? -INFINITY : s;
}

template <int BPL>
__device__ __forceinline__ void lr_tri_start(lr_par_chain& S, const lr_par_bins<BPL, true>& B, const lr_tri_run& run, int lane) {
    const double init[LR_TR_NPAR] = {.1, .1, 0.0, 0.0, 1.0, 1.0};          // trend_rate.py:137
    S.A = 0.0;
#pragma unroll
    for (int i = 0; i < LR_TR_NPAR; ++i) S.A = (lane == i) ? init[i] : S.A;
    S.likA = lr_tri_loglik<BPL>(S.A, B, run.n_bins, run.const_b, run.const_d, lane);
    S.priorA = lr_trend_prior(S.A, lane);
    S.prop0 = S.prop1 = S.acc0 = S.acc1 = 0.0;
}

template <int BPL>
__device__ __forceinline__ void lr_tri_iterate(lr_par_chain& S, const lr_par_bins<BPL, true>& B, const lr_tri_run& run,
                                               const lr_stream& rng, long long it, int lane) {
    // the wave-uniform draws in one Philox call: lane 0 the acceptance uniform, lane 1 the move selector (as the trend
    // engine's proposal takes them)
    const lr_u2 ud = lr_pair(rng, (uint64_t)it, lane == 0 ? LR_P_TR_ACCEPT : LR_P_TR_MOVE, 0u);
    const double log_u = lr_bcast(lr_log(lane == 0 ? ud.a : 1.0), 0);
    const lr_u2 d = lr_pair(rng, (uint64_t)it, LR_P_TR_MULT, lane);
    double P = S.A, hasting = 0.0;
    int move;
    bool moved = true;
    if (lr_bcast(ud.a, 1) < .33) {
        const double z = lr_normal(rng, (uint64_t)it, LR_P_TR_NORM, lane);   // update_normal_nobound_vec (lib:140-146)
        const bool fires = lane < LR_TR_NPAR && d.a < run.f_norm;
        if (fires) P = S.A + z * run.win;
        // a step whose mask fires for no slope proposes the state itself: it is always accepted and says nothing about
        // the window, so it is not counted (the windows are tuned from these counters)
        moved = __ballot(fires) != 0ull;
        move = 1;
    } else {
        hasting = lr_wave_multiplier(P, LR_TR_NPAR, d.a < run.f_mult, d.b, run.mult_l, lane);   // lib:156-165
        move = 0;
    }
    const double prior = lr_trend_prior(P, lane);
    const double lik = lr_tri_loglik<BPL>(P, B, run.n_bins, run.const_b, run.const_d, lane);
    const double dl = run.beta == 0.0 ? 0.0 : run.beta * (lik - S.likA);
    const bool ok = (dl + (prior - S.priorA) + hasting > log_u) || it == 0;      // trend_rate.py:176
    S.prop0 += move ? 0.0 : 1.0, S.prop1 += (move && moved) ? 1.0 : 0.0;
    if (ok) S.A = P, S.likA = lik, S.priorA = prior, S.acc0 += move ? 0.0 : 1.0, S.acc1 += (move && moved) ? 1.0 : 0.0;
}

#endif
