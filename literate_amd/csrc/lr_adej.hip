// lr_adej.hip - age-dependent extinction sampled jointly (include/literate_hip_adej.h): a Metropolis-Hastings sampler over
// (the death-rate skyline, the Weibull shape), one workgroup of four waves per chain, every chain's launch inside one kernel.
//
//   (lr_ade_prepare_tables of lr_ade.hip writes the workspace: the tables of lr_ade_tables.h)
//   lr_adej_loglik_kernel  one block per row: l(mu, k)
//   lr_adej_chain_kernel   one block per chain: its initial state, or n_iters iterations from its state
//
// The likelihood in the form without a cumulative sum:
//   l(mu, k) = -sum_j w_k[j] M[j] + sum_classes n log(-expm1(-mu[je] w_k[a])),   M[j] = sum_{jb < A - j} R[jb][j] mu[jb + j]
// M does not depend on the shape and w not on the rates: the chain keeps the accepted state's per-bin rates, w and M in LDS, a
// shape move rebuilds w alone (A exponentials) and a rate or RJ move the rates and M alone (A (A + 1) / 2 multiply-adds over
// the 256 threads); the class terms are evaluated for every proposal.  Wave 0 carries the chain step with the lane-per-element
// functions of lr_chain.h (lane j holds rate j and time j), all four waves evaluate the likelihood, and every thread takes
// the Metropolis-Hastings decision from the same numbers in the same order.  Every block-wide sum is a fixed tree (a DPP scan
// per wave, the four waves in order): no floating-point atomics, a chain's bits depend on its own arguments alone.
//
// R and the class list live in LDS as 32-bit integers while every count fits (any data set below 2^31 lineages) and the
// classes number at most LR_ADEJ_LDS_CLASSES; otherwise they are read from the workspace through L2, where all chains share
// them.  At 128 bins a workgroup then holds 33 KiB of R and 17 KiB of the rest.
#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_adej.h"
#include "lr_ade_tables.h"
#include "lr_chain.h"

// draw purposes of this sampler, beside the engines' LR_P_MOVE, LR_P_MULT, LR_P_RJ, LR_P_BETA_A / _B and LR_P_ACCEPT
#define LR_P_ADEJ_SHAPE 48
#define LR_P_ADEJ_INIT 49
#define LR_P_ADEJ_GIBBS_POI 50
#define LR_P_ADEJ_GIBBS_RATE 51

#define LR_ADEJ_THREADS 256
#define LR_ADEJ_WAVES (LR_ADEJ_THREADS / 64)
#define LR_ADEJ_LDS_CLASSES 1024
#define LR_ADEJ_LOG_SHAPE_MAX 2.0794415416798357   /* log 8 */
#define LR_ADEJ_INIT_RATE_SCALE 0.2
#define LR_ADEJ_INIT_LOG_SHAPE_SPAN 2.772588722239781 /* 2 log 4 */
#define LR_ADEJ_UPDATE_FRACTION 0.75
// state slots (include/literate_hip_adej.h)
#define LR_ADEJ_S_K 0
#define LR_ADEJ_S_G 1
#define LR_ADEJ_S_RATE_HP 2
#define LR_ADEJ_S_POI_HP 3
#define LR_ADEJ_S_LIK 4
#define LR_ADEJ_S_PRIOR 5
#define LR_ADEJ_S_COUNTS 6
#define LR_ADEJ_S_RATES 16
#define LR_ADEJ_S_TIMES 48
#define LR_ADEJ_ROW_HEAD 10
#define LR_UD_LANE_ADEJ 32     /* first of the four lanes that hold the wave-uniform draws of an iteration's one Philox call */

static_assert(LR_ADEJ_S_TIMES + LR_KMAX + 1 <= LR_ADEJ_STATE_W, "the state holds K + 1 times");
static_assert(LR_ADEJ_ROW_W == LR_ADEJ_ROW_HEAD + 2 * LR_KMAX - 1, "row layout");
static_assert(LR_ADEJ_MAX_BINS <= LR_ADEJ_THREADS / 2, "a thread per bin, two partial sums per age");
static_assert(LR_ADEJ_MAX_BINS <= LR_ADE_MAX_BINS, "the tables are prepared for up to LR_ADE_MAX_BINS bins");

struct lr_adej_cfg {
    double t0, win, poisson_prior, mult_l, log_A;
    int A, const_rates, use_rate_hp, s_freq;
    uint32_t seed;
    int chain0, n_chains;
};

// ------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------
// the LDS of a likelihood evaluation; the chain kernel carves R32 [A (A + 1) / 2] behind it (dynamic LDS only: its base
// stays 16-byte aligned)
struct lr_adej_lds {
    double w[LR_ADEJ_MAX_BINS], M[LR_ADEJ_MAX_BINS], mu[LR_ADEJ_MAX_BINS];        // the accepted state's
    double wp[LR_ADEJ_MAX_BINS], Mp[LR_ADEJ_MAX_BINS], mup[LR_ADEJ_MAX_BINS];     // the proposal's
    double part[LR_ADEJ_THREADS];
    double red[LR_ADEJ_WAVES];
    double seg_rate[LR_KMAX];
    double ctl_f[8];          // shape of the proposal, lik, prior, Hastings term, log u, prior of the accepted state
    int seg_edge[LR_KMAX + 2];
    int ctl_i[6];             // kind, invalid, K of the proposal, gibbs
    int cls_cell[LR_ADEJ_LDS_CLASSES];
    int cls_n[LR_ADEJ_LDS_CLASSES];
};
static_assert(sizeof(lr_adej_lds) % 16 == 0, "R32 behind the struct starts 16-byte aligned");

// x summed over the block, the same in every thread
// (not lr_ade_sum2: that one adds the lanes in a __shfl_down tree, and the bits would differ)
__device__ __forceinline__ double lr_adej_block_sum(double x, double* s_red) {
    const double v = lr_wave_sum(x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    double t = s_red[0];
#pragma unroll
    for (int w = 1; w < LR_ADEJ_WAVES; ++w) t += s_red[w];
    __syncthreads();
    return t;
}

// w_k[j] of this thread's age j = tid (lj = log j, l1 = log1p(1 / j))
// (not lr_ade_profile_kernel's pow(j, k): the logs are kept across iterations, and exp(k log j) rounds differently)
__device__ __forceinline__ double lr_adej_weight(int j, double k, double lj, double l1) {
    return j == 0 ? 1.0 : exp(k * lj) * expm1(k * l1);
}

// M[j] = sum_jb R[jb][j] mu[jb + j] over the block: age j by 256 / Apad threads, each a strided part of jb, the parts added in
// order.  mu and M in LDS; R from LDS (r32) or the workspace (rg).  Ends on a barrier.
__device__ __forceinline__ void lr_adej_risk_sums(int A, const double* mu, double* M, double* part, const int* r32,
                                                  const double* __restrict__ rg) {
    const int tid = threadIdx.x;
    const int Apad = A <= 32 ? 32 : (A <= 64 ? 64 : 128);
    const int P = LR_ADEJ_THREADS / Apad;
    const int j = tid & (Apad - 1), p = tid / Apad;
    double acc = 0.0;
    if (j < A) {
        if (r32) {
            for (int jb = p; jb < A - j; jb += P) acc = fma((double)r32[lr_ade_row(jb, A) + j], mu[jb + j], acc);
        } else {
            for (int jb = p; jb < A - j; jb += P) acc = fma(rg[lr_ade_row(jb, A) + j], mu[jb + j], acc);
        }
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < A) {
        double m = part[tid];
        for (int q = 1; q < P; ++q) m += part[q * Apad + tid];
        M[tid] = m;
    }
    __syncthreads();
}

// l(mu, k) from w, M and mu in LDS; the classes from LDS (s_cell) or the workspace.  The same value in every thread.
__device__ __forceinline__ double lr_adej_eval(int A, int n_cls, const double* w, const double* M, const double* mu,
                                               const int* s_cell, const int* s_n, const lr_ade_data& d, double* s_red) {
    const int tid = threadIdx.x;
    double acc = tid < A ? -(w[tid] * M[tid]) : 0.0;
    if (s_cell) {
        for (int i = tid; i < n_cls; i += LR_ADEJ_THREADS) {
            const int cell = s_cell[i];
            acc += lr_ade_term((double)s_n[i], mu[cell & 0xFFFF] * w[cell >> 16]);
        }
    } else {
        for (int i = tid; i < n_cls; i += LR_ADEJ_THREADS) {
            const int cell = d.cls_cell[i];
            acc += lr_ade_term(d.cls_n[i], mu[cell & 0xFFFF] * w[cell >> 16]);
        }
    }
    return lr_adej_block_sum(acc, s_red);
}

__global__ __launch_bounds__(LR_ADEJ_THREADS) void lr_adej_loglik_kernel(lr_ade_data d, int A,
                                                                        const double* __restrict__ mu_bins,
                                                                        const double* __restrict__ shapes,
                                                                        double* __restrict__ out_ll,
                                                                        int* __restrict__ out_flag) {
    extern __shared__ __attribute__((aligned(16))) char lr_adej_smem[];
    lr_adej_lds& s = *reinterpret_cast<lr_adej_lds*>(lr_adej_smem);
    const int row = blockIdx.x, tid = threadIdx.x;
    const double k = shapes[row];
    int bad = 0;
    if (tid < A) {
        const double m = mu_bins[(size_t)row * A + tid];
        s.mu[tid] = m;
        bad = lr_ade_bad_rate(m, d.death_bin, tid);
    }
    bad = __syncthreads_or(bad) ? 1 : 0;
    if (!(k > 0.0) || !(k < __builtin_inf())) bad |= 2;
    // (everything the block branches on is the same in all its threads)
    if (bad) {
        if (tid == 0) out_ll[row] = __builtin_nan(""), out_flag[row] = bad;
        return;
    }
    if (tid < A) s.w[tid] = lr_adej_weight(tid, k, tid ? log((double)tid) : 0.0, tid ? log1p(1.0 / (double)tid) : 0.0);
    lr_adej_risk_sums(A, s.mu, s.M, s.part, nullptr, d.R);
    const double ll = lr_adej_eval(A, lr_ade_class_count(d, A), s.w, s.M, s.mu, nullptr, nullptr, d, s.red);
    if (tid == 0) out_ll[row] = ll, out_flag[row] = 0;
}

// per-bin rates of the segments wave 0 left in LDS: bin b takes the segment with edge[seg] <= b < edge[seg + 1]
__device__ __forceinline__ void lr_adej_expand(int A, int K, const lr_adej_lds& s, double* mu) {
    const int b = threadIdx.x;
    if (b < A) {
        int seg = 0;
        for (int j = 1; j < K; ++j) seg += s.seg_edge[j] <= b ? 1 : 0;
        mu[b] = s.seg_rate[seg];
    }
}

// mode 0: lr_adej_init; mode 1: n_iters iterations from it0
__global__ __launch_bounds__(LR_ADEJ_THREADS) void lr_adej_chain_kernel(lr_ade_data d, lr_adej_cfg cfg, int mode,
                                                                       double* __restrict__ state, long long it0,
                                                                       long long n_iters, double* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) char lr_adej_smem[];
    lr_adej_lds& s = *reinterpret_cast<lr_adej_lds*>(lr_adej_smem);
    int* s_R32 = reinterpret_cast<int*>(lr_adej_smem + sizeof(lr_adej_lds));
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int A = cfg.A;
    const int n_cls = lr_ade_class_count(d, A);
    const bool fits = d.hdr[LR_ADE_HDR_FITS32] != 0;
    const int* r32 = fits ? s_R32 : nullptr;
    const int* s_cell = fits && n_cls <= LR_ADEJ_LDS_CLASSES ? s.cls_cell : nullptr;
    const int* s_n = s.cls_n;
    if (fits) {
        const int tri = A * (A + 1) / 2;
        for (int i = tid; i < tri; i += LR_ADEJ_THREADS) s_R32[i] = d.R32[i];
    }
    if (s_cell) {
        for (int i = tid; i < n_cls; i += LR_ADEJ_THREADS) s.cls_cell[i] = d.cls_cell[i], s.cls_n[i] = d.cls_n32[i];
    }
    const double lj = tid ? log((double)tid) : 0.0, l1 = tid ? log1p(1.0 / (double)tid) : 0.0;   // this thread's age
    double* S = state + (size_t)c * LR_ADEJ_STATE_W;
    const lr_stream rng{cfg.seed, (uint32_t)(cfg.chain0 + c)};

    // the chain's state in the registers of wave 0: lane j holds rate j and time j, lane l < 10 counter l
    double R = 0.0, T = 0.0, cnt = 0.0;
    int K = 1;
    double g = 0.0, rate_hp = 1.0, poi_hp = cfg.poisson_prior > 0.0 ? cfg.poisson_prior : 1.0;
    double likA = 0.0, priorA = 0.0;
    if (wave == 0) {
        if (mode == 0) {
            const double g2 = lr_gamma(rng, 0, LR_P_ADEJ_INIT, 0, 2.0);
            const lr_u2 u = lr_pair(rng, 0, LR_P_ADEJ_INIT, 64);
            R = lane == 0 ? g2 * LR_ADEJ_INIT_RATE_SCALE : 0.0;
            T = lane == 0 ? cfg.t0 : (lane == 1 ? cfg.t0 + (double)A : 0.0);
            g = (u.a - 0.5) * LR_ADEJ_INIT_LOG_SHAPE_SPAN;
        } else {
            K = min(max((int)S[LR_ADEJ_S_K], 1), LR_KMAX), g = S[LR_ADEJ_S_G], rate_hp = S[LR_ADEJ_S_RATE_HP], poi_hp = S[LR_ADEJ_S_POI_HP];
            likA = S[LR_ADEJ_S_LIK], priorA = S[LR_ADEJ_S_PRIOR];
            R = lane < LR_KMAX ? S[LR_ADEJ_S_RATES + lane] : 0.0;
            T = lane <= LR_KMAX ? S[LR_ADEJ_S_TIMES + lane] : 0.0;
            cnt = lane < 2 * LR_ADEJ_MOVES ? S[LR_ADEJ_S_COUNTS + lane] : 0.0;
        }
        const int E = lr_wave_edges(T, 0);
        if (lane < LR_KMAX) s.seg_rate[lane] = R;
        if (lane <= LR_KMAX) s.seg_edge[lane] = E;
        if (lane == 0) s.ctl_i[2] = K, s.ctl_f[0] = exp(g);
    }
    __syncthreads();
    // the accepted state's rates per bin, w and M: functions of the state alone, the doubles an earlier launch held
    {
        const int K0 = s.ctl_i[2];
        const double k0 = s.ctl_f[0];
        lr_adej_expand(A, K0, s, s.mu);
        if (tid < A) s.w[tid] = lr_adej_weight(tid, k0, lj, l1);
        __syncthreads();
        lr_adej_risk_sums(A, s.mu, s.M, s.part, r32, d.R);
    }
    double lrh = 0.0, lpoi = 0.0;
    if (wave == 0) {
        const double lx = lr_log(lane == 0 ? rate_hp : (lane == 1 ? poi_hp : 1.0));
        lrh = lr_bcast(lx, 0), lpoi = lr_bcast(lx, 1);
    }
    if (mode == 0) {
        const double lik = lr_adej_eval(A, n_cls, s.w, s.M, s.mu, s_cell, s_n, d, s.red);
        if (wave == 0) {
            const double logR = lr_log(lane < K ? R : 1.0);
            likA = lik;
            priorA = lr_wave_prior_gamma2(R, logR, K, rate_hp, lrh, lane) - cfg.log_A * (K - 1) + lr_poisson_prior(K, poi_hp, lpoi);
        }
        n_iters = 0;
    }

    const double nan = __builtin_nan("");
    for (long long i = 0; i < n_iters; ++i) {
        const unsigned long long it = (unsigned long long)(it0 + i);
        double pR = R, pT = T, pg = g, p_rate_hp = rate_hp, p_poi = poi_hp, p_lrh = lrh, p_lpoi = lpoi;
        double hasting = 0.0, priorP = 0.0, log_u = 0.0;
        int pK = K, kind = 0, invalid = 0;
        if (wave == 0) {
            // the draws of the iteration in one Philox call: lanes 0 .. 31 the multiplier pairs of their rates, lanes 32 .. 35
            // the acceptance uniform, the move selector, the RJ position, the shape window
            const int ul = lane - LR_UD_LANE_ADEJ;
            const uint32_t purpose = ul < 0 ? LR_P_MULT : (ul == 0 ? LR_P_ACCEPT : (ul == 1 ? LR_P_MOVE : (ul == 2 ? LR_P_RJ : LR_P_ADEJ_SHAPE)));
            const lr_u2 ud = lr_pair(rng, it, purpose, ul < 0 ? (uint32_t)lane : (ul == 2 ? 1u : 0u));
            const double lu = lr_log(ul == 0 ? ud.a : 1.0);
            log_u = lr_bcast(lu, LR_UD_LANE_ADEJ);
            const double r0 = lr_bcast(ud.a, LR_UD_LANE_ADEJ + 1), r1 = lr_bcast(ud.b, LR_UD_LANE_ADEJ + 1);
            const double q_a = lr_bcast(ud.a, LR_UD_LANE_ADEJ + 2), q_b = lr_bcast(ud.b, LR_UD_LANE_ADEJ + 2);
            const double u_sh = lr_bcast(ud.a, LR_UD_LANE_ADEJ + 3);
            if (r0 < 0.30) {
                kind = 0;
                hasting = lr_wave_multiplier(pR, K, ud.a < LR_ADEJ_UPDATE_FRACTION, ud.b, cfg.mult_l, lane);
            } else if (r0 < 0.60) {
                kind = 1;
                pg = g + (u_sh - 0.5) * cfg.win;
                invalid = !(pg >= -LR_ADEJ_LOG_SHAPE_MAX && pg <= LR_ADEJ_LOG_SHAPE_MAX);
            } else if (r0 < 0.999 && cfg.const_rates == 0) {
                if (r1 > 0.5) {
                    kind = 2;
                    if (K >= LR_KMAX) {
                        invalid = 1;
                    } else {
                        const int ind = min((int)(q_a * K), K - 1);
                        const double delta = q_b * (lr_bcast(T, ind + 1) - lr_bcast(T, ind));
                        double ga, gb;
                        lr_wave_gamma2(rng, it, LR_P_BETA_A, LR_SHAPE_BETA_RJ, LR_P_BETA_B, LR_SHAPE_BETA_RJ, lane, &ga, &gb);
                        hasting = lr_wave_add_shift(pR, pT, pK, ind, delta, ga / (ga + gb), lane);
                    }
                } else {
                    kind = 3;
                    if (K > 1) {
                        const int idx = 1 + min((int)(q_a * (K - 1)), K - 2);
                        hasting = lr_wave_remove_shift(pR, pT, pK, idx, lane);
                    }
                }
            } else {
                kind = 4;
                double gp = 0.0, gr = 0.0;
                lr_wave_gamma2(rng, it, LR_P_ADEJ_GIBBS_POI, LR_RJHP_SHAPE + K, LR_P_ADEJ_GIBBS_RATE,
                               LR_HP_GAMMA_SHAPE + LR_GAMMA_SHAPE * K, lane, &gp, &gr);
                if (cfg.poisson_prior == 0.0) p_poi = gp * (1. / (LR_RJHP_RATE + 1.0));
                if (cfg.use_rate_hp) p_rate_hp = gr * (1. / (LR_HP_GAMMA_RATE + lr_wave_sum(lane < K ? R : 0.0)));
                const double lx = lr_log(lane == 0 ? p_rate_hp : (lane == 1 ? p_poi : 1.0));
                p_lrh = lr_bcast(lx, 0), p_lpoi = lr_bcast(lx, 1);
            }
            if (kind != 4 && !invalid && lr_wave_min_segment(pT, pK, lane) <= LR_MIN_ALLOWED_T) invalid = 1;
            if (!invalid) {
                const double logR = lr_log(lane < pK ? pR : 1.0);
                priorP = lr_wave_prior_gamma2(pR, logR, pK, p_rate_hp, p_lrh, lane) - cfg.log_A * (pK - 1) +
                         lr_poisson_prior(pK, p_poi, p_lpoi);
            }
            if (kind != 1 && kind != 4 && !invalid) {
                const int E = lr_wave_edges(pT, 0);
                if (lane < LR_KMAX) s.seg_rate[lane] = pR;
                if (lane <= LR_KMAX) s.seg_edge[lane] = E;
            }
            if (lane == 0) {
                s.ctl_i[0] = kind, s.ctl_i[1] = invalid, s.ctl_i[2] = pK;
                s.ctl_f[0] = kind == 1 && !invalid ? exp(pg) : 0.0;
#ifdef LR_ADEJ_REBUILD_ALL
                s.ctl_f[6] = exp(g);
#endif
                s.ctl_f[1] = likA, s.ctl_f[2] = priorP, s.ctl_f[3] = priorA, s.ctl_f[4] = hasting, s.ctl_f[5] = log_u;
            }
        }
        __syncthreads();
        kind = s.ctl_i[0], invalid = s.ctl_i[1];
        bool accept = kind == 4;
        double lik = s.ctl_f[1];
        if (kind != 4 && !invalid) {
            // (every thread takes the same branches: the control words are the block's)
            if (kind == 1) {
                if (tid < A) s.wp[tid] = lr_adej_weight(tid, s.ctl_f[0], lj, l1);
                __syncthreads();
#ifdef LR_ADEJ_REBUILD_ALL      // (scratch/exp_adej.py: what keeping the accepted state's w and M saves)
                lr_adej_risk_sums(A, s.mu, s.M, s.part, r32, d.R);
#endif
                lik = lr_adej_eval(A, n_cls, s.wp, s.M, s.mu, s_cell, s_n, d, s.red);
            } else {
                lr_adej_expand(A, s.ctl_i[2], s, s.mup);
#ifdef LR_ADEJ_REBUILD_ALL
                if (tid < A) s.w[tid] = lr_adej_weight(tid, s.ctl_f[6], lj, l1);
#endif
                __syncthreads();
                lr_adej_risk_sums(A, s.mup, s.Mp, s.part, r32, d.R);
                lik = lr_adej_eval(A, n_cls, s.w, s.Mp, s.mup, s_cell, s_n, d, s.red);
            }
            accept = lik - s.ctl_f[1] + s.ctl_f[2] - s.ctl_f[3] + s.ctl_f[4] >= s.ctl_f[5];
            if (accept && tid < A) {
                if (kind == 1) s.w[tid] = s.wp[tid];
                else s.mu[tid] = s.mup[tid], s.M[tid] = s.Mp[tid];
            }
        }
        if (wave == 0) {
            if (lane == kind) cnt += 1.0;
            if (accept) {
                R = pR, T = pT, K = pK, g = pg, rate_hp = p_rate_hp, poi_hp = p_poi, lrh = p_lrh, lpoi = p_lpoi;
                likA = lik, priorA = priorP;
                if (lane == LR_ADEJ_MOVES + kind) cnt += 1.0;
            }
            if (it % (unsigned long long)cfg.s_freq == 0ull) {
                const unsigned long long sf = (unsigned long long)cfg.s_freq;
                const unsigned long long slot = it / sf - ((unsigned long long)it0 + sf - 1ull) / sf;
                double* row = rows + ((size_t)slot * cfg.n_chains + c) * LR_ADEJ_ROW_W;
                const double mean = lr_wave_sum(lane < K ? R : 0.0) / K;
                const double shape = exp(g);
                double h = 0.0;
                switch (lane) {
                    case 0: h = (double)it; break;
                    case 1: h = likA + priorA; break;
                    case 2: h = likA; break;
                    case 3: h = priorA; break;
                    case 4: h = shape; break;
                    case 5: h = g; break;
                    case 6: h = K; break;
                    case 7: h = mean; break;
                    case 8: h = rate_hp; break;
                    case 9: h = poi_hp; break;
                }
                if (lane < LR_ADEJ_ROW_HEAD) row[lane] = h;
                if (lane < LR_KMAX) row[LR_ADEJ_ROW_HEAD + lane] = lane < K ? R : nan;
                if (lane >= 1 && lane < LR_KMAX) row[LR_ADEJ_ROW_HEAD + LR_KMAX + lane - 1] = lane < K ? T : nan;
            }
        }
        // (the next iteration's control words are written by wave 0 after this barrier only: the other waves have read
        // this iteration's by then, and the accepted arrays are whole before anyone reads them again)
        __syncthreads();
    }

    if (wave == 0) {
        double v = 0.0;
        switch (lane) {
            case LR_ADEJ_S_K: v = K; break;
            case LR_ADEJ_S_G: v = g; break;
            case LR_ADEJ_S_RATE_HP: v = rate_hp; break;
            case LR_ADEJ_S_POI_HP: v = poi_hp; break;
            case LR_ADEJ_S_LIK: v = likA; break;
            case LR_ADEJ_S_PRIOR: v = priorA; break;
        }
        if (lane < LR_ADEJ_S_COUNTS) S[lane] = v;
        if (lane < 2 * LR_ADEJ_MOVES) S[LR_ADEJ_S_COUNTS + lane] = cnt;
        if (lane < LR_KMAX) S[LR_ADEJ_S_RATES + lane] = lane < K ? R : 0.0;
        if (lane <= LR_KMAX) S[LR_ADEJ_S_TIMES + lane] = lane <= K ? T : 0.0;
        if (lane < LR_ADEJ_STATE_W - (LR_ADEJ_S_TIMES + LR_KMAX + 1)) S[LR_ADEJ_S_TIMES + LR_KMAX + 1 + lane] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static bool lr_adej_bins_ok(int n_bins) { return n_bins >= 1 && n_bins <= LR_ADEJ_MAX_BINS; }

extern "C" int64_t lr_adej_workspace_bytes(int32_t n_bins) {
    if (!lr_adej_bins_ok(n_bins)) return LR_ERR_SIZE;
    return (int64_t)lr_ade_layout(n_bins).total;
}

extern "C" int lr_adej_prepare(const int64_t* dead, const int64_t* cens, int32_t n_bins, void* workspace,
                               int64_t workspace_bytes, void* stream_) {
    if (!dead || !cens || !workspace) return LR_ERR_NULL;
    if (!lr_adej_bins_ok(n_bins)) return LR_ERR_SIZE;
    const int A = n_bins;
    if ((int64_t)lr_ade_layout(A).total > workspace_bytes) return LR_ERR_WORKSPACE;
    return lr_ade_prepare_tables(dead, cens, A, workspace, (hipStream_t)stream_);
}

extern "C" int lr_adej_loglik(const void* workspace, int64_t workspace_bytes, int32_t n_bins, const double* mu_bins,
                              const double* shapes, int32_t S, double* out_ll, int32_t* out_flag, void* stream_) {
    if (!workspace || !mu_bins || !shapes || !out_ll || !out_flag) return LR_ERR_NULL;
    if (S < 1 || !lr_adej_bins_ok(n_bins)) return LR_ERR_SIZE;
    if ((int64_t)lr_ade_layout(n_bins).total > workspace_bytes) return LR_ERR_WORKSPACE;
    hipLaunchKernelGGL(lr_adej_loglik_kernel, dim3((unsigned)S), dim3(LR_ADEJ_THREADS), sizeof(lr_adej_lds), (hipStream_t)stream_,
                       lr_ade_view(workspace, n_bins), (int)n_bins, mu_bins, shapes, out_ll, (int*)out_flag);
    return (int)hipGetLastError();
}

static int lr_adej_chain_args(const void* workspace, int64_t workspace_bytes, int32_t n_bins, double t0, int32_t const_rates,
                              int32_t use_rate_hp, double poisson_prior, double win, uint64_t seed, int32_t chain0,
                              int32_t n_chains, const double* state, int64_t it0, int64_t n_iters, int32_t s_freq,
                              const double* rows, int64_t n_rows, bool steps, lr_adej_cfg* cfg) {
    // (rows may be NULL where no row is due)
    int64_t need;
    const bool counts_ok = lr_rows_due(it0, n_iters, s_freq, &need);
    if (!workspace || !state || (steps && !rows && !(counts_ok && need == 0))) return LR_ERR_NULL;
    if (!lr_adej_bins_ok(n_bins) || n_chains < 1 || chain0 < 0) return LR_ERR_SIZE;
    if (steps && (!counts_ok || n_rows < need)) return LR_ERR_SIZE;
    if (!std::isfinite(win) || !std::isfinite(poisson_prior) || !(win > 0.0) || poisson_prior < 0.0) return LR_ERR_MODEL;
    if (!std::isfinite(t0) || t0 != std::floor(t0)) return LR_ERR_T0;
    if ((int64_t)lr_ade_layout(n_bins).total > workspace_bytes) return LR_ERR_WORKSPACE;
    cfg->t0 = t0, cfg->win = win, cfg->poisson_prior = poisson_prior;
    cfg->mult_l = 2.0 * std::log(LR_MULT_D), cfg->log_A = std::log((double)n_bins);
    cfg->A = n_bins, cfg->const_rates = const_rates ? 1 : 0, cfg->use_rate_hp = use_rate_hp ? 1 : 0, cfg->s_freq = steps ? s_freq : 1;
    cfg->seed = (uint32_t)seed, cfg->chain0 = chain0, cfg->n_chains = n_chains;
    return LR_OK;
}

static size_t lr_adej_chain_lds(int A) { return sizeof(lr_adej_lds) + (size_t)A * (A + 1) / 2 * sizeof(int); }

extern "C" int lr_adej_init(const void* workspace, int64_t workspace_bytes, int32_t n_bins, double t0, int32_t const_rates,
                            int32_t use_rate_hp, double poisson_prior, double win, uint64_t seed, int32_t chain0,
                            int32_t n_chains, double* state, void* stream_) {
    lr_adej_cfg cfg;
    const int rc = lr_adej_chain_args(workspace, workspace_bytes, n_bins, t0, const_rates, use_rate_hp, poisson_prior, win, seed,
                                      chain0, n_chains, state, 0, 0, 1, nullptr, 0, false, &cfg);
    if (rc != LR_OK) return rc;
    hipLaunchKernelGGL(lr_adej_chain_kernel, dim3((unsigned)n_chains), dim3(LR_ADEJ_THREADS), lr_adej_chain_lds(n_bins),
                       (hipStream_t)stream_, lr_ade_view(workspace, n_bins), cfg, 0, state, 0ll, 0ll,
                       (double*)nullptr);
    return (int)hipGetLastError();
}

extern "C" int lr_adej_steps(const void* workspace, int64_t workspace_bytes, int32_t n_bins, double t0, int32_t const_rates,
                             int32_t use_rate_hp, double poisson_prior, double win, uint64_t seed, int32_t chain0,
                             int32_t n_chains, double* state, int64_t it0, int64_t n_iters, int32_t s_freq, double* rows,
                             int64_t n_rows, void* stream_) {
    lr_adej_cfg cfg;
    const int rc = lr_adej_chain_args(workspace, workspace_bytes, n_bins, t0, const_rates, use_rate_hp, poisson_prior, win, seed,
                                      chain0, n_chains, state, it0, n_iters, s_freq, rows, n_rows, true, &cfg);
    if (rc != LR_OK) return rc;
    if (n_iters == 0) return LR_OK;
    hipLaunchKernelGGL(lr_adej_chain_kernel, dim3((unsigned)n_chains), dim3(LR_ADEJ_THREADS), lr_adej_chain_lds(n_bins),
                       (hipStream_t)stream_, lr_ade_view(workspace, n_bins), cfg, 1, state, (long long)it0,
                       (long long)n_iters, rows);
    return (int)hipGetLastError();
}
