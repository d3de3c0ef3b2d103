// lr_mtrend.hip - the joint covariate model (include/literate_hip_mtrend.h): birth and death rates log-linear in several
// covariates at once, a selection indicator per covariate and side, a Metropolis-Hastings loop for many chains on one data
// set - all of them in one launch.
//
//   lr_mtrend_chain_kernel<BPL>   one wave per chain, four independent waves per workgroup: its initial state, or n_iters
//                                 iterations from its state
//
// The likelihood is a function of the per-bin statistics and the covariate matrix, so an iteration costs O(n_bins x included
// covariates) whatever the number of lineages: bin b sits in lane b % 64, BPL = 1, 2, 4 or 8 bins to a lane, and n_spec,
// n_exti, DT stay in registers for the whole launch (only DT is read per iteration: the counts enter through N and SX).  X is
// the workgroup's: staged in LDS once per launch, X[j, b] at j n_bins + b, so that a wave's read of one covariate is 64
// consecutive doubles - no bank conflict.  One barrier, behind the staging; after it a wave never waits for another.  The
// coefficients sit one per lane at the lane that stores them (a_j in lane 48 + j, b_j in lane 16 + j), the counters
// likewise (lane = state element), the indicators in one wave-uniform mask.  Every sum is a fixed tree (a lane's bins in
// order, then lr_wave_sum; covariates in ascending order), no floating-point atomics: a chain's bits depend on its own
// arguments alone.
#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_mtrend.h"
#include "lr_chain.h"             // lr_bcast, LR_MULT_D
#include "lr_internal.h"          // lr_rows_due

#define LR_MTREND_THREADS 256
#define LR_MTREND_WAVES (LR_MTREND_THREADS / LR_WAVE)
#define LR_MTREND_HALF_LOG_2PI 0.91893853320467274178
#define LR_MTREND_LOG_10 2.30258509299404568402
#define LR_MTREND_LANE_A 48          /* a_j sits in lane 48 + j: st[lane] */
#define LR_MTREND_LANE_B 16          /* b_j sits in lane 16 + j: st[64 + lane] */

static_assert(LR_MTREND_MAX_BINS == 8 * LR_WAVE, "a lane holds at most 8 bins");
static_assert(LR_MTREND_S_A == LR_MTREND_LANE_A && LR_MTREND_S_B == LR_WAVE + LR_MTREND_LANE_B && LR_MTREND_S_IM == LR_WAVE &&
              LR_MTREND_S_IL + LR_MTREND_MAX_COVS == LR_MTREND_S_A && LR_MTREND_S_B + LR_MTREND_MAX_COVS == LR_MTREND_STATE_W,
              "state layout: a lane stores what it holds");
static_assert(LR_MTREND_S_PROPOSED + LR_MTREND_MOVES <= LR_MTREND_S_ACCEPTED && LR_MTREND_S_ACCEPTED + LR_MTREND_MOVES <= LR_MTREND_S_IL,
              "the counters sit in lanes 8 .. 23");
static_assert(LR_MTREND_R_IL + 4 * LR_MTREND_MAX_COVS == LR_MTREND_ROW_W && LR_MTREND_ROW_W <= 2 * LR_WAVE, "a row is two stores of a wave");
static_assert(LR_MTREND_MAX_COVS * LR_MTREND_MAX_BINS * sizeof(double) <= 65536, "X fits the LDS a workgroup may ask for");

struct lr_mtrend_cfg {
    double sx[2][LR_MTREND_MAX_COVS];          // SX of the birth and of the death side
    double log_pI, log_1mpI, mult_l, slab_sd, norm_c, win[2];
    long long rows_cap, slot0, chain0, bvs_from;
    int n_bins, P, n_chains, free_b, free_d, no_death, bvs, s_freq;
    uint32_t seed;
};

// a chain: coef and cnt one element per lane (see above), the rest wave-uniform
struct lr_mtrend_chain {
    double coef, cnt, base[2], lik[2], E[2], prior;
    unsigned I;          // bit 16 s + j: I_j of side s
};

__device__ __forceinline__ int lr_mtrend_lane_of(int side) { return side ? LR_MTREND_LANE_B : LR_MTREND_LANE_A; }

// E = sum_b DT_b exp(eta_b) of a side under the coefficients `coef` and its indicators I16 (bit j: I_j)
template <int BPL>
__device__ __forceinline__ double lr_mtrend_E(const double* __restrict__ Xs, const double (&dt)[BPL], double coef, unsigned I16, int side,
                                              const lr_mtrend_cfg& cfg, int nb, int lane) {
    double eta[BPL];
#pragma unroll
    for (int i = 0; i < BPL; ++i) eta[i] = 0.0;
    const int l0 = lr_mtrend_lane_of(side);
    for (int j = 0; j < cfg.P; ++j) {
        if (!((I16 >> j) & 1u)) continue;          // wave-uniform
        const double c = lr_bcast(coef, l0 + j);
        const double* Xj = Xs + j * cfg.n_bins;
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int b = lane + LR_WAVE * i;
            if (i < nb) eta[i] = fma(c, b < cfg.n_bins ? Xj[b] : 0.0, eta[i]);
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < BPL; ++i)
        if (i < nb) acc += dt[i] * exp(eta[i]);          // (a lane's bin behind n_bins: DT = 0, eta = 0)
    return lr_wave_sum(acc);
}

// N log(base) + sum_j I_j coef_j SX_j - base E
__device__ __forceinline__ double lr_mtrend_side_lik(double N, double base, double coef, double sx, unsigned I16, int side, double E, int P) {
    const int l0 = lr_mtrend_lane_of(side);
    double d = 0.0;
    for (int j = 0; j < P; ++j)
        if ((I16 >> j) & 1u) d = fma(lr_bcast(coef, l0 + j), lr_bcast(sx, l0 + j), d);
    return N * lr_log(base) + d - base * E;
}

__device__ __forceinline__ double lr_mtrend_total(double lik_b, double lik_d) {
    const double t = lik_b + lik_d;
    return t != t ? -INFINITY : t;
}

__device__ __forceinline__ bool lr_mtrend_free_lane(const lr_mtrend_cfg& cfg, int lane) {
    return (cfg.free_b && lane >= LR_MTREND_LANE_A && lane < LR_MTREND_LANE_A + cfg.P) ||
           (cfg.free_d && lane >= LR_MTREND_LANE_B && lane < LR_MTREND_LANE_B + cfg.P);
}

__device__ __forceinline__ double lr_mtrend_prior_base(double x) { return x < .001 ? -INFINITY : -(x - .001) / 10.0 - LR_MTREND_LOG_10; }

__device__ __forceinline__ double lr_mtrend_prior(double l0, double m0, double coef, unsigned I, const lr_mtrend_cfg& cfg, int lane) {
    double t = 0.0;
    if (lr_mtrend_free_lane(cfg, lane)) {
        const double z = coef / cfg.slab_sd;
        t = cfg.norm_c - 0.5 * z * z;
    }
    const int F = (cfg.free_b + cfg.free_d) * cfg.P, on = __popc(I);
    return lr_wave_sum(t) + lr_mtrend_prior_base(l0) + lr_mtrend_prior_base(m0) + (cfg.log_pI * (double)on + cfg.log_1mpI * (double)(F - on));
}

template <int BPL>
__device__ __forceinline__ void lr_mtrend_iterate(lr_mtrend_chain& S, const double* __restrict__ Xs, const double (&dt)[BPL], const double (&N)[2],
                                                  double sx, const lr_mtrend_cfg& cfg, const lr_stream& rng, long long it, int nb, int lane) {
    // the wave-uniform draws in one Philox call: lane 0 ACCEPT[0], lane 1 MOVE[0], lane 2 MOVE[1], lane 3 NORM[0]
    const uint32_t purpose = lane == 0 ? LR_P_MTREND_ACCEPT : (lane == 3 ? LR_P_MTREND_NORM : LR_P_MTREND_MOVE);
    const lr_u2 ud = lr_pair(rng, (uint64_t)it, purpose, lane == 2 ? 1u : 0u);
    const double log_u = lr_bcast(lr_log(lane == 0 ? ud.a : 1.0), 0);
    const double r = lr_bcast(ud.a, 1), pick = lr_bcast(ud.b, 1), coin = lr_bcast(ud.a, 2), um = lr_bcast(ud.b, 2);
    const int P = cfg.P, F = (cfg.free_b + cfg.free_d) * P;
    const bool flips = cfg.bvs && it >= cfg.bvs_from;
    const double th1 = F == 0 ? 1.0 : 0.10, th2 = (F == 0 || !flips) ? 1.0 : 0.60;
    double coef = S.coef, base[2] = {S.base[0], S.base[1]}, lik[2] = {S.lik[0], S.lik[1]}, E[2] = {S.E[0], S.E[1]}, hasting = 0.0;
    unsigned I = S.I;
    // the counters' elements: 0 multiplier, 1 + side coefficient, 3 flip, 4 + side an included coefficient (kind2; none: no lane's)
    int kind, kind2 = INT_MAX;
    if (r < th1) {
        kind = 0;
        const int side = (cfg.no_death || coin < 0.5) ? 0 : 1;
        hasting = cfg.mult_l * (um - .5);
        base[side] = S.base[side] * exp(hasting);
        if (!(side == 1 && cfg.no_death))
            lik[side] = lr_mtrend_side_lik(N[side], base[side], coef, sx, (I >> (16 * side)) & 0xffffu, side, E[side], P);
    } else {
        const int k = min((int)(pick * (double)F), F - 1);
        const int side = cfg.free_b ? k / P : 1, j = k % P;
        const int pos = lr_mtrend_lane_of(side) + j;
        const unsigned bit = 1u << (16 * side + j);
        bool sum = true;
        if (r < th2) {
            kind = 1 + side;
            // lr_normal's expression on the pair every lane drew; lane 3's is NORM[0]
            const double z = lr_bcast(sqrt(-2.0 * lr_log(1.0 - ud.a)) * cospi(2.0 * ud.b), 3);
            if (lane == pos) coef = S.coef + cfg.win[side] * z;
            sum = (I & bit) != 0u;          // an excluded coefficient: the likelihood is the accepted one
            if (sum) kind2 = 4 + side;
        } else {
            kind = 3;
            I ^= bit;
        }
        if (sum) {
            const unsigned I16 = (I >> (16 * side)) & 0xffffu;
            E[side] = lr_mtrend_E<BPL>(Xs, dt, coef, I16, side, cfg, nb, lane);
            lik[side] = lr_mtrend_side_lik(N[side], base[side], coef, sx, I16, side, E[side], P);
        }
    }
    const double prior = lr_mtrend_prior(base[0], base[1], coef, I, cfg, lane);
    const double tot = lr_mtrend_total(lik[0], lik[1]), totA = lr_mtrend_total(S.lik[0], S.lik[1]);
    const bool ok = it == 0 || (tot - totA) + (prior - S.prior) + hasting > log_u;
    const int lp = lane - LR_MTREND_S_PROPOSED, la = lane - LR_MTREND_S_ACCEPTED;
    S.cnt += (lp == kind || lp == kind2) ? 1.0 : 0.0;
    if (ok) {
        S.coef = coef, S.I = I, S.prior = prior;
        S.base[0] = base[0], S.base[1] = base[1], S.lik[0] = lik[0], S.lik[1] = lik[1], S.E[0] = E[0], S.E[1] = E[1];
        S.cnt += (la == kind || la == kind2) ? 1.0 : 0.0;
    }
}

// mode 0: the initial state drawn; 1: the parameters taken from the state; 2: iterations
template <int BPL>
__global__ __launch_bounds__(LR_MTREND_THREADS) void lr_mtrend_chain_kernel(
    const double* __restrict__ n_spec, const double* __restrict__ n_exti, const double* __restrict__ DT, const double* __restrict__ X,
    lr_mtrend_cfg cfg, int mode, double* __restrict__ state, long long it0, long long n_iters, double* __restrict__ rows) {
    extern __shared__ double Xs[];          // [P, n_bins]
    for (int i = threadIdx.x; i < cfg.P * cfg.n_bins; i += LR_MTREND_THREADS) Xs[i] = X[i];
    __syncthreads();
    const int lane = threadIdx.x & (LR_WAVE - 1), wave = threadIdx.x / LR_WAVE;
    const int c = blockIdx.x * LR_MTREND_WAVES + wave;
    if (c >= cfg.n_chains) return;          // the whole wave: no barrier anywhere below
    const lr_stream rng{cfg.seed, (uint32_t)(cfg.chain0 + c)};
    const int P = cfg.P, nb = (cfg.n_bins + LR_WAVE - 1) / LR_WAVE;
    double dt[BPL], N[2], sdt;
    {
        double a_s = 0.0, a_e = 0.0, a_t = 0.0;
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int b = lane + LR_WAVE * i;
            const bool in = i < nb && b < cfg.n_bins;
            dt[i] = in ? DT[b] : 0.0;
            a_s += in ? n_spec[b] : 0.0, a_e += in ? n_exti[b] : 0.0, a_t += dt[i];
        }
        N[0] = lr_wave_sum(a_s), N[1] = lr_wave_sum(a_e), sdt = lr_wave_sum(a_t);
    }
    // SX beside the coefficient it multiplies
    double sx = 0.0;
#pragma unroll
    for (int j = 0; j < LR_MTREND_MAX_COVS; ++j) {
        if (lane == LR_MTREND_LANE_A + j) sx = cfg.sx[0][j];
        if (lane == LR_MTREND_LANE_B + j) sx = cfg.sx[1][j];
    }
    const bool free_lane = lr_mtrend_free_lane(cfg, lane);
    const unsigned free_bits = (cfg.free_b ? (1u << P) - 1u : 0u) | (cfg.free_d ? ((1u << P) - 1u) << 16 : 0u);
    double* st = state + (size_t)c * LR_MTREND_STATE_W;
    lr_mtrend_chain S;
    if (mode == 0) {
        const double l0 = N[0] / sdt, m0 = N[1] / sdt;
        S.base[0] = (l0 > 0.0 && l0 < INFINITY) ? l0 : 0.1, S.base[1] = (m0 > 0.0 && m0 < INFINITY) ? m0 : 0.1;
        const uint32_t idx = lane >= LR_MTREND_LANE_A ? (uint32_t)(lane - LR_MTREND_LANE_A) : (uint32_t)(P + lane - LR_MTREND_LANE_B);
        const double z = lr_normal(rng, 0ull, LR_P_MTREND_INIT, free_lane ? idx : 0u);
        S.coef = free_lane ? 0.1 * z : 0.0;
        S.I = cfg.bvs ? 0u : free_bits;
    } else {
        const double lo = st[lane], hi = lane < 32 ? st[LR_WAVE + lane] : 0.0;
        S.base[0] = lr_bcast(lo, LR_MTREND_S_L0), S.base[1] = lr_bcast(lo, LR_MTREND_S_M0);
        S.coef = free_lane ? (lane >= LR_MTREND_LANE_A ? lo : hi) : 0.0;
        const unsigned long long bl = __ballot(lo != 0.0), bm = __ballot(lane < 16 && hi != 0.0);
        S.I = (((unsigned)(bl >> LR_MTREND_S_IL) & 0xffffu) | (((unsigned)bm & 0xffffu) << 16)) & free_bits;
        S.lik[0] = lr_bcast(lo, LR_MTREND_S_LIK_B), S.lik[1] = lr_bcast(lo, LR_MTREND_S_LIK_D), S.prior = lr_bcast(lo, LR_MTREND_S_PRIOR);
        S.E[0] = lr_bcast(lo, LR_MTREND_S_E_B), S.E[1] = lr_bcast(lo, LR_MTREND_S_E_D);
        S.cnt = (lane >= LR_MTREND_S_PROPOSED && lane < LR_MTREND_S_IL) ? lo : 0.0;
    }
    if (mode != 2) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            if (side == 1 && cfg.no_death) {
                S.E[1] = 0.0, S.lik[1] = 0.0;
                continue;
            }
            const unsigned I16 = (S.I >> (16 * side)) & 0xffffu;
            S.E[side] = lr_mtrend_E<BPL>(Xs, dt, S.coef, I16, side, cfg, nb, lane);
            S.lik[side] = lr_mtrend_side_lik(N[side], S.base[side], S.coef, sx, I16, side, S.E[side], P);
        }
        S.prior = lr_mtrend_prior(S.base[0], S.base[1], S.coef, S.I, cfg, lane);
        S.cnt = 0.0;
    } else {
        // iterations to go until the next one with it % s_freq == 0: one 64-bit modulo per launch, not one per iteration
        long long until_row = (cfg.s_freq - it0 % cfg.s_freq) % cfg.s_freq;
        long long slot = cfg.slot0;
        for (long long it = it0; it < it0 + n_iters; ++it) {
            lr_mtrend_iterate<BPL>(S, Xs, dt, N, sx, cfg, rng, it, nb, lane);
            const bool sample = until_row == 0;
            until_row = sample ? cfg.s_freq - 1 : until_row - 1;
            if (sample) {
                // [it, posterior, likelihood, likelihood_birth, likelihood_death, prior, l0, m0, I_l[P], a[P], I_m[P], b[P]], the
                // rest 0 (rare path)
                double* row = rows + ((size_t)slot * cfg.n_chains + c) * LR_MTREND_ROW_W;
                slot += 1;
                const double tot = lr_mtrend_total(S.lik[0], S.lik[1]);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int p = lane + LR_WAVE * jj, q = p - LR_MTREND_R_IL;
                    const int blk = q >= 0 ? q / P : -1, j = q >= 0 ? q % P : 0;          // 0 I_l, 1 a, 2 I_m, 3 b
                    const double cj = __shfl(S.coef, (blk == 3 ? LR_MTREND_LANE_B : LR_MTREND_LANE_A) + j);
                    double h = 0.0;
                    if (p == LR_MTREND_R_IT) h = (double)it;
                    else if (p == LR_MTREND_R_POST) h = tot + S.prior;
                    else if (p == LR_MTREND_R_LIK) h = tot;
                    else if (p == LR_MTREND_R_LIK_B) h = S.lik[0];
                    else if (p == LR_MTREND_R_LIK_D) h = S.lik[1];
                    else if (p == LR_MTREND_R_PRIOR) h = S.prior;
                    else if (p == LR_MTREND_R_L0) h = S.base[0];
                    else if (p == LR_MTREND_R_M0) h = S.base[1];
                    else if (blk == 0) h = (double)((S.I >> j) & 1u);
                    else if (blk == 2) h = (double)((S.I >> (16 + j)) & 1u);
                    else if (blk == 1 || blk == 3) h = cj;
                    if (p < LR_MTREND_ROW_W) row[p] = h;
                }
            }
        }
    }
    // the state: a lane stores what it holds; what lies behind P in a block is 0 (coef is 0 there), as is every unnamed element
    double so = 0.0;
    if (lane == LR_MTREND_S_L0) so = S.base[0];
    if (lane == LR_MTREND_S_M0) so = S.base[1];
    if (lane == LR_MTREND_S_LIK_B) so = S.lik[0];
    if (lane == LR_MTREND_S_LIK_D) so = S.lik[1];
    if (lane == LR_MTREND_S_PRIOR) so = S.prior;
    if (lane == LR_MTREND_S_E_B) so = S.E[0];
    if (lane == LR_MTREND_S_E_D) so = S.E[1];
    if (lane >= LR_MTREND_S_PROPOSED && lane < LR_MTREND_S_IL) so = S.cnt;
    if (lane >= LR_MTREND_S_IL && lane < LR_MTREND_S_A) so = (double)((S.I >> (lane - LR_MTREND_S_IL)) & 1u);
    if (lane >= LR_MTREND_S_A) so = S.coef;
    st[lane] = so;
    if (lane < 32) st[LR_WAVE + lane] = lane < 16 ? (double)((S.I >> (16 + lane)) & 1u) : S.coef;
}

// ---- host -------------------------------------------------------------------------------------------------------------
// the checks of lr_mtrend_init (steps = false) and lr_mtrend_steps, in the header's order -> cfg
static int lr_mtrend_args(const lr_mtrend_problem* p, bool steps, int32_t given, int64_t it0, int64_t n_iters, int32_t s_freq,
                          const double* rows, int64_t rows_cap, int64_t slot0, lr_mtrend_cfg* cfg) {
    // (rows may be NULL where no row is due)
    int64_t need = 0;
    const bool counts_ok = !steps || lr_rows_due(it0, n_iters, s_freq, &need);
    if (!p) return LR_ERR_NULL;
    if (!p->n_spec || !p->n_exti || !p->DT || !p->X || !p->sx_spec || !p->sx_exti || !p->state ||
        (steps && !rows && counts_ok && need > 0))
        return LR_ERR_NULL;
    if (p->n_bins < 1 || p->n_bins > LR_MTREND_MAX_BINS || p->P < 1 || p->P > LR_MTREND_MAX_COVS || p->C < 1) return LR_ERR_SIZE;
    if (!steps && given != 0 && given != 1) return LR_ERR_SIZE;
    if ((p->m_birth != 0 && p->m_birth != 1) || (p->m_death != 0 && p->m_death != 1) || (p->no_death != 0 && p->no_death != 1) ||
        (p->bvs != 0 && p->bvs != 1) || !(p->pI > 0.0 && p->pI < 1.0) || !(p->slab_sd > 0.0 && std::isfinite(p->slab_sd)) ||
        !(p->win[0] >= 0.0 && std::isfinite(p->win[0])) || !(p->win[1] >= 0.0 && std::isfinite(p->win[1])) || p->bvs_from < 0)
        return LR_ERR_MODEL;
    if (steps && (!counts_ok || slot0 < 0 || rows_cap < 0 || rows_cap - slot0 < need)) return LR_ERR_SIZE;
    for (int j = 0; j < LR_MTREND_MAX_COVS; ++j)
        cfg->sx[0][j] = j < p->P ? p->sx_spec[j] : 0.0, cfg->sx[1][j] = j < p->P ? p->sx_exti[j] : 0.0;
    cfg->log_pI = std::log(p->pI), cfg->log_1mpI = std::log1p(-p->pI), cfg->mult_l = 2.0 * std::log(LR_MULT_D);
    cfg->slab_sd = p->slab_sd, cfg->norm_c = -LR_MTREND_HALF_LOG_2PI - std::log(p->slab_sd);
    cfg->win[0] = p->win[0], cfg->win[1] = p->win[1];
    cfg->rows_cap = steps ? rows_cap : 0, cfg->slot0 = steps ? slot0 : 0, cfg->chain0 = p->chain0, cfg->bvs_from = p->bvs_from;
    cfg->n_bins = p->n_bins, cfg->P = p->P, cfg->n_chains = p->C;
    cfg->free_b = p->m_birth ? 0 : 1, cfg->free_d = (p->m_death || p->no_death) ? 0 : 1, cfg->no_death = p->no_death;
    cfg->bvs = p->bvs, cfg->s_freq = steps ? s_freq : 1, cfg->seed = (uint32_t)p->seed;
    return LR_OK;
}

template <int BPL>
static void lr_mtrend_launch_as(const lr_mtrend_problem* p, const lr_mtrend_cfg& cfg, int mode, int64_t it0, int64_t n_iters, double* rows) {
    const unsigned blocks = (unsigned)((cfg.n_chains + LR_MTREND_WAVES - 1) / LR_MTREND_WAVES);
    const size_t lds = (size_t)cfg.P * cfg.n_bins * sizeof(double);
    hipLaunchKernelGGL((lr_mtrend_chain_kernel<BPL>), dim3(blocks), dim3(LR_MTREND_THREADS), lds, (hipStream_t)p->stream, p->n_spec, p->n_exti,
                       p->DT, p->X, cfg, mode, p->state, (long long)it0, (long long)n_iters, rows);
}

static int lr_mtrend_launch(const lr_mtrend_problem* p, const lr_mtrend_cfg& cfg, int mode, int64_t it0, int64_t n_iters, double* rows) {
    const int bpl = (cfg.n_bins + LR_WAVE - 1) / LR_WAVE;
    if (bpl <= 1) lr_mtrend_launch_as<1>(p, cfg, mode, it0, n_iters, rows);
    else if (bpl <= 2) lr_mtrend_launch_as<2>(p, cfg, mode, it0, n_iters, rows);
    else if (bpl <= 4) lr_mtrend_launch_as<4>(p, cfg, mode, it0, n_iters, rows);
    else lr_mtrend_launch_as<8>(p, cfg, mode, it0, n_iters, rows);
    return (int)hipGetLastError();
}

extern "C" int lr_mtrend_init(const lr_mtrend_problem* p, int32_t given) {
    lr_mtrend_cfg cfg;
    const int rc = lr_mtrend_args(p, false, given, 0, 0, 1, nullptr, 0, 0, &cfg);
    if (rc != LR_OK) return rc;
    return lr_mtrend_launch(p, cfg, given ? 1 : 0, 0, 0, nullptr);
}

extern "C" int lr_mtrend_steps(const lr_mtrend_problem* p, int64_t it0, int64_t n_iters, int32_t s_freq, double* rows, int64_t rows_cap,
                               int64_t slot0) {
    lr_mtrend_cfg cfg;
    const int rc = lr_mtrend_args(p, true, 0, it0, n_iters, s_freq, rows, rows_cap, slot0, &cfg);
    if (rc != LR_OK) return rc;
    if (n_iters == 0) return LR_OK;
    return lr_mtrend_launch(p, cfg, 2, it0, n_iters, rows);
}
