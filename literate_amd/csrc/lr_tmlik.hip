// lr_tmlik.hip - marginal likelihoods of the trend_rate.py models (include/literate_hip_tmlik.h): trend_rate.py's
// Metropolis-Hastings sampler on the power posteriors L^beta p of a ladder of temperatures, for a grid of (model, replicate,
// temperature) chains in one launch.  A sibling of lr_mlik_chain_kernel (lr_mlik.hip); the rows are lr_mlik_estimate's.
//
//   lr_tmlik_chain_kernel    one wave per chain, four independent waves per workgroup: its initial state, or n_iters
//                            iterations from its state
//
// The trend likelihood is a function of the per-bin statistics and the covariate alone (trend_rate.py:73-91), so an iteration
// costs O(n_bins) whatever the number of lineages: bin b sits in lane b % 64, at most 8 bins to a lane, and N_SPEC, N_EXTI, DT
// and the LOGARITHM of the chain's covariate column stay in registers for the whole launch.  The six parameters sit in lanes
// 0-5 and the rate map, prior and update probabilities are lr_dd.h's - the expressions the trend engine evaluates.  No LDS, no
// barrier: a wave never waits for another.  Every sum is a fixed tree (lr_wave_sum over the lanes, a lane's bins in order), no
// floating-point atomics: a chain's bits depend on its own arguments alone.
#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_tmlik.h"
#include "lr_dd.h"
#include "lr_internal.h"

#define LR_TMLIK_THREADS 256
#define LR_TMLIK_WAVES (LR_TMLIK_THREADS / LR_WAVE)
#define LR_TMLIK_BPL (LR_TMLIK_MAX_BINS / LR_WAVE) /* bins per lane */
#define LR_TMLIK_S_LIK 6
#define LR_TMLIK_S_PRIOR 7
#define LR_TMLIK_S_PROPOSED 8
#define LR_TMLIK_S_ACCEPTED 10
#define LR_TMLIK_S_BETA 12
#define LR_TMLIK_S_SCALE 13
#define LR_TMLIK_S_WIN 14
#define LR_TMLIK_S_MODEL 15

static_assert(LR_TMLIK_BPL == 8, "a lane holds at most 8 bins");
static_assert(LR_TMLIK_S_MODEL + 1 == LR_TMLIK_STATE_W && 4 + LR_TR_NPAR + 2 == LR_TMLIK_ROW_W, "state and row layout");

struct lr_tmlik_cfg {
    double mult_l;
    long long rows_cap, slot0;
    int n_bins, M, R, T, n_chains, s_freq;
    uint32_t seed;
};
// the host tables of a call: per temperature and per model
struct lr_tmlik_tables {
    double beta[LR_TMLIK_MAX_TEMPS], scale[LR_TMLIK_MAX_TEMPS];
    int32_t col[LR_TMLIK_MAX_MODELS], key0[LR_TMLIK_MAX_MODELS];
    uint8_t flags[LR_TMLIK_MAX_MODELS];
};
// (the kernel's argument block: five input pointers, the state and the rows, the mode and the iteration range beside these)
static_assert(sizeof(lr_tmlik_cfg) + sizeof(lr_tmlik_tables) + 7 * sizeof(void*) + 3 * sizeof(long long) < 4096,
              "the kernel arguments stay under 4 KB");

// a lane's bins: b = lane + 64 i, i < nb; lt = lr_log of the chain's covariate
struct lr_tmlik_bins {
    double ns[LR_TMLIK_BPL], ne[LR_TMLIK_BPL], dt[LR_TMLIK_BPL], lt[LR_TMLIK_BPL];
    int nb;
};

// likelihood_function's sum (trend_rate.py:89-91) under the parameters in lanes 0-5 of P; NaN -> -inf
__device__ __forceinline__ double lr_tmlik_loglik(double P, const lr_tmlik_bins& B, int n_bins, int const_b, int const_d,
                                                  int lane) {
    const lr_trend_params p = lr_trend_unpack(P);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < LR_TMLIK_BPL; ++i) {
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

__global__ __launch_bounds__(LR_TMLIK_THREADS) void lr_tmlik_chain_kernel(
    const double* __restrict__ n_spec, const double* __restrict__ n_exti, const double* __restrict__ DT,
    const double* __restrict__ trends, const double* __restrict__ wins, lr_tmlik_cfg cfg, lr_tmlik_tables tb, int mode,
    double* __restrict__ state, long long it0, long long n_iters, double* __restrict__ rows) {
    const int lane = threadIdx.x & (LR_WAVE - 1), wave = threadIdx.x / LR_WAVE;
    const int c = blockIdx.x * LR_TMLIK_WAVES + wave;
    if (c >= cfg.n_chains) return;          // the whole wave: no barrier anywhere below
    const int j = c % cfg.T, mr = c / cfg.T, r = mr % cfg.R, m = mr / cfg.R;
    const double beta = tb.beta[j], scale = tb.scale[j];
    const int const_b = tb.flags[m] & 1, const_d = (tb.flags[m] >> 1) & 1;
    const lr_stream rng{cfg.seed, (uint32_t)((tb.key0[m] + r) * cfg.T + j)};
    const double win = wins[(size_t)m * cfg.T + j];
    const double* trend = trends + (size_t)tb.col[m] * cfg.n_bins;
    lr_tmlik_bins B;
    B.nb = (cfg.n_bins + LR_WAVE - 1) / LR_WAVE;
#pragma unroll
    for (int i = 0; i < LR_TMLIK_BPL; ++i) {
        const int b = lane + LR_WAVE * i;
        const bool in = i < B.nb && b < cfg.n_bins;
        B.ns[i] = in ? n_spec[b] : 0.0, B.ne[i] = in ? n_exti[b] : 0.0, B.dt[i] = in ? DT[b] : 1.0;
        B.lt[i] = lr_log(in ? trend[b] : 1.0);
    }
    double* st = state + (size_t)c * LR_TMLIK_STATE_W;
    double A, likA, priorA, prop0, prop1, acc0, acc1;          // proposals made / accepted per move kind
    if (mode == 0) {
        const double init[LR_TR_NPAR] = {.1, .1, 0.0, 0.0, 1.0, 1.0};          // trend_rate.py:137
        A = 0.0;
#pragma unroll
        for (int i = 0; i < LR_TR_NPAR; ++i) A = (lane == i) ? init[i] : A;
        likA = lr_tmlik_loglik(A, B, cfg.n_bins, const_b, const_d, lane);
        priorA = lr_trend_prior(A, lane);
        prop0 = prop1 = acc0 = acc1 = 0.0;
    } else {
        A = lane < LR_TR_NPAR ? st[lane] : 0.0;
        likA = st[LR_TMLIK_S_LIK], priorA = st[LR_TMLIK_S_PRIOR];
        prop0 = st[LR_TMLIK_S_PROPOSED], prop1 = st[LR_TMLIK_S_PROPOSED + 1];
        acc0 = st[LR_TMLIK_S_ACCEPTED], acc1 = st[LR_TMLIK_S_ACCEPTED + 1];
        double f_mult, f_norm;
        lr_trend_update_freq(const_b, const_d, lane, &f_mult, &f_norm);
        const double mult_l = scale * cfg.mult_l;
        // iterations to go until the next one with it % s_freq == 0: one 64-bit modulo per launch, not one per iteration
        long long until_row = (cfg.s_freq - it0 % cfg.s_freq) % cfg.s_freq;
        long long slot = cfg.slot0;
        for (long long it = it0; it < it0 + n_iters; ++it) {
            // the wave-uniform draws in one Philox call: lane 0 the acceptance uniform, lane 1 the move selector (as the trend
            // engine's proposal takes them)
            const lr_u2 ud = lr_pair(rng, (uint64_t)it, lane == 0 ? LR_P_TR_ACCEPT : LR_P_TR_MOVE, 0u);
            const double log_u = lr_bcast(lr_log(lane == 0 ? ud.a : 1.0), 0);
            const lr_u2 d = lr_pair(rng, (uint64_t)it, LR_P_TR_MULT, lane);
            double P = A, hasting = 0.0;
            int move;
            bool moved = true;
            if (lr_bcast(ud.a, 1) < .33) {
                const double z = lr_normal(rng, (uint64_t)it, LR_P_TR_NORM, lane);   // update_normal_nobound_vec (lib:140-146)
                const bool fires = lane < LR_TR_NPAR && d.a < f_norm;
                if (fires) P = A + z * win;
                // a step whose mask fires for no slope proposes the state itself: it is always accepted and says nothing about
                // the window, so it is not counted (the windows are tuned from these counters)
                moved = __ballot(fires) != 0ull;
                move = 1;
            } else {
                hasting = lr_wave_multiplier(P, LR_TR_NPAR, d.a < f_mult, d.b, mult_l, lane);   // lib:156-165
                move = 0;
            }
            const double prior = lr_trend_prior(P, lane);
            const double lik = lr_tmlik_loglik(P, B, cfg.n_bins, const_b, const_d, lane);
            const double dl = beta == 0.0 ? 0.0 : beta * (lik - likA);
            const bool ok = (dl + (prior - priorA) + hasting > log_u) || it == 0;      // trend_rate.py:176
            prop0 += move ? 0.0 : 1.0, prop1 += (move && moved) ? 1.0 : 0.0;
            if (ok) A = P, likA = lik, priorA = prior, acc0 += move ? 0.0 : 1.0, acc1 += (move && moved) ? 1.0 : 0.0;
            const bool sample = until_row == 0;
            until_row = sample ? cfg.s_freq - 1 : until_row - 1;
            if (sample) {
                double* row = rows + ((((size_t)m * cfg.rows_cap + slot) * cfg.R + r) * cfg.T + j) * LR_TMLIK_ROW_W;
                slot += 1;
                const double Aj = __shfl(A, (lane - 4) & (LR_WAVE - 1));        // rare path (sampling only)
                double h = Aj;
                if (lane == 0) h = (double)it;
                if (lane == 1) h = beta;
                if (lane == 2) h = likA;
                if (lane == 3) h = priorA;
                if (lane == 4 + LR_TR_NPAR) h = win;
                if (lane == 5 + LR_TR_NPAR) h = (double)m;
                if (lane < LR_TMLIK_ROW_W) row[lane] = h;
            }
        }
    }
    double so = A;
    if (lane == LR_TMLIK_S_LIK) so = likA;
    if (lane == LR_TMLIK_S_PRIOR) so = priorA;
    if (lane == LR_TMLIK_S_PROPOSED) so = prop0;
    if (lane == LR_TMLIK_S_PROPOSED + 1) so = prop1;
    if (lane == LR_TMLIK_S_ACCEPTED) so = acc0;
    if (lane == LR_TMLIK_S_ACCEPTED + 1) so = acc1;
    if (lane == LR_TMLIK_S_BETA) so = beta;
    if (lane == LR_TMLIK_S_SCALE) so = scale;
    if (lane == LR_TMLIK_S_WIN) so = win;
    if (lane == LR_TMLIK_S_MODEL) so = (double)m;
    if (lane < LR_TMLIK_STATE_W) st[lane] = so;
}

// ---- host -------------------------------------------------------------------------------------------------------------
static int lr_tmlik_args(const lr_tmlik_problem* p, bool steps, int64_t it0, int64_t n_iters, int32_t s_freq, const double* rows,
                         int64_t rows_cap, int64_t slot0, lr_tmlik_cfg* cfg, lr_tmlik_tables* tb) {
    // (rows may be NULL where no row is due)
    int64_t need = 0;
    const bool counts_ok = !steps || lr_rows_due(it0, n_iters, s_freq, &need);
    if (!p) return LR_ERR_NULL;
    if (!p->n_spec || !p->n_exti || !p->DT || !p->trends || !p->wins || !p->state || !p->betas || !p->scales || !p->col ||
        !p->flags || !p->key0 || (steps && !rows && counts_ok && need > 0))
        return LR_ERR_NULL;          // (rows: only where the step arguments are valid and a row is due - else they are named below)
    const int T = p->T, M = p->n_models, R = p->n_reps;
    if (p->n_bins < 1 || p->n_bins > LR_TMLIK_MAX_BINS || p->n_cols < 1 || T < 2 || T > LR_TMLIK_MAX_TEMPS || M < 1 ||
        M > LR_TMLIK_MAX_MODELS || R < 1)
        return LR_ERR_SIZE;
    if ((int64_t)M * R * T > INT32_MAX) return LR_ERR_SIZE;
    for (int m = 0; m < M; ++m) {
        if (p->col[m] < 0 || p->col[m] >= p->n_cols || p->flags[m] < 0 || p->flags[m] > 3) return LR_ERR_MODEL;
        if (p->key0[m] < 0 || p->key0[m] > INT32_MAX || (p->key0[m] + R) * T > INT32_MAX) return LR_ERR_MODEL;
        tb->col[m] = p->col[m], tb->flags[m] = (uint8_t)p->flags[m], tb->key0[m] = (int32_t)p->key0[m];
    }
    if (p->betas[0] != 0.0 || p->betas[T - 1] != 1.0) return LR_ERR_MODEL;
    for (int j = 0; j + 1 < T; ++j)
        if (!(p->betas[j + 1] > p->betas[j])) return LR_ERR_MODEL;
    for (int j = 0; j < T; ++j) {
        if (!(std::isfinite(p->scales[j]) && p->scales[j] > 0.0)) return LR_ERR_MODEL;
        tb->beta[j] = p->betas[j], tb->scale[j] = p->scales[j];
    }
    if (steps && (!counts_ok || slot0 < 0 || rows_cap < 0 || rows_cap - slot0 < need)) return LR_ERR_SIZE;
    cfg->mult_l = 2.0 * std::log(LR_MULT_D);
    cfg->rows_cap = steps ? rows_cap : 0, cfg->slot0 = steps ? slot0 : 0;
    cfg->n_bins = p->n_bins, cfg->M = M, cfg->R = R, cfg->T = T, cfg->n_chains = M * R * T;
    cfg->s_freq = steps ? s_freq : 1, cfg->seed = (uint32_t)p->seed;
    return LR_OK;
}

static int lr_tmlik_launch(const lr_tmlik_problem* p, const lr_tmlik_cfg& cfg, const lr_tmlik_tables& tb, int mode, int64_t it0,
                           int64_t n_iters, double* rows) {
    const unsigned blocks = (unsigned)((cfg.n_chains + LR_TMLIK_WAVES - 1) / LR_TMLIK_WAVES);
    hipLaunchKernelGGL(lr_tmlik_chain_kernel, dim3(blocks), dim3(LR_TMLIK_THREADS), 0, (hipStream_t)p->stream, p->n_spec,
                       p->n_exti, p->DT, p->trends, p->wins, cfg, tb, mode, p->state, (long long)it0, (long long)n_iters, rows);
    return (int)hipGetLastError();
}

extern "C" int lr_tmlik_init(const lr_tmlik_problem* p) {
    lr_tmlik_cfg cfg;
    lr_tmlik_tables tb = {};
    const int rc = lr_tmlik_args(p, false, 0, 0, 1, nullptr, 0, 0, &cfg, &tb);
    if (rc != LR_OK) return rc;
    return lr_tmlik_launch(p, cfg, tb, 0, 0, 0, nullptr);
}

extern "C" int lr_tmlik_steps(const lr_tmlik_problem* p, int64_t it0, int64_t n_iters, int32_t s_freq, double* rows,
                              int64_t rows_cap, int64_t slot0) {
    lr_tmlik_cfg cfg;
    lr_tmlik_tables tb = {};
    const int rc = lr_tmlik_args(p, true, it0, n_iters, s_freq, rows, rows_cap, slot0, &cfg, &tb);
    if (rc != LR_OK) return rc;
    if (n_iters == 0) return LR_OK;
    return lr_tmlik_launch(p, cfg, tb, 1, it0, n_iters, rows);
}
