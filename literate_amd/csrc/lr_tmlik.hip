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
#include "lr_par_iter.h"          // the chain and its iteration: shared with lr_parbin.hip

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
    lr_par_bins<LR_TMLIK_BPL, true> B;          // (with lr_log of the chain's covariate)
    lr_par_load_bins<LR_TMLIK_BPL, true>(B, n_spec, n_exti, DT, trend, cfg.n_bins, lane);
    lr_tri_run run;
    run.beta = beta, run.mult_l = scale * cfg.mult_l, run.win = win;
    run.n_bins = cfg.n_bins, run.const_b = const_b, run.const_d = const_d;
    lr_trend_update_freq(const_b, const_d, lane, &run.f_mult, &run.f_norm);
    double* st = state + (size_t)c * LR_TMLIK_STATE_W;
    lr_par_chain S;
    if (mode == 0) {
        lr_tri_start<LR_TMLIK_BPL>(S, B, run, lane);
    } else {
        S.A = lane < LR_TR_NPAR ? st[lane] : 0.0;
        S.likA = st[LR_TMLIK_S_LIK], S.priorA = st[LR_TMLIK_S_PRIOR];
        S.prop0 = st[LR_TMLIK_S_PROPOSED], S.prop1 = st[LR_TMLIK_S_PROPOSED + 1];
        S.acc0 = st[LR_TMLIK_S_ACCEPTED], S.acc1 = st[LR_TMLIK_S_ACCEPTED + 1];
        // iterations to go until the next one with it % s_freq == 0: one 64-bit modulo per launch, not one per iteration
        long long until_row = (cfg.s_freq - it0 % cfg.s_freq) % cfg.s_freq;
        long long slot = cfg.slot0;
        for (long long it = it0; it < it0 + n_iters; ++it) {
            lr_tri_iterate<LR_TMLIK_BPL>(S, B, run, rng, it, lane);          // lr_par_iter.h: shared with lr_parbin.hip
            const bool sample = until_row == 0;
            until_row = sample ? cfg.s_freq - 1 : until_row - 1;
            if (sample) {
                double* row = rows + ((((size_t)m * cfg.rows_cap + slot) * cfg.R + r) * cfg.T + j) * LR_TMLIK_ROW_W;
                slot += 1;
                const double Aj = __shfl(S.A, (lane - 4) & (LR_WAVE - 1));        // rare path (sampling only)
                double h = Aj;
                if (lane == 0) h = (double)it;
                if (lane == 1) h = beta;
                if (lane == 2) h = S.likA;
                if (lane == 3) h = S.priorA;
                if (lane == 4 + LR_TR_NPAR) h = win;
                if (lane == 5 + LR_TR_NPAR) h = (double)m;
                if (lane < LR_TMLIK_ROW_W) row[lane] = h;
            }
        }
    }
    const double A = S.A, likA = S.likA, priorA = S.priorA, prop0 = S.prop0, prop1 = S.prop1, acc0 = S.acc0, acc1 = S.acc1;
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
