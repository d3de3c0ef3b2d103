// lr_parbin.hip - the parametric samplers on per-chain binned statistics (include/literate_hip_parbin.h): DDRate.py's and
// trend_rate.py's Metropolis-Hastings loops for chains that do not share their data - replicate data sets, one stochastic
// imputation each - all of them in one launch.
//
//   lr_parbin_chain_kernel<BPL, SAMPLER>   one wave per chain, four independent waves per workgroup: its initial state, or
//                                          n_iters iterations from its state
//
// Both likelihoods are functions of the per-bin statistics alone, so an iteration costs O(n_bins) whatever the number of
// lineages: bin b sits in lane b % 64, BPL = 1, 2, 4 or 8 bins to a lane, and the replicate's N_SPEC, N_EXTI and DT - for
// sampler 2 also the LOGARITHM of the covariate, taken once per launch - stay in registers for the whole launch.  The chain
// and its iteration are lr_par_iter.h's, the ones lr_mlik.hip and lr_tmlik.hip run on their ladders, here at beta = 1,
// scale = 1 (and window 0.001).  No LDS, no barrier: a wave never waits for another.  Every sum is a fixed tree (a lane's
// bins in order, then lr_wave_sum), no floating-point atomics: a chain's bits depend on its own arguments alone.
#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_parbin.h"
#include "lr_dd.h"
#include "lr_internal.h"
#include "lr_par_iter.h"          // the chain and its iteration: shared with lr_mlik.hip and lr_tmlik.hip

#define LR_PARBIN_THREADS 256
#define LR_PARBIN_WAVES (LR_PARBIN_THREADS / LR_WAVE)
#define LR_PARBIN_WIN 0.001 /* update_normal_nobound_vec's d (trend_rate.py:167) */

static_assert(LR_PARBIN_S_ACCEPTED + 4 == LR_PARBIN_STATE_W && LR_PARBIN_S_LIK == LR_DD_NPAR && LR_TR_NPAR <= LR_DD_NPAR,
              "state layout");
static_assert(4 + LR_DD_NPAR <= LR_WAVE && 2 * LR_WAVE < LR_TRACE_W && LR_TRACE_W <= 3 * LR_WAVE, "a row is three stores of a wave");
static_assert(LR_PARBIN_MAX_BINS == 8 * LR_WAVE, "a lane holds at most 8 bins");

struct lr_parbin_cfg {
    double init_death, mult_l;
    long long rows_cap, slot0, chain0;
    int n_bins, n_chains, chains_per_rep, m_birth, m_death, s_freq;
    uint32_t seed;
};

template <int BPL, int SAMPLER>
__global__ __launch_bounds__(LR_PARBIN_THREADS) void lr_parbin_chain_kernel(
    const double* __restrict__ n_spec, const double* __restrict__ n_exti, const double* __restrict__ DT,
    const double* __restrict__ origin, const double* __restrict__ present, const double* __restrict__ trend, lr_parbin_cfg cfg,
    int mode, double* __restrict__ state, long long it0, long long n_iters, double* __restrict__ rows) {
    constexpr bool TREND = SAMPLER == 2;
    constexpr int NPAR = TREND ? LR_TR_NPAR : LR_DD_NPAR;
    const int lane = threadIdx.x & (LR_WAVE - 1), wave = threadIdx.x / LR_WAVE;
    const int c = blockIdx.x * LR_PARBIN_WAVES + wave;
    if (c >= cfg.n_chains) return;          // the whole wave: no barrier anywhere below
    const int rep = c / cfg.chains_per_rep;
    const lr_stream rng{cfg.seed, (uint32_t)(cfg.chain0 + c)};
    const size_t off = (size_t)rep * cfg.n_bins;
    lr_par_bins<BPL, TREND> B;
    const double dt_max = lr_par_load_bins<BPL, TREND>(B, n_spec + off, n_exti + off, DT + off, trend, cfg.n_bins, lane);
    lr_ddi_run dd;
    lr_tri_run tr;
    if constexpr (TREND) {
        tr.beta = 1.0, tr.mult_l = cfg.mult_l, tr.win = LR_PARBIN_WIN;
        tr.n_bins = cfg.n_bins, tr.const_b = cfg.m_birth, tr.const_d = cfg.m_death;
        lr_trend_update_freq(tr.const_b, tr.const_d, lane, &tr.f_mult, &tr.f_norm);
    } else {
        dd.origin = origin[rep], dd.present = present[rep], dd.beta = 1.0;
        dd.n_bins = cfg.n_bins, dd.m_birth = cfg.m_birth, dd.m_death = cfg.m_death;
        lr_ddi_run_of(dd, dt_max, 1.0, cfg.mult_l, lane);
    }
    double* st = state + (size_t)c * LR_PARBIN_STATE_W;
    lr_par_chain S;
    if (mode == 0) {
        if constexpr (TREND) lr_tri_start<BPL>(S, B, tr, lane);
        else lr_ddi_start<BPL>(S, B, dd, cfg.init_death, lane);
    } else {
        S.A = lane < NPAR ? st[lane] : 0.0;
        S.likA = st[LR_PARBIN_S_LIK], S.priorA = st[LR_PARBIN_S_PRIOR];
        S.prop0 = st[LR_PARBIN_S_PROPOSED], S.prop1 = st[LR_PARBIN_S_PROPOSED + 1];
        S.acc0 = st[LR_PARBIN_S_ACCEPTED], S.acc1 = st[LR_PARBIN_S_ACCEPTED + 1];
        // iterations to go until the next one with it % s_freq == 0: one 64-bit modulo per launch, not one per iteration
        long long until_row = (cfg.s_freq - it0 % cfg.s_freq) % cfg.s_freq;
        long long slot = cfg.slot0;
        for (long long it = it0; it < it0 + n_iters; ++it) {
            if constexpr (TREND) lr_tri_iterate<BPL>(S, B, tr, rng, it, lane);
            else lr_ddi_iterate<BPL>(S, B, dd, rng, it, lane);
            const bool sample = until_row == 0;
            until_row = sample ? cfg.s_freq - 1 : until_row - 1;
            if (sample) {
                // the engines' trace row of this sampler: [it, posterior, likelihood, prior, args], the rest 0
                double* row = rows + ((size_t)slot * cfg.n_chains + c) * LR_TRACE_W;
                slot += 1;
                const double Aj = __shfl(S.A, (lane - 4) & (LR_WAVE - 1));        // rare path (sampling only)
                double h = lane < 4 + NPAR ? Aj : 0.0;
                if (lane == 0) h = (double)it;
                if (lane == 1) h = S.likA + S.priorA;
                if (lane == 2) h = S.likA;
                if (lane == 3) h = S.priorA;
                row[lane] = h, row[LR_WAVE + lane] = 0.0;
                if (2 * LR_WAVE + lane < LR_TRACE_W) row[2 * LR_WAVE + lane] = 0.0;
            }
        }
    }
    double so = lane < NPAR ? S.A : 0.0;
    if (lane == LR_PARBIN_S_LIK) so = S.likA;
    if (lane == LR_PARBIN_S_PRIOR) so = S.priorA;
    if (lane == LR_PARBIN_S_PROPOSED) so = S.prop0;
    if (lane == LR_PARBIN_S_PROPOSED + 1) so = S.prop1;
    if (lane == LR_PARBIN_S_ACCEPTED) so = S.acc0;
    if (lane == LR_PARBIN_S_ACCEPTED + 1) so = S.acc1;
    if (lane < LR_PARBIN_STATE_W) st[lane] = so;
}

// ---- host -------------------------------------------------------------------------------------------------------------
// the checks of lr_parbin_init (steps = false) and lr_parbin_steps, in the header's order -> cfg
static int lr_parbin_args(const lr_parbin_problem* p, bool steps, int64_t it0, int64_t n_iters, int32_t s_freq, const double* rows,
                          int64_t rows_cap, int64_t slot0, lr_parbin_cfg* cfg) {
    // (rows may be NULL where no row is due)
    int64_t need = 0;
    const bool counts_ok = !steps || lr_rows_due(it0, n_iters, s_freq, &need);
    if (!p) return LR_ERR_NULL;
    if (!p->n_spec || !p->n_exti || !p->DT || !p->origin || !p->present || !p->state || (p->sampler == 2 && !p->trend) ||
        (steps && !rows && counts_ok && need > 0))
        return LR_ERR_NULL;
    if (p->n_bins < 1 || p->n_bins > LR_PARBIN_MAX_BINS || p->R < 1 || p->chains_per_rep < 1) return LR_ERR_SIZE;
    if ((int64_t)p->R * p->chains_per_rep > INT32_MAX) return LR_ERR_SIZE;
    if (p->sampler != 1 && p->sampler != 2) return LR_ERR_MODEL;
    if (p->sampler == 1 && (p->m_birth < 0 || p->m_birth > 2 || p->m_death < -2 || p->m_death > 2 || !std::isfinite(p->init_death)))
        return LR_ERR_MODEL;
    if (p->sampler == 2 && (p->m_birth < 0 || p->m_birth > 1 || p->m_death < 0 || p->m_death > 1)) return LR_ERR_MODEL;
    if (steps && (!counts_ok || slot0 < 0 || rows_cap < 0 || rows_cap - slot0 < need)) return LR_ERR_SIZE;
    cfg->init_death = p->init_death, cfg->mult_l = 2.0 * std::log(LR_MULT_D);
    cfg->rows_cap = steps ? rows_cap : 0, cfg->slot0 = steps ? slot0 : 0, cfg->chain0 = p->chain0;
    cfg->n_bins = p->n_bins, cfg->n_chains = p->R * p->chains_per_rep, cfg->chains_per_rep = p->chains_per_rep;
    cfg->m_birth = p->m_birth, cfg->m_death = p->m_death, cfg->s_freq = steps ? s_freq : 1, cfg->seed = (uint32_t)p->seed;
    return LR_OK;
}

template <int BPL, int SAMPLER>
static void lr_parbin_launch_as(const lr_parbin_problem* p, const lr_parbin_cfg& cfg, int mode, int64_t it0, int64_t n_iters,
                                double* rows) {
    const unsigned blocks = (unsigned)((cfg.n_chains + LR_PARBIN_WAVES - 1) / LR_PARBIN_WAVES);
    hipLaunchKernelGGL((lr_parbin_chain_kernel<BPL, SAMPLER>), dim3(blocks), dim3(LR_PARBIN_THREADS), 0, (hipStream_t)p->stream,
                       p->n_spec, p->n_exti, p->DT, p->origin, p->present, p->trend, cfg, mode, p->state, (long long)it0,
                       (long long)n_iters, rows);
}

template <int SAMPLER>
static void lr_parbin_launch_bpl(const lr_parbin_problem* p, const lr_parbin_cfg& cfg, int mode, int64_t it0, int64_t n_iters,
                                 double* rows) {
    const int bpl = (cfg.n_bins + LR_WAVE - 1) / LR_WAVE;
    if (bpl <= 1) lr_parbin_launch_as<1, SAMPLER>(p, cfg, mode, it0, n_iters, rows);
    else if (bpl <= 2) lr_parbin_launch_as<2, SAMPLER>(p, cfg, mode, it0, n_iters, rows);
    else if (bpl <= 4) lr_parbin_launch_as<4, SAMPLER>(p, cfg, mode, it0, n_iters, rows);
    else lr_parbin_launch_as<8, SAMPLER>(p, cfg, mode, it0, n_iters, rows);
}

static int lr_parbin_launch(const lr_parbin_problem* p, const lr_parbin_cfg& cfg, int mode, int64_t it0, int64_t n_iters,
                            double* rows) {
    if (p->sampler == 1) lr_parbin_launch_bpl<1>(p, cfg, mode, it0, n_iters, rows);
    else lr_parbin_launch_bpl<2>(p, cfg, mode, it0, n_iters, rows);
    return (int)hipGetLastError();
}

extern "C" int lr_parbin_init(const lr_parbin_problem* p) {
    lr_parbin_cfg cfg;
    const int rc = lr_parbin_args(p, false, 0, 0, 1, nullptr, 0, 0, &cfg);
    if (rc != LR_OK) return rc;
    return lr_parbin_launch(p, cfg, 0, 0, 0, nullptr);
}

extern "C" int lr_parbin_steps(const lr_parbin_problem* p, int64_t it0, int64_t n_iters, int32_t s_freq, double* rows,
                               int64_t rows_cap, int64_t slot0) {
    lr_parbin_cfg cfg;
    const int rc = lr_parbin_args(p, true, it0, n_iters, s_freq, rows, rows_cap, slot0, &cfg);
    if (rc != LR_OK) return rc;
    if (n_iters == 0) return LR_OK;
    return lr_parbin_launch(p, cfg, 1, it0, n_iters, rows);
}
