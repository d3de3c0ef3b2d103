// lr_mlik.hip - marginal likelihoods of the DDRate models (include/literate_hip_mlik.h): DDRate.py's Metropolis-Hastings
// sampler on the power posteriors L^beta p of a ladder of temperatures, and the estimators that read its rows.
//
//   lr_mlik_chain_kernel     one wave per chain, four independent waves per workgroup: its initial state, or n_iters
//                            iterations from its state
//   lr_mlik_stats_kernel     one workgroup per (replicate, temperature): mean, variance and stone of its likelihoods; one per
//                            temperature more: the stone over all replicates' samples
//   lr_mlik_sums_kernel      the sums over the temperatures: ss, ti per replicate and the pooled sum
//
// The DDRate likelihood is a function of the per-bin statistics alone (DD:71-107), so an iteration costs O(n_bins) whatever
// the number of lineages: bin b sits in lane b % 64, at most 8 bins to a lane, and N_SPEC, N_EXTI and DT stay in registers for
// the whole launch.  The eight parameters sit in lanes 0-7 and the proposal, prior and rate map are lr_dd.h's - the expressions
// the DD engine evaluates: lr_dd_update_freq(), lr_dd_prior() and lr_dd_bin_rates() are called from the chain's iteration,
// which stands in lr_par_iter.h (lr_ddi_*) since lr_parbin.hip runs the same chain on replicate data sets.
// No LDS, no barrier: a wave never waits for another.  Every sum is a fixed tree (lr_wave_sum over
// the lanes, a lane's bins in order; the estimators: a thread's samples in order, the lanes, the four waves in order), no
// floating-point atomics: a chain's bits depend on its own arguments alone.
#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_mlik.h"
#include "lr_dd.h"
#include "lr_internal.h"
#include "lr_par_iter.h"          // the chain and its iteration: shared with lr_parbin.hip

#define LR_MLIK_THREADS 256
#define LR_MLIK_WAVES (LR_MLIK_THREADS / LR_WAVE)
#define LR_MLIK_BPL (LR_MLIK_MAX_BINS / LR_WAVE) /* bins per lane */
#define LR_MLIK_S_LIK 8
#define LR_MLIK_S_PRIOR 9
#define LR_MLIK_S_PROPOSED 10
#define LR_MLIK_S_ACCEPTED 12
#define LR_MLIK_S_BETA 14
#define LR_MLIK_S_SCALE 15
#define LR_MLIK_R_LIK 2

static_assert(LR_MLIK_BPL == 8, "a lane holds at most 8 bins");
static_assert(LR_MLIK_S_SCALE + 1 == LR_MLIK_STATE_W && 4 + LR_DD_NPAR == LR_MLIK_ROW_W, "state and row layout");

struct lr_mlik_cfg {
    double origin, present, init_death, mult_l;
    int n_bins, m_birth, m_death, T, n_chains, chain0, s_freq;
    uint32_t seed;
};
struct lr_mlik_temps {
    double beta[LR_MLIK_MAX_TEMPS], scale[LR_MLIK_MAX_TEMPS];
};

__global__ __launch_bounds__(LR_MLIK_THREADS) void lr_mlik_chain_kernel(const double* __restrict__ n_spec,
                                                                         const double* __restrict__ n_exti,
                                                                         const double* __restrict__ DT, lr_mlik_cfg cfg,
                                                                         lr_mlik_temps tp, int mode, double* __restrict__ state,
                                                                         long long it0, long long n_iters,
                                                                         double* __restrict__ rows) {
    const int lane = threadIdx.x & (LR_WAVE - 1), wave = threadIdx.x / LR_WAVE;
    const int c = blockIdx.x * LR_MLIK_WAVES + wave;
    if (c >= cfg.n_chains) return;          // the whole wave: no barrier anywhere below
    const int j = c % cfg.T;
    const double beta = tp.beta[j], scale = tp.scale[j];
    const lr_stream rng{cfg.seed, (uint32_t)(cfg.chain0 + c)};
    lr_par_bins<LR_MLIK_BPL, false> B;
    const double dt_max = lr_par_load_bins<LR_MLIK_BPL, false>(B, n_spec, n_exti, DT, nullptr, cfg.n_bins, lane);
    lr_ddi_run run;
    run.origin = cfg.origin, run.present = cfg.present, run.beta = beta;
    run.n_bins = cfg.n_bins, run.m_birth = cfg.m_birth, run.m_death = cfg.m_death;
    lr_ddi_run_of(run, dt_max, scale, cfg.mult_l, lane);
    double* st = state + (size_t)c * LR_MLIK_STATE_W;
    lr_par_chain S;
    if (mode == 0) {
        lr_ddi_start<LR_MLIK_BPL>(S, B, run, cfg.init_death, lane);
    } else {
        S.A = lane < LR_DD_NPAR ? st[lane] : 0.0;
        S.likA = st[LR_MLIK_S_LIK], S.priorA = st[LR_MLIK_S_PRIOR];
        S.prop0 = st[LR_MLIK_S_PROPOSED], S.prop1 = st[LR_MLIK_S_PROPOSED + 1];
        S.acc0 = st[LR_MLIK_S_ACCEPTED], S.acc1 = st[LR_MLIK_S_ACCEPTED + 1];
        const long long s = cfg.s_freq;
        long long slot = 0;
        for (long long it = it0; it < it0 + n_iters; ++it) {
            lr_ddi_iterate<LR_MLIK_BPL>(S, B, run, rng, it, lane);          // lr_par_iter.h: shared with lr_parbin.hip
            if (it % s == 0) {
                double* row = rows + ((size_t)slot * cfg.n_chains + c) * LR_MLIK_ROW_W;
                slot += 1;
                const double Aj = __shfl(S.A, (lane - 4) & (LR_WAVE - 1));        // rare path (sampling only)
                double h = Aj;
                if (lane == 0) h = (double)it;
                if (lane == 1) h = beta;
                if (lane == 2) h = S.likA;
                if (lane == 3) h = S.priorA;
                if (lane < LR_MLIK_ROW_W) row[lane] = h;
            }
        }
    }
    const double A = S.A, likA = S.likA, priorA = S.priorA, prop0 = S.prop0, prop1 = S.prop1, acc0 = S.acc0, acc1 = S.acc1;
    double so = A;
    if (lane == LR_MLIK_S_LIK) so = likA;
    if (lane == LR_MLIK_S_PRIOR) so = priorA;
    if (lane == LR_MLIK_S_PROPOSED) so = prop0;
    if (lane == LR_MLIK_S_PROPOSED + 1) so = prop1;
    if (lane == LR_MLIK_S_ACCEPTED) so = acc0;
    if (lane == LR_MLIK_S_ACCEPTED + 1) so = acc1;
    if (lane == LR_MLIK_S_BETA) so = beta;
    if (lane == LR_MLIK_S_SCALE) so = scale;
    if (lane < LR_MLIK_STATE_W) st[lane] = so;
}

// ---- the estimators ---------------------------------------------------------------------------------------------------
// sum / maximum over the workgroup in a fixed order; every thread gets the result.  red: LR_MLIK_WAVES doubles of LDS
__device__ __forceinline__ double lr_mlik_block_sum(double v, double* red, int wave, int lane) {
    const double s = lr_wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double lr_mlik_block_max(double v, double* red, int wave, int lane) {
    const double s = -lr_wave_min(-v);
    __syncthreads();
    if (lane == 0) red[wave] = s;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
static_assert(LR_MLIK_WAVES == 4, "the block reductions add four waves");

// log mean exp(d x) of the n values x(i), i < n, shifted by their maximum; -inf where every x is -inf
template <class F>
__device__ __forceinline__ double lr_mlik_stone(F x, long long n, double d, double* red, int wave, int lane) {
    double m = -INFINITY;
    for (long long i = threadIdx.x; i < n; i += LR_MLIK_THREADS) m = fmax(m, x(i));
    m = lr_mlik_block_max(m, red, wave, lane);
    if (m == -INFINITY) return -INFINITY;          // (uniform over the block)
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += LR_MLIK_THREADS) {
        const double v = x(i);
        acc += v == -INFINITY ? 0.0 : exp(d * (v - m));
    }
    const double tot = lr_mlik_block_sum(acc, red, wave, lane);
    return d * m + lr_log(tot / (double)n);
}

__global__ __launch_bounds__(LR_MLIK_THREADS) void lr_mlik_stats_kernel(const double* __restrict__ rows, long long n_rows,
                                                                         int R, int T, long long row0, lr_mlik_temps tp,
                                                                         double* __restrict__ stone,
                                                                         double* __restrict__ lik_mean,
                                                                         double* __restrict__ lik_var,
                                                                         double* __restrict__ pooled) {
    __shared__ double red[LR_MLIK_WAVES];
    const int lane = threadIdx.x & (LR_WAVE - 1), wave = threadIdx.x / LR_WAVE;
    const long long n = n_rows - row0;
    const size_t chains = (size_t)R * T;
    if ((int)blockIdx.x < R * T) {
        const int r = blockIdx.x / T, j = blockIdx.x % T;
        const double* col = rows + ((size_t)row0 * chains + blockIdx.x) * LR_MLIK_ROW_W + LR_MLIK_R_LIK;
        auto x = [&](long long i) { return col[(size_t)i * chains * LR_MLIK_ROW_W]; };
        double acc = 0.0;
        for (long long i = threadIdx.x; i < n; i += LR_MLIK_THREADS) acc += x(i);
        const double mean = lr_mlik_block_sum(acc, red, wave, lane) / (double)n;
        acc = 0.0;
        for (long long i = threadIdx.x; i < n; i += LR_MLIK_THREADS) {
            const double dv = x(i) - mean;
            acc += dv * dv;
        }
        const double var = lr_mlik_block_sum(acc, red, wave, lane) / (double)(n - 1);
        if (threadIdx.x == 0) lik_mean[blockIdx.x] = mean, lik_var[blockIdx.x] = var;
        if (j < T - 1) {
            const double s = lr_mlik_stone(x, n, tp.beta[j + 1] - tp.beta[j], red, wave, lane);
            if (threadIdx.x == 0) stone[(size_t)r * (T - 1) + j] = s;
        }
    } else {
        // all replicates' samples of temperature j as one sample: item q = (row q / R, replicate q % R)
        const int j = blockIdx.x - R * T;
        const double* col = rows + ((size_t)row0 * chains + j) * LR_MLIK_ROW_W + LR_MLIK_R_LIK;
        auto x = [&](long long q) { return col[(size_t)q * T * LR_MLIK_ROW_W]; };
        const double s = lr_mlik_stone(x, n * R, tp.beta[j + 1] - tp.beta[j], red, wave, lane);
        if (threadIdx.x == 0) pooled[j] = s;
    }
}

__global__ __launch_bounds__(LR_MLIK_THREADS) void lr_mlik_sums_kernel(int R, int T, lr_mlik_temps tp,
                                                                        const double* __restrict__ stone,
                                                                        const double* __restrict__ lik_mean,
                                                                        double* __restrict__ ss, double* __restrict__ ti,
                                                                        double* __restrict__ pooled) {
    const int r = blockIdx.x * LR_MLIK_THREADS + threadIdx.x;
    if (r < R) {
        double s = 0.0, t = 0.0;
        for (int j = 0; j < T - 1; ++j) {
            s += stone[(size_t)r * (T - 1) + j];
            t += (tp.beta[j + 1] - tp.beta[j]) * ((lik_mean[(size_t)r * T + j] + lik_mean[(size_t)r * T + j + 1]) / 2.0);
        }
        ss[r] = s, ti[r] = t;
    }
    if (r == 0) {
        double s = 0.0;
        for (int j = 0; j < T - 1; ++j) s += pooled[j];
        pooled[T - 1] = s;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------
static int lr_mlik_temps_args(const double* betas, const double* scales, int T, lr_mlik_temps* tp) {
    if (betas[0] != 0.0 || betas[T - 1] != 1.0) return LR_ERR_MODEL;
    for (int j = 0; j + 1 < T; ++j)
        if (!(betas[j + 1] > betas[j])) return LR_ERR_MODEL;
    for (int j = 0; j < T; ++j) {
        if (scales && !(std::isfinite(scales[j]) && scales[j] > 0.0)) return LR_ERR_MODEL;
        tp->beta[j] = betas[j], tp->scale[j] = scales ? scales[j] : 1.0;
    }
    return LR_OK;
}

static int lr_mlik_chain_args(const double* n_spec, const double* n_exti, const double* DT, int32_t n_bins, double origin,
                              double present, int32_t m_birth, int32_t m_death, double init_death, const double* betas,
                              const double* scales, int32_t T, uint64_t seed, int32_t rep0, int32_t n_reps,
                              const double* state, int64_t it0, int64_t n_iters, int32_t s_freq, const double* rows,
                              int64_t n_rows, bool steps, lr_mlik_cfg* cfg, lr_mlik_temps* tp) {
    // (rows may be NULL where no row is due)
    int64_t need;
    const bool counts_ok = lr_rows_due(it0, n_iters, s_freq, &need);
    if (!n_spec || !n_exti || !DT || !betas || !scales || !state || (steps && !rows && !(counts_ok && need == 0)))
        return LR_ERR_NULL;
    if (n_bins < 1 || n_bins > LR_MLIK_MAX_BINS || T < 2 || T > LR_MLIK_MAX_TEMPS || n_reps < 1 || rep0 < 0) return LR_ERR_SIZE;
    if (((int64_t)rep0 + n_reps) * T > INT32_MAX) return LR_ERR_SIZE;
    if (m_birth < 0 || m_birth > 2 || m_death < -2 || m_death > 2) return LR_ERR_MODEL;
    if (!std::isfinite(origin) || !std::isfinite(present) || !std::isfinite(init_death)) return LR_ERR_MODEL;
    const int rc = lr_mlik_temps_args(betas, scales, T, tp);
    if (rc != LR_OK) return rc;
    if (steps && (!counts_ok || n_rows < need)) return LR_ERR_SIZE;
    cfg->origin = origin, cfg->present = present, cfg->init_death = init_death, cfg->mult_l = 2.0 * std::log(LR_MULT_D);
    cfg->n_bins = n_bins, cfg->m_birth = m_birth, cfg->m_death = m_death, cfg->T = T, cfg->n_chains = n_reps * T;
    cfg->chain0 = rep0 * T, cfg->s_freq = steps ? s_freq : 1, cfg->seed = (uint32_t)seed;
    return LR_OK;
}

static unsigned lr_mlik_blocks(const lr_mlik_cfg& cfg) { return (unsigned)((cfg.n_chains + LR_MLIK_WAVES - 1) / LR_MLIK_WAVES); }

extern "C" int lr_mlik_init(const double* n_spec, const double* n_exti, const double* DT, int32_t n_bins, double origin,
                            double present, int32_t m_birth, int32_t m_death, double init_death, const double* betas,
                            const double* scales, int32_t T, uint64_t seed, int32_t rep0, int32_t n_reps, double* state,
                            void* stream_) {
    lr_mlik_cfg cfg;
    lr_mlik_temps tp;
    const int rc = lr_mlik_chain_args(n_spec, n_exti, DT, n_bins, origin, present, m_birth, m_death, init_death, betas, scales, T,
                                      seed, rep0, n_reps, state, 0, 0, 1, nullptr, 0, false, &cfg, &tp);
    if (rc != LR_OK) return rc;
    hipLaunchKernelGGL(lr_mlik_chain_kernel, dim3(lr_mlik_blocks(cfg)), dim3(LR_MLIK_THREADS), 0, (hipStream_t)stream_, n_spec,
                       n_exti, DT, cfg, tp, 0, state, 0ll, 0ll, (double*)nullptr);
    return (int)hipGetLastError();
}

extern "C" int lr_mlik_steps(const double* n_spec, const double* n_exti, const double* DT, int32_t n_bins, double origin,
                             double present, int32_t m_birth, int32_t m_death, double init_death, const double* betas,
                             const double* scales, int32_t T, uint64_t seed, int32_t rep0, int32_t n_reps, double* state,
                             int64_t it0, int64_t n_iters, int32_t s_freq, double* rows, int64_t n_rows, void* stream_) {
    lr_mlik_cfg cfg;
    lr_mlik_temps tp;
    const int rc = lr_mlik_chain_args(n_spec, n_exti, DT, n_bins, origin, present, m_birth, m_death, init_death, betas, scales, T,
                                      seed, rep0, n_reps, state, it0, n_iters, s_freq, rows, n_rows, true, &cfg, &tp);
    if (rc != LR_OK) return rc;
    if (n_iters == 0) return LR_OK;
    hipLaunchKernelGGL(lr_mlik_chain_kernel, dim3(lr_mlik_blocks(cfg)), dim3(LR_MLIK_THREADS), 0, (hipStream_t)stream_, n_spec,
                       n_exti, DT, cfg, tp, 1, state, (long long)it0, (long long)n_iters, rows);
    return (int)hipGetLastError();
}

extern "C" int lr_mlik_estimate(const double* rows, int64_t n_rows, int32_t n_reps, int32_t T, int64_t row0, const double* betas,
                                double* stone, double* ss, double* lik_mean, double* lik_var, double* ti, double* pooled,
                                void* stream_) {
    if (!rows || !betas || !stone || !ss || !lik_mean || !lik_var || !ti || !pooled) return LR_ERR_NULL;
    if (n_rows < 1 || n_reps < 1 || T < 2 || T > LR_MLIK_MAX_TEMPS || row0 < 0 || row0 >= n_rows) return LR_ERR_SIZE;
    if ((int64_t)n_reps * T + T > INT32_MAX) return LR_ERR_SIZE;
    lr_mlik_temps tp;
    const int rc = lr_mlik_temps_args(betas, nullptr, T, &tp);
    if (rc != LR_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(lr_mlik_stats_kernel, dim3((unsigned)(n_reps * T + T - 1)), dim3(LR_MLIK_THREADS), 0, stream, rows,
                       (long long)n_rows, (int)n_reps, (int)T, (long long)row0, tp, stone, lik_mean, lik_var, pooled);
    int err = (int)hipGetLastError();
    if (err) return err;
    hipLaunchKernelGGL(lr_mlik_sums_kernel, dim3((unsigned)((n_reps + LR_MLIK_THREADS - 1) / LR_MLIK_THREADS)),
                       dim3(LR_MLIK_THREADS), 0, stream, (int)n_reps, (int)T, tp, stone, lik_mean, ss, ti, pooled);
    return (int)hipGetLastError();
}
