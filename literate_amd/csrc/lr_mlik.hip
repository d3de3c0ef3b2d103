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
// the DD engine evaluates.  No LDS, no barrier: a wave never waits for another.  Every sum is a fixed tree (lr_wave_sum over
// the lanes, a lane's bins in order; the estimators: a thread's samples in order, the lanes, the four waves in order), no
// floating-point atomics: a chain's bits depend on its own arguments alone.
#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_mlik.h"
#include "lr_dd.h"
#include "lr_internal.h"

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

// a lane's bins: b = lane + 64 i, i < nb
struct lr_mlik_bins {
    double ns[LR_MLIK_BPL], ne[LR_MLIK_BPL], dt[LR_MLIK_BPL];
    int nb;
};

// likelihood_function's sum (DD:101-107) under the parameters in lanes 0-7 of P; NaN -> -inf
__device__ __forceinline__ double lr_mlik_loglik(double P, const lr_mlik_bins& B, const lr_mlik_cfg& cfg, int lane) {
    const lr_dd_params p = lr_dd_unpack(P);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < LR_MLIK_BPL; ++i) {
        const int b = lane + LR_WAVE * i;
        if (i < B.nb && b < cfg.n_bins) {
            double br, dr, niche, frac;
            lr_dd_bin_rates(p, (double)b, B.dt[i], cfg.m_birth, cfg.m_death, &br, &dr, &niche, &frac);
            acc += (lr_log(br) * B.ns[i] - br * B.dt[i]) + (lr_log(dr) * B.ne[i] - dr * B.dt[i]);
        }
    }
    const double s = lr_wave_sum(acc);
    return s != s ? -INFINITY : s;
}

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
    lr_mlik_bins B;
    B.nb = (cfg.n_bins + LR_WAVE - 1) / LR_WAVE;
    double dt_max = -INFINITY;
#pragma unroll
    for (int i = 0; i < LR_MLIK_BPL; ++i) {
        const int b = lane + LR_WAVE * i;
        const bool in = i < B.nb && b < cfg.n_bins;
        B.ns[i] = in ? n_spec[b] : 0.0, B.ne[i] = in ? n_exti[b] : 0.0, B.dt[i] = in ? DT[b] : 1.0;
        if (in) dt_max = fmax(dt_max, B.dt[i]);
    }
    const double k0 = -lr_wave_min(-dt_max), log_k0 = lr_log(k0);        // PRIOR_K0_L = np.max(DT) (DD:45)
    double* st = state + (size_t)c * LR_MLIK_STATE_W;
    double A, likA, priorA, prop0, prop1, acc0, acc1;          // proposals made / accepted per move kind
    if (mode == 0) {
        const double x0 = cfg.present - (cfg.origin + cfg.present) / 2.0;       // PRESENT - np.mean([ORIGIN, PRESENT])
        const double init[LR_DD_NPAR] = {0.5, 1.5, x0, 10.0, 20000.0, cfg.init_death, 1.0, 1.0};
        A = 0.0;
#pragma unroll
        for (int i = 0; i < LR_DD_NPAR; ++i) A = (lane == i) ? init[i] : A;
        likA = lr_mlik_loglik(A, B, cfg, lane);
        priorA = lr_dd_prior(A, cfg.origin, cfg.present, k0, log_k0, lane);
        prop0 = prop1 = acc0 = acc1 = 0.0;
    } else {
        A = lane < LR_DD_NPAR ? st[lane] : 0.0;
        likA = st[LR_MLIK_S_LIK], priorA = st[LR_MLIK_S_PRIOR];
        prop0 = st[LR_MLIK_S_PROPOSED], prop1 = st[LR_MLIK_S_PROPOSED + 1];
        acc0 = st[LR_MLIK_S_ACCEPTED], acc1 = st[LR_MLIK_S_ACCEPTED + 1];
        const bool niche = cfg.m_birth == 2 || cfg.m_death == 2;
        const double f = lr_dd_update_freq(cfg.m_birth, cfg.m_death, lane);
        const double mult_l = scale * cfg.mult_l, slide_d = 1.5 * scale, norm_d = 0.2 * scale;
        const long long s = cfg.s_freq;
        long long slot = 0;
        for (long long it = it0; it < it0 + n_iters; ++it) {
            // the wave-uniform draws in one Philox call: lane 0 the acceptance uniform, lane 1 the move selector, lane 2 the
            // sliding-window uniform (as lr_propose_dd takes them)
            const uint32_t purpose = lane == 0 ? LR_P_DD_ACCEPT : (lane == 1 ? LR_P_DD_MOVE : LR_P_DD_SLIDE);
            const lr_u2 ud = lr_pair(rng, (uint64_t)it, purpose, 0u);
            const double log_u = lr_bcast(lr_log(lane == 0 ? ud.a : 1.0), 0);
            double P = A, hasting = 0.0;
            int move;
            if (lr_bcast(ud.b, 1) < 0.1 && niche) {
                // update_sliding_win(x0, m = 0, M = PRESENT, d = 1.5 s) (lib:124-128)
                double ii = lr_bcast(A, 2) + (lr_bcast(ud.a, 2) - .5) * slide_d;
                if (ii > cfg.present) ii = cfg.present - (ii - cfg.present);
                ii = fabs(ii);
                if (lane == 2) P = ii;
                if (cfg.m_death == -1) {
                    const double z = lr_normal(rng, (uint64_t)it, LR_P_DD_SLIDE, 1);   // update_normal_nobound(k, d = 0.2 s) (lib:136-138)
                    if (lane == 1) P = A + z * norm_d;
                }
                move = 1;
            } else {
                const lr_u2 d = lr_pair(rng, (uint64_t)it, LR_P_DD_MULT, lane);
                hasting = lr_wave_multiplier(P, LR_DD_NPAR, d.a < f, d.b, mult_l, lane);   // lib:156-165
                move = 0;
            }
            const double prior = lr_dd_prior(P, cfg.origin, cfg.present, k0, log_k0, lane);
            const double lik = lr_mlik_loglik(P, B, cfg, lane);
            const double dl = beta == 0.0 ? 0.0 : beta * (lik - likA);
            const bool ok = (dl + (prior - priorA) + hasting > log_u) || it == 0;      // DD:211
            prop0 += move ? 0.0 : 1.0, prop1 += move ? 1.0 : 0.0;
            if (ok) A = P, likA = lik, priorA = prior, acc0 += move ? 0.0 : 1.0, acc1 += move ? 1.0 : 0.0;
            if (it % s == 0) {
                double* row = rows + ((size_t)slot * cfg.n_chains + c) * LR_MLIK_ROW_W;
                slot += 1;
                const double Aj = __shfl(A, (lane - 4) & (LR_WAVE - 1));        // rare path (sampling only)
                double h = Aj;
                if (lane == 0) h = (double)it;
                if (lane == 1) h = beta;
                if (lane == 2) h = likA;
                if (lane == 3) h = priorA;
                if (lane < LR_MLIK_ROW_W) row[lane] = h;
            }
        }
    }
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
