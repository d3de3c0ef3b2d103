// lr_rjmc3.hip - the Metropolis-coupled RJ sampler (include/literate_hip_rjmc3.h): lr_rjbin's chains with a ladder of heated
// replicas beside every cold one.
//
//   lr_rjmc3_ladder_kernel<BPL, NW>   one workgroup per ladder, one wave per replica (T <= NW waves are launched): the initial
//                                     states, or n_iters iterations and the swap rounds that fall among them
//
// The iteration is lr_rjbin's (lr_rjbin_iter.h) with the likelihood difference of its acceptance test times beta.  A replica
// keeps its state, its key and its registers; what a swap exchanges is the position on the ladder, one integer.  In a swap
// iteration every wave publishes (likA, position) in LDS, the workgroup meets at ONE barrier, and every wave evaluates the
// whole round from the published values - the same arithmetic on the same numbers, so all agree without a second exchange.
// The published pairs are double-buffered on the parity of the round: a wave writes buffer n % 2 again in round n + 2, which
// it reaches only through the barrier of round n + 1, behind which every wave has read round n.  Every wave of a block runs
// the same iterations, so the barrier is uniform; between rounds no wave waits for another.  The swap counts are kept in
// registers of wave 0 and added to the buffer once, at the end of the launch: no atomics.
#include <hip/hip_runtime.h>

#include "../../include/literate_hip_rjmc3.h"
#include "lr_chain.h"
#include "lr_internal.h"
#include "lr_rjbin_iter.h"

static_assert(LR_RJMC3_S_POS > LR_RJBIN_S_ACCEPTED && LR_RJMC3_S_POS < LR_ROW, "the position sits behind lr_rjbin's scalars");
static_assert(LR_RJMC3_MAX_TEMPS == 8, "one wave per temperature, at most 8 waves to a workgroup");

struct lr_rjmc3_cfg {
    lr_rjbin_cfg c;          // n_chains = G, the ladders: the rows' stride
    double betas[LR_RJMC3_MAX_TEMPS];
    int T, swap_every;
};

// betas[j] for a j the compiler does not know: a chain of selects, no indexed access to the kernel arguments
__device__ __forceinline__ double lr_rjmc3_beta(const lr_rjmc3_cfg& cfg, int j) {
    double b = cfg.betas[0];
#pragma unroll
    for (int i = 1; i < LR_RJMC3_MAX_TEMPS; ++i) b = (j == i) ? cfg.betas[i] : b;
    return b;
}

template <int BPL, int NW>
__global__ __launch_bounds__(NW* LR_WAVE) void lr_rjmc3_ladder_kernel(
    const double* __restrict__ sp, const double* __restrict__ ex, const double* __restrict__ br,
    const double* __restrict__ ex_dead, const double* __restrict__ br_dead, const double* __restrict__ start_time,
    const double* __restrict__ end_time, lr_rjmc3_cfg cfg, int mode, long long it0, long long n_iters, double* __restrict__ state,
    unsigned int* __restrict__ warn, double* __restrict__ rows, double* __restrict__ ladder, long long* __restrict__ swaps,
    const double* __restrict__ L0, const double* __restrict__ M0, const double* __restrict__ tL0, const double* __restrict__ tM0,
    const int* __restrict__ KL0, const int* __restrict__ KM0) {
    __shared__ double s_lik[2][LR_RJMC3_MAX_TEMPS];
    __shared__ int s_pos[2][LR_RJMC3_MAX_TEMPS];
    // (blockDim.x = T waves: every wave is a replica and none returns before the last barrier)
    const int lane = threadIdx.x & (LR_WAVE - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LR_WAVE);
    const int T = cfg.T, g = blockIdx.x, G = cfg.c.n_chains;
    const size_t c = (size_t)g * T + wave;
    const int rep = g / cfg.c.chains_per_rep;
    const lr_stream rng{cfg.c.seed, (uint32_t)(cfg.c.chain0 + (long long)c)};
    const lr_stream rng0{cfg.c.seed, (uint32_t)(cfg.c.chain0 + (long long)g * T)};          // the swap uniforms: replica 0's stream
    const lr_rjbin_run run = lr_rjbin_run_of(cfg.c, start_time[rep], end_time[rep]);
    lr_rjbin_bins<BPL> B;
    lr_rjbin_load_bins<BPL>(B, sp, ex, br, ex_dead, br_dead, rep, cfg.c.model, cfg.c.n_bins, lane);
    double* st = state + c * LR_RJBIN_STATE_W;
    lr_rjbin_chain S;
    int pos = wave;
    long long n_prop = 0, n_acc = 0;          // wave 0, lane j: the pair of positions (j, j + 1) in this launch
    if (mode == 0) {
        lr_rjbin_start<BPL>(S, B, cfg.c, run, rng, c, L0, M0, tL0, tM0, KL0, KM0, lane);
        if (wave == 0 && lane < 2 * (T - 1)) swaps[(size_t)g * (T - 1) * 2 + lane] = 0;
    } else {
        lr_rjbin_load(S, st, lane);
        // (a state that is not the sampler's own: the position stays inside the ladder, so that every store stays in bounds)
        pos = min(max(__builtin_amdgcn_readfirstlane((int)st[LR_RJBIN_ROW_SCALARS * LR_ROW + LR_RJMC3_S_POS]), 0), T - 1);
        // lane j < T: betas[j], for the whole launch in one register: the kernel arguments are read once, not in the loop
        const double beta_lane = lr_rjmc3_beta(cfg, lane);
        double beta = lr_bcast(beta_lane, pos);
        const int se = cfg.swap_every;
        long long until_row = (cfg.c.s_freq - it0 % cfg.c.s_freq) % cfg.c.s_freq;
        long long slot = cfg.c.slot0;
        // iterations to go until the next one with (it + 1) % swap_every == 0, and the parity of that round's number
        long long until_swap = se > 0 ? (se - 1 - it0 % se) : -1;
        int par = se > 0 ? (int)(((it0 + until_swap + 1) / se) & 1) : 0;
        for (long long it = it0; it < it0 + n_iters; ++it) {
            lr_rjbin_iterate<BPL, true>(S, B, cfg.c, run, rng, it, beta, warn, lane);
            const bool sample = until_row == 0;
            until_row = sample ? cfg.c.s_freq - 1 : until_row - 1;
            if (sample) {
                if (pos == 0) lr_rjbin_trace_row(S, run, it, rows + ((size_t)slot * G + g) * LR_TRACE_W, lane);
                if (ladder && lane < LR_RJMC3_LADDER_W) {
                    const double v = lane == 0 ? (double)wave : (lane == 1 ? S.likA : (lane == 2 ? (double)S.KL : (double)S.KM));
                    ladder[(((size_t)slot * G + g) * T + pos) * LR_RJMC3_LADDER_W + lane] = v;
                }
                slot += 1;
            }
            if (se > 0) {
                const bool swap = until_swap == 0;
                until_swap = swap ? se - 1 : until_swap - 1;
                if (swap) {
                    if (lane == 0) s_lik[par][wave] = S.likA, s_pos[par][wave] = pos;
                    __syncthreads();
                    // lane r < T: replica r's likelihood and position; lane j < T - 1: log u of the pair (j, j + 1)
                    const double lik_r = lane < T ? s_lik[par][lane] : 0.0;
                    int pos_r = lane < T ? s_pos[par][lane] : -1;
                    const double log_u = lr_log(lr_pair(rng0, (uint64_t)it, LR_P_SWAP, (uint32_t)lane).a);
                    for (int j = par; j + 1 < T; j += 2) {
                        const unsigned long long ma = __ballot(pos_r == j), mb = __ballot(pos_r == j + 1);
                        if (ma == 0ull || mb == 0ull) continue;          // (not a permutation: a state that is not the sampler's own)
                        const int a = __builtin_ctzll(ma), b = __builtin_ctzll(mb);
                        const double d = (lr_bcast(beta_lane, j) - lr_bcast(beta_lane, j + 1)) * (lr_bcast(lik_r, b) - lr_bcast(lik_r, a));
                        const bool acc = d >= lr_bcast(log_u, j);
                        if (lane == j) n_prop += 1, n_acc += acc ? 1 : 0;
                        if (acc) pos_r = (lane == a) ? j + 1 : ((lane == b) ? j : pos_r);
                    }
                    pos = lr_bcast_i(pos_r, wave);
                    beta = lr_bcast(beta_lane, pos);
                    par ^= 1;
                }
            }
        }
        if (wave == 0 && lane < T - 1) {
            long long* sw = swaps + ((size_t)g * (T - 1) + lane) * 2;
            sw[0] += n_prop, sw[1] += n_acc;
        }
    }
    lr_rjbin_store(S, st, lane);
    if (lane == LR_RJMC3_S_POS) st[LR_RJBIN_ROW_SCALARS * LR_ROW + lane] = (double)pos;
}

// ---- host -------------------------------------------------------------------------------------------------------------
static int lr_rjmc3_args(const lr_rjmc3_problem* p, bool steps, const void* const* init6, int64_t it0, int64_t n_iters,
                         int32_t s_freq, const double* rows, int64_t rows_cap, int64_t slot0, lr_rjmc3_cfg* cfg) {
    if (!p) return LR_ERR_NULL;
    lr_rjbin_problem q;
    q.sp = p->sp, q.ex = p->ex, q.br = p->br, q.ex_dead = p->ex_dead, q.br_dead = p->br_dead;
    q.start_time = p->start_time, q.end_time = p->end_time, q.state = p->state, q.warn = p->warn;
    q.n_bins = p->n_bins, q.R = p->R, q.chains_per_rep = p->chains_per_rep, q.model = p->model, q.const_rates = p->const_rates;
    q.const_death_rate = p->const_death_rate, q.use_rate_HP = p->use_rate_HP, q.chain0 = p->chain0;
    q.poisson_HP = p->poisson_HP, q.update_fraction = p->update_fraction, q.seed = p->seed, q.stream = p->stream;
    const int rc = lr_rjbin_args(&q, steps, init6, it0, n_iters, s_freq, rows, rows_cap, slot0, &cfg->c);
    if (rc != LR_OK) return rc;
    if (p->T < 1 || p->T > LR_RJMC3_MAX_TEMPS) return LR_ERR_SIZE;
    if (!p->betas || (p->T > 1 && !p->swaps)) return LR_ERR_NULL;
    if (!(p->betas[0] == 1.0) || p->swap_every < 0) return LR_ERR_MODEL;
    for (int j = 1; j < p->T; ++j)
        if (!(p->betas[j] > 0.0 && p->betas[j] < p->betas[j - 1])) return LR_ERR_MODEL;
    if ((int64_t)cfg->c.n_chains * p->T > INT32_MAX) return LR_ERR_SIZE;
    if (p->n_bins > LR_RJMC3_WIDE_MAX_BINS && p->T > 4) return LR_ERR_SIZE;
    for (int j = 0; j < LR_RJMC3_MAX_TEMPS; ++j) cfg->betas[j] = j < p->T ? p->betas[j] : 0.0;
    cfg->T = p->T, cfg->swap_every = p->swap_every;
    return LR_OK;
}

template <int BPL, int NW>
static void lr_rjmc3_launch_as(const lr_rjmc3_problem* p, const lr_rjmc3_cfg& cfg, int mode, const void* const* i6, int64_t it0,
                               int64_t n_iters, double* rows, double* ladder) {
    hipLaunchKernelGGL((lr_rjmc3_ladder_kernel<BPL, NW>), dim3((unsigned)cfg.c.n_chains), dim3((unsigned)(cfg.T * LR_WAVE)), 0,
                       (hipStream_t)p->stream, p->sp, p->ex, p->br, p->ex_dead, p->br_dead, p->start_time, p->end_time, cfg, mode,
                       (long long)it0, (long long)n_iters, p->state, (unsigned int*)p->warn, rows, ladder, (long long*)p->swaps,
                       (const double*)i6[0], (const double*)i6[1], (const double*)i6[2], (const double*)i6[3], (const int*)i6[4],
                       (const int*)i6[5]);
}

// a workgroup of up to 4 waves leaves a wave 512 registers, one of 5 to 8 leaves 256: the kernel is compiled for both, and 8
// bins to a lane for the first only (lr_rjmc3_args refuses the shape)
static int lr_rjmc3_launch(const lr_rjmc3_problem* p, const lr_rjmc3_cfg& cfg, int mode, const void* const* i6, int64_t it0,
                           int64_t n_iters, double* rows, double* ladder) {
    const int bpl = (cfg.c.n_bins + LR_WAVE - 1) / LR_WAVE;
    if (cfg.T <= 4) {
        if (bpl <= 1) lr_rjmc3_launch_as<1, 4>(p, cfg, mode, i6, it0, n_iters, rows, ladder);
        else if (bpl <= 2) lr_rjmc3_launch_as<2, 4>(p, cfg, mode, i6, it0, n_iters, rows, ladder);
        else if (bpl <= 4) lr_rjmc3_launch_as<4, 4>(p, cfg, mode, i6, it0, n_iters, rows, ladder);
        else lr_rjmc3_launch_as<8, 4>(p, cfg, mode, i6, it0, n_iters, rows, ladder);
    } else {
        if (bpl <= 1) lr_rjmc3_launch_as<1, 8>(p, cfg, mode, i6, it0, n_iters, rows, ladder);
        else if (bpl <= 2) lr_rjmc3_launch_as<2, 8>(p, cfg, mode, i6, it0, n_iters, rows, ladder);
        else lr_rjmc3_launch_as<4, 8>(p, cfg, mode, i6, it0, n_iters, rows, ladder);
    }
    return (int)hipGetLastError();
}

extern "C" int lr_rjmc3_init(const lr_rjmc3_problem* p, const double* L, const double* M, const double* tL, const double* tM,
                             const int32_t* K_l, const int32_t* K_m) {
    const void* i6[6] = {L, M, tL, tM, K_l, K_m};
    lr_rjmc3_cfg cfg;
    const int rc = lr_rjmc3_args(p, false, i6, 0, 0, 1, nullptr, 0, 0, &cfg);
    if (rc != LR_OK) return rc;
    return lr_rjmc3_launch(p, cfg, 0, i6, 0, 0, nullptr, nullptr);
}

extern "C" int lr_rjmc3_steps(const lr_rjmc3_problem* p, int64_t it0, int64_t n_iters, int32_t s_freq, double* rows, double* ladder,
                              int64_t rows_cap, int64_t slot0) {
    const void* i6[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    lr_rjmc3_cfg cfg;
    const int rc = lr_rjmc3_args(p, true, nullptr, it0, n_iters, s_freq, rows, rows_cap, slot0, &cfg);
    if (rc != LR_OK) return rc;
    if (n_iters == 0) return LR_OK;
    return lr_rjmc3_launch(p, cfg, 1, i6, it0, n_iters, rows, ladder);
}
