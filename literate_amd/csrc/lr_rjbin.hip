// lr_rjbin.hip - the RJ sampler on per-chain binned statistics (include/literate_hip_rjbin.h): runMCMC (LRF:216-373) for
// chains that do not share their data - replicate data sets, one stochastic imputation each - all of them in one launch.
//
//   lr_rjbin_chain_kernel<BPL>   one wave per chain, four independent waves per workgroup: its initial state, or n_iters
//                                iterations from its state
//
// The likelihood of runMCMC is a function of the per-bin statistics alone, so an iteration costs O(n_bins) whatever the
// number of lineages: bin b sits in lane b % 64, BPL = 1, 2, 4 or 8 bins to a lane, and the replicate's statistics and log
// br stay in REGISTERS for the whole launch (5 arrays of BPL doubles: 80 VGPRs at 512 bins, where one wave per SIMD may
// hold 512 - the allocator spills nothing).  Lane j holds rate j and shift time j; the moves, priors and
// Gibbs draws are the lane-per-element functions of lr_chain.h, the draws the engines' (lr_step.h's addresses).  A
// proposal's likelihood takes the logarithms of its K segment rates in one call and no transcendental per bin: the
// segment of a bin is found by broadcasting the K edges with v_readlane.  No LDS, no barrier: a wave never waits for
// another.  Every sum is a fixed tree (a lane's bins in order, then lr_wave_sum), no floating-point atomics: a chain's bits
// depend on its own arguments alone.
#include <hip/hip_runtime.h>

#include "../../include/literate_hip_rjbin.h"
#include "lr_chain.h"
#include "lr_internal.h"
#include "lr_rjbin_iter.h"          // the chain, its iteration and the argument checks: shared with lr_rjmc3.hip

#define LR_RJBIN_THREADS 256
#define LR_RJBIN_WAVES (LR_RJBIN_THREADS / LR_WAVE)

template <int BPL>
__global__ __launch_bounds__(LR_RJBIN_THREADS) void lr_rjbin_chain_kernel(
    const double* __restrict__ sp, const double* __restrict__ ex, const double* __restrict__ br,
    const double* __restrict__ ex_dead, const double* __restrict__ br_dead, const double* __restrict__ start_time,
    const double* __restrict__ end_time, lr_rjbin_cfg cfg, int mode, double* __restrict__ state, unsigned int* __restrict__ warn,
    const double* __restrict__ L0, const double* __restrict__ M0, const double* __restrict__ tL0, const double* __restrict__ tM0,
    const int* __restrict__ KL0, const int* __restrict__ KM0, long long it0, long long n_iters, double* __restrict__ rows) {
    const int lane = threadIdx.x & (LR_WAVE - 1), wave = threadIdx.x / LR_WAVE;
    const int c = blockIdx.x * LR_RJBIN_WAVES + wave;
    if (c >= cfg.n_chains) return;          // the whole wave: no barrier anywhere below
    const int rep = c / cfg.chains_per_rep;
    const lr_stream rng{cfg.seed, (uint32_t)(cfg.chain0 + c)};
    const lr_rjbin_run run = lr_rjbin_run_of(cfg, start_time[rep], end_time[rep]);
    lr_rjbin_bins<BPL> B;
    lr_rjbin_load_bins<BPL>(B, sp, ex, br, ex_dead, br_dead, rep, cfg.model, cfg.n_bins, lane);
    double* st = state + (size_t)c * LR_RJBIN_STATE_W;
    lr_rjbin_chain S;
    if (mode == 0) {
        lr_rjbin_start<BPL>(S, B, cfg, run, rng, (size_t)c, L0, M0, tL0, tM0, KL0, KM0, lane);
    } else {
        lr_rjbin_load(S, st, lane);
        // iterations to go until the next one with it % s_freq == 0: one 64-bit modulo per launch, not one per iteration
        long long until_row = (cfg.s_freq - it0 % cfg.s_freq) % cfg.s_freq;
        long long slot = cfg.slot0;
        for (long long it = it0; it < it0 + n_iters; ++it) {
            lr_rjbin_iterate<BPL, false>(S, B, cfg, run, rng, it, 1.0, warn, lane);
            const bool sample = until_row == 0;
            until_row = sample ? cfg.s_freq - 1 : until_row - 1;
            if (sample) {
                lr_rjbin_trace_row(S, run, it, rows + ((size_t)slot * cfg.n_chains + c) * LR_TRACE_W, lane);
                slot += 1;
            }
        }
    }
    lr_rjbin_store(S, st, lane);
}

// ---- host -------------------------------------------------------------------------------------------------------------
template <int BPL>
static void lr_rjbin_launch_bpl(const lr_rjbin_problem* p, const lr_rjbin_cfg& cfg, int mode, const void* const* i6, int64_t it0,
                                int64_t n_iters, double* rows) {
    const unsigned blocks = (unsigned)((cfg.n_chains + LR_RJBIN_WAVES - 1) / LR_RJBIN_WAVES);
    hipLaunchKernelGGL(lr_rjbin_chain_kernel<BPL>, dim3(blocks), dim3(LR_RJBIN_THREADS), 0, (hipStream_t)p->stream, p->sp, p->ex,
                       p->br, p->ex_dead, p->br_dead, p->start_time, p->end_time, cfg, mode, p->state, (unsigned int*)p->warn,
                       (const double*)i6[0], (const double*)i6[1], (const double*)i6[2], (const double*)i6[3], (const int*)i6[4],
                       (const int*)i6[5], (long long)it0, (long long)n_iters, rows);
}

static int lr_rjbin_launch(const lr_rjbin_problem* p, const lr_rjbin_cfg& cfg, int mode, const void* const* i6, int64_t it0,
                           int64_t n_iters, double* rows) {
    const int bpl = (cfg.n_bins + LR_WAVE - 1) / LR_WAVE;
    if (bpl <= 1) lr_rjbin_launch_bpl<1>(p, cfg, mode, i6, it0, n_iters, rows);
    else if (bpl <= 2) lr_rjbin_launch_bpl<2>(p, cfg, mode, i6, it0, n_iters, rows);
    else if (bpl <= 4) lr_rjbin_launch_bpl<4>(p, cfg, mode, i6, it0, n_iters, rows);
    else lr_rjbin_launch_bpl<8>(p, cfg, mode, i6, it0, n_iters, rows);
    return (int)hipGetLastError();
}

extern "C" int lr_rjbin_init(const lr_rjbin_problem* p, const double* L, const double* M, const double* tL, const double* tM,
                             const int32_t* K_l, const int32_t* K_m) {
    const void* i6[6] = {L, M, tL, tM, K_l, K_m};
    lr_rjbin_cfg cfg;
    const int rc = lr_rjbin_args(p, false, i6, 0, 0, 1, nullptr, 0, 0, &cfg);
    if (rc != LR_OK) return rc;
    return lr_rjbin_launch(p, cfg, 0, i6, 0, 0, nullptr);
}

extern "C" int lr_rjbin_steps(const lr_rjbin_problem* p, int64_t it0, int64_t n_iters, int32_t s_freq, double* rows,
                              int64_t rows_cap, int64_t slot0) {
    const void* i6[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    lr_rjbin_cfg cfg;
    const int rc = lr_rjbin_args(p, true, nullptr, it0, n_iters, s_freq, rows, rows_cap, slot0, &cfg);
    if (rc != LR_OK) return rc;
    if (n_iters == 0) return LR_OK;
    return lr_rjbin_launch(p, cfg, 1, i6, it0, n_iters, rows);
}
