// lr_mcmc.hip - proposal scorers with explicit draws (A7/A8/A10) and the fused multi-chain
// RJMCMC engine (A11: runMCMC, LiteRateForward.py:216-373).
//
// Engine iteration = [lr_scan_kernel over all lineages x all chains] -> [lr_chain_step_kernel:
// one wave per chain: reduce the tile partials in order, Metropolis-Hastings accept, write the
// trace row, draw the next proposal from the chain's Philox stream, build its lookup tables].
// Iterations are captured in a hipGraph so the host only replays it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <type_traits>

#include "lr_chain.h"
#include "lr_dd.h"
#include "lr_engine.h"
#include "lr_internal.h"
#include "lr_scan.h"
#include "lr_step.h"

// ------------------------------------------------------------------------------------------
// explicit-draw scorers (parity with reference-generated vectors)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LR_WAVE) void lr_rj_propose_score_kernel(
    const double* __restrict__ rates, const double* __restrict__ times, const int* __restrict__ K, int kmax,
    const int* __restrict__ move, const int* __restrict__ index, const double* __restrict__ draws, double mult_d,
    double* __restrict__ out_rates, double* __restrict__ out_times, int* __restrict__ out_K,
    double* __restrict__ out_score) {
    const int c = blockIdx.x, lane = threadIdx.x;
    int k = K[c];
    double R = (lane < k) ? rates[(size_t)c * kmax + lane] : 0.0;
    double T = (lane <= k) ? times[(size_t)c * (kmax + 1) + lane] : 0.0;
    const double* dr = draws + (size_t)c * 2 * kmax;
    const int mv = move[c];
    double score = 0.0;
    if (mv == 0) {
        const bool ff = (lane < k) ? (dr[lane] != 0.0) : false;
        const double u = (lane < k) ? dr[kmax + lane] : 0.5;
        score = lr_wave_multiplier(R, k, ff, u, 2.0 * lr_log(mult_d), lane);
    } else if (mv == 1) {
        score = lr_wave_add_shift(R, T, k, index[c], dr[0], dr[1], lane);
    } else if (mv == 2) {
        score = lr_wave_remove_shift(R, T, k, index[c], lane);
    }
    if (lane < kmax) out_rates[(size_t)c * kmax + lane] = (lane < k) ? R : 0.0;
    if (lane <= kmax) out_times[(size_t)c * (kmax + 1) + lane] = (lane <= k) ? T : 0.0;
    if (lane == 0) out_K[c] = k, out_score[c] = score;
}

extern "C" int lr_rj_propose_score(const double* rates, const double* times, const int32_t* K, int32_t kmax,
                                   int32_t n_chains, const int32_t* move, const int32_t* index, const double* draws,
                                   double mult_d, double* out_rates, double* out_times, int32_t* out_K,
                                   double* out_score, void* stream_) {
    if (!rates || !times || !K || !move || !index || !draws || !out_rates || !out_times || !out_K || !out_score)
        return LR_ERR_NULL;
    // an add needs room for K+1 rates: kmax must leave it (caller pads), and a wave holds 64 lanes
    if (kmax < 2 || kmax > LR_WAVE - 1 || n_chains < 1) return LR_ERR_SIZE;
    hipLaunchKernelGGL(lr_rj_propose_score_kernel, dim3(n_chains), dim3(LR_WAVE), 0, (hipStream_t)stream_, rates, times,
                       K, kmax, move, index, draws, mult_d, out_rates, out_times, out_K, out_score);
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(LR_WAVE) void lr_log_priors_kernel(const double* __restrict__ rates,
                                                                const int* __restrict__ K, int kmax, double shape,
                                                                const double* __restrict__ gamma_rate,
                                                                const double* __restrict__ poi_rate,
                                                                double* __restrict__ out) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int k = K[c];
    const double R = (lane < k) ? rates[(size_t)c * kmax + lane] : 1.0;
    double p = lr_wave_prior_gamma(R, k, shape, gamma_rate[c], lane);
    if (poi_rate) p += lr_wave_poisson_prior(k, poi_rate[c], lane);
    if (lane == 0) out[c] = p;
}

extern "C" int lr_log_priors(const double* rates, const int32_t* K, int32_t kmax, int32_t n_chains, double shape,
                             const double* gamma_rate, const double* poi_rate, double* out, void* stream_) {
    if (!rates || !K || !gamma_rate || !out) return LR_ERR_NULL;
    if (kmax < 1 || kmax > LR_WAVE - 1 || n_chains < 1) return LR_ERR_SIZE;
    hipLaunchKernelGGL(lr_log_priors_kernel, dim3(n_chains), dim3(LR_WAVE), 0, (hipStream_t)stream_, rates, K, kmax,
                       shape, gamma_rate, poi_rate, out);
    return (int)hipGetLastError();
}

// debug/parity hook for the RNG: out[i] = draw kind[i] at (it[i], purpose[i], idx[i]) of chain stream
//   kind 0: u_a   1: u_b   2: normal   3: gamma(shape[i])
__global__ void lr_debug_draws_kernel(uint32_t seed, uint32_t chain, const long long* it, const int* purpose,
                                      const int* idx, const int* kind, const double* shape, int n, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lr_stream s{seed, chain};
    const uint64_t t = (uint64_t)it[i];
    double v;
    switch (kind[i]) {
        case 0: v = lr_pair(s, t, purpose[i], idx[i]).a; break;
        case 1: v = lr_pair(s, t, purpose[i], idx[i]).b; break;
        case 2: v = lr_normal(s, t, purpose[i], idx[i]); break;
        default: v = lr_gamma(s, t, purpose[i], idx[i], shape[i]); break;
    }
    out[i] = v;
}

extern "C" int lr_debug_draws(uint64_t seed, int64_t chain, const int64_t* it, const int32_t* purpose,
                              const int32_t* idx, const int32_t* kind, const double* shape, int32_t n, double* out,
                              void* stream_) {
    if (!it || !purpose || !idx || !kind || !shape || !out) return LR_ERR_NULL;
    hipLaunchKernelGGL(lr_debug_draws_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream_, (uint32_t)seed,
                       (uint32_t)chain, (const long long*)it, purpose, idx, kind, shape, n, out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// the engine
// ------------------------------------------------------------------------------------------
#define LR_STEP_WAVES (LR_SCAN_THREADS / LR_WAVE)

// chains [chain_base, chain_base + n_sub): one wave per chain, LR_STEP_WAVES chains per block
__global__ __launch_bounds__(LR_SCAN_THREADS) void lr_chain_step_kernel(lr_step_args a, int mode, int chain_base,
                                                                        int n_sub) {
    __shared__ lr_seg_scratch scratch[LR_STEP_WAVES];
    const int wave = threadIdx.x / LR_WAVE, lane = threadIdx.x & (LR_WAVE - 1);
    const int j = blockIdx.x * LR_STEP_WAVES + wave;
    if (j < n_sub) lr_chain_step_body<32>(a, mode, chain_base + j, lane, &scratch[wave]);
}

// Fused launch of the software-pipelined engine: the first `step_blocks` blocks run the chain step of the
// half whose scan finished in the PREVIOUS launch, all other blocks scan the lineages for the other half.
// The step is latency bound (a serial stream per wave) and the scan is throughput bound, so they overlap.
struct lr_fused_args {
    const double* ts;
    const double* te;
    long long n, chunk;
    double t0;
    int n_bins, tiles;
    int scan_base, scan_n;     // chains scanned by this launch
    int step_base, step_n;     // chains stepped by this launch
    int step_blocks;
};

template <int CB, int H, bool UNIT>
__global__ __launch_bounds__(LR_SCAN_THREADS) void lr_fused_iter_kernel(lr_step_args a, lr_fused_args f) {
    extern __shared__ double2 lds[];
    // the step blocks do not stage tables: their per-wave scratch lives in the same dynamic LDS (a static array on top
    // of the tables would cost the scan blocks one resident block per CU)
    lr_seg_scratch* scratch = reinterpret_cast<lr_seg_scratch*>(lds);
    const int bid = blockIdx.x;
    if (bid < f.step_blocks) {
        const int wave = threadIdx.x / LR_WAVE, lane = threadIdx.x & (LR_WAVE - 1);
        const int j = bid * LR_STEP_WAVES + wave;
        if (j < f.step_n) lr_chain_step_body(a, 0, f.step_base + j, lane, &scratch[wave]);
        return;
    }
    int group, tile;
    if ((f.step_blocks & 7) == 0) {
        lr_xcd_remap(bid - f.step_blocks, f.tiles, (f.scan_n + CB - 1) / CB, &group, &tile);
    } else {
        const int sb = bid - f.step_blocks;
        tile = sb % f.tiles, group = sb / f.tiles;
    }
    const double2* tables = a.tables + (size_t)f.scan_base * a.tab_stride;
    const int tile_stride = lr_tile_stride(a.tiles);
    double* partials = const_cast<double*>(a.partials) + (size_t)f.scan_base * tile_stride;
    if (UNIT)
        lr_scan_unit_body<CB, H>(lds, tile, group * CB, f.ts, f.te, f.n, f.t0, f.n_bins, tables, f.scan_n, f.chunk,
                                 partials, tile_stride);
    else
        lr_scan_fast_body<CB, H>(lds, tile, group * CB, f.ts, f.te, f.n, f.t0, f.n_bins, tables, f.scan_n, f.chunk,
                                 partials, tile_stride);
}

// ------------------------------------------------------------------------------------------
// Persistent engine for unit-resolution data and many chains (>= one pair of chains per block slot).
//
// One 512-thread block owns TWO chains for the whole call and iterates inside the kernel: all 8 waves
// scan every lineage against the pair's lookup table in LDS, the sums are reduced in the block, then waves
// 0 and 1 run the chain step of "their" chain on register-resident state and rebuild the table in LDS while
// the others wait at the barrier.  No launch per iteration, no inter-block communication at all (a block
// never needs another block's data), state and tables touch global memory only at entry and exit.
// The lineages are read as one packed uint16 per lineage (table indices of its birth and death bins,
// lr_pack_lineages_kernel), 8 lineages per 16-byte load: 200 KB per pass for 100k lineages, L2 resident.
// ------------------------------------------------------------------------------------------
#ifndef LR_PERSIST_THREADS
#define LR_PERSIST_THREADS 512
#endif
#ifndef LR_PERSIST_MINWAVES
#define LR_PERSIST_MINWAVES 4
#endif

// One pass of the packed lineages against the pair tables in global memory: the launch-based twin of the persistent
// scan, used where the engines need the sums outside their kernels (the initial state's likelihood, LRF:224-226, and
// the lr_mcmc_time_scan hook).  Block (tile, pair): partials[2 pair .. 2 pair + 1][tile].
template <int H, bool GENERAL>
__global__ __launch_bounds__(256) void lr_pairscan_kernel(lr_packed_lineages pk, long long n8, const double2* __restrict__ tables,
                                                          int n_chains, int n_bins, int tiles, double* __restrict__ partials) {
    constexpr int ENT = GENERAL ? 2 : 1;                       // double2 per pair entry in global memory
    __shared__ double2 tab[LR_UNIT_PLANES * H];                       // S, E (and their slopes) + the pair planes (lr_scan.h)
    __shared__ double red[4][2];
    const int tid = threadIdx.x, lane = tid & (LR_WAVE - 1), wave = tid / LR_WAVE;
    const int tile = blockIdx.x, pair = blockIdx.y;
    const double2* src = tables + (size_t)pair * (2 * H * ENT);
    for (int i = tid; i < 2 * H * ENT; i += 256) tab[GENERAL ? lr_pairgen_lds_entry(i, H) : i] = src[i];
    __syncthreads();
    if (GENERAL) lr_pair_planes_block_general(tab, H, n_bins, tid, 256);
    else lr_pair_planes_block(tab, H, n_bins, tid, 256);
    __syncthreads();
    const long long per = (n8 + tiles - 1) / tiles;
    const long long g0 = min((long long)tile * per, n8), g1 = min(g0 + per, n8);
    double acc0 = 0.0, acc1 = 0.0;
    lr_persist_scan<H, GENERAL>(reinterpret_cast<const char*>(tab), pk, g0, g1 - g0, tid, 256, &acc0, &acc1);
    const double s0 = lr_wave_sum(acc0), s1 = lr_wave_sum(acc1);
    if (lane == 0) red[wave][0] = s0, red[wave][1] = s1;
    __syncthreads();
    if (tid < 2 && 2 * pair + tid < n_chains)
        partials[(size_t)(2 * pair + tid) * lr_tile_stride(tiles) + tile] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// The chain step of the persistent kernels lives in functions of its own (lr_persist4_steppers, lr_persist2_steppers:
// the stepper waves' whole launch; lr_persist_step: one step, for the diagnostic build): its ~120 live registers then do
// not add to the scan loop's, and both fit the 128-VGPR budget of 4 waves per SIMD.
// Every pointer is LDS-typed: the argument block (copied to LDS once per launch; reading it through the generic pointer
// to global memory costs an L2 round trip per field), the per-wave scratch, the state rows and the pair table.
typedef __attribute__((address_space(3))) double lr_lds_f64;
typedef __attribute__((address_space(3))) int lr_lds_i32;
// PB: bins per lane of the one-pass table builder for the kernel's table size (0: choose at run time), ES: the builders'
// `so` - both known to the calling kernel at compile time, so the builder dispatch and the layout switches fold away
// SAMPLER: -1 = both chain steps compiled in, chosen at run time (two-chain kernel); 0 = the RJ sampler's only; 1 = the
// parametric samplers' only (four-chain kernel: the launch picks the instantiation - a stepper function that carries one
// step is a third smaller, and the kernel's instruction footprint is shared by two CUs' instruction cache)
// HAND: the proposal's tables are built by a helper wave from the segments this wave hands over (`hand`, epoch `hand_epoch`)
// CFG: the four-chain kernel's configuration word (LR_P4_CFG_*, lr_step.h); LEAN: the draws come from lr_spec_draw_lean
template <int PB, int ES, bool PRE = false, int SAMPLER = -1, bool HAND = false, int CFG = LR_P4_CFG_GENERIC, bool LEAN = false>
__device__ __forceinline__ void lr_persist_step_body(const __attribute__((address_space(3))) lr_step_args* a3, int c, int lane,
                                                     __attribute__((address_space(3))) lr_seg_scratch* scratch3,
                                                     lr_lds_f64* st_f64, lr_lds_i32* st_i32, double lik, lr_lds_f64* table3,
                                                     lr_lds_f64* br3 /* [2][LR_H_WIDE]: br_length, log br_length */,
                                                     const lr_draw_slot* draws = nullptr /* of the iteration proposed now, made ahead */,
                                                     lr_table_hand* hand = nullptr, int hand_epoch = 0) {
    constexpr int table_es = ES;
    const lr_step_args& a = *(const lr_step_args*)a3;
    const double* br_lds = (const double*)br3;
    LR_SSTAMP(0);
    lr_chain_regs st;
    lr_chain_load(st, (double*)st_f64, (int*)st_i32, lane);
    if (SAMPLER == 1 || (SAMPLER == -1 && a.cfg.sampler != 0))
        lr_dd_step_core<true>(st, a, 0, c, lane, lik, reinterpret_cast<double2*>((double*)table3), table_es, br_lds);
    else if (PRE) {
        lr_rj_draws pre;
        lr_draws_load(draws, pre, lane);
        lr_chain_step_core<true, PB, HAND, CFG, LEAN>(st, a, 0, c, lane, (lr_seg_scratch*)scratch3, lik, reinterpret_cast<double2*>((double*)table3),
                                           table_es, br_lds, br_lds + LR_H_WIDE, &pre, hand, hand_epoch);
    } else
        lr_chain_step_core<true, PB>(st, a, 0, c, lane, (lr_seg_scratch*)scratch3, lik, reinterpret_cast<double2*>((double*)table3),
                                     table_es, br_lds, br_lds + LR_H_WIDE);
    if (HAND) lr_chain_store_handed(st, (double*)st_f64, (int*)st_i32, lane);
    else lr_chain_store(st, (double*)st_f64, (int*)st_i32, lane);
    LR_SSTAMP(8);
}

// End of a wave's share of scan number `scans_done` in the four-chain kernel: the lanes' sums into slot `slot` of
// `part`, count in, and - the wave that arrives LAST of the NA scanning waves - add the block's sums up, per lane over the
// slots in slot order, then across the lanes (the same order whoever is last), into out[0..1].
// BATCH: the last arriver reads the slots BATCH at a time (the additions and their order are the same; a wave that keeps
// resident scan groups has no room for all NA entries at once)
template <int NA, int BATCH = NA>
__device__ __forceinline__ void lr_p4_leave_sums(double2 (*part)[LR_WAVE], int* arrived, double* out, int slot, int lane,
                                                 int& scans_done, double s0, double s1) {
    part[slot][lane] = make_double2(s0, s1);
    int prev = 0;
    if (lane == 0) prev = __hip_atomic_fetch_add(arrived, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    prev = __builtin_amdgcn_readfirstlane(prev);
    if (prev == NA * (scans_done + 1) - 1) {
        asm volatile("" ::: "memory");     // the sums are read after the count was seen (a wave's LDS operations execute in order)
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int w = 0; w < NA; ++w) {
            if (BATCH < NA && w > 0 && w % BATCH == 0) asm volatile("" : "+v"(a0), "+v"(a1) :: "memory");
            const double2 v = part[w][lane];
            a0 += v.x, a1 += v.y;
        }
        a0 = lr_wave_sum(a0), a1 = lr_wave_sum(a1);
        if (lane == 0) out[0] = a0, out[1] = a1;
    }
    ++scans_done;
}

template <int PB, int ES>
__device__ __attribute__((noinline)) void lr_persist_step(const __attribute__((address_space(3))) lr_step_args* a3, int c, int lane,
                                                          __attribute__((address_space(3))) lr_seg_scratch* scratch3,
                                                          lr_lds_f64* st_f64, lr_lds_i32* st_i32, double lik, lr_lds_f64* table3,
                                                          lr_lds_f64* br3) {
    lr_persist_step_body<PB, ES>(a3, c, lane, scratch3, st_f64, st_i32, lik, table3, br3);
}

// The stepper waves' whole launch in the four-chain kernel as ONE call: a call per step costs the callee-saved
// registers' round trip through scratch memory every time (24 dwords x 64 lanes out and back: 0.5 + 0.2 us of a 3.6 us
// step, measured with in-kernel stamps), a call per launch costs it once.  The function keeps the step's own register
// allocation (the reason the step is not inlined into the kernel) and executes the same barriers as the scanner
// waves' loop in lr_persist4_kernel.
//   st_f64 / st_i32: the four chains' state rows; red: [pair][wave][chain of the pair] scan sums; tab: the two pair
//   tables, tab_doubles apart
//   HELP: waves 2, 3 are helper waves - hands[wave] is this stepper's hand-over to wave 2 + wave (lr_persist4_kernel)
//   TAG: not used - the kernel's NR, so that the kernels with resident scan groups call instantiations of their own: the
//   function is specialised for what its callers pass alike (LDS addresses among it), and a second caller of the
//   instantiation of a kernel without resident groups would take that away from it
//   LEAN: the draws made ahead are lr_spec_draw_lean's (lr_persist4_kernel's LEAN)
template <int PB, int ES, int NW, int SAMPLER, bool HELP, int CFG = LR_P4_CFG_GENERIC, int TAG = 0, bool LEAN = false>
__device__ __attribute__((noinline)) void lr_persist4_steppers(const __attribute__((address_space(3))) lr_step_args* a3, int c0,
                                                               int n_chains, int wave, int lane,
                                                               __attribute__((address_space(3))) lr_seg_scratch* scratch3,
                                                               lr_lds_f64* st_f64, lr_lds_i32* st_i32, lr_lds_f64* red,
                                                               lr_lds_f64* tab, int tab_doubles, lr_lds_f64* br3, long long n_iters,
                                                               const lr_draw_slot* draws /* [4]: made ahead (RJ sampler) */,
                                                               lr_table_hand* hands /* [2] */) {
    static_assert(!HELP || (ES == 2 && SAMPLER == 0), "helper waves: RJ sampler at unit resolution");
    static_assert(CFG == LR_P4_CFG_GENERIC || HELP, "a configuration word comes with the helper waves");
    for (long long iter = 0; iter < n_iters; ++iter) {
#pragma unroll 1
        for (int ph = 0; ph < 2; ++ph) {
#ifdef LR_DIAG
            const unsigned long long dq0 = wall_clock64();
#endif
            const int c = c0 + 2 * ph + wave;
            if (c < n_chains) {
                double lik = 0.0;
#pragma unroll
                for (int w2 = 2; w2 < (ES == 2 /* unit resolution: the block's sums in slot 2 */ ? 3 : NW); ++w2) lik += red[(ph * NW + w2) * 2 + wave];
                lr_persist_step_body<PB, ES, ES == 2 /* unit resolution: draws made ahead */ && SAMPLER == 0, SAMPLER, HELP, CFG, LEAN>(
                    a3, c, lane, scratch3, st_f64 + (2 * ph + wave) * (LR_STATE_ROWS * LR_ROW),
                    st_i32 + (2 * ph + wave) * (LR_ISTATE_ROWS * LR_ROW), lik, tab + ph * tab_doubles + wave, br3,
                    draws + (2 * ph + wave), HELP ? hands + wave : nullptr, (int)((2 * iter + ph + 1) & 0x3fffffff));
            }
#ifdef LR_DIAG
            const unsigned long long dq1 = wall_clock64();
#endif
            __syncthreads();
#ifdef LR_DIAG
            if (lane == 0 && blockIdx.x < 64) {
                atomicAdd(&lr_diag_step[16384 + (blockIdx.x * 16 + wave) * 4 + 0], dq1 - dq0);
                atomicAdd(&lr_diag_step[16384 + (blockIdx.x * 16 + wave) * 4 + 1], wall_clock64() - dq1);
            }
#endif
        }
    }
}

// The same for the two-chain kernel, whose waves 0 and 1 scan their share like every other wave and then step: their
// whole launch - scan, reduction, barrier, step, barrier - is one call.
template <int H, int T, int PB>
__device__ __attribute__((noinline)) void lr_persist2_steppers(const __attribute__((address_space(3))) lr_step_args* a3, int c, int wave,
                                                               int lane, __attribute__((address_space(3))) lr_seg_scratch* scratch3,
                                                               lr_lds_f64* st_f64, lr_lds_i32* st_i32, lr_lds_f64* red /* [T/64][2] */,
                                                               lr_lds_f64* tab, lr_lds_f64* br3, const uint4* __restrict__ idx8,
                                                               long long n8w, long long n_iters, int prio_shift, int grp) {
    const int tid = wave * LR_WAVE + lane;
    for (long long iter = 0; iter < n_iters; ++iter) {
        if (prio_shift > 0) {
            if (((wall_clock64() >> prio_shift) + grp) & 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        double acc0 = 0.0, acc1 = 0.0;
        lr_scan_tail tail;
        lr_persist_scan_pair<H, 1, true>((const char*)(const double*)tab, idx8, n8w, tid, T, &acc0, &acc1, nullptr, &tail);
        const double s0 = lr_wave_sum(acc0), s1 = lr_wave_sum(acc1);
        if (lane == 0) red[wave * 2 + 0] = s0, red[wave * 2 + 1] = s1;
        lr_scan_drain(tail);
        __syncthreads();
        double lik = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < T / LR_WAVE; ++w2) lik += red[w2 * 2 + wave];
        lr_persist_step_body<PB, 2>(a3, c, lane, scratch3, st_f64, st_i32, lik, tab + wave, br3);
        __syncthreads();
    }
}

// T = threads per block: 512 (two blocks share a CU) or, when there are no more blocks than CUs anyway (at most 512
// chains), 1024 - all 16 waves of the CU scan the one pair.
template <int H, int T>
__global__ __launch_bounds__(T, LR_PERSIST_MINWAVES) void lr_persist_kernel(
    const lr_step_args* __restrict__ ap /* in global memory: taking the address of a by-value kernel argument would
                                           copy it to scratch */,
    const uint4* __restrict__ idx8, long long n8, lr_p4_shares sh, long long n_iters, int prio_shift) {
    const lr_step_args& a = *ap;
    __shared__ double2 tab[LR_UNIT_PLANES * H];  // the pair table: S' entries [0,H), E' [H,2H), pair sums behind; (.x, .y) = (chain 0, chain 1)
    __shared__ double red[T / LR_WAVE][2];
    __shared__ lr_seg_scratch scratch[2];
    // the two chains' state rows live in LDS between iterations (registers are needed by the step itself)
    __shared__ double st_f64[2][LR_STATE_ROWS * LR_ROW];
    __shared__ int st_i32[2][LR_ISTATE_ROWS * LR_ROW];
    __shared__ lr_step_args a_lds;
    __shared__ double br_lds[2][LR_H_WIDE];   // per-bin data constants of the table builders: br_length / DT / TREND, log br_length
    const int tid = threadIdx.x, lane = tid & (LR_WAVE - 1), wave = tid / LR_WAVE;
    if (tid < (int)(sizeof(lr_step_args) / 4)) reinterpret_cast<int*>(&a_lds)[tid] = reinterpret_cast<const int*>(ap)[tid];
    for (int b = tid; b < LR_H_WIDE; b += blockDim.x) {
        const bool in = b < ap->cfg.n_bins;
        br_lds[0][b] = (in && ap->br_length) ? ap->br_length[b] : 0.0;
        br_lds[1][b] = in ? ap->log_br[b] : 0.0;
    }
    const int c0 = blockIdx.x * 2;
    const int c = c0 + wave;
    const bool stepper = (wave < 2) && (c < a.cfg.n_chains);
    double2* gpair = lr_chain_table(a, c0);  // the pair (c0, c0+1) shares one table in the unit layout
    if (stepper) {
        const double* S = a.state_f64 + (size_t)c * LR_STATE_ROWS * LR_ROW;
        const int* I = a.state_i32 + (size_t)c * LR_ISTATE_ROWS * LR_ROW;
        for (int r = 0; r < LR_STATE_ROWS; ++r) st_f64[wave][r * LR_ROW + lane] = S[r * LR_ROW + lane];
        for (int r = 0; r < LR_ISTATE_ROWS; ++r) st_i32[wave][r * LR_ROW + lane] = I[r * LR_ROW + lane];
    }
    for (int i = tid; i < 2 * H; i += T) tab[i] = gpair[i];
    __syncthreads();
    lr_pair_planes_block(tab, H, a.cfg.n_bins, tid, T);
    __syncthreads();
    const char* lbase = reinterpret_cast<const char*>(tab);
    // unequal shares of the waves (see lr_persist4_kernel): older waves 0..3 take trips from the younger 4..7
    const long long n8w = sh.delta[0] != 0 ? ((n8 + T - 1) / T + sh.delta[wave]) * T : n8;
    const int grp = (blockIdx.x >> 8) & 1;
#ifdef LR_DIAG
    unsigned long long d_t0 = 0, d_t1 = 0, d_t2 = 0, d_scan = 0, d_red = 0, d_step = 0;
#endif
#ifndef LR_DIAG
    if (stepper) {
        lr_persist2_steppers<H, T, (H <= 264 ? lr_bins_per_lane(H) : 0)>(
            (const __attribute__((address_space(3))) lr_step_args*)&a_lds, c, wave, lane,
            (__attribute__((address_space(3))) lr_seg_scratch*)&scratch[wave], (lr_lds_f64*)st_f64[wave], (lr_lds_i32*)st_i32[wave],
            (lr_lds_f64*)&red[0][0], (lr_lds_f64*)reinterpret_cast<double*>(tab), (lr_lds_f64*)&br_lds[0][0], idx8, n8w, n_iters,
            prio_shift, grp);
    } else
#endif
    for (long long iter = 0; iter < n_iters; ++iter) {
        // Two blocks share a CU; the one dispatched second is the younger wave on every SIMD and loses issue
        // arbitration to its older neighbour all the time (+30 % per iteration, measured).  Both read the same
        // 100 MHz clock, so slicing it gives them complementary priorities that even the two out
        // (MI355X_MICROARCH.md "Two waves per SIMD" item 4; block id >= 256 = second dispatch: speed only).
        if (prio_shift > 0) {
            if (((wall_clock64() >> prio_shift) + grp) & 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
#ifdef LR_DIAG
        d_t0 = wall_clock64();
#endif
        double acc0 = 0.0, acc1 = 0.0;
        lr_scan_tail tail;
        lr_persist_scan_pair<H, 1, true>(lbase, idx8, n8w, tid, T, &acc0, &acc1, nullptr, &tail);
#ifdef LR_DIAG
        if (lane == 0 && blockIdx.x < 512) atomicAdd(&lr_diag_step[20000 + blockIdx.x * 8 + wave], wall_clock64() - d_t0);
#endif
#ifdef LR_DIAG
        d_t1 = wall_clock64();
#endif
        const double s0 = lr_wave_sum(acc0), s1 = lr_wave_sum(acc1);
        if (lane == 0) red[wave][0] = s0, red[wave][1] = s1;
        lr_scan_drain(tail);      // the idle prefetch of the scan's last trip (lr_scan.h)
        __syncthreads();  // every scan is done: sums visible, table free to be rebuilt
#ifdef LR_DIAG
        d_t2 = wall_clock64();
#endif
        if (stepper) {
            double lik = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < T / LR_WAVE; ++w2) lik += red[w2][wave];
            lr_persist_step<(H <= 264 ? lr_bins_per_lane(H) : 0), 2>(
                (const __attribute__((address_space(3))) lr_step_args*)&a_lds, c, lane,
                (__attribute__((address_space(3))) lr_seg_scratch*)&scratch[wave], (lr_lds_f64*)st_f64[wave],
                (lr_lds_i32*)st_i32[wave], lik, (lr_lds_f64*)(reinterpret_cast<double*>(tab) + wave), (lr_lds_f64*)&br_lds[0][0]);
        }
        __syncthreads();  // new tables ready
#ifdef LR_DIAG
        d_scan += d_t1 - d_t0, d_red += d_t2 - d_t1, d_step += wall_clock64() - d_t2;
#endif
    }
#ifdef LR_DIAG
    if (lane == 0 && blockIdx.x < 512) {
        unsigned long long* o = lr_diag_step + 4096 * 12 - 4096 + (blockIdx.x * 8 + wave) % 4096;
        (void)o;
    }
    if (tid == 0 && blockIdx.x < 340) {
        lr_diag_step[blockIdx.x * 12 + 9] = d_scan, lr_diag_step[blockIdx.x * 12 + 10] = d_red;
        lr_diag_step[blockIdx.x * 12 + 11] = d_step;
    }
    if (tid == 0 && blockIdx.x < 1024) lr_diag_step[2048 * 12 + blockIdx.x * 2 + 1] = wall_clock64();
#endif
    if (stepper) {
        double* S = a.state_f64 + (size_t)c * LR_STATE_ROWS * LR_ROW;
        int* I = a.state_i32 + (size_t)c * LR_ISTATE_ROWS * LR_ROW;
        for (int r = 0; r < LR_STATE_ROWS; ++r) S[r * LR_ROW + lane] = st_f64[wave][r * LR_ROW + lane];
        for (int r = 0; r < LR_ISTATE_ROWS; ++r) I[r * LR_ROW + lane] = st_i32[wave][r * LR_ROW + lane];
    }
    for (int i = tid; i < 2 * H; i += T) gpair[i] = tab[i];  // pending tables back to global
}

// Four chains per 1024-thread block (one block per CU), two pairs in ping-pong: while waves 0 and 1 run the chain
// steps of one pair, waves 2..15 scan the lineages for the OTHER pair, so the latency-bound step always hides
// under a scan of the same block and the LDS pipe never waits for it.  Used when there are enough chains to give
// every CU four (cfg4: 1024 chains = 256 blocks).
#ifndef LR_P4_THREADS
#define LR_P4_THREADS 1024
#endif
#ifdef LR_DIAG
#define LR_PSTAMP(k) if (threadIdx.x == 0 && blockIdx.x < 64) lr_diag_step[28672 + blockIdx.x * 8 + (k)] = wall_clock64()
#else
#define LR_PSTAMP(k)
#endif

// HELP (RJ sampler at unit resolution): waves 2, 3 - the oldest waves of the two SIMDs that carry no stepper - are HELPER
// waves and twelve waves scan.  A stepper hands the segments of its proposal over through LDS as soon as they stand
// (lr_propose_rj's HAND, ~1.2 us into a 3.2 us step) and goes on with guard, prior and state; its helper builds the table
// with its pair planes meanwhile: the serial path of a phase is load + move + staging + table instead of the whole step,
// and every SIMD carries one wave of the step and three scanners.  Before the hand-over arrives a helper scores the first
// groups of the scan (sh.help_trips trips of the 128 helper lanes; the scanners stride over the rest), and the draws of the
// OTHER pair's next step are one Philox call on each of the two oldest scanner waves (four waves, a call each, otherwise).
// CFG (HELP only): the configuration word (LR_P4_CFG_*, lr_step.h).  The role waves - steppers, helpers' table duty, the
// draw duty - are one wave's instruction stream per chain step and sit on the oldest wave of every SIMD, so what they
// issue is taken from the scanners beside them as well; a specialised word compiles the run's model class and the default
// switches into them as constants (constant propagation only: the same floating-point operations in the same order as
// LR_P4_CFG_GENERIC executes for that configuration).  The launch picks the word (lr_p4_cfg_choice).
// NR (HELP only): > 0 = every scanner lane keeps the decoded groups of its first NR trips (LR_P4_NR_DRAW on the two waves
// that also make the draws ahead), every helper lane those of its first LR_P4_RES_HELP trips, in registers for the whole
// launch (lr_resident_groups, lr_scan.h) and the scans run those trips without load, wait and decode; the same groups per
// lane in the same order through the same operations, so the sums are the doubles of NR = 0, which runs
// lr_persist_scan_pair's loop for every trip.  The launch picks between 0 and LR_P4_NR (lr_p4_resident_choice).
#ifndef LR_P4_NR
#define LR_P4_NR 8            /* resident trips per scanner lane; 0: the resident form is not built */
#endif
#ifndef LR_P4_RES_HDR
#define LR_P4_RES_HDR 0       /* 1: the header kept decoded (three registers per trip), 0: as its word (one) */
#endif
#ifndef LR_P4_NR_DRAW
#define LR_P4_NR_DRAW 4       /* ... per lane of the two scanner waves that also make the draws ahead (waves 4, 5) */
#endif
#define LR_P4_RES_HELP 5      /* resident trips per helper lane: every trip lr_set_shares' rule gives the helpers */
// PIPE (NR > 0 only): 1 = a wave that runs all its resident trips takes them as one basic block without the scalar test
// and branch per trip (lr_resident_trips_block, lr_scan.h): the same operations on every accumulator in the same order,
// every gather where the trip-by-trip form has it.  The launch picks between 0 and LR_P4_PIPE (lr_p4_pipe_choice).
#ifndef LR_P4_PIPE
#define LR_P4_PIPE 1          /* 0: the one-block form is not built */
#endif
// LEAN (PIPE > 0 only): the draw duty of waves 4, 5 is lr_spec_draw_lean (lr_step.h) - no logarithm of the acceptance
// uniform (the stepper's packed lr_log takes it along in its free lane), the multiplier draws only in iterations that can
// read them, the scalars stored by the lanes that drew them.  The Philox addresses, every value a step reads and every
// floating-point operation on it are those of LEAN = false.  The launch picks (lr_p4_lean_choice).
template <int H, bool GENERAL, bool PARAM /* a parametric sampler's chain step (DDRate, trend_rate) instead of the RJ sampler's */,
          bool HELP = false, int CFG = LR_P4_CFG_GENERIC, int NR = 0, int PIPE = 0, bool LEAN = false>
__global__ __launch_bounds__(LR_P4_THREADS, LR_P4_THREADS / 256) void lr_persist4_kernel(const lr_step_args* __restrict__ ap /* in global memory: a by-value argument struct measured
                                                                       0.2 us per launch faster, but one instantiation then kept a copy of it in scratch
                                                                       memory and read its fields from there in every phase */,
                                                                       lr_packed_lineages pk, long long n8,
                                                                       lr_p4_shares sh, long long n_iters, char* carry_all) {
    static_assert(!HELP || (!GENERAL && !PARAM), "helper waves: RJ sampler at unit resolution");
    static_assert(CFG == LR_P4_CFG_GENERIC || (HELP && H <= 264), "a configuration word comes with the helper waves");
    static_assert(NR == 0 || HELP, "resident groups come with the helper waves");
    static_assert(PIPE == 0 || (PIPE == 1 && NR > 0), "the one-block form is one of the resident trips");
    static_assert(!LEAN || PIPE > 0, "the lean draw duty comes with the one-block form");
    const lr_step_args& a = *ap;
    LR_PSTAMP(0);      // entry (LR_DIAG: wall-clock stamps of a launch's stages, blocks < 64; scratch/diag_p4_launch.py)
    constexpr int NW = LR_P4_THREADS / LR_WAVE;          // 16 waves: 2 steppers + 14 scanners (HELP: 2 + 2 helpers + 12)
    constexpr int W0 = HELP ? 4 : 2;                      // first scanner wave
    constexpr int NS = NW - W0;                           // scanner waves
    constexpr int LR_P4_SCANNERS = NS * LR_WAVE;
    constexpr int ENT = GENERAL ? 2 : 1;                  // double2 per pair-table entry (LR_TAB_PAIRGEN / LR_TAB_UNIT)
    constexpr int ES = GENERAL ? 6 * H : 2;               // the builders' `so`: doubles from a value to its slope in the LDS image
    __shared__ double2 tab[2][LR_UNIT_PLANES * H];        // pair tables: S, E (general times: and their slopes) + the pair planes
    __shared__ double red[2][NW][2];                      // [pair][scanner wave][chain of the pair]; LAST_SUMS: slot [2] = the block's sums
    // Unit resolution: every scanner lane's two accumulators of the current scan, and the count of scanner waves that
    // have left theirs: the wave that arrives LAST adds them up (one wave's reduction instead of fourteen: the kernel is
    // bound by instruction issue) - per lane over the waves in wave order, then across the lanes: the same order whoever
    // is last.  (On general times the scans are the longer side of a phase and the serial tail costs more than it saves.)
    constexpr bool LAST_SUMS = !GENERAL;
    __shared__ double2 part[LAST_SUMS ? NW - 2 : 1][LR_WAVE];
    __shared__ int arrived;
    __shared__ lr_table_hand hands[2];                    // HELP: stepper k's hand-over to helper wave 2 + k
    __shared__ lr_seg_scratch scratch[2];                 // stepper k's scratch (HELP: the segments it hands over)
    __shared__ double st_f64[4][LR_STATE_ROWS * LR_ROW];
    __shared__ int st_i32[4][LR_ISTATE_ROWS * LR_ROW];
    __shared__ lr_step_args a_lds;
    __shared__ double br_lds[2][LR_H_WIDE];   // per-bin data constants of the table builders: br_length / DT / TREND, log br_length
    // The state-independent draws of a chain's next proposal (acceptance uniform and its logarithm, move selectors,
    // multiplier exponents and factors, the split move's beta variate), made one phase ahead by the scanner waves that
    // finish first: the steppers are the kernel's critical path (one wave's instruction stream per chain step), the
    // scanners of a phase wait 1-2 us at its barrier.  Same (iteration, purpose, index) Philox addresses as the draws
    // made inside the step: the stream does not change.  RJ sampler only; the parametric samplers draw in the step.
    // (Reached through a pointer that draw_duty captures: with the array itself the inliner also takes prologue_draws
    // into the kernels without helper waves, and their stepper functions then save callee-saved registers in scratch.)
    __shared__ lr_draw_slot draws_s[4];
    lr_draw_slot* const draws = draws_s;
    const int tid = threadIdx.x, lane = tid & (LR_WAVE - 1), wave = tid / LR_WAVE;
    if (tid < (int)(sizeof(lr_step_args) / 4)) reinterpret_cast<int*>(&a_lds)[tid] = reinterpret_cast<const int*>(ap)[tid];
    for (int b = tid; b < LR_H_WIDE; b += blockDim.x) {
        const bool in = b < ap->cfg.n_bins;
        br_lds[0][b] = (in && ap->br_length) ? ap->br_length[b] : 0.0;
        br_lds[1][b] = in ? ap->log_br[b] : 0.0;
    }
    // (unit resolution only: on general times the scan loops are the longer side of a phase and have nothing to spare)
    constexpr bool draw_ahead = !GENERAL && !PARAM;
    // draw duty of scanner wave 2 + q, q < 4, for the pair `pr` that has just been scanned: part q >> 1 of chain q & 1
    // (HELP: waves 4, 5 - the oldest scanners - sit on the steppers' SIMDs and end their scans last of all scanners (in-kernel
    // stamps: 3.1 us of a 3.15 us phase against 2.2-2.9 for the others) - and still the draws cost least there: by waves 6, 7
    // (SIMDs 2, 3, beside the helpers) cfg4 ran 6.37-6.40 us per iteration against 6.25, A/B twice on one box)
    auto draw_duty = [&](int pr) {
        const int q = wave - W0, k = q & 1, ch = 2 * pr + k;      // (the oldest scanner waves: the first to finish)
        if (!draw_ahead || q < 0 || q >= (HELP ? 2 : 4) || (int)(blockIdx.x * 4) + ch >= ap->cfg.n_chains) return;
        const int* I = st_i32[ch] + LR_IROW_SCALARS * LR_ROW;
        const unsigned long long it = ((unsigned long long)(unsigned int)I[LR_I_IT_HI] << 32 | (unsigned int)I[LR_I_IT_LO]) + 1ull;
        lr_draw_slot* slot = &draws[ch];
        // (HELP: one wave per chain, one Philox call for both parts)
        if (LEAN) lr_spec_draw_lean<CFG>(a_lds, (int)(blockIdx.x * 4) + ch, lane, it, slot, I);
        else if (HELP) lr_spec_draw_both<CFG>(a_lds, (int)(blockIdx.x * 4) + ch, lane, it, slot);
        else lr_spec_draw_part(a_lds, (int)(blockIdx.x * 4) + ch, lane, it, slot, q >> 1);
    };
    // a helper wave's table duty of a phase whose steppers advance pair `ph`: once the stepper has handed them over, the
    // tables of its chain of pair ph
    auto help_duty = [&](int ph, int epoch) {
        const int k = wave - 2;
        const int ch = 2 * ph + k;
        if ((int)(blockIdx.x * 4) + ch >= ap->cfg.n_chains) return;
        lr_table_hand* hand = &hands[k];
#ifdef LR_DIAG
        const unsigned long long dh0 = wall_clock64();
#endif
        while (__hip_atomic_load(&hand->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != epoch) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
#ifdef LR_DIAG
        if (lane == 0 && blockIdx.x < 64) atomicAdd(&lr_diag_step[16384 + (blockIdx.x * 16 + wave) * 4 + 2], wall_clock64() - dh0);
#endif
        const lr_seg_scratch* sc = &scratch[k];
        const int eL = lane <= LR_KMAX ? sc->edge[0][lane] : 0, eM = lane <= LR_KMAX ? sc->edge[1][lane] : 0;
        double* tabd = reinterpret_cast<double*>(tab[ph]) + k;
        // the builder's model, table size and in-bin fractions: read from the configuration, or the word's constants
        int model = a_lds.cfg.model;
        if (CFG == LR_P4_CFG_BDI) __builtin_assume((unsigned int)model < 2u);     // (lr_p4_cfg_choice: model 0 or 1)
        if (CFG == LR_P4_CFG_KEIDING) model = LR_MODEL_KEIDING;
        constexpr bool fixed = CFG != LR_P4_CFG_GENERIC;
        const double constP = lr_build_tables_segments<(H <= 264 ? lr_bins_per_lane(H) : 1), 2>(
            sc, eL, eM, hand->KL, hand->KM, br_lds[0], br_lds[1], model, a_lds.cfg.n_bins, a_lds.n_cls, fixed ? H : a_lds.H,
            reinterpret_cast<double2*>(tabd), lane, LR_TAB_UNIT, fixed ? LR_P4_FRAC_BIRTH : a_lds.cfg.frac_birth,
            fixed ? LR_P4_FRAC_DEATH : a_lds.cfg.frac_death, ES, nullptr);
        LR_WAVE_LDS_ORDER();
        lr_pair_planes_wave(tabd, H, a_lds.cfg.n_bins, lane, 0);
        if (lane == 0) st_f64[ch][LR_ROW_SCALARS * LR_ROW + LR_S_CONST_P] = constP;
    };
    if (tid == 0) arrived = 0;
    if (tid < 2) hands[tid].epoch = 0;
    for (int i = tid; i < 2 * NW * 2; i += LR_P4_THREADS) (&red[0][0][0])[i] = 0.0;
    int scans_done = 0;
    // a scanning wave's end of scan number `scans_done` for pair `pr` (HELP: the helper waves score a share too - slots NS,
    // NS + 1)
    constexpr int NA = NS + (HELP ? 2 : 0);
    auto leave_sums = [&](int pr, double s0, double s1) {
        if (LAST_SUMS) {
            lr_p4_leave_sums<NA, (NR > 0 ? NA / 2 : NA)>(part, &arrived, &red[pr][2][0], wave >= W0 ? wave - W0 : NS + wave - 2, lane, scans_done, s0, s1);
        } else {
            // (general times: every scanning wave adds its own lanes up; the stepper adds the waves' sums in wave order)
            s0 = lr_wave_sum(s0), s1 = lr_wave_sum(s1);
            if (lane == 0) red[pr][wave][0] = s0, red[pr][wave][1] = s1;
        }
    };
    const int c0 = blockIdx.x * 4;
    const int C = a.cfg.n_chains;
    if (wave < 4 && c0 + wave < C) {
        const int c = c0 + wave;
        const double* S = a.state_f64 + (size_t)c * LR_STATE_ROWS * LR_ROW;
        const int* I = a.state_i32 + (size_t)c * LR_ISTATE_ROWS * LR_ROW;
        for (int r = 0; r < LR_STATE_ROWS; ++r) st_f64[wave][r * LR_ROW + lane] = S[r * LR_ROW + lane];
        for (int r = 0; r < LR_ISTATE_ROWS; ++r) st_i32[wave][r * LR_ROW + lane] = I[r * LR_ROW + lane];
    }
    double2* g0 = lr_chain_table(a, c0);
    double2* g1 = lr_chain_table(a, c0 + 2);             // tables are allocated for whole groups of cb >= 4 chains
    for (int i = tid; i < 2 * H * ENT; i += LR_P4_THREADS) {
        const int e = GENERAL ? lr_pairgen_lds_entry(i, H) : i;
        tab[0][e] = g0[i], tab[1][e] = g1[i];
    }
    __syncthreads();
    LR_PSTAMP(1);      // arguments, data constants, the four chains' state rows and the two pair tables are in LDS
    if (GENERAL) {
        lr_pair_planes_block_general(tab[0], H, a.cfg.n_bins, tid, LR_P4_THREADS);
        lr_pair_planes_block_general(tab[1], H, a.cfg.n_bins, tid, LR_P4_THREADS);
    } else {
        lr_pair_planes_block(tab[0], H, a.cfg.n_bins, tid, LR_P4_THREADS);
        lr_pair_planes_block(tab[1], H, a.cfg.n_bins, tid, LR_P4_THREADS);
    }
    __syncthreads();
    LR_PSTAMP(2);      // pair planes derived
    const bool scanner = wave >= W0;
    const bool helper = HELP && (wave == 2 || wave == 3);
    const int sid = tid - W0 * LR_WAVE;
    // The SIMD issue arbiter serves its oldest wave first: with equal shares the scanner waves of a SIMD finish one
    // after the other (5.0 / 6.4 / 7.9 / 9.5 us per phase, measured with in-kernel stamps), the youngest runs the tail
    // alone, and SIMDs 0, 1 carry the stepper waves on top.  So the waves get unequal shares (lr_p4_shares) chosen to
    // make them finish together.  lr_pack_lineages_kernel stores the moved groups where the takers keep striding, so
    // this is only a per-wave end of the loop: a fixed partition, the summation order - and with it bitwise
    // reproducibility - stays.
    // (HELP: the first sh.help_trips * 128 groups are the helper waves'; the shares apply to the scanners' region behind them)
    const long long nh_ = HELP ? (long long)sh.help_trips * (2 * LR_WAVE) : 0;
    const int k_tot = (int)((n8 - nh_ + LR_P4_SCANNERS - 1) / LR_P4_SCANNERS);
    const int k_mine = k_tot + (scanner ? sh.delta[wave - W0] : 0);
    // equal shares (short scans): the true end, so that the ragged last trip costs only the lanes that have a group
    bool any_shift = false;
#pragma unroll
    for (int q = 0; q < NS; ++q) any_shift |= sh.delta[q] != 0;
    // HELP: the first `nh` groups are the helper waves' (equal shares behind them)
    // ([0, nh): helper waves, the rest: the scanner waves)
    const long long nh = HELP ? (long long)sh.help_trips * (2 * LR_WAVE) : 0;
    const long long n8w = any_shift ? (long long)k_mine * LR_P4_SCANNERS : n8 - nh;
    // (the pair is a compile-time constant at every call, as it is in the scanners' unrolled loop: the table's LDS address
    // then sits in the offset field of the slice's gathers - indexed by a run-time phase, each of the eight gathers of a
    // trip took a vector add with the table base first)
    // NR > 0: the resident groups of a scanner lane and of a helper lane (equal shares: the helper form has no others),
    // loaded once per launch BEHIND the prologue, whose scan goes through the loop: they are live in the iterations' loop of
    // their role alone, not beside the prologue's draw duty
    constexpr bool HDR = LR_P4_RES_HDR != 0;
    lr_resident_groups<(NR > 0 ? NR : 1), HDR> res;
    lr_resident_groups<LR_P4_RES_HELP, HDR> hres;
    constexpr int NRD = NR > 0 ? LR_P4_NR_DRAW : 0;
    lr_resident_groups<(NRD > 0 ? NRD : 1), HDR> dres;
    // (the two scanner waves with the draw duty - Philox, exp, lr_log live beside the groups - keep NRD trips, in `dres`)
    const bool res_scanner = NR > 0 && scanner && !(draw_ahead && wave - W0 < 2);
    auto help_scan = [&](auto pr_, auto resident_) {
        constexpr int pr = decltype(pr_)::value;
        double s0 = 0.0, s1 = 0.0;
        if (decltype(resident_)::value) {
            // (trips behind the resident ones - LR_P4_HELP_TRIPS above LR_P4_RES_HELP - as before)
            const long long done = (long long)hres.trips * (2 * LR_WAVE);
            lr_resident_trips<LR_P4_RES_HELP, HDR, (PIPE > 0)>(reinterpret_cast<const char*>(tab[pr]), hres, s0, s1);
            if (nh > done) lr_persist_scan<H, GENERAL, 1, false, false>(reinterpret_cast<const char*>(tab[pr]), pk, done, nh - done, tid - 2 * LR_WAVE, 2 * LR_WAVE, &s0, &s1);
        } else if (nh > 0) lr_persist_scan<H, GENERAL, 1, false, false>(reinterpret_cast<const char*>(tab[pr]), pk, 0, nh, tid - 2 * LR_WAVE, 2 * LR_WAVE, &s0, &s1);
        leave_sums(pr, s0, s1);
    };
    // NR > 0: a scanner wave's share of the scan for pair `pr` (a compile-time constant here too)
    auto scan_resident = [&](auto pr_, double* s0, double* s1, lr_scan_tail* tail) {
        constexpr int pr = decltype(pr_)::value;
        lr_persist_scan_pair_resident<(PIPE > 0)>(reinterpret_cast<const char*>(tab[pr]), pk.idx8 + nh, n8w, sid, LR_P4_SCANNERS, res, s0, s1, tail);
    };
    // prologue: pair 0's pending proposal is scanned so that phase A can step it - unless the launch before this one has
    // left the sums of that very scan (its last phase scored pair 0; lr_prepare_constants clears the flag whenever the
    // state is set from outside): the same doubles, the scan uses the same partition
    static_assert(2 * NW * 8 + 4 <= LR_P4_CARRY_BYTES, "");
    char* carry = carry_all ? carry_all + (size_t)blockIdx.x * LR_P4_CARRY_BYTES : nullptr;
    const bool carried = carry && *reinterpret_cast<const int*>(carry + 2 * NW * 8) == 1;
    auto prologue_draws = [&]() { draw_duty(0); };      // the draws of the first phase's steps
    if (carried) {
        if (tid < 2 * NW) (&red[0][0][0])[tid] = reinterpret_cast<const double*>(carry)[tid];
        if (scanner) prologue_draws();
    } else if (scanner) {
        double s0 = 0.0, s1 = 0.0;
        lr_scan_tail tail;
        lr_persist_scan<H, GENERAL, 1, false, true>(reinterpret_cast<const char*>(tab[0]), pk, nh, n8w, sid, LR_P4_SCANNERS, &s0, &s1, nullptr, &tail);
        leave_sums(0, s0, s1);
        lr_scan_drain(tail);
        prologue_draws();
    }
    if (helper && !carried) help_scan(std::integral_constant<int, 0>(), std::false_type());
    __syncthreads();
    LR_PSTAMP(3);      // prologue done: pair 0's sums (scanned or carried), the first draws
    // phase ph of an iteration: the steppers advance pair `ph`, the scanners score pair `1 - ph`
    if (helper) {
        if (NR > 0) lr_resident_load(hres, pk.idx8, nh, tid - 2 * LR_WAVE, 2 * LR_WAVE);
        for (long long iter = 0; iter < n_iters; ++iter) {
#pragma unroll 1
            for (int ph = 0; ph < 2; ++ph) {
#ifdef LR_DIAG
                const unsigned long long dq0 = wall_clock64();
#endif
                if (ph == 0) help_scan(std::integral_constant<int, 1>(), std::integral_constant<bool, (NR > 0)>());
                else help_scan(std::integral_constant<int, 0>(), std::integral_constant<bool, (NR > 0)>());
                help_duty(ph, (int)((2 * iter + ph + 1) & 0x3fffffff));
#ifdef LR_DIAG
                const unsigned long long dq1 = wall_clock64();
#endif
                __syncthreads();
#ifdef LR_DIAG
                if (lane == 0 && blockIdx.x < 64) {
                    atomicAdd(&lr_diag_step[16384 + (blockIdx.x * 16 + wave) * 4 + 0], dq1 - dq0);
                    atomicAdd(&lr_diag_step[16384 + (blockIdx.x * 16 + wave) * 4 + 1], wall_clock64() - dq1);
                }
#endif
            }
        }
    } else if (!scanner)
        lr_persist4_steppers<(H <= 264 ? lr_bins_per_lane(H) : 0), ES, NW, PARAM ? 1 : 0, HELP, CFG, NR + 64 * PIPE, LEAN>(
            (const __attribute__((address_space(3))) lr_step_args*)&a_lds, c0, C, wave, lane,
            (__attribute__((address_space(3))) lr_seg_scratch*)&scratch[wave], (lr_lds_f64*)&st_f64[0][0], (lr_lds_i32*)&st_i32[0][0],
            (lr_lds_f64*)&red[0][0][0], (lr_lds_f64*)reinterpret_cast<double*>(tab[0]), 2 * LR_UNIT_PLANES * H,
            (lr_lds_f64*)&br_lds[0][0], n_iters, &draws[0], &hands[0]);
    else if (res_scanner) {
        // the ten scanner waves without a draw duty: the loop below without it, so that their NR trips of registers are
        // not live beside its code
        if constexpr (NR > 0) {
        lr_resident_load(res, pk.idx8 + nh, n8w, sid, LR_P4_SCANNERS);
        for (long long iter = 0; iter < n_iters; ++iter) {
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) {
#ifdef LR_DIAG
                const unsigned long long dq0 = wall_clock64();
#endif
                {
                    double s0 = 0.0, s1 = 0.0;
                    lr_scan_tail tail;
                    if (ph == 0) scan_resident(std::integral_constant<int, 1>(), &s0, &s1, &tail);
                    else scan_resident(std::integral_constant<int, 0>(), &s0, &s1, &tail);
                    leave_sums(1 - ph, s0, s1);
                    lr_scan_drain(tail);
                }
#ifdef LR_DIAG
                const unsigned long long dq1 = wall_clock64();
#endif
                __syncthreads();
#ifdef LR_DIAG
                if (lane == 0 && blockIdx.x < 64) {
                    atomicAdd(&lr_diag_step[16384 + (blockIdx.x * 16 + wave) * 4 + 0], dq1 - dq0);
                    atomicAdd(&lr_diag_step[16384 + (blockIdx.x * 16 + wave) * 4 + 1], wall_clock64() - dq1);
                }
#endif
            }
        }
        }
    } else {
    if constexpr (NRD > 0) lr_resident_load(dres, pk.idx8 + nh, n8w, sid, LR_P4_SCANNERS);
    for (long long iter = 0; iter < n_iters; ++iter) {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
#ifdef LR_DIAG
            const unsigned long long dq0 = wall_clock64();
#endif
            {
                double s0 = 0.0, s1 = 0.0;
                lr_scan_tail tail;
                if constexpr (NRD > 0) {
                    if (ph == 0) lr_persist_scan_pair_resident<(PIPE > 0)>(reinterpret_cast<const char*>(tab[1]), pk.idx8 + nh, n8w, sid, LR_P4_SCANNERS, dres, &s0, &s1, &tail);
                    else lr_persist_scan_pair_resident<(PIPE > 0)>(reinterpret_cast<const char*>(tab[0]), pk.idx8 + nh, n8w, sid, LR_P4_SCANNERS, dres, &s0, &s1, &tail);
                } else
                lr_persist_scan<H, GENERAL, 1, false, true>(reinterpret_cast<const char*>(tab[1 - ph]), pk, nh, n8w, sid, LR_P4_SCANNERS, &s0, &s1, nullptr, &tail);
                leave_sums(1 - ph, s0, s1);
                lr_scan_drain(tail);      // the idle prefetch of the scan's last trip (lr_scan.h)
                draw_duty(1 - ph);
            }
#ifdef LR_DIAG
            const unsigned long long dq1 = wall_clock64();
#endif
            __syncthreads();
#ifdef LR_DIAG
            if (lane == 0 && blockIdx.x < 64) {
                atomicAdd(&lr_diag_step[16384 + (blockIdx.x * 16 + wave) * 4 + 0], dq1 - dq0);
                atomicAdd(&lr_diag_step[16384 + (blockIdx.x * 16 + wave) * 4 + 1], wall_clock64() - dq1);
            }
#endif
        }
    }
    }
    LR_PSTAMP(4);      // the launch's iterations done
    if (wave < 4 && c0 + wave < C) {
        const int c = c0 + wave;
        double* S = a.state_f64 + (size_t)c * LR_STATE_ROWS * LR_ROW;
        int* I = a.state_i32 + (size_t)c * LR_ISTATE_ROWS * LR_ROW;
        for (int r = 0; r < LR_STATE_ROWS; ++r) S[r * LR_ROW + lane] = st_f64[wave][r * LR_ROW + lane];
        for (int r = 0; r < LR_ISTATE_ROWS; ++r) I[r * LR_ROW + lane] = st_i32[wave][r * LR_ROW + lane];
    }
    for (int i = tid; i < 2 * H * ENT; i += LR_P4_THREADS) {
        const int e = GENERAL ? lr_pairgen_lds_entry(i, H) : i;
        g0[i] = tab[0][e], g1[i] = tab[1][e];
    }
    // the last phase has scored pair 0's pending proposal: its sums for the next launch's first phase
    if (carry) {
        if (tid < 2 * NW) reinterpret_cast<double*>(carry)[tid] = (&red[0][0][0])[tid];
        if (tid == 0) *reinterpret_cast<int*>(carry + 2 * NW * 8) = 1;
    }
    LR_PSTAMP(5);      // state, tables and carried sums stored (issued: the stores drain behind the last instruction)
}

__global__ void lr_store_args_kernel(lr_step_args a, lr_step_args* dst) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *dst = a;
}

// log(br_length) once per engine (data constant used by models 0/1)
__global__ void lr_log_br_kernel(const double* __restrict__ br, int n_bins, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_bins) out[b] = (br && br[b] > 0.0) ? lr_log(br[b]) : 0.0;
}

// initial state (LRF:580-583 or the caller's runMCMC argument) -> state rows and the tables of
// the initial state (so that the first scan evaluates likA, LRF:224-226)
__global__ __launch_bounds__(LR_WAVE) void lr_chain_init_kernel(lr_step_args a, const double* L0, const double* M0,
                                                                const double* tL0, const double* tM0,
                                                                const int* KL0, const int* KM0, int kmax) {
    __shared__ lr_seg_scratch scratch;
    const lr_mcmc_config& cfg = a.cfg;
    const int c = blockIdx.x, lane = threadIdx.x, n_bins = cfg.n_bins;
    double* S = a.state_f64 + (size_t)c * LR_STATE_ROWS * LR_ROW;
    int* I = a.state_i32 + (size_t)c * LR_ISTATE_ROWS * LR_ROW;
    const lr_stream rng{(uint32_t)cfg.seed, (uint32_t)(cfg.chain_offset + c)};
    if (cfg.sampler != 0) {
        // initial parameter vector of the parametric samplers (DD:151-161, trend_rate.py:141-147) or the caller's
        // [C, kmax] rows; its tables, so that the first scan evaluates likA (DD:184-186)
        const bool trend = cfg.sampler == 2;
        const int npar = trend ? LR_TR_NPAR : LR_DD_NPAR;
        double A = 0.0;
        if (L0) {
            if (lane < npar) A = L0[(size_t)c * kmax + lane];
        } else if (trend) {
            const double init[LR_TR_NPAR] = {.1, .1, 0.0, 0.0, 1.0, 1.0};
            if (lane < npar) A = init[lane];
        } else {
            const double x0 = cfg.dd_present - (cfg.t0 + cfg.dd_present) / 2.0;       // PRESENT - np.mean([ORIGIN, PRESENT])
            const double init[LR_DD_NPAR] = {0.5, 1.5, x0, 10.0, 20000.0, cfg.dd_init_death, 1.0, 1.0};
            if (lane < npar) A = init[lane];
        }
        if (trend) {
            const lr_trend_params tp = lr_trend_unpack(A);
            const double* aux = a.br_length;
            lr_rates_build_tables_wave([&](int b, double* br, double* dr) { lr_trend_bin_rates(tp, aux[b], cfg.m_birth, cfg.m_death, br, dr); },
                                       n_bins, a.H, lr_chain_table(a, c), lane, a.unit, cfg.frac_birth, cfg.frac_death, lr_tab_es(a.unit, a.H));
        } else {
            const lr_dd_params pp = lr_dd_unpack(A);
            lr_dd_build_tables_wave(pp, a.br_length, cfg.m_birth, cfg.m_death, n_bins, a.H, lr_chain_table(a, c), lane,
                                    a.unit, cfg.frac_birth, cfg.frac_death, lr_tab_es(a.unit, a.H));
        }
        for (int r = 0; r < LR_STATE_ROWS; ++r) S[r * LR_ROW + lane] = 0.0;
        for (int r = 0; r < LR_ISTATE_ROWS; ++r) I[r * LR_ROW + lane] = 0;
        S[LR_ROW_L * LR_ROW + lane] = A, S[LR_ROW_PL * LR_ROW + lane] = A;
        int io = 0;
        if (lane == LR_I_KL || lane == LR_I_PKL || lane == LR_I_KM || lane == LR_I_PKM) io = npar;
        I[LR_IROW_SCALARS * LR_ROW + lane] = io;
        return;
    }
    double L = 0.0, M = 0.0, tL = 0.0, tM = 0.0;
    int KL = 1, KM = 1;
    if (L0) {
        KL = KL0[c], KM = KM0[c];
        if (lane < KL) L = L0[(size_t)c * kmax + lane];
        if (lane < KM) M = M0[(size_t)c * kmax + lane];
        if (lane <= KL) tL = tL0[(size_t)c * (kmax + 1) + lane];
        if (lane <= KM) tM = tM0[(size_t)c * (kmax + 1) + lane];
    } else {
        const double l0 = lr_gamma(rng, 0, LR_P_INIT, 0, 2.0) * 2.0;   // np.random.gamma(2,2,1), LRF:580
        const double m0 = lr_gamma(rng, 0, LR_P_INIT, 64, 2.0) * 2.0;  // LRF:581
        if (lane == 0) L = l0, M = m0, tL = tM = cfg.start_time;
        if (lane == 1) tL = tM = cfg.end_time;
    }
    // the initial index comes from get_rate_index on the RAW times: round, not floor (LRF:224-225, 129)
    const int eL = lr_wave_edges(tL, 1), eM = lr_wave_edges(tM, 1);
    double logL, logM;
    lr_stage_segments(&scratch, L, M, eL, eM, KL, KM, lane, &logL, &logM);
    const double constA = lr_build_tables_segments(&scratch, eL, eM, KL, KM, a.br_length, a.log_br, cfg.model, n_bins,
                                                   a.n_cls, a.H, lr_chain_table(a, c), lane,
                                                   a.unit, cfg.frac_birth, cfg.frac_death, lr_tab_es(a.unit, a.H));
    S[LR_ROW_L * LR_ROW + lane] = L, S[LR_ROW_M * LR_ROW + lane] = M;
    S[LR_ROW_TL * LR_ROW + lane] = tL, S[LR_ROW_TM * LR_ROW + lane] = tM;
    S[LR_ROW_PL * LR_ROW + lane] = L, S[LR_ROW_PM * LR_ROW + lane] = M;
    S[LR_ROW_PTL * LR_ROW + lane] = tL, S[LR_ROW_PTM * LR_ROW + lane] = tM;
    I[LR_IROW_EL * LR_ROW + lane] = eL, I[LR_IROW_EM * LR_ROW + lane] = eM;
    I[LR_IROW_PEL * LR_ROW + lane] = eL, I[LR_IROW_PEM * LR_ROW + lane] = eM;
    const double poi0 = (cfg.poisson_HP == 0.0) ? 1.0 : cfg.poisson_HP;             // LRF:220-221
    double so = 0.0;
    if (lane == LR_S_GRATE_L || lane == LR_S_GRATE_M) so = 1.0;                       // LRF:222 (log = 0)
    if (lane == LR_S_POI) so = poi0;
    if (lane == LR_S_LOG_POI) so = lr_log(poi0);
    if (lane == LR_S_CONST_A || lane == LR_S_CONST_P) so = constA;
    S[LR_ROW_SCALARS * LR_ROW + lane] = so;
    int io = 0;
    if (lane == LR_I_KL || lane == LR_I_PKL) io = KL;
    if (lane == LR_I_KM || lane == LR_I_PKM) io = KM;
    I[LR_IROW_SCALARS * LR_ROW + lane] = io;
}

// ---- host -------------------------------------------------------------------------------
extern "C" int lr_mcmc_query_layout(const lr_mcmc_config* cfg, lr_mcmc_layout* out) {
    lr_engine_plan plan;
    return lr_plan_layout(cfg, &plan, out);
}

extern "C" int lr_mcmc_create(const lr_mcmc_config* cfg, const double* ts, const double* te, const double* br_length,
                              void* workspace, int64_t workspace_bytes, lr_engine** out) {
    if (!ts || !te || !workspace || !out) return LR_ERR_NULL;
    lr_engine_plan plan;
    lr_mcmc_layout lay;
    int rc = lr_plan_layout(cfg, &plan, &lay);
    if (rc) return rc;
    if ((cfg->model == LR_MODEL_BD || cfg->model == LR_MODEL_ID || cfg->sampler != 0) && !br_length) return LR_ERR_MODEL;
    if (lay.total_bytes > workspace_bytes) return LR_ERR_WORKSPACE;
    lr_engine* e = new (std::nothrow) lr_engine();
    if (!e) return (int)hipErrorOutOfMemory;
    e->cfg = *cfg;
    e->lay = lay;
    e->plan = plan;
    e->ts = ts, e->te = te, e->br_length = br_length;
    e->ws = (char*)workspace;
    e->initialised = false;
    e->n8 = 0;                                          // groups of packed lineages: known once lr_pack_lineages has run
    e->n8_alloc = lr_groups_alloc(cfg->n_lineages);
    for (int j = 0; j < 16; ++j) e->p4.delta[j] = 0;
    e->p4.n_slots = 8;
    e->p4_help = lr_p4_help_choice(e);                  // (lr_mcmc_describe before init; latched again by lr_set_shares)
    e->p4_cfg = lr_p4_cfg_choice(e);
    e->p4_resident = lr_p4_resident_choice(e);
    e->p4_pipe = lr_p4_pipe_choice(e);
    e->p4_lean = lr_p4_lean_choice(e);
    e->streaming = false;
    e->packed_scan = plan.packed_scan;
    e->fork = nullptr;
    e->ev0 = e->ev1 = nullptr;
    for (int p = 0; p < plan.n_parts; ++p) {
        lr_part& q = e->part[p];
        q.base = plan.base[p], q.count = plan.base[p + 1] - plan.base[p], q.hA = plan.hA[p], q.pipelined = plan.pipelined[p];
        q.stream = nullptr, q.done = nullptr, q.graph_exec = nullptr, q.graph_units = 0;
    }
    {
        // the two timing events of lr_mcmc_time_steps / lr_mcmc_time_scan live as long as the engine: creating and
        // destroying them per call cost the host tens of microseconds inside every timed region
        hipError_t he = hipEventCreate(&e->ev0);
        if (he == hipSuccess) he = hipEventCreate(&e->ev1);
        if (he != hipSuccess) {
            lr_mcmc_destroy(e);
            return (int)he;
        }
    }
    // (a persistent kernel takes all chains in one launch: lr_mcmc_steps never reaches the partitions' schedule, and they get no streams)
    if (plan.family == 0 && plan.n_parts > 1) {
        hipError_t he = hipEventCreateWithFlags(&e->fork, hipEventDisableTiming);
        for (int p = 0; p < plan.n_parts && he == hipSuccess; ++p) {
            he = hipStreamCreateWithFlags(&e->part[p].stream, hipStreamNonBlocking);
            if (he == hipSuccess) he = hipEventCreateWithFlags(&e->part[p].done, hipEventDisableTiming);
        }
        if (he != hipSuccess) {
            lr_mcmc_destroy(e);
            return (int)he;
        }
    }
    if (plan.streaming) {
        // the resident kernel's blocks wait for each other: it runs only where the whole grid fits at once (LR_ERR_STATE =
        // it does not: the launches take over, same plan, same results)
        const int rcq = lr_launch_stream(e, lr_make_args(e), 0, true, nullptr);
        if (rcq != LR_OK && rcq != LR_ERR_STATE) {
            lr_mcmc_destroy(e);
            return rcq;
        }
        e->streaming = rcq == LR_OK;
    }
    *out = e;
    return LR_OK;
}

lr_step_args lr_make_args(const lr_engine* e) {
    lr_step_args a;
    a.cfg = e->cfg;
    a.state_f64 = (double*)(e->ws + e->lay.state_f64);
    a.state_i32 = (int*)(e->ws + e->lay.state_i32);
    a.log_br = (const double*)(e->ws + e->lay.bin_consts);
    a.dd_consts = a.log_br + e->cfg.n_bins;
    a.log_T = log(e->cfg.end_time - e->cfg.start_time);
    a.mult_l = 2.0 * log(LR_MULT_D);
    a.tables = (double2*)(e->ws + e->lay.tables);
    a.partials = (const double*)(e->ws + e->lay.partials);
    a.trace = (double*)(e->ws + e->lay.trace);
    a.br_length = e->br_length;
    a.tab_stride = e->plan.scan.tab_stride;
    a.n_cls = e->plan.scan.n_cls;
    a.tiles = e->plan.scan.tiles;
    a.H = e->plan.scan.H;
    a.unit = e->plan.scan.unit;
    a.cb = e->plan.scan.cb;
    a.warn = (unsigned int*)(e->ws + e->lay.status) + 1;
    return a;
}

template <int H>
static int lr_launch_pairscan(const lr_engine* e, hipStream_t stream) {
    lr_packed_lineages pk;
    pk.idx8 = (const uint4*)(e->ws + e->lay.lineage_idx), pk.frac = (const uint4*)(e->ws + e->lay.lineage_frac);
    pk.fstride = e->n8_alloc;
    const dim3 grid(e->plan.scan.tiles, (e->cfg.n_chains + 1) / 2);
    if (e->plan.scan.unit == LR_TAB_PAIRGEN)
        hipLaunchKernelGGL((lr_pairscan_kernel<H, true>), grid, dim3(256), 0, stream, pk, e->n8,
                           (const double2*)(e->ws + e->lay.tables), e->cfg.n_chains, e->cfg.n_bins, e->plan.scan.tiles, (double*)(e->ws + e->lay.partials));
    else
        hipLaunchKernelGGL((lr_pairscan_kernel<H, false>), grid, dim3(256), 0, stream, pk, e->n8,
                           (const double2*)(e->ws + e->lay.tables), e->cfg.n_chains, e->cfg.n_bins, e->plan.scan.tiles, (double*)(e->ws + e->lay.partials));
    return (int)hipGetLastError();
}

static int lr_enqueue_scan_range(const lr_engine* e, int base, int count, hipStream_t stream) {
    if (e->packed_scan) return lr_launch_packscan(e, base, count, stream);      // (never pipelined: a partition's chains in one launch)
    if (e->plan.pair_only) {
        // pair-general tables / the extant block of model 3: the launch-based twin of the persistent scan, all chains at once
        if (base != 0 || count != e->cfg.n_chains) return LR_ERR_STATE;
        switch (e->plan.scan.H) {
            case 40: return lr_launch_pairscan<40>(e, stream);
            case 72: return lr_launch_pairscan<72>(e, stream);
            case 136: return lr_launch_pairscan<136>(e, stream);
            case 264: return lr_launch_pairscan<264>(e, stream);
            default: return lr_launch_pairscan<LR_H_WIDE>(e, stream);
        }
    }
    return lr_launch_scan(e->plan.scan, e->ts, e->te, e->cfg.n_lineages, e->cfg.t0, e->cfg.n_bins, e->cfg.end_time,
                          (const double2*)(e->ws + e->lay.tables) + (size_t)base * e->plan.scan.tab_stride, count,
                          (double*)(e->ws + e->lay.partials) + (size_t)base * lr_tile_stride(e->plan.scan.tiles), lr_tile_stride(e->plan.scan.tiles), stream);
}
static int lr_enqueue_scan(const lr_engine* e, hipStream_t stream) {
    return lr_enqueue_scan_range(e, 0, e->cfg.n_chains, stream);
}
static int lr_enqueue_step_range(const lr_engine* e, const lr_step_args& a, int mode, int base, int count,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(lr_chain_step_kernel, dim3((count + LR_STEP_WAVES - 1) / LR_STEP_WAVES), dim3(LR_SCAN_THREADS),
                       0, stream, a, mode, base, count);
    return (int)hipGetLastError();
}

// DD sampler: PRIOR_K0_L = np.max(DT) (DD:45) and its logarithm, behind the n_bins entries of bin_consts
__global__ void lr_dd_consts_kernel(const double* __restrict__ DT, int n_bins, double* __restrict__ out) {
    const int lane = threadIdx.x;
    double m = -INFINITY;
    for (int b = lane; b < n_bins; b += LR_WAVE) m = fmax(m, DT[b]);
    m = -lr_wave_min(-m);
    if (lane == 0) out[0] = m, out[1] = lr_log(m);
}

// everything in the workspace that holds device addresses or derives from the data alone
static void lr_prepare_constants(const lr_engine* e, const lr_step_args& a, hipStream_t stream, bool restored) {
    // a fresh or restored run starts with a clear status word (a checkpoint never carries a void run on:
    // ChainEngine.save refuses to write one).  A fresh run clears the warning word behind it too; a restored one keeps
    // the checkpoint's: its trace still holds the rows of the iterations that raised LR_WARN_KCAP.
    if (restored) {
        (void)hipMemsetAsync(e->ws + e->lay.status, 0, 4, stream);
        (void)hipMemsetAsync(e->ws + e->lay.status + 8, 0, 248, stream);
    } else {
        (void)hipMemsetAsync(e->ws + e->lay.status, 0, 256, stream);
    }
    // ... and nothing carried over from the launches before it (four-chain kernel)
    if (e->plan.family == 2) (void)hipMemsetAsync(e->ws + e->lay.xchg, 0, (size_t)((e->cfg.n_chains + 3) / 4) * LR_P4_CARRY_BYTES, stream);
    hipLaunchKernelGGL(lr_log_br_kernel, dim3((e->cfg.n_bins + 127) / 128), dim3(128), 0, stream, e->br_length,
                       e->cfg.n_bins, (double*)(e->ws + e->lay.bin_consts));
    if (e->cfg.sampler == 1)
        hipLaunchKernelGGL(lr_dd_consts_kernel, dim3(1), dim3(LR_WAVE), 0, stream, e->br_length, e->cfg.n_bins,
                           (double*)(e->ws + e->lay.bin_consts) + e->cfg.n_bins);
    if (e->plan.family) {
        static_assert(sizeof(lr_step_args) <= 1024, "args blob too small");
        hipLaunchKernelGGL(lr_store_args_kernel, dim3(1), dim3(64), 0, stream, a, (lr_step_args*)(e->ws + e->lay.args_blob));
    }
}

// the launch-based engine's packed scan: (re)pack; an input the packing refuses (unsorted beyond LR_MAX_RUNS runs of one
// birth bin) falls back to the scan of ts / te - same plan, same partials, same results to rounding
// (general times have no such twin: their tables are the pair-general ones - the error is the caller's
static int lr_pack_for_scan(lr_engine* e, hipStream_t stream) {
    if (!e->plan.packed_scan) return LR_OK;
    const int rc = lr_pack_lineages(e, stream);
    e->packed_scan = rc == LR_OK;
    // (... nor has model 3 on these tables: the extant block is reached through the packed slots only)
    // (... nor the H = 520 class: the scans of ts / te are instantiated up to H = 264)
    return (rc != LR_OK && e->plan.pair_only) ? rc : LR_OK;
}

extern "C" int lr_mcmc_restore(lr_engine* e, void* stream_) {
    if (!e) return LR_ERR_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    const lr_step_args a = lr_make_args(e);
    lr_prepare_constants(e, a, stream, true);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    if (e->plan.family) rc = lr_pack_lineages(e, stream);
    if (rc) return rc;
    rc = lr_pack_for_scan(e, stream);
    if (rc) return rc;
    e->initialised = true;
    return LR_OK;
}

extern "C" int lr_mcmc_init(lr_engine* e, const double* L, const double* M, const double* tL, const double* tM,
                            const int32_t* KL, const int32_t* KM, int32_t kmax, void* stream_) {
    if (!e) return LR_ERR_NULL;
    if (L && e->cfg.sampler == 0 && (!M || !tL || !tM || !KL || !KM)) return LR_ERR_NULL;
    if (L && (kmax < 1 || kmax > LR_KMAX)) return LR_ERR_SIZE;
    if (L && e->cfg.sampler != 0 && kmax < LR_DD_NPAR) return LR_ERR_SIZE;
    hipStream_t stream = (hipStream_t)stream_;
    const lr_step_args a = lr_make_args(e);
    lr_prepare_constants(e, a, stream, false);
    if (e->plan.family) {
        const int rcp = lr_pack_lineages(e, stream);
        if (rcp) return rcp;
    }
    {
        const int rcp = lr_pack_for_scan(e, stream);
        if (rcp) return rcp;
    }
    hipLaunchKernelGGL(lr_chain_init_kernel, dim3(e->cfg.n_chains), dim3(LR_WAVE), 0, stream, a, L, M, tL, tM, KL, KM,
                       kmax);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    rc = lr_enqueue_scan(e, stream);
    if (rc) return rc;
    rc = lr_enqueue_step_range(e, a, 1, 0, e->cfg.n_chains, stream);
    if (rc) return rc;
    e->initialised = true;
    return LR_OK;
}

// iterations captured per hipGraph; LR_GRAPH_ITERS=0 in the environment disables graph replay
static int lr_graph_iters() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("LR_GRAPH_ITERS");
        v = e ? atoi(e) : 32;
        if (v < 0) v = 0;
        if (v > 4096) v = 4096;
    }
    return v;
}

// ---- software-pipelined schedule --------------------------------------------------------------
// Chains are split into halves A = [0, hA) and B = [hA, C).  A call of n iterations enqueues
//     scan(A);  (n-1) x { fused(scan B | step A); fused(scan A | step B) };  fused(scan B | step A);  step(B)
// so that every launch but the first and last overlaps the latency-bound chain step of one half with
// the throughput-bound lineage scan of the other.  LR_PIPELINE=0 falls back to scan; step; ...
template <int CB, int H, bool UNIT>
static int lr_launch_fused(const lr_engine* e, const lr_step_args& a, const lr_fused_args& f, hipStream_t stream) {
    const int groups = (f.scan_n + CB - 1) / CB;
    const int blocks = f.step_blocks + groups * f.tiles;
    const size_t lds_bytes = e->plan.scan.lds_bytes > (int)(LR_STEP_WAVES * sizeof(lr_seg_scratch)) ? (size_t)e->plan.scan.lds_bytes : LR_STEP_WAVES * sizeof(lr_seg_scratch);
    hipLaunchKernelGGL((lr_fused_iter_kernel<CB, H, UNIT>), dim3(blocks), dim3(LR_SCAN_THREADS), lds_bytes,
                       stream, a, f);
    return (int)hipGetLastError();
}

// instantiated shapes: see lr_fused_supported()
template <int H>
static int lr_launch_fused_h(const lr_engine* e, const lr_step_args& a, const lr_fused_args& f, hipStream_t stream) {
    if (e->plan.scan.unit) {
        switch (e->plan.scan.cb) {
            case 16: return lr_launch_fused<16, H, true>(e, a, f, stream);
            case 8: return lr_launch_fused<8, H, true>(e, a, f, stream);
            default: return LR_ERR_SIZE;
        }
    }
    switch (e->plan.scan.cb) {
        case 8: return lr_launch_fused<8, H, false>(e, a, f, stream);
        case 4: return lr_launch_fused<4, H, false>(e, a, f, stream);
        default: return LR_ERR_SIZE;
    }
}

// one fused launch: scan chains [scan_base, +scan_n), step chains [step_base, +step_n)
static int lr_enqueue_fused(const lr_engine* e, const lr_step_args& a, int scan_base, int scan_n, int step_base,
                            int step_n, hipStream_t stream) {
    lr_fused_args f;
    f.ts = e->ts, f.te = e->te, f.n = e->cfg.n_lineages, f.chunk = e->plan.scan.chunk, f.t0 = e->cfg.t0;
    f.n_bins = e->cfg.n_bins, f.tiles = e->plan.scan.tiles;
    f.scan_base = scan_base, f.scan_n = scan_n, f.step_base = step_base, f.step_n = step_n;
    f.step_blocks = (step_n + LR_STEP_WAVES - 1) / LR_STEP_WAVES;
    switch (e->plan.scan.H) {
        case 40: return lr_launch_fused_h<40>(e, a, f, stream);
        case 72: return lr_launch_fused_h<72>(e, a, f, stream);
        case 136: return lr_launch_fused_h<136>(e, a, f, stream);
        case 264: return lr_launch_fused_h<264>(e, a, f, stream);
        default: return LR_ERR_SIZE;
    }
}

// ---- schedule of one partition ------------------------------------------------------------------
// pipelined, n iterations:
//     scan(A);  (n-1) x { fused(scan B | step A); fused(scan A | step B) };  fused(scan B | step A);  step(B)
// every launch but the first and last overlaps the latency-bound chain step of one half with the
// throughput-bound lineage scan of the other.  Not pipelined: n x { scan; step }.
// The repeating unit {...} is captured once per partition in a hipGraph of LR_GRAPH_ITERS units.
static int lr_enqueue_unit(const lr_engine* e, const lr_step_args& a, const lr_part& q, hipStream_t stream) {
    if (!q.pipelined) {
        int rc = lr_enqueue_scan_range(e, q.base, q.count, stream);
        if (rc) return rc;
        return lr_enqueue_step_range(e, a, 0, q.base, q.count, stream);
    }
    int rc = lr_enqueue_fused(e, a, q.base + q.hA, q.count - q.hA, q.base, q.hA, stream);      // scan B | step A
    if (rc) return rc;
    return lr_enqueue_fused(e, a, q.base, q.hA, q.base + q.hA, q.count - q.hA, stream);       // scan A | step B
}

static int lr_run_units(lr_engine* e, const lr_step_args& a, lr_part& q, int64_t units, hipStream_t stream) {
    int64_t done = 0;
    const int G = lr_graph_iters();
    if (G > 0 && units >= G) {
        if (!q.graph_exec) {
            // capture G units once; the kernels read the iteration number from device memory, so the
            // same graph is valid for every replay
            hipStream_t cs = nullptr;
            hipGraph_t graph = nullptr;
            hipError_t he = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
            if (he != hipSuccess) return (int)he;
            int rc = LR_OK;
            he = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
            if (he == hipSuccess) {
                for (int i = 0; i < G && rc == LR_OK; ++i) rc = lr_enqueue_unit(e, a, q, cs);
                he = hipStreamEndCapture(cs, &graph);       // always ended, so that the stream leaves capture mode
            }
            if (he == hipSuccess && rc == LR_OK) he = hipGraphInstantiate(&q.graph_exec, graph, nullptr, nullptr, 0);
            // the capture stream and the graph are released on every path
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipStreamDestroy(cs);
            if (rc) return rc;
            if (he != hipSuccess) return (int)he;
            q.graph_units = G;
        }
        while (units - done >= q.graph_units) {
            hipError_t he = hipGraphLaunch(q.graph_exec, stream);
            if (he != hipSuccess) return (int)he;
            done += q.graph_units;
        }
    }
    for (; done < units; ++done) {
        const int rc = lr_enqueue_unit(e, a, q, stream);
        if (rc) return rc;
    }
    return LR_OK;
}

static int lr_run_part(lr_engine* e, const lr_step_args& a, lr_part& q, int64_t n_iters, hipStream_t stream) {
    if (!q.pipelined) return lr_run_units(e, a, q, n_iters, stream);
    // prologue: scan A alone (the fused kernel with no step blocks, so that the stand-alone scan kernel is
    // launched only at full size - by lr_mcmc_init and the lr_mcmc_time_scan measurement hook)
    int rc = lr_enqueue_fused(e, a, q.base, q.hA, q.base, 0, stream);                          // scan A
    if (rc) return rc;
    rc = lr_run_units(e, a, q, n_iters - 1, stream);
    if (rc) return rc;
    rc = lr_enqueue_fused(e, a, q.base + q.hA, q.count - q.hA, q.base, q.hA, stream);          // scan B | step A
    if (rc) return rc;
    return lr_enqueue_step_range(e, a, 0, q.base + q.hA, q.count - q.hA, stream);              // step B
}

extern "C" int lr_mcmc_steps(lr_engine* e, int64_t n_iters, void* stream_) {
    if (!e) return LR_ERR_NULL;
    if (!e->initialised) return LR_ERR_STATE;
    if (n_iters < 0) return LR_ERR_SIZE;
    if (n_iters == 0) return LR_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const lr_step_args a = lr_make_args(e);
    if (e->plan.family) {
        const uint4* idx8 = (const uint4*)(e->ws + e->lay.lineage_idx);
        const bool general = e->plan.scan.unit == LR_TAB_PAIRGEN;
        lr_packed_lineages pk;
        pk.idx8 = idx8, pk.frac = general ? (const uint4*)(e->ws + e->lay.lineage_frac) : nullptr, pk.fstride = e->n8_alloc;
        if (e->n8 <= 0) return LR_ERR_STATE;
        const lr_step_args* ap = (const lr_step_args*)(e->ws + e->lay.args_blob);
        const int blocks = (e->cfg.n_chains + 1) / 2;
        const bool p4 = e->plan.family == 2;
        const bool param = e->cfg.sampler != 0;
        static const int prio = lr_env_int("LR_PERSIST_PRIO", 12);   // clock bits per priority slice, 0 = off
        // one block per CU at most: give it the whole CU (16 waves on the one pair)
        const bool wide = e->plan.threads == 1024;   // (short scans keep 512: the 16-wave barrier costs more than it buys)
        if (e->plan.family == 3) return lr_launch_spec(e, a, pk, n_iters, stream);
        for (int64_t done = 0; done < n_iters;) {
            const int64_t n = (n_iters - done > 4096) ? 4096 : n_iters - done;   // keep single launches short
        static const int carry_env = lr_env_int("LR_P4_CARRY", 1);   // 0: every launch scans pair 0 again (A/B runs)
        char* p4_carry = (p4 && carry_env) ? e->ws + e->lay.xchg : nullptr;
#define LR_P_LAUNCH(HH)                                                                                                       \
    if (p4) {                                                                                                                 \
        const dim3 g4((e->cfg.n_chains + 3) / 4), b4(LR_P4_THREADS);                                                          \
        if (general && param) hipLaunchKernelGGL((lr_persist4_kernel<HH, true, true>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry);   \
        else if (general) hipLaunchKernelGGL((lr_persist4_kernel<HH, true, false>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry);      \
        else if (param) hipLaunchKernelGGL((lr_persist4_kernel<HH, false, true>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry);        \
        else if (LR_P4_NR > 0 && LR_P4_PIPE > 0 && e->p4_help && e->p4_resident && e->p4_pipe && e->p4_lean && e->p4_cfg == LR_P4_CFG_BDI)   /* (the lean draw duty: lr_p4_lean_choice) */ \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_BDI, LR_P4_NR, LR_P4_PIPE, true>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (LR_P4_NR > 0 && LR_P4_PIPE > 0 && e->p4_help && e->p4_resident && e->p4_pipe && e->p4_lean && e->p4_cfg == LR_P4_CFG_KEIDING)                                   \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_KEIDING, LR_P4_NR, LR_P4_PIPE, true>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (LR_P4_NR > 0 && LR_P4_PIPE > 0 && e->p4_help && e->p4_resident && e->p4_pipe && e->p4_lean)                                                                     \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_GENERIC, LR_P4_NR, LR_P4_PIPE, true>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (LR_P4_NR > 0 && LR_P4_PIPE > 0 && e->p4_help && e->p4_resident && e->p4_pipe && e->p4_cfg == LR_P4_CFG_BDI)   /* (resident trips as one block: lr_p4_pipe_choice) */ \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_BDI, LR_P4_NR, LR_P4_PIPE>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (LR_P4_NR > 0 && LR_P4_PIPE > 0 && e->p4_help && e->p4_resident && e->p4_pipe && e->p4_cfg == LR_P4_CFG_KEIDING)                                  \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_KEIDING, LR_P4_NR, LR_P4_PIPE>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (LR_P4_NR > 0 && LR_P4_PIPE > 0 && e->p4_help && e->p4_resident && e->p4_pipe)                                                                    \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_GENERIC, LR_P4_NR, LR_P4_PIPE>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (LR_P4_NR > 0 && e->p4_help && e->p4_resident && e->p4_cfg == LR_P4_CFG_BDI)   /* (resident groups: lr_p4_resident_choice) */ \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_BDI, LR_P4_NR>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (LR_P4_NR > 0 && e->p4_help && e->p4_resident && e->p4_cfg == LR_P4_CFG_KEIDING)                                              \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_KEIDING, LR_P4_NR>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (LR_P4_NR > 0 && e->p4_help && e->p4_resident)                                                                                \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_GENERIC, LR_P4_NR>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (e->p4_help && e->p4_cfg == LR_P4_CFG_BDI)      /* (helper waves: H <= 264, lr_p4_help_choice; the word: lr_p4_cfg_choice) */ \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_BDI>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (e->p4_help && e->p4_cfg == LR_P4_CFG_KEIDING)                                                                \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true, LR_P4_CFG_KEIDING>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else if (e->p4_help)                                                                                                  \
            hipLaunchKernelGGL((lr_persist4_kernel<(HH <= 264 ? HH : 264), false, false, true>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry); \
        else hipLaunchKernelGGL((lr_persist4_kernel<HH, false, false>), g4, b4, 0, stream, ap, pk, e->n8, e->p4, (long long)n, p4_carry);                  \
    } else if (wide) {                                                                                                        \
        hipLaunchKernelGGL((lr_persist_kernel<HH, 1024>), dim3(blocks), dim3(1024), 0, stream, ap, idx8, e->n8, e->p4, (long long)n, 0); \
    } else {                                                                                                                  \
        hipLaunchKernelGGL((lr_persist_kernel<HH, 512>), dim3(blocks), dim3(512), 0, stream, ap, idx8, e->n8, e->p4, (long long)n, prio); \
    }
            switch (e->plan.scan.H) {
                case 40: LR_P_LAUNCH(40); break;
                case 72: LR_P_LAUNCH(72); break;
                case 136: LR_P_LAUNCH(136); break;
                case 264: LR_P_LAUNCH(264); break;
                default: LR_P_LAUNCH(LR_H_WIDE); break;
            }
#undef LR_P_LAUNCH
            const int rc = (int)hipGetLastError();
            if (rc) return rc;
            done += n;
        }
        return LR_OK;
    }
    if (e->streaming) return lr_launch_stream(e, a, n_iters, false, stream);
    if (e->plan.n_parts == 1) return lr_run_part(e, a, e->part[0], n_iters, stream);
    // fork: every partition's stream waits for the caller's stream, runs its own sequence, and is joined back
    hipError_t he = hipEventRecord(e->fork, stream);
    if (he != hipSuccess) return (int)he;
    for (int p = 0; p < e->plan.n_parts; ++p) {
        lr_part& q = e->part[p];
        he = hipStreamWaitEvent(q.stream, e->fork, 0);
        if (he != hipSuccess) return (int)he;
        const int rc = lr_run_part(e, a, q, n_iters, q.stream);
        if (rc) return rc;
        he = hipEventRecord(q.done, q.stream);
        if (he != hipSuccess) return (int)he;
        he = hipStreamWaitEvent(stream, q.done, 0);
        if (he != hipSuccess) return (int)he;
    }
    return LR_OK;
}

extern "C" int lr_mcmc_time_steps(lr_engine* e, int64_t n_iters, float* total_ms, void* stream_) {
    if (!e || !total_ms) return LR_ERR_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    int rc = (int)hipEventRecord(e->ev0, stream);
    if (rc == LR_OK) rc = lr_mcmc_steps(e, n_iters, stream_);
    if (rc == LR_OK) rc = (int)hipEventRecord(e->ev1, stream);
    if (rc == LR_OK) rc = (int)hipEventSynchronize(e->ev1);
    float ms = 0.f;
    if (rc == LR_OK) rc = (int)hipEventElapsedTime(&ms, e->ev0, e->ev1);
    *total_ms = ms;
    return rc;
}

extern "C" int lr_mcmc_time_scan(lr_engine* e, int32_t reps, float* avg_ms, void* stream_) {
    if (!e || !avg_ms) return LR_ERR_NULL;
    if (!e->initialised) return LR_ERR_STATE;
    if (reps < 1) return LR_ERR_SIZE;
    hipStream_t stream = (hipStream_t)stream_;
    int rc = lr_enqueue_scan(e, stream);  // warm
    if (rc == LR_OK) rc = (int)hipEventRecord(e->ev0, stream);
    for (int i = 0; i < reps && rc == LR_OK; ++i) rc = lr_enqueue_scan(e, stream);
    if (rc == LR_OK) rc = (int)hipEventRecord(e->ev1, stream);
    if (rc == LR_OK) rc = (int)hipEventSynchronize(e->ev1);
    float ms = 0.f;
    if (rc == LR_OK) rc = (int)hipEventElapsedTime(&ms, e->ev0, e->ev1);
    *avg_ms = ms / reps;
    return rc;
}

extern "C" int lr_mcmc_status(lr_engine* e, int32_t* status, void* stream_) {
    if (!e || !status) return LR_ERR_NULL;
    unsigned int v = 0;
    hipError_t he = hipMemcpyAsync(&v, e->ws + e->lay.status, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream_);
    if (he == hipSuccess) he = hipStreamSynchronize((hipStream_t)stream_);
    *status = (int32_t)v;
    return (int)he;
}

extern "C" int lr_mcmc_warnings(lr_engine* e, int32_t* warnings, void* stream_) {
    if (!e || !warnings) return LR_ERR_NULL;
    unsigned int v = 0;
    hipError_t he = hipMemcpyAsync(&v, e->ws + e->lay.status + 4, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)stream_);
    if (he == hipSuccess) he = hipStreamSynchronize((hipStream_t)stream_);
    *warnings = (int32_t)v;
    return (int)he;
}

// configuration word of the four-chain kernel an engine runs (0 = the generic instantiation, or another kernel)
extern "C" int lr_mcmc_p4_config(const lr_engine* e, int32_t* word) {
    if (!e || !word) return LR_ERR_NULL;
    *word = (e->plan.family == 2 && e->p4_help) ? e->p4_cfg : LR_P4_CFG_GENERIC;
    return LR_OK;
}

// the four-chain kernel's resident scan groups in use (lr_resident_groups; all zero trips under LR_P4_RESIDENT=0 and for
// every other kernel): out = resident trips per scanner lane (waves 6..15; waves 4, 5 keep at most LR_P4_NR_DRAW), per helper
// lane, packed groups, the helpers' trips
extern "C" int lr_mcmc_p4_resident(const lr_engine* e, int32_t* out) {
    if (!e || !out) return LR_ERR_NULL;
    const bool help = e->plan.family == 2 && e->p4_help;
    const long long h = help ? e->p4.help_trips : 0;
    const long long k_tot = (e->n8 - h * 128 + 767) / 768;        // trips of the first scanner wave: the most any wave makes
    const bool on = help && e->p4_resident && LR_P4_NR > 0;
    out[0] = on ? (int32_t)(k_tot < LR_P4_NR ? k_tot : LR_P4_NR) : 0;
    out[1] = on ? (int32_t)(h < LR_P4_RES_HELP ? h : LR_P4_RES_HELP) : 0;
    out[2] = (int32_t)e->n8;
    out[3] = (int32_t)h;
    return LR_OK;
}

// the four-chain kernel's one-block form of the resident trips in use (lr_resident_trips_block; all zero under
// LR_P4_PIPE=0, without resident groups and for every other kernel): out = 1, and how many waves run all their resident
// trips and so take the block - of the ten scanner waves 6..15, of the two waves 4, 5 with the draw duty, of the two helper
// waves.  The counts are worked out HERE, on the host, the way lr_resident_load works out r.trips on the device, for the
// equal shares that the helper form has (lr_set_shares gives it no others: n8w = n8 - nh in the kernel); should that form
// ever get unequal shares (lr_p4_shares.delta), a wave's end is k_mine x 768 and this must follow.
extern "C" int lr_mcmc_p4_pipe(const lr_engine* e, int32_t* out) {
    if (!e || !out) return LR_ERR_NULL;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!(e->plan.family == 2 && e->p4_help && e->p4_resident && e->p4_pipe && LR_P4_NR > 0 && LR_P4_PIPE > 0)) return LR_OK;
    const long long h = e->p4.help_trips, n = e->n8 - h * 128;
    out[0] = 1;
    for (int q = 0; q < 12; ++q) {          // scanner wave 4 + q: the trips k with 64 q + 768 k < n (lr_resident_load)
        const long long mine = 64 * q < n ? (n - 64 * q + 767) / 768 : 0;
        if (q < 2) out[2] += mine >= LR_P4_NR_DRAW;
        else out[1] += mine >= LR_P4_NR;
    }
    out[3] = h >= LR_P4_RES_HELP ? 2 : 0;
    return LR_OK;
}

// the draw duty of the four-chain kernel's waves 4, 5 in use: out = 1 for the lean form (lr_spec_draw_lean), 0 for
// lr_spec_draw_both (LR_P4_LEAN_DRAWS=0, without the one-block form) and for every other kernel
extern "C" int lr_mcmc_p4_draws(const lr_engine* e, int32_t* out) {
    if (!e || !out) return LR_ERR_NULL;
    *out = (e->plan.family == 2 && e->p4_help && e->p4_resident && e->p4_pipe && e->p4_lean && LR_P4_NR > 0 && LR_P4_PIPE > 0) ? 1 : 0;
    return LR_OK;
}

// name of the kernel lr_mcmc_steps spends its time in, as rocprofv3's kernel trace prints it (without arguments; the
// four-chain kernel: without its configuration word, which lr_mcmc_p4_config tells)
extern "C" int lr_mcmc_describe(const lr_engine* e, char* buf, int32_t n) {
    if (!e || !buf) return LR_ERR_NULL;
    if (n < 64) return LR_ERR_SIZE;
    if (e->plan.family) {
        const char* gen = e->plan.scan.unit == LR_TAB_PAIRGEN ? "true" : "false";
        if (e->plan.family == 3)
            snprintf(buf, (size_t)n, "lr_spec_kernel<%d, %d, %s, %s, %d>", e->plan.scan.H, e->plan.threads, e->cfg.sampler == 0 ? "true" : "false", gen,
                     lr_spec_mode(e));
        else if (e->plan.family == 2)
            snprintf(buf, (size_t)n, "lr_persist4_kernel<%d, %s, %s, %s>", e->plan.scan.H, gen, e->cfg.sampler != 0 ? "true" : "false",
                     e->p4_help ? "true" : "false");
        else snprintf(buf, (size_t)n, "lr_persist_kernel<%d, %d>", e->plan.scan.H, e->plan.threads);
    } else if (e->packed_scan) {
        snprintf(buf, (size_t)n, "lr_packscan_kernel<%d, %d, %s>", lr_packscan_pairs(e->plan.scan, e->cfg.n_chains), e->plan.scan.H,
                 e->plan.scan.unit == LR_TAB_PAIRGEN ? "true" : "false");
    } else if (e->streaming) {
        snprintf(buf, (size_t)n, "lr_stream_kernel<%d, %d, %s>", e->plan.scan.cb, e->plan.scan.H, e->plan.scan.unit ? "true" : "false");
    } else if (e->part[0].pipelined) {
        snprintf(buf, (size_t)n, "lr_fused_iter_kernel<%d, %d, %s>", e->plan.scan.cb, e->plan.scan.H, e->plan.scan.unit ? "true" : "false");
    } else if (e->plan.scan.fast && !e->plan.scan.unit && e->plan.scan.cb == 16) {
        snprintf(buf, (size_t)n, "lr_scan_wide_kernel<%d>", e->plan.scan.H);
    } else if (e->plan.scan.fast) {
        snprintf(buf, (size_t)n, "%s<%d, %d>", e->plan.scan.unit ? "lr_scan_unit_kernel" : "lr_scan_fast_kernel", e->plan.scan.cb, e->plan.scan.H);
    } else {
        snprintf(buf, (size_t)n, "lr_scan_kernel<%d>", e->plan.scan.cb);
    }
    return LR_OK;
}

extern "C" int lr_mcmc_destroy(lr_engine* e) {
    if (!e) return LR_ERR_NULL;
    for (int p = 0; p < e->plan.n_parts; ++p) {
        lr_part& q = e->part[p];
        if (q.graph_exec) (void)hipGraphExecDestroy(q.graph_exec);
        if (q.done) (void)hipEventDestroy(q.done);
        if (q.stream) (void)hipStreamDestroy(q.stream);
    }
    if (e->fork) (void)hipEventDestroy(e->fork);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    delete e;
    return LR_OK;
}

#ifdef LR_DIAG
extern "C" int lr_diag_dump_step(unsigned long long* host_out, int n_words) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(lr_diag_step), (size_t)n_words * 8);
}
extern "C" int lr_diag_dump_seg(unsigned long long* host_out, int n_words, int reset) {
    int rc = (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(lr_diag_seg), (size_t)n_words * 8);
    if (reset) {
        static unsigned long long zeros[64 * 16];
        rc = (int)hipMemcpyToSymbol(HIP_SYMBOL(lr_diag_seg), zeros, sizeof(zeros));
    }
    return rc;
}
#endif
