// lr_age.hip - posterior predictive deaths by age (lr_ppc_age, include/literate_hip_age.h): every lineage, born when the
// data say, is given a death time under every posterior draw of the per-bin death rates by inverting the draw's cumulative
// hazard at an exponential variate, and the simulated lifespans are counted per age class beside the observed ones.
//
//   lr_age_tables_kernel   one thread per draw: the cumulative hazard C_s[0 .. n_bins] by SEQUENTIAL additions (np.cumsum's
//                          order) into the workspace, and the draw's flag
//   lr_age_init_kernel     out_rep: 0 where the draw is good, -1 where it is flagged; the two draw totals
//   lr_age_kernel          grid (tiles, slices): a block owns a tile of lineages (more than 2^31 - 1 tiles: several),
//                          whose (x, jb, fs, censor class) stay in registers, and walks the draws of its slice a chunk
//                          at a time: the chunk's C tables and rates in LDS, one [2, A] histogram of 32-bit LDS counters
//                          per draw of the chunk, flushed per chunk into out_rep with 64-bit integer atomics.  The blocks
//                          of slice 0 also count the data (out_obs, the two lineage totals).
//
// A pair (lineage i, draw s) is one Philox block (counter (i, LR_P_PPC_AGE, s)), one lr_log, an upper_bound over C_s from
// the birth bin (C_s is non-decreasing: sequential sums of non-negative rates), one division and one LDS atomic.  Every
// product, sum and quotient the definition rounds on its own is rounded on its own here (__dmul_rn / __dadd_rn /
// __ddiv_rn: hipcc contracts a * b + c into an FMA by default).
//
// All outputs are integers reached by integer atomics only: they depend on the arguments alone, not on the plan, the grid
// or the schedule.  No 32-bit counter can overflow: a block adds at most LR_AGE_TILE lineages to the counters of a draw.
#include <climits>
#include <cmath>
#include <cstdlib>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_age.h"
#include "lr_device.h"
#include "lr_internal.h"

#define LR_P_PPC_AGE 41                                  /* (lr_prior.hip holds 40) */
#define LR_AGE_THREADS 256
#define LR_AGE_LPT 4                                     /* lineages per thread */
#define LR_AGE_TILE (LR_AGE_THREADS * LR_AGE_LPT)
#define LR_AGE_LDS (32 * 1024)                           /* a chunk of draws takes at most this much LDS, or one draw */
#define LR_AGE_CHUNK_MAX 64
#define LR_AGE_BLOCKS 512                                /* blocks aimed at: two per CU */

struct lr_age_shape {
    int chunk;      // draws per LDS chunk
    int slices;     // draw slices (grid.y)
    int dps;        // draws per slice
    long long tiles;    // lineage tiles (grid.x, as far as a grid goes)
    size_t lds_bytes;
};

// ------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------
// C[s * (n_bins + 1) + b] = mu[s, 0] + ... + mu[s, b - 1], added one after the other; flag[s] = 1 when a rate is not
// finite or negative, or the total is not finite
__global__ __launch_bounds__(LR_AGE_THREADS) void lr_age_tables_kernel(const double* __restrict__ mu_bins, int n_bins,
                                                                       int n_draws, double* __restrict__ C,
                                                                       int* __restrict__ flag) {
    const int s = blockIdx.x * LR_AGE_THREADS + threadIdx.x;
    if (s >= n_draws) return;
    const double* mu = mu_bins + (size_t)s * n_bins;
    double* c = C + (size_t)s * (n_bins + 1);
    double cum = 0.0;
    int bad = 0;
    c[0] = 0.0;
    for (int b = 0; b < n_bins; ++b) {
        const double m = mu[b];
        bad |= !(m >= 0.0) || !(m < __builtin_inf());
        cum = __dadd_rn(cum, m);
        c[b + 1] = cum;
    }
    bad |= !(fabs(cum) < __builtin_inf());
    flag[s] = bad;
}

// out_rep[s][.][.] = flag[s] ? -1 : 0; totals[2] += good draws, totals[3] += flagged draws (totals zeroed before)
__global__ __launch_bounds__(LR_AGE_THREADS) void lr_age_init_kernel(const int* __restrict__ flag, int n_draws, int two_a,
                                                                     long long* __restrict__ out_rep,
                                                                     long long* __restrict__ totals) {
    __shared__ int s_cnt[2];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long total = (long long)n_draws * two_a, stride = (long long)gridDim.x * LR_AGE_THREADS;
    for (long long e = (long long)blockIdx.x * LR_AGE_THREADS + threadIdx.x; e < total; e += stride) {
        const int s = (int)(e / two_a);
        const int f = flag[s];
        out_rep[e] = f ? -1ll : 0ll;
        if (e == (long long)s * two_a) atomicAdd(&s_cnt[f ? 1 : 0], 1);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x])
        atomicAdd((unsigned long long*)(totals + 2 + threadIdx.x), (unsigned long long)s_cnt[threadIdx.x]);
}

// cnt[0 .. n_cnt) into dst[0 .. n_cnt), zeros skipped; all threads of the block call, between barriers of the caller
__device__ __forceinline__ void lr_age_flush(const int* cnt, int n_cnt, long long* __restrict__ dst) {
    for (int i = threadIdx.x; i < n_cnt; i += LR_AGE_THREADS) {
        const int v = cnt[i];
        if (v) atomicAdd((unsigned long long*)(dst + i), (unsigned long long)v);
    }
}

// dynamic LDS: [chunk (n_bins + 1) doubles: C | chunk n_bins doubles: mu | chunk 2A + 2 ints: counters]
__global__ __launch_bounds__(LR_AGE_THREADS) void lr_age_kernel(
    const double* __restrict__ ts, const double* __restrict__ te, long long n, long long tiles, double t0, double t_end,
    int n_bins, const double* __restrict__ mu_bins, const double* __restrict__ C, const int* __restrict__ flag,
    int n_draws, int chunk, int dps, uint32_t k0, uint32_t k1, long long* __restrict__ out_obs,
    long long* __restrict__ out_rep, long long* __restrict__ out_totals) {
    extern __shared__ double2 lds_raw[];
    const int tid = threadIdx.x, A = n_bins, H = n_bins + 1;
    double* s_C = reinterpret_cast<double*>(lds_raw);
    double* s_mu = s_C + (size_t)chunk * H;
    int* s_cnt = reinterpret_cast<int*>(s_mu + (size_t)chunk * n_bins);
    const int n_cnt = chunk * 2 * A;
    const int d0 = blockIdx.y * dps, d1 = min(d0 + dps, n_draws);
    const double nb = (double)n_bins;
    const lr_stream stream{k0, k1};

    // (one tile per block, unless there are more tiles than a grid holds blocks; the trip count is the block's)
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long first = tile * LR_AGE_TILE;
        // the tile, from the data alone
        double x[LR_AGE_LPT], fs[LR_AGE_LPT];
        int jb[LR_AGE_LPT], cc[LR_AGE_LPT];     // birth bin (-1: not used), censor class
        int oc[LR_AGE_LPT];                      // observed class, + A when censored; -1: in no tile; -2: not used
#pragma unroll
        for (int k = 0; k < LR_AGE_LPT; ++k) {
            const long long i = first + k * LR_AGE_THREADS + tid;
            jb[k] = -1, cc[k] = 0, oc[k] = -1, x[k] = 0.0, fs[k] = 0.0;
            if (i < n) {
                const double s = ts[i], e = te[i];
                const double xx = __dadd_rn(s, -t0);
                oc[k] = -2;
                if (xx >= 0.0 && xx < nb && e > s) {
                    const double fl = floor(xx);
                    x[k] = xx, jb[k] = (int)fl, fs[k] = __dadd_rn(xx, -fl);
                    const bool dead = e <= t_end;
                    const double life = floor(__dadd_rn(dead ? e : t_end, -s));
                    const double cens = floor(__dadd_rn(t_end, -s));
                    cc[k] = (int)fmin(fmax(cens, 0.0), nb - 1.0);
                    oc[k] = (int)fmin(fmax(life, 0.0), nb - 1.0) + (dead ? 0 : A);
                }
            }
        }

        if (blockIdx.y == 0) {
            // the data's own histogram and the two lineage totals: counters [2A] and, behind all draws' counters, [2]
            for (int i = tid; i < 2 * A; i += LR_AGE_THREADS) s_cnt[i] = 0;
            if (tid < 2) s_cnt[n_cnt + tid] = 0;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < LR_AGE_LPT; ++k) {
                if (oc[k] >= 0) atomicAdd(&s_cnt[oc[k]], 1), atomicAdd(&s_cnt[n_cnt], 1);
                else if (oc[k] == -2) atomicAdd(&s_cnt[n_cnt + 1], 1);
            }
            __syncthreads();
            lr_age_flush(s_cnt, 2 * A, out_obs);
            lr_age_flush(s_cnt + n_cnt, 2, out_totals);
            __syncthreads();
        }

        for (int dc = d0; dc < d1; dc += chunk) {
            const int nd = min(chunk, d1 - dc);
            {
                const double* srcC = C + (size_t)dc * H;
                const double* srcM = mu_bins + (size_t)dc * n_bins;
                for (int i = tid; i < nd * H; i += LR_AGE_THREADS) s_C[i] = srcC[i];
                for (int i = tid; i < nd * n_bins; i += LR_AGE_THREADS) s_mu[i] = srcM[i];
                for (int i = tid; i < nd * 2 * A; i += LR_AGE_THREADS) s_cnt[i] = 0;
            }
            __syncthreads();
            for (int q = 0; q < nd; ++q) {
                const int d = dc + q;
                if (flag[d]) continue;                              // (the same for every thread)
                const double* c = s_C + (size_t)q * H;
                const double* m = s_mu + (size_t)q * n_bins;
                int* cnt = s_cnt + (size_t)q * 2 * A;
#pragma unroll
                for (int k = 0; k < LR_AGE_LPT; ++k) {
                    if (jb[k] < 0) continue;
                    const unsigned long long i = (unsigned long long)(first + k * LR_AGE_THREADS + tid);
                    const double u = lr_pair(stream, i, LR_P_PPC_AGE, (uint32_t)d).a;
                    const double E = -lr_log(1.0 - u);
                    const double target = __dadd_rn(__dadd_rn(c[jb[k]], __dmul_rn(m[jb[k]], fs[k])), E);
                    // the smallest b in [jb, n_bins) with C[b + 1] > target (n_bins: none)
                    int lo = jb[k], hi = n_bins;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (c[mid + 1] > target) hi = mid;
                        else lo = mid + 1;
                    }
                    int slot = A + cc[k];
                    if (lo < n_bins) {
                        const double t_in = __ddiv_rn(__dadd_rn(target, -c[lo]), m[lo]);
                        const double life = __dadd_rn(__dadd_rn((double)lo, t_in), -x[k]);
                        slot = (int)fmin(fmax(floor(life), 0.0), nb - 1.0);
                    }
                    atomicAdd(&cnt[slot], 1);
                }
            }
            __syncthreads();
            lr_age_flush(s_cnt, nd * 2 * A, out_rep + (size_t)dc * 2 * A);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int lr_age_shape_of(long long n, int n_bins, int n_draws, lr_age_shape* p) {
    if (n < 1 || n_draws < 1 || n_bins < 1 || n_bins > LR_MAX_BINS) return LR_ERR_SIZE;
    if (n > ((1ll << 62) - 1) / n_draws) return LR_ERR_SIZE;
    const long long tiles = (n + LR_AGE_TILE - 1) / LR_AGE_TILE;
    p->tiles = tiles;
    const size_t per_draw = (size_t)(2 * n_bins + 1) * sizeof(double) + (size_t)2 * n_bins * sizeof(int);
    int chunk = (int)(LR_AGE_LDS / per_draw);
    if (chunk > LR_AGE_CHUNK_MAX) chunk = LR_AGE_CHUNK_MAX;
    if (chunk > n_draws) chunk = n_draws;
    if (chunk < 1) chunk = 1;
    p->chunk = chunk;
    p->lds_bytes = (size_t)lr_align_up64((long long)(per_draw * chunk + 2 * sizeof(int)), 16);
    // few tiles: slices of draws along grid.y until two blocks per CU exist, each slice at least a chunk long
    int s = 1;
    if (tiles < LR_AGE_BLOCKS) {
        s = (int)((LR_AGE_BLOCKS + tiles - 1) / tiles);
        const int most = n_draws / chunk;
        if (s > most) s = most;
    }
    const char* env = getenv("LR_PPC_AGE_SLICES");
    const int forced = env ? atoi(env) : 0;
    if (forced > 0) s = forced;
    if (s > n_draws) s = n_draws;
    if (s > 65535) s = 65535;
    if (s < 1) s = 1;
    p->dps = (n_draws + s - 1) / s;
    p->slices = (n_draws + p->dps - 1) / p->dps;
    return LR_OK;
}

// workspace: [C tables | flags], each 256-byte aligned
static void lr_age_ws(int n_bins, int n_draws, size_t* o_C, size_t* o_flag, size_t* total) {
    size_t o = 0;
    *o_C = o, o += lr_align_up64((long long)n_draws * (n_bins + 1) * sizeof(double), 256);
    *o_flag = o, o += lr_align_up64((long long)n_draws * sizeof(int), 256);
    *total = o;
}

extern "C" int64_t lr_ppc_age_workspace_bytes(int64_t n, int32_t n_bins, int32_t n_draws) {
    lr_age_shape p;
    const int rc = lr_age_shape_of(n, n_bins, n_draws, &p);
    if (rc != LR_OK) return rc;
    size_t a, b, total;
    lr_age_ws(n_bins, n_draws, &a, &b, &total);
    return (int64_t)total;
}

extern "C" int lr_ppc_age_plan(int64_t n, int32_t n_bins, int32_t n_draws, int32_t* out) {
    if (!out) return LR_ERR_NULL;
    lr_age_shape p;
    const int rc = lr_age_shape_of(n, n_bins, n_draws, &p);
    if (rc != LR_OK) return rc;
    out[0] = LR_AGE_TILE, out[1] = p.dps, out[2] = p.slices, out[3] = (int32_t)(p.tiles < INT_MAX ? p.tiles : INT_MAX);
    return LR_OK;
}

extern "C" int lr_ppc_age(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins, const double* mu_bins,
                          int32_t n_draws, uint64_t seed, int64_t* out_obs, int64_t* out_rep, int64_t* out_totals,
                          void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!ts || !te || !mu_bins || !out_obs || !out_rep || !out_totals || !workspace) return LR_ERR_NULL;
    lr_age_shape p;
    int rc = lr_age_shape_of(n, n_bins, n_draws, &p);
    if (rc != LR_OK) return rc;
    if (!std::isfinite(t0) || t0 != std::floor(t0)) return LR_ERR_T0;
    size_t o_C, o_flag, total;
    lr_age_ws(n_bins, n_draws, &o_C, &o_flag, &total);
    if ((int64_t)total > workspace_bytes) return LR_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    double* C = (double*)((char*)workspace + o_C);
    int* flag = (int*)((char*)workspace + o_flag);
    const int two_a = 2 * n_bins;
    if (p.lds_bytes > 64 * 1024) {
        // (per call: the attribute belongs to the function on the CURRENT device, and a process may drive several)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&lr_age_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipError_t e = hipMemsetAsync(out_totals, 0, 4 * sizeof(int64_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(out_obs, 0, (size_t)two_a * sizeof(int64_t), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lr_age_tables_kernel, dim3((n_draws + LR_AGE_THREADS - 1) / LR_AGE_THREADS), dim3(LR_AGE_THREADS), 0,
                       stream, mu_bins, n_bins, n_draws, C, flag);
    rc = (int)hipGetLastError();
    if (rc) return rc;
    const long long cells = (long long)n_draws * two_a;
    const long long want = (cells + LR_AGE_THREADS - 1) / LR_AGE_THREADS;
    hipLaunchKernelGGL(lr_age_init_kernel, dim3((unsigned)(want < (1 << 20) ? want : (1 << 20))), dim3(LR_AGE_THREADS), 0,
                       stream, flag, n_draws, two_a, (long long*)out_rep, (long long*)out_totals);
    rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(lr_age_kernel, dim3((unsigned)(p.tiles < INT_MAX ? p.tiles : INT_MAX), p.slices),
                       dim3(LR_AGE_THREADS), p.lds_bytes, stream, ts, te, (long long)n, p.tiles, t0, t0 + (double)n_bins,
                       n_bins, mu_bins, (const double*)C, (const int*)flag, n_draws, p.chunk, p.dps, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (long long*)out_obs, (long long*)out_rep, (long long*)out_totals);
    return (int)hipGetLastError();
}
