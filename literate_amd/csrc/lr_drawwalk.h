// lr_drawwalk.h - a tile of lineages walked over posterior draws: what lr_waic.hip and lr_loo.hip share.
//
// lr_scan_kernel (lr_loglik.hip) sums lr_score_lineage's term over the lineages of a tile, per chain.  Here a block owns
// a tile of lineages and walks the DRAWS: a thread holds its lineages' times in registers (the index rule of
// lr_score_lineage depends on them alone, so the compiler keeps js / je / fs / fe and the table class out of the draw
// loop), the tables lr_build_tables_kernel made of a chunk of draws sit in LDS, and the next chunk travels from L2 into
// registers while the current one is scored.  Every (lineage, draw) is two 16-byte LDS gathers and the four fp64
// operations of the term; what becomes of the term is the caller's: lr_walk_draws hands it to a sink (WAIC folds it into
// running moments, PSIS-LOO stores it).  Each kernel instantiates the walk once, with its sink inlined.
//
//   the constants            one set of tuning values for both kernels
//   lr_draw_shape(_of)       the plan: table classes and the three LDS regimes;  lr_draw_slices: draws along grid.y
//   lr_walk_draws<Sink>      the walk, from the ts / te loads to the last barrier
//   lr_draw_begin            what both entry points do between their plan and their first launch
//   lr_block_sum / _max, lr_ordered_sum<N>   the fixed-order reductions of both units
#pragma once
#include "lr_device.h"
#include "lr_internal.h"

#define LR_DRAW_THREADS 256
#define LR_DRAW_LPT 2                                    /* lineages per thread */
#define LR_DRAW_TILE (LR_DRAW_THREADS * LR_DRAW_LPT)
#define LR_DRAW_PF 8                                     /* double2 per thread of the next chunk held in registers */
#define LR_DRAW_LDS_HALF (32 * 1024)                     /* one of the two chunk buffers when two blocks share a CU */
#define LR_DRAW_LDS_ONE (152 * 1024)                     /* both buffers of a block that has the CU to itself */
#define LR_DRAW_BLOCKS 512                               /* blocks aimed at: two per CU */

// ------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------
// block sum in a fixed order (lanes by the DPP scan, then the nw waves in ascending order); every thread gets it
__device__ __forceinline__ double lr_block_sum(double v, double* red, int tid, int nw) {
    const double w = lr_wave_sum(v);
    __syncthreads();
    if ((tid & (LR_WAVE - 1)) == 0) red[tid / LR_WAVE] = w;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < nw; ++k) t += red[k];
    return t;
}

__device__ __forceinline__ double lr_block_max(double v, double* red, int tid, int nw) {
    const double w = -lr_wave_min(-v);
    __syncthreads();
    if ((tid & (LR_WAVE - 1)) == 0) red[tid / LR_WAVE] = w;
    __syncthreads();
    double t = red[0];
    for (int k = 1; k < nw; ++k) t = fmax(t, red[k]);
    return t;
}

// the sum over the N = W * W threads of a block: the N values are added W by W in ascending order, the W sums by every
// thread in ascending order - the order of lr_reduce_partials_kernel.  red: N + W doubles.
template <int N>
__device__ __forceinline__ double lr_ordered_sum(double v, double* red, int j) {
    constexpr int W = N == 256 ? 16 : 32;
    static_assert(W * W == N, "lr_ordered_sum: 256 or 1024 threads");
    __syncthreads();
    red[j] = v;
    __syncthreads();
    if (j < W) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < W; ++q) t += red[j * W + q];
        red[N + j] = t;
    }
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < W; ++q) t += red[N + q];
    return t;
}

// The block's tile (slot k of thread tid is lineage first + k * LR_DRAW_THREADS + tid) against the draws [d0, d1):
// sink(k, d, l) once per lineage slot k and draw d with the term l, draws ascending, k inner.  A slot past n scores a
// lineage of its own (indices stay in the table); its sink calls are the sink's to ignore.  All threads of the block
// call; the dynamic LDS is the walk's.
template <class Sink>
__device__ __forceinline__ void lr_walk_draws(const double* __restrict__ ts, const double* __restrict__ te, long long n,
                                              long long first, double t0, int n_bins, int n_cls, int H, double end_time,
                                              const double2* __restrict__ tables, int tab_stride, int d0, int d1, int chunk,
                                              int nbuf, const Sink& sink) {
    extern __shared__ double2 lds[];
    const int tid = threadIdx.x;
    const double nb1 = (double)(n_bins + 1);

    double s[LR_DRAW_LPT], e[LR_DRAW_LPT];
#pragma unroll
    for (int k = 0; k < LR_DRAW_LPT; ++k) {
        const long long i = first + k * LR_DRAW_THREADS + tid;
        s[k] = i < n ? ts[i] : 0.0;
        e[k] = i < n ? te[i] : 0.0;
    }

    const int chunk_entries = chunk * tab_stride;
    {
        const double2* src = tables + (size_t)d0 * tab_stride;
        const int nent = min(chunk, d1 - d0) * tab_stride;
        for (int i = tid; i < nent; i += LR_DRAW_THREADS) lds[i] = src[i];
    }
    __syncthreads();
    int cur = 0;
    for (int dc = d0; dc < d1; dc += chunk) {
        const int nd = min(chunk, d1 - dc);
        const int nx = dc + chunk;
        const int nent = nx < d1 ? min(chunk, d1 - nx) * tab_stride : 0;
        const double2* nsrc = tables + (size_t)nx * tab_stride;
        // the next chunk's first LR_DRAW_PF * 256 entries (all of it when two blocks share a CU) travel while this one is scored
        double2 r[LR_DRAW_PF];
#pragma unroll
        for (int q = 0; q < LR_DRAW_PF; ++q) {
            const int idx = q * LR_DRAW_THREADS + tid;
            r[q] = idx < nent ? nsrc[idx] : make_double2(0.0, 0.0);
        }
        const double2* buf = lds + (size_t)cur * chunk_entries;
        for (int d = 0; d < nd; ++d) {
#pragma unroll
            for (int k = 0; k < LR_DRAW_LPT; ++k) {
                double acc[1] = {0.0};
                lr_score_lineage<1>(s[k], e[k], t0, nb1, H, n_cls, end_time, buf + (size_t)d * tab_stride, tab_stride, acc);
                sink(k, dc + d, acc[0]);
            }
        }
        if (nbuf == 1) __syncthreads();     // one buffer: everybody is done with it before it is overwritten
        double2* dst = lds + (size_t)(nbuf == 2 ? (cur ^ 1) : 0) * chunk_entries;
#pragma unroll
        for (int q = 0; q < LR_DRAW_PF; ++q) {
            const int idx = q * LR_DRAW_THREADS + tid;
            if (idx < nent) dst[idx] = r[q];
        }
        for (int idx = LR_DRAW_PF * LR_DRAW_THREADS + tid; idx < nent; idx += LR_DRAW_THREADS) dst[idx] = nsrc[idx];
        __syncthreads();
        if (nbuf == 2) cur ^= 1;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct lr_draw_shape {
    int n_cls, H, tab_stride;
    int chunk;      // draws per LDS buffer
    int nbuf;       // 2: the next chunk lands in the other buffer; 1: a table takes most of the LDS, one buffer
    size_t lds_bytes;
};

static inline int lr_draw_shape_of(long long n, int n_bins, int n_draws, int model, lr_draw_shape* p) {
    if (model != LR_MODEL_BD && model != LR_MODEL_KEIDING && model != LR_MODEL_KEIDING_DEAD) return LR_ERR_MODEL;
    lr_scan_plan sp;                                   // the bin counts lr_bd_loglik_batch accepts, by its own planner
    const int rc = lr_plan_scan(n, n_draws, n_bins, model, 0, &sp, 1);
    if (rc != LR_OK) return rc;
    p->n_cls = sp.n_cls;
    p->H = n_bins + 2;
    p->tab_stride = p->n_cls * 2 * p->H;
    const size_t per_draw = (size_t)p->tab_stride * sizeof(double2);
    if (per_draw <= LR_DRAW_LDS_HALF) {
        p->chunk = (int)(LR_DRAW_LDS_HALF / per_draw), p->nbuf = 2;
    } else if (2 * per_draw <= LR_DRAW_LDS_ONE) {
        p->chunk = 1, p->nbuf = 2;
    } else {
        if (per_draw > LR_DRAW_LDS_ONE) return LR_ERR_SIZE;
        p->chunk = 1, p->nbuf = 1;
    }
    p->lds_bytes = per_draw * p->chunk * p->nbuf;
    return LR_OK;
}

// few tiles: slices of draws along grid.y until two blocks per CU exist, each slice at least two chunks long (forced > 0:
// that many slices instead, within [1, min(n_draws, 65535)]); dps draws per slice
static inline void lr_draw_slices(long long tiles, int n_draws, int chunk, int forced, int* slices, int* dps) {
    int s = 1;
    if (tiles < LR_DRAW_BLOCKS) {
        s = (int)((LR_DRAW_BLOCKS + tiles - 1) / tiles);
        const int most = n_draws / (2 * chunk);
        if (s > most) s = most;
    }
    if (forced > 0) s = forced;
    if (s > n_draws) s = n_draws;
    if (s > 65535) s = 65535;
    if (s < 1) s = 1;
    *dps = (n_draws + s - 1) / s;
    *slices = (n_draws + *dps - 1) / *dps;
}

// What lr_waic_pointwise and lr_loo_pointwise do between their plan and their first launch of the walk, with the return
// codes in the ABI's order of precedence: br_length, t0, the workspace (ws_bytes of it are needed), then the tables and
// consts of all draws at their offsets in it and, above 64 KiB, the LDS attribute of `kernel`.
static inline int lr_draw_begin(const lr_draw_shape& p, int model, const double* br_length, double t0, size_t ws_bytes,
                                void* workspace, int64_t workspace_bytes, size_t o_tab, size_t o_cst, const double* lam_bins,
                                const double* mu_bins, int n_bins, int n_draws, const void* kernel, hipStream_t stream) {
    if (model == LR_MODEL_BD && !br_length) return LR_ERR_MODEL;
    if (t0 != floor(t0)) return LR_ERR_T0;
    if ((int64_t)ws_bytes > workspace_bytes) return LR_ERR_WORKSPACE;
    double2* tables = (double2*)((char*)workspace + o_tab);
    double* consts = (double*)((char*)workspace + o_cst);      // (zero under models 0, 2 and 3: nothing of the likelihood lies outside the lineages)
    const int rc = lr_launch_build_tables(lam_bins, mu_bins, br_length, model, n_bins, p.n_cls, p.H, p.tab_stride, n_draws,
                                          tables, consts, stream);
    if (rc) return rc;
    if (p.lds_bytes > 64 * 1024) {
        // (per call: the attribute belongs to the function on the CURRENT device, and a process may drive several)
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    return LR_OK;
}
