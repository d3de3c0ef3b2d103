// lr_loo.hip - PSIS-LOO over posterior draws: Pareto-smoothed importance-sampling leave-one-out cross-validation
// (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry, "Pareto smoothed importance sampling"; the
// generalized-Pareto fit of Zhang & Stephens 2009 as loo::gpdfit does it).
//
// WAIC (lr_waic.hip) needs running moments over a lineage's draws and never stores a term.  PSIS needs ORDER statistics:
// the M largest importance ratios of every lineage in sorted order.  So the work is two stages per batch of lineages:
//
//   lr_loo_terms_kernel   the walk WAIC takes (lr_walk_draws, csrc/lr_drawwalk.h: a tile of lineages, the draws' tables
//                         through LDS), but the term is STORED: a batch of B lineages gives a [B, S] row-major
//                         slab in the workspace (at most 64 MiB; the host loops over the batches); grid.y slices the
//                         draws, since a batch alone is too few tiles to fill the device
//   lr_psis_rows_kernel   one workgroup per row: the row's S terms go to LDS as keys r = -l with their draw indices, a
//                         bitonic network over S padded to a power of two sorts them ascending by (r, draw), the top M are
//                         the tail and the one below them the cutoff; the fit is m x M log1p evaluations (one wave per
//                         grid point, lanes over the tail), then the smoothed tail and the two logsumexp passes run over
//                         the SORTED row in LDS (every output is a symmetric function of the draws, so nothing is unsorted)
//   lr_loo_totals_kernel  one block over the pointwise outputs in a fixed order
//
// The network is a fixed sequence of compare-exchanges and equal keys are ordered by draw index, every sum runs lanes,
// then waves in ascending order, and the plan is a function of the sizes alone: results are bitwise reproducible, and a
// row's outputs depend on nothing but the row.
//
// LDS.  A row at the cap (8192 draws) is 64 KiB of keys and 16 KiB of 16-bit draw indices: one workgroup per CU there;
// at 1000 draws (1024 slots, 10 KiB) eight workgroups of 256 threads share a CU.  Keys are 8 bytes wide, so a
// compare-exchange distance j >= 32 elements reads consecutive elements per lane (conflict-free ds_read_b64); the last five
// distances of every merge (j = 16 ... 1) put two lanes of a half-wave on one bank pair (2-way).
#include <climits>
#include <cstdlib>

#include "lr_drawwalk.h"

#define LR_LOO_SLAB_BYTES (64ll * 1024 * 1024)
#define LR_LOO_MAX_DRAWS 8192
#define LR_PSIS_MAX_THREADS 256
#define LR_PSIS_MAX_TAIL 272                             /* ceil(3 sqrt(8192)) */
#define LR_PSIS_MAX_GRID 64                              /* 30 + floor(sqrt(272)) = 46 grid points, one lane each */
#define LR_LOO_TOT_THREADS 1024

struct lr_loo_shape {
    lr_draw_shape w;
    long long batch;     // lineages per batch
    int batches;
};

struct lr_psis_shape {
    int P;               // slots: n_draws padded to a power of two (at least 2)
    int M;               // tail length
    int m;               // grid points of the fit (0: no fit)
    int threads;
    size_t lds_bytes;
};

// ------------------------------------------------------------------------------------------
// stage 1: the terms
// ------------------------------------------------------------------------------------------
// the walk's sink: row[k] is lineage slot k's row of the slab (null past the end)
struct lr_loo_sink {
    double* row[LR_DRAW_LPT];
    __device__ __forceinline__ void operator()(int k, int d, double l) const {
        if (row[k]) row[k][d] = l;
    }
};

__global__ __launch_bounds__(LR_DRAW_THREADS) void lr_loo_terms_kernel(
    const double* __restrict__ ts, const double* __restrict__ te, long long n, double t0, int n_bins, int n_cls, int H,
    double end_time, const double2* __restrict__ tables, int tab_stride, int n_draws, int chunk, int nbuf, int dps,
    double* __restrict__ slab) {
    const long long first = (long long)blockIdx.x * LR_DRAW_TILE;
    const int d0 = blockIdx.y * dps, d1 = min(d0 + dps, n_draws);     // this block's slice of the draws (no state crosses draws)
    lr_loo_sink sink;
#pragma unroll
    for (int k = 0; k < LR_DRAW_LPT; ++k) {
        const long long i = first + k * LR_DRAW_THREADS + threadIdx.x;
        sink.row[k] = i < n ? slab + (size_t)i * (size_t)n_draws : nullptr;
    }
    lr_walk_draws(ts, te, n, first, t0, n_bins, n_cls, H, end_time, tables, tab_stride, d0, d1, chunk, nbuf, sink);
}

// ------------------------------------------------------------------------------------------
// stage 2: one row per workgroup
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lr_psis_finite(double v) { return fabs(v) < __builtin_inf(); }

// out_pointwise[4 row ...] = elpd_loo, pareto_k, lppd, n_eff; tails (may be null): [n_rows, M] draw indices of the tail in
// its sorted order (-1 in a flagged row)
__global__ __launch_bounds__(LR_PSIS_MAX_THREADS) void lr_psis_rows_kernel(const double* __restrict__ loglik, int n_draws,
                                                                           int P, int M, int m,
                                                                           double* __restrict__ out_pointwise,
                                                                           int* __restrict__ tails) {
    extern __shared__ double keys[];                     // [P] keys, then [P] 16-bit draw indices
    __shared__ double x[LR_PSIS_MAX_TAIL];               // the tail values, later the tail's smoothed log weights
    __shared__ double th[LR_PSIS_MAX_GRID], el[LR_PSIS_MAX_GRID];
    __shared__ double red[LR_PSIS_MAX_THREADS / LR_WAVE];
    __shared__ double fit[2];
    unsigned short* idx = (unsigned short*)(keys + P);
    const int tid = threadIdx.x, T = blockDim.x, nw = T / LR_WAVE, lane = tid & (LR_WAVE - 1), wave = tid / LR_WAVE;
    const size_t rowi = blockIdx.x;
    const double* src = loglik + rowi * (size_t)n_draws;
    double* out = out_pointwise + 4 * rowi;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const int S = n_draws, lo = P - S, t_at = P - M;     // real entries sit at [lo, P) after the sort, the tail at [t_at, P)

    int bad = 0;
    for (int s = tid; s < P; s += T) {
        double v = -inf;                                 // the padding sorts below every finite key
        if (s < S) {
            const double l = src[s];
            bad |= !lr_psis_finite(l);
            v = -l;
        }
        keys[s] = v;
        idx[s] = (unsigned short)s;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) out[0] = nan, out[1] = nan, out[2] = nan, out[3] = nan;
        if (tails)
            for (int j = tid; j < M; j += T) tails[rowi * (size_t)M + j] = -1;
        return;
    }

    // ascending by (key, draw index): the bitonic network
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += T) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int b = a | j;
                const double ka = keys[a], kb = keys[b];
                const unsigned short ia = idx[a], ib = idx[b];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == ((a & k) == 0)) {
                    keys[a] = kb, keys[b] = ka;
                    idx[a] = ib, idx[b] = ia;
                }
            }
            __syncthreads();
        }
    }
    if (tails)
        for (int j = tid; j < M; j += T) tails[rowi * (size_t)M + j] = (int)idx[t_at + j];

    const double rmax = keys[P - 1], rmin = keys[lo];
    // lppd = max l + log(1/S sum exp(l - max l)), max l = -rmin
    double acc = 0.0;
    for (int s = lo + tid; s < P; s += T) acc += exp(rmin - keys[s]);
    const double lppd = -rmin + log(lr_block_sum(acc, red, tid, nw) / (double)S);

    const double c = keys[t_at - 1];                     // the largest r not in the tail (M = 0: rmax itself)
    const double ec = exp(c - rmax);
    double k_rep = inf;
    bool smoothed = false;
    if (M >= 5 && keys[P - 1] != keys[t_at]) {
        for (int j = tid; j < M; j += T) x[j] = exp(keys[t_at + j] - rmax) - ec;
        __syncthreads();
        const double dM = (double)M;
        const double xM = x[M - 1], xq = x[(int)floor(dM / 4.0 + 0.5) - 1];
        for (int jj = wave; jj < m; jj += nw) {          // a wave per grid point, its lanes over the tail
            const double theta = 1.0 / xM + (1.0 - sqrt((double)m / ((double)jj + 0.5))) / (3.0 * xq);
            double p = 0.0;
            for (int i = lane; i < M; i += LR_WAVE) p += log1p(-theta * x[i]);
            const double kj = lr_wave_sum(p) / dM;
            if (lane == 0) th[jj] = theta, el[jj] = dM * (log(-theta / kj) - kj - 1.0);
        }
        __syncthreads();
        if (wave == 0) {
            double contrib = 0.0;
            if (lane < m) {
                const double me = el[lane];
                double ssum = 0.0;
                for (int i = 0; i < m; ++i) ssum += exp(el[i] - me);
                contrib = th[lane] * (1.0 / ssum);
            }
            const double theta_hat = lr_wave_sum(contrib);
            double p = 0.0;
            for (int i = lane; i < M; i += LR_WAVE) p += log1p(-theta_hat * x[i]);
            const double kh = lr_wave_sum(p) / dM;
            if (lane == 0) fit[0] = kh, fit[1] = -kh / theta_hat;
        }
        __syncthreads();
        const double kh = fit[0], sigma = fit[1];
        smoothed = lr_psis_finite(kh) && lr_psis_finite(sigma);
        if (smoothed) {
            k_rep = (dM * kh + 5.0) / (dM + 10.0);
            for (int j = tid; j < M; j += T) {
                const double lp = log1p(-((double)j + 0.5) / dM);
                const double q = kh == 0.0 ? -sigma * lp : sigma * expm1(-kh * lp) / kh;
                x[j] = fmin(log(q + ec), 0.0);
            }
        }
        __syncthreads();
    }

    // lw: the tail's smoothed log weights in its sorted order, r - rmax elsewhere; a = l + lw
    double mA = -inf, mB = -inf;
    for (int s = lo + tid; s < P; s += T) {
        const double lw = (smoothed && s >= t_at) ? x[s - t_at] : keys[s] - rmax;
        mA = fmax(mA, lw - keys[s]);
        mB = fmax(mB, lw);
    }
    mA = lr_block_max(mA, red, tid, nw);
    mB = lr_block_max(mB, red, tid, nw);
    double sA = 0.0, sB = 0.0, s2 = 0.0;
    for (int s = lo + tid; s < P; s += T) {
        const double lw = (smoothed && s >= t_at) ? x[s - t_at] : keys[s] - rmax;
        const double w = exp(lw - mB);
        sA += exp((lw - keys[s]) - mA);
        sB += w;
        s2 += w * w;
    }
    sA = lr_block_sum(sA, red, tid, nw);
    sB = lr_block_sum(sB, red, tid, nw);
    s2 = lr_block_sum(s2, red, tid, nw);
    if (tid == 0) {
        out[0] = (mA - mB) + log(sA / sB);               // logsumexp(l + lw) - logsumexp(lw)
        out[1] = k_rep;
        out[2] = lppd;
        out[3] = (sB * sB) / s2;
    }
}

// ------------------------------------------------------------------------------------------
// totals: thread j takes rows j, j + 1024, ... in ascending order; the 1024 sums are added by lr_ordered_sum.  The
// standard error is two passes (the mean, then the squares about it).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LR_LOO_TOT_THREADS) void lr_loo_totals_kernel(const double* __restrict__ pw, long long n,
                                                                           double* __restrict__ out_totals) {
    __shared__ double red[LR_LOO_TOT_THREADS + 32];
    const int j = threadIdx.x;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // used, flagged, elpd, lppd - elpd, lppd, k > 0.5, k > 0.7, unsmoothed
    double kmax = -inf;
    for (long long i = j; i < n; i += LR_LOO_TOT_THREADS) {
        const double elpd = pw[4 * i], k = pw[4 * i + 1], lppd = pw[4 * i + 2];
        if (lppd != lppd) {
            a[1] += 1.0;
            continue;
        }
        a[0] += 1.0, a[2] += elpd, a[3] += lppd - elpd, a[4] += lppd;
        if (k < inf) {
            a[5] += k > 0.5 ? 1.0 : 0.0, a[6] += k > 0.7 ? 1.0 : 0.0;
            kmax = fmax(kmax, k);
        } else {
            a[7] += 1.0;
        }
    }
    double tot[8];
    for (int q = 0; q < 8; ++q) tot[q] = lr_ordered_sum<LR_LOO_TOT_THREADS>(a[q], red, j);
    __syncthreads();
    red[j] = kmax;
    __syncthreads();
    if (j == 0)
        for (int q = 1; q < LR_LOO_TOT_THREADS; ++q) kmax = fmax(kmax, red[q]);
    const double used = tot[0];
    const double mean = used > 0.0 ? tot[2] / used : 0.0;
    double m2 = 0.0;
    for (long long i = j; i < n; i += LR_LOO_TOT_THREADS) {
        const double elpd = pw[4 * i], lppd = pw[4 * i + 2];
        if (lppd == lppd) m2 += (elpd - mean) * (elpd - mean);
    }
    m2 = lr_ordered_sum<LR_LOO_TOT_THREADS>(m2, red, j);
    if (j == 0) {
        const bool any = used > 0.0;
        out_totals[0] = used, out_totals[1] = tot[1];
        out_totals[2] = any ? tot[2] : nan;
        out_totals[3] = used >= 2.0 ? sqrt(used * (m2 / (used - 1.0))) : nan;
        out_totals[4] = any ? tot[3] : nan;
        out_totals[5] = any ? tot[4] : nan;
        out_totals[6] = tot[5], out_totals[7] = tot[6], out_totals[8] = tot[7];
        out_totals[9] = kmax > -inf ? kmax : nan;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int lr_psis_shape_of(long long n_rows, int n_draws, lr_psis_shape* p) {
    if (n_rows < 1 || n_rows > INT_MAX || n_draws < 2 || n_draws > LR_LOO_MAX_DRAWS) return LR_ERR_SIZE;
    int P = 2;
    while (P < n_draws) P <<= 1;
    int M = n_draws / 5;                                 // floor(0.2 S)
    int M2 = (int)ceil(3.0 * sqrt((double)n_draws));
    while (M2 > 0 && (long long)(M2 - 1) * (M2 - 1) >= 9ll * n_draws) --M2;      // (exactly ceil(3 sqrt S), whatever sqrt rounds to)
    while ((long long)M2 * M2 < 9ll * n_draws) ++M2;
    if (M2 < M) M = M2;
    p->P = P, p->M = M;
    int rt = 0;
    while ((rt + 1) * (rt + 1) <= M) ++rt;
    p->m = M >= 5 ? 30 + rt : 0;
    int T = P / 2;
    if (T < LR_WAVE) T = LR_WAVE;
    if (T > LR_PSIS_MAX_THREADS) T = LR_PSIS_MAX_THREADS;
    p->threads = T;
    p->lds_bytes = (size_t)P * (sizeof(double) + sizeof(unsigned short));
    return LR_OK;
}

static int lr_psis_launch(const lr_psis_shape& p, const double* loglik, long long n_rows, int n_draws, double* out_pointwise,
                          int* tails, hipStream_t stream) {
    if (p.lds_bytes > 48 * 1024) {
        // (per call: the attribute belongs to the function on the CURRENT device, and a process may drive several)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&lr_psis_rows_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(lr_psis_rows_kernel, dim3((unsigned)n_rows), dim3(p.threads), p.lds_bytes, stream, loglik, n_draws, p.P,
                       p.M, p.m, out_pointwise, tails);
    return (int)hipGetLastError();
}

static size_t lr_psis_tail_bytes(long long n_rows, int M) {
    return (size_t)lr_align_up64(n_rows * (long long)(M > 0 ? M : 1) * (long long)sizeof(int), 256);
}

extern "C" int64_t lr_psis_rows_workspace_bytes(int64_t n_rows, int32_t n_draws) {
    lr_psis_shape p;
    const int rc = lr_psis_shape_of(n_rows, n_draws, &p);
    if (rc != LR_OK) return rc;
    return (int64_t)lr_psis_tail_bytes(n_rows, p.M);
}

extern "C" int lr_psis_rows(const double* loglik, int64_t n_rows, int32_t n_draws, double* out_pointwise, double* out_totals,
                            void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!loglik || !out_pointwise || !out_totals || !workspace) return LR_ERR_NULL;
    lr_psis_shape p;
    int rc = lr_psis_shape_of(n_rows, n_draws, &p);
    if (rc != LR_OK) return rc;
    if ((int64_t)lr_psis_tail_bytes(n_rows, p.M) > workspace_bytes) return LR_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    rc = lr_psis_launch(p, loglik, n_rows, n_draws, out_pointwise, (int*)workspace, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(lr_loo_totals_kernel, dim3(1), dim3(LR_LOO_TOT_THREADS), 0, stream, out_pointwise, (long long)n_rows,
                       out_totals);
    return (int)hipGetLastError();
}

static int lr_loo_shape_of(long long n, int n_bins, int n_draws, int model, lr_loo_shape* p, lr_psis_shape* q) {
    if (n < 1 || n_draws < 2 || n_draws > LR_LOO_MAX_DRAWS) return LR_ERR_SIZE;
    const int rc = lr_draw_shape_of(n, n_bins, n_draws, model, &p->w);
    if (rc != LR_OK) return rc;
    // lineages per batch: the slab of terms stays within 64 MiB (whole tiles when the lineages do not fit one slab)
    long long B = LR_LOO_SLAB_BYTES / (8ll * n_draws);
    if (B >= n) B = n;
    else B = B / LR_DRAW_TILE * LR_DRAW_TILE;
    const char* env = getenv("LR_LOO_BATCH");
    if (env && atoll(env) > 0) B = atoll(env) < n ? atoll(env) : n;
    const long long batches = (n + B - 1) / B;
    if (batches > INT_MAX || (B + LR_DRAW_TILE - 1) / LR_DRAW_TILE > INT_MAX) return LR_ERR_SIZE;
    p->batch = B, p->batches = (int)batches;
    return lr_psis_shape_of(B, n_draws, q);
}

// workspace: [slab of terms | tables | consts], each 256-byte aligned (the slab first: a caller that ran ONE batch finds the
// [n, n_draws] matrix of terms at the start of its workspace)
static void lr_loo_ws(const lr_loo_shape& p, int n_draws, size_t* o_slab, size_t* o_tab, size_t* o_cst, size_t* total) {
    size_t o = 0;
    *o_slab = o, o += lr_align_up64(p.batch * (long long)n_draws * (long long)sizeof(double), 256);
    *o_tab = o, o += lr_align_up64((long long)n_draws * p.w.tab_stride * sizeof(double2), 256);
    *o_cst = o, o += lr_align_up64((long long)n_draws * sizeof(double), 256);
    *total = o;
}

extern "C" int64_t lr_loo_workspace_bytes(int64_t n, int32_t n_bins, int32_t n_draws, int32_t model) {
    lr_loo_shape p;
    lr_psis_shape q;
    const int rc = lr_loo_shape_of(n, n_bins, n_draws, model, &p, &q);
    if (rc != LR_OK) return rc;
    size_t a, b, c, total;
    lr_loo_ws(p, n_draws, &a, &b, &c, &total);
    return (int64_t)total;
}

extern "C" int lr_loo_plan(int64_t n, int32_t n_bins, int32_t n_draws, int32_t model, int32_t* out) {
    if (!out) return LR_ERR_NULL;
    lr_loo_shape p;
    lr_psis_shape q;
    const int rc = lr_loo_shape_of(n, n_bins, n_draws, model, &p, &q);
    if (rc != LR_OK) return rc;
    if (p.batch > INT_MAX) return LR_ERR_SIZE;
    out[0] = q.M, out[1] = q.m, out[2] = (int)p.batch, out[3] = p.batches;
    return LR_OK;
}

extern "C" int lr_loo_pointwise(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins,
                                const double* lam_bins, const double* mu_bins, int32_t n_draws, int32_t model,
                                const double* br_length, double end_time, double* out_pointwise, double* out_totals,
                                void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!ts || !te || !lam_bins || !mu_bins || !out_pointwise || !out_totals || !workspace) return LR_ERR_NULL;
    lr_loo_shape p;
    lr_psis_shape q;
    int rc = lr_loo_shape_of(n, n_bins, n_draws, model, &p, &q);
    if (rc != LR_OK) return rc;
    size_t o_slab, o_tab, o_cst, total;
    lr_loo_ws(p, n_draws, &o_slab, &o_tab, &o_cst, &total);
    hipStream_t stream = (hipStream_t)stream_;
    rc = lr_draw_begin(p.w, model, br_length, t0, total, workspace, workspace_bytes, o_tab, o_cst, lam_bins, mu_bins, n_bins,
                       n_draws, reinterpret_cast<const void*>(&lr_loo_terms_kernel), stream);
    if (rc) return rc;
    char* ws = (char*)workspace;
    double* slab = (double*)(ws + o_slab);
    const double2* tables = (const double2*)(ws + o_tab);
    for (long long start = 0; start < n; start += p.batch) {
        const long long cnt = n - start < p.batch ? n - start : p.batch;
        const int tiles = (int)((cnt + LR_DRAW_TILE - 1) / LR_DRAW_TILE);
        // a batch is few tiles (16 at 1000 draws): grid.y slices the draws.  Every term is computed as before, whatever the
        // slice it falls into.
        int slices, dps;
        lr_draw_slices(tiles, n_draws, p.w.chunk, 0, &slices, &dps);
        hipLaunchKernelGGL(lr_loo_terms_kernel, dim3(tiles, slices), dim3(LR_DRAW_THREADS), p.w.lds_bytes, stream, ts + start,
                           te + start, cnt, t0, n_bins, p.w.n_cls, p.w.H, end_time, tables, p.w.tab_stride, n_draws, p.w.chunk,
                           p.w.nbuf, dps, slab);
        rc = (int)hipGetLastError();
        if (rc) return rc;
        rc = lr_psis_launch(q, slab, cnt, n_draws, out_pointwise + 4 * start, nullptr, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(lr_loo_totals_kernel, dim3(1), dim3(LR_LOO_TOT_THREADS), 0, stream, out_pointwise, (long long)n,
                       out_totals);
    return (int)hipGetLastError();
}
