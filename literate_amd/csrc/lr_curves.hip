// lr_curves.hip - posterior summaries of the parametric samplers (DDRate.py, trend_rate.py) and of any row table:
// mean and 95 % HPD of chosen columns (lr_col_summary) and of the per-bin curves a parameter vector implies
// (lr_curve_summary: birth, death, net, carrying capacity, niche fraction).
//
// Restates plotDD.py make_vec_dict (:11-57) and utilities/logAverager.py (:18-51) - np.mean and calcHPD (lib:25-41) of
// the l_i, m_i, niche_i columns of a log - without the log: the per-bin columns are functions of the logged parameter
// vector alone (lr_dd_bin_rates / lr_trend_bin_rates of lr_dd.h, which lr_dd_rates, lr_trend_rates and the engine steps
// evaluate), so they are derived from the resident rows.  Per pass over a chunk of columns / bins, the shape of
// lr_summary.hip:
//   1. lr_cv_gather_kernel / lr_cv_expand_kernel   one thread per sample: strided columns of the row table, or the
//                                                  sample's value in every bin of the chunk for every kind, written
//                                                  column-major - column (q, group) is n contiguous doubles;
//   2. rocprim::segmented_radix_sort_keys over the columns of the pass;
//   3. lr_cv_hpd_kernel                            one block per sorted column: NaN check, fixed-order sum (the mean)
//                                                  and the HPD window's arg-min.
// Every output of a column depends on that column's values alone, so a call cut into chunks writes the same bits.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "lr_dd.h"
#include "lr_internal.h"

#define LR_CV_THREADS 256
#define LR_CV_COLS_PER_LAUNCH 64
#define LR_CV_DD 1       /* lr_mcmc_config.sampler of DDRate.py */
#define LR_CV_TREND 2    /* ... of trend_rate.py */

struct lr_cv_geom {
    int S, C, G, W;       // rows per chain, chains, groups (1 pooled, C per chain), doubles per row
    int burn;             // rows dropped at the start of every chain
    int per;              // rows kept per chain = S - burn
    long long n;          // samples per group
    long long n_in;       // samples inside the HPD window
};

// where the triple of column q (of `nq` per kind in this pass) of group g goes: out[g * group + kind * outer + (q0 + i) *
// inner + {0, 1, 2} * triple]
struct lr_cv_out {
    long long group, outer, inner, triple;
    int q0, nq;
};

struct lr_cv_cols {       // the columns of one gather launch (by value: no host-to-device copy of the column list)
    int col[LR_CV_COLS_PER_LAUNCH];
    int nc;
};

// sample j of group `grp` -> its row.  Pooled samples are chain-major (combine_logs appends log after log).
__device__ __forceinline__ const double* lr_cv_row(const double* rows, const lr_cv_geom& g, int grp, long long j) {
    int c = grp, s;
    if (g.G == 1 && g.C > 1) {
        c = (int)(j / g.per);
        s = g.burn + (int)(j - (long long)c * g.per);
    } else {
        s = g.burn + (int)j;
    }
    return rows + ((size_t)s * g.C + c) * g.W;
}

// ---- 1a. chosen columns of the row table -------------------------------------------------------------------------------
// grid (ceil(n / 256), G).  vals[((q0 + i) * G + grp) * n + j]: lane j writes element j of a column.
__global__ __launch_bounds__(LR_CV_THREADS) void lr_cv_gather_kernel(const double* __restrict__ rows, lr_cv_geom g,
                                                                   lr_cv_cols cs, int q0, double* __restrict__ vals) {
    const int grp = blockIdx.y;
    const long long j = (long long)blockIdx.x * LR_CV_THREADS + threadIdx.x;
    if (j >= g.n) return;
    const double* row = lr_cv_row(rows, g, grp, j);
    const size_t col = (size_t)g.G * g.n;
    double* out = vals + (size_t)q0 * col + (size_t)grp * g.n + j;
    for (int i = 0; i < cs.nc; ++i) out[(size_t)i * col] = row[cs.col[i]];
}

// ---- 1b. per-sample curves of a chunk of bins ----------------------------------------------------------------------------
// grid (ceil(n / 256), G, bin slices).  One thread per sample and slice: the sample's parameters (48-64 bytes at a
// row_width stride) -> its value in every bin of the slice, through the functions the log columns come from.
// vals[((kind * nb + ib) * G + grp) * n + j].  DDRate kinds: 0 birth, 1 death, 2 net = birth - death (one rounded
// subtraction), 3 niche, 4 nicheFrac; trend_rate: 0 birth, 1 death, 2 net.  x of a DDRate bin = its index (TIME_RANGE).
template <int SAMPLER>
__global__ __launch_bounds__(LR_CV_THREADS) void lr_cv_expand_kernel(const double* __restrict__ rows, lr_cv_geom g,
                                                                   int arg_col, int m_birth, int m_death,
                                                                   const double* __restrict__ aux, int b0, int nb,
                                                                   double* __restrict__ vals) {
    const int grp = blockIdx.y;
    const long long j = (long long)blockIdx.x * LR_CV_THREADS + threadIdx.x;
    if (j >= g.n) return;
    const double* a = lr_cv_row(rows, g, grp, j) + arg_col;
    const size_t col = (size_t)g.G * g.n;
    double* out = vals + (size_t)grp * g.n + j;
    const int per_z = (nb + gridDim.z - 1) / gridDim.z;
    const int i0 = blockIdx.z * per_z, i1 = min(i0 + per_z, nb);
    if (SAMPLER == LR_CV_DD) {
        const lr_dd_params p{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]};
        for (int ib = i0; ib < i1; ++ib) {
            const int b = b0 + ib;
            double br, dr, niche, frac;
            lr_dd_bin_rates(p, (double)b, aux[b], m_birth, m_death, &br, &dr, &niche, &frac);
            out[(size_t)(0 * nb + ib) * col] = br;
            out[(size_t)(1 * nb + ib) * col] = dr;
            out[(size_t)(2 * nb + ib) * col] = __dsub_rn(br, dr);
            out[(size_t)(3 * nb + ib) * col] = niche;
            out[(size_t)(4 * nb + ib) * col] = frac;
        }
    } else {
        const lr_trend_params p{a[0], a[1], a[2], a[3], a[4], a[5]};
        for (int ib = i0; ib < i1; ++ib) {
            double br, dr;
            lr_trend_bin_rates(p, aux[b0 + ib], m_birth, m_death, &br, &dr);
            out[(size_t)(0 * nb + ib) * col] = br;
            out[(size_t)(1 * nb + ib) * col] = dr;
            out[(size_t)(2 * nb + ib) * col] = __dsub_rn(br, dr);
        }
    }
}

__global__ void lr_cv_offsets_kernel(unsigned int* __restrict__ off, int n_off, unsigned int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_off) off[i] = (unsigned int)i * n;
}

// ---- 3. mean and HPD of each sorted column -------------------------------------------------------------------------------
// Sum: thread t adds d[t], d[t + 256], d[t + 512], ... in that order, then the 256 partial sums are added pairwise in LDS
// (s[t] += s[t + w] for w = 128, 64, ..., 1): one fixed order per column length, on sorted values, so the same bits on
// every call and for every chunking.  HPD (calcHPD): widths w_k = d[k + n_in - 1] - d[k], k = 0 .. n - n_in; the first k
// of minimum width (the reference's strict `rk < r` scan) - each thread keeps its first minimum, the tree keeps the
// smaller width and, on a tie, the smaller k.  A width that is NaN (inf - inf, a column with infinities of one sign at both
// ends of a window) does what it does in that scan: as w_0 it is never replaced (window 0), later it never wins (counted
// as +inf here).  A column that holds a NaN (the sort leaves it at either end, by its sign
// bit) reports NaN three times.  Segment `seg` = (kind * nq + i) * G + grp.
__global__ __launch_bounds__(LR_CV_THREADS) void lr_cv_hpd_kernel(const double* __restrict__ sorted, lr_cv_geom g,
                                                                lr_cv_out o, double* __restrict__ out) {
    __shared__ double s_sum[LR_CV_THREADS];
    __shared__ double s_w[LR_CV_THREADS];
    __shared__ long long s_k[LR_CV_THREADS];
    const int seg = blockIdx.x, tid = threadIdx.x;
    const int grp = seg % g.G, kq = seg / g.G, i = kq % o.nq, kind = kq / o.nq;
    const long long n = g.n, n_in = g.n_in;
    const double* d = sorted + (size_t)seg * n;
    double sum = 0.0;
    int has_nan = 0;
    for (long long e = tid; e < n; e += LR_CV_THREADS) {
        const double v = d[e];
        has_nan |= v != v;
        sum += v;
    }
    double bw = INFINITY;
    long long bk = -1;
    for (long long k = tid; k <= n - n_in; k += LR_CV_THREADS) {
        double w = d[k + n_in - 1] - d[k];
        if (w != w) w = INFINITY;      // inf - inf: the scan's `rk < r` is false for it, it never becomes the minimum
        if (bk < 0 || w < bw) bw = w, bk = k;
    }
    s_sum[tid] = sum, s_w[tid] = bw, s_k[tid] = bk;
    has_nan = __syncthreads_or(has_nan);
    for (int w = LR_CV_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_sum[tid] += s_sum[tid + w];
            const long long ok = s_k[tid + w];
            if (ok >= 0 && (s_k[tid] < 0 || s_w[tid + w] < s_w[tid] || (s_w[tid + w] == s_w[tid] && ok < s_k[tid])))
                s_w[tid] = s_w[tid + w], s_k[tid] = ok;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* t = out + grp * o.group + kind * o.outer + (o.q0 + i) * o.inner;
        // (a first width that is inf - inf is the scan's starting r: nothing compares below it, the scan stays at 0)
        const double w0 = d[n_in - 1] - d[0];
        const long long k = w0 != w0 ? 0 : s_k[0];
        t[0] = has_nan ? NAN : s_sum[0] / (double)n;
        t[o.triple] = has_nan ? NAN : d[k];
        t[2 * o.triple] = has_nan ? NAN : d[k + n_in - 1];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int lr_cv_setup(int32_t n_samples, int32_t n_chains, int32_t row_width, double burnin, int32_t pooled,
                       lr_cv_geom* g) {
    if (n_samples < 1 || n_chains < 1 || n_chains > 65535 || row_width < 1) return LR_ERR_SIZE;   // (groups are grid.y)
    if (!(burnin >= 0.0 && burnin < 1.0)) return LR_ERR_SIZE;
    const long long S = n_samples;
    const long long burn = (long long)(burnin * (double)S);    // int(burnin * S), Python's truncation of the fp64 product
    g->S = n_samples, g->C = n_chains, g->G = pooled ? 1 : n_chains, g->W = row_width;
    g->burn = (int)burn, g->per = (int)(S - burn);
    g->n = pooled ? (long long)n_chains * g->per : g->per;
    if (g->n > 0x7FFFFFFFll) return LR_ERR_SIZE;               // one column is one segment of the sort (32-bit offsets)
    // calcHPD: nIn = int(round(0.95 * n)), round half to even (the default rounding mode of nearbyint)
    g->n_in = (long long)std::nearbyint(0.95 * (double)g->n);
    if (g->n_in < 2) return LR_ERR_SIZE;
    return LR_OK;
}

static int lr_cv_kinds(int sampler) { return sampler == LR_CV_DD ? 5 : 3; }

static int lr_curve_setup(int32_t n_samples, int32_t n_chains, int32_t row_width, int32_t arg_col, int32_t sampler,
                          int32_t m_birth, int32_t m_death, int32_t n_bins, double burnin, int32_t pooled, lr_cv_geom* g) {
    if (sampler != LR_CV_DD && sampler != LR_CV_TREND) return LR_ERR_MODEL;
    if (sampler == LR_CV_DD && (m_birth < 0 || m_birth > 2 || m_death < -2 || m_death > 2)) return LR_ERR_MODEL;
    const int npar = sampler == LR_CV_DD ? LR_DD_NPAR : LR_TR_NPAR;
    if (n_bins < 1 || n_bins > LR_MAX_BINS || arg_col < 0 || (long long)arg_col + npar > row_width) return LR_ERR_SIZE;
    return lr_cv_setup(n_samples, n_chains, row_width, burnin, pooled, g);
}

static int lr_col_setup(int32_t n_samples, int32_t n_chains, int32_t row_width, const int32_t* cols, int32_t n_cols,
                        double burnin, int32_t pooled, lr_cv_geom* g) {
    if (n_cols < 1) return LR_ERR_SIZE;
    if (!cols) return LR_ERR_NULL;
    const int rc = lr_cv_setup(n_samples, n_chains, row_width, burnin, pooled, g);
    if (rc != LR_OK) return rc;
    for (int i = 0; i < n_cols; ++i)
        if (cols[i] < 0 || cols[i] >= row_width) return LR_ERR_SIZE;
    return LR_OK;
}

struct lr_cv_ws {
    size_t off, vals, sorted, tmp, total, tmp_bytes;
};

static size_t lr_cv_up(size_t x) { return (x + 255) / 256 * 256; }

// workspace of a pass over `segs` columns: column offsets | values | sorted values | sort temporaries
static int lr_cv_layout(const lr_cv_geom& g, size_t segs, lr_cv_ws* w) {
    const size_t elems = segs * (size_t)g.n;
    if (elems > 0x7FFFFFFFull) return LR_ERR_SIZE;      // rocprim's sizes are 32 bit: such a pass is cut into smaller ones
    size_t tmp = 0;
    hipError_t he = rocprim::segmented_radix_sort_keys(nullptr, tmp, (const double*)nullptr, (double*)nullptr,
                                                       (unsigned int)elems, (unsigned int)segs, (const unsigned int*)nullptr,
                                                       (const unsigned int*)nullptr);
    if (he != hipSuccess) return (int)he;
    w->tmp_bytes = tmp;
    w->off = 0;
    w->vals = w->off + lr_cv_up(sizeof(unsigned int) * (segs + 1));
    w->sorted = w->vals + lr_cv_up(sizeof(double) * elems);
    w->tmp = w->sorted + lr_cv_up(sizeof(double) * elems);
    w->total = w->tmp + lr_cv_up(tmp);
    return LR_OK;
}

// *chunk = the largest number of units (columns, or bins of `mult` columns each per group) per pass whose workspace fits
// `cap` bytes (and rocprim's 32-bit sizes), 0 when not even one does; returns a hipError_t when the sort's size query
// fails (it asks the current device)
static int lr_cv_chunk(const lr_cv_geom& g, int units, int mult, int64_t cap, lr_cv_ws* w, int* chunk) {
    int lo = 0, hi = units;
    lr_cv_ws t;
    while (lo < hi) {               // the workspace grows with the units per pass: bisect for the last count that fits
        const int mid = (lo + hi + 1) / 2;
        const int rc = lr_cv_layout(g, (size_t)mid * mult * g.G, &t);
        if (rc > 0) return rc;
        if (rc == LR_OK && (int64_t)t.total <= cap) lo = mid;
        else hi = mid - 1;
    }
    *chunk = lo;
    return lo > 0 ? lr_cv_layout(g, (size_t)lo * mult * g.G, w) : LR_OK;
}

// the size query behind both entry points: per_pass = 0 -> the fewest passes rocprim's sizes allow (one, as a rule)
static int64_t lr_cv_query(const lr_cv_geom& g, int units, int mult, int per_pass) {
    if (per_pass < 0 || per_pass > units) return LR_ERR_SIZE;
    lr_cv_ws w;
    int rc;
    if (per_pass > 0) {
        if ((rc = lr_cv_layout(g, (size_t)per_pass * mult * g.G, &w)) != LR_OK) return rc > 0 ? LR_ERR_STATE : rc;
        return (int64_t)w.total;
    }
    int chunk = 0;
    if ((rc = lr_cv_chunk(g, units, mult, INT64_MAX, &w, &chunk)) != LR_OK) return rc > 0 ? LR_ERR_STATE : rc;
    if (chunk < 1) return LR_ERR_SIZE;
    return (int64_t)w.total;
}

// sort the `segs` columns in vals and reduce each into its triple
static int lr_cv_sort_reduce(const lr_cv_geom& g, const lr_cv_ws& w, char* ws, unsigned segs, const lr_cv_out& o,
                             double* out, hipStream_t stream) {
    unsigned int* off = (unsigned int*)(ws + w.off);
    const double* vals = (const double*)(ws + w.vals);
    double* sorted = (double*)(ws + w.sorted);
    int rc;
    hipLaunchKernelGGL(lr_cv_offsets_kernel, dim3((segs + 1 + 255) / 256), dim3(256), 0, stream, off, (int)segs + 1,
                       (unsigned)g.n);
    if ((rc = (int)hipGetLastError()) != 0) return rc;
    size_t tmp = w.tmp_bytes;
    hipError_t he = rocprim::segmented_radix_sort_keys(ws + w.tmp, tmp, vals, sorted, (unsigned)((size_t)segs * g.n), segs,
                                                       (const unsigned int*)off, (const unsigned int*)off + 1, 0, 64, stream);
    if (he != hipSuccess) return (int)he;
    hipLaunchKernelGGL(lr_cv_hpd_kernel, dim3(segs), dim3(LR_CV_THREADS), 0, stream, (const double*)sorted, g, o, out);
    return (int)hipGetLastError();
}

extern "C" int64_t lr_col_summary_workspace_bytes(int32_t n_samples, int32_t n_chains, int32_t row_width,
                                                  const int32_t* cols, int32_t n_cols, double burnin, int32_t pooled,
                                                  int32_t cols_per_pass) {
    lr_cv_geom g;
    const int rc = lr_col_setup(n_samples, n_chains, row_width, cols, n_cols, burnin, pooled, &g);
    if (rc != LR_OK) return rc;
    return lr_cv_query(g, n_cols, 1, cols_per_pass);
}

extern "C" int lr_col_summary(const double* rows, int32_t n_samples, int32_t n_chains, int32_t row_width, const int32_t* cols,
                              int32_t n_cols, double burnin, int32_t pooled, double* out, void* workspace,
                              int64_t workspace_bytes, void* stream_) {
    if (!rows || !out || !workspace) return LR_ERR_NULL;
    lr_cv_geom g;
    int rc = lr_col_setup(n_samples, n_chains, row_width, cols, n_cols, burnin, pooled, &g);
    if (rc != LR_OK) return rc;
    lr_cv_ws w;
    int chunk = 0;
    if ((rc = lr_cv_chunk(g, n_cols, 1, workspace_bytes, &w, &chunk)) != LR_OK) return rc;
    if (chunk < 1) return LR_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const dim3 grid((unsigned)((g.n + LR_CV_THREADS - 1) / LR_CV_THREADS), (unsigned)g.G);
    for (int c0 = 0; c0 < n_cols; c0 += chunk) {
        const int nc = std::min(chunk, n_cols - c0);
        for (int q0 = 0; q0 < nc; q0 += LR_CV_COLS_PER_LAUNCH) {
            lr_cv_cols cs;
            cs.nc = std::min(LR_CV_COLS_PER_LAUNCH, nc - q0);
            for (int i = 0; i < LR_CV_COLS_PER_LAUNCH; ++i) cs.col[i] = i < cs.nc ? cols[c0 + q0 + i] : 0;
            hipLaunchKernelGGL(lr_cv_gather_kernel, grid, dim3(LR_CV_THREADS), 0, stream, rows, g, cs, q0,
                               (double*)(ws + w.vals));
            if ((rc = (int)hipGetLastError()) != 0) return rc;
        }
        const lr_cv_out o{(long long)n_cols * 3, 0, 3, 1, c0, nc};
        if ((rc = lr_cv_sort_reduce(g, w, ws, (unsigned)(nc * g.G), o, out, stream)) != 0) return rc;
    }
    return LR_OK;
}

extern "C" int64_t lr_curve_summary_workspace_bytes(int32_t n_samples, int32_t n_chains, int32_t row_width, int32_t arg_col,
                                                    int32_t sampler, int32_t n_bins, double burnin, int32_t pooled,
                                                    int32_t bins_per_pass) {
    lr_cv_geom g;
    const int rc = lr_curve_setup(n_samples, n_chains, row_width, arg_col, sampler, 0, 0, n_bins, burnin, pooled, &g);
    if (rc != LR_OK) return rc;
    return lr_cv_query(g, n_bins, lr_cv_kinds(sampler), bins_per_pass);
}

extern "C" int lr_curve_summary(const double* rows, int32_t n_samples, int32_t n_chains, int32_t row_width, int32_t arg_col,
                                int32_t sampler, int32_t m_birth, int32_t m_death, const double* aux, int32_t n_bins,
                                double burnin, int32_t pooled, double* out, void* workspace, int64_t workspace_bytes,
                                void* stream_) {
    if (!rows || !aux || !out || !workspace) return LR_ERR_NULL;
    lr_cv_geom g;
    int rc = lr_curve_setup(n_samples, n_chains, row_width, arg_col, sampler, m_birth, m_death, n_bins, burnin, pooled, &g);
    if (rc != LR_OK) return rc;
    const int kinds = lr_cv_kinds(sampler);
    lr_cv_ws w;
    int chunk = 0;
    if ((rc = lr_cv_chunk(g, n_bins, kinds, workspace_bytes, &w, &chunk)) != LR_OK) return rc;
    if (chunk < 1) return LR_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const long long bx = (g.n + LR_CV_THREADS - 1) / LR_CV_THREADS;
    for (int b0 = 0; b0 < n_bins; b0 += chunk) {
        const int nb = std::min(chunk, n_bins - b0);
        // slices of bins (grid.z) until ~1024 blocks are in flight, so that a few thousand samples are not left on a few
        // CUs (a choice, not a measurement: at cfg5's shape the sample blocks alone pass 1024 and nz = 1)
        const long long nz = std::max(1LL, std::min((long long)nb, 1024 / std::max(1LL, bx * g.G)));
        const dim3 grid((unsigned)bx, (unsigned)g.G, (unsigned)nz);
        if (sampler == LR_CV_DD)
            hipLaunchKernelGGL(lr_cv_expand_kernel<LR_CV_DD>, grid, dim3(LR_CV_THREADS), 0, stream, rows, g, arg_col, m_birth,
                               m_death, aux, b0, nb, (double*)(ws + w.vals));
        else
            hipLaunchKernelGGL(lr_cv_expand_kernel<LR_CV_TREND>, grid, dim3(LR_CV_THREADS), 0, stream, rows, g, arg_col,
                               m_birth != 0, m_death != 0, aux, b0, nb, (double*)(ws + w.vals));
        if ((rc = (int)hipGetLastError()) != 0) return rc;
        const lr_cv_out o{(long long)kinds * 3 * n_bins, (long long)3 * n_bins, 1, n_bins, b0, nb};
        if ((rc = lr_cv_sort_reduce(g, w, ws, (unsigned)(kinds * nb * g.G), o, out, stream)) != 0) return rc;
    }
    return LR_OK;
}
