// lr_summary.hip - posterior rates through time from the resident trace (lr_rtt_summary): per unit bin the mean and 95 %
// HPD of the birth, death and net-diversification rates, the frequency of rate shifts, and the K histograms.
//
// Restates plotRJforward.v3.py get_marginal_rates (:92-139), plot_net_rate (:234-270), the shift histogram of get_r_plot
// (:166-178), get_K_values (:292-305) and calcHPD (:12-28 = literate_library.py:25-41).  Per call of bins [b0, b0 + nb):
//   1. lr_rtt_count_kernel   (first call only) K_l / K_m and shift-time histograms, integer counters only;
//   2. lr_rtt_expand_kernel  one thread per sample: the sample's rate in every bin of the chunk, for birth, death and net,
//                            written bin-major - column (kind, bin, group) is n contiguous doubles;
//   3. rocprim::segmented_radix_sort_keys over the 3 * nb * G columns;
//   4. lr_rtt_hpd_kernel     one block per sorted column: fixed-order sum (the mean) and the HPD window's arg-min.
// Every output of a column depends on that column's values alone, so a call cut into chunks of bins writes the same bits.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "lr_rtt.h"          // the geometry, edges, bins and K clamp shared with lr_score.hip

// sample j of group `grp` -> its trace row.  Pooled samples are chain-major (combine_logs appends chain after chain).
__device__ __forceinline__ const double* lr_rtt_row(const double* trace, const lr_rtt_geom& g, int grp, long long j) {
    int c = grp, s;
    if (g.G == 1 && g.C > 1) {
        c = (int)(j / g.per);
        s = g.burn + (int)(j - (long long)c * g.per);
    } else {
        s = g.burn + (int)j;
    }
    return trace + ((size_t)s * g.C + c) * LR_TRACE_W;
}

// ---- 1. counters ---------------------------------------------------------------------------------------------------
// grid (slices, G).  LDS: K histograms [2][LR_KMAX], shift histograms [2][n_bins], all shifts [2]; flushed into the
// int64 counters with integer atomics (exact, in any order).  cnt: [G][2][n_bins + 1], entry n_bins = every shift time
// of the group's rows, inside the edges or not (get_r_plot's `len(res[4]) > 1`).
__global__ __launch_bounds__(LR_RTT_THREADS) void lr_rtt_count_kernel(const double* __restrict__ trace, lr_rtt_geom g,
                                                                    long long* __restrict__ k_counts,
                                                                    long long* __restrict__ cnt) {
    extern __shared__ int s_h[];
    const int nb = g.n_bins, grp = blockIdx.y;
    int* s_k = s_h;                       // [2][LR_KMAX]
    int* s_s = s_h + 2 * LR_KMAX;         // [2][nb + 1]
    const int n_h = 2 * LR_KMAX + 2 * (nb + 1);
    for (int i = threadIdx.x; i < n_h; i += LR_RTT_THREADS) s_h[i] = 0;
    __syncthreads();
    const long long per_block = (g.n + gridDim.x - 1) / gridDim.x;
    const long long j0 = (long long)blockIdx.x * per_block, j1 = min(j0 + per_block, g.n);
    for (long long j = j0 + threadIdx.x; j < j1; j += LR_RTT_THREADS) {
        const double* row = lr_rtt_row(trace, g, grp, j);
#pragma unroll
        for (int kind = 0; kind < 2; ++kind) {
            const int K = lr_rtt_k(row[6 + kind]);
            const double* t = row + (kind ? LR_RTT_TM : LR_RTT_TL);
            atomicAdd(&s_k[kind * LR_KMAX + K - 1], 1);
            int* h = s_s + kind * (nb + 1);
            for (int k = 0; k < K - 1; ++k) {
                const int b = lr_rtt_bin(g, t[k]);
                if (b != LR_RTT_NONE) atomicAdd(&h[b], 1);
            }
            if (K > 1) atomicAdd(&h[nb], K - 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_h; i += LR_RTT_THREADS) {
        const int v = s_h[i];
        if (v == 0) continue;
        unsigned long long* dst = (unsigned long long*)(i < 2 * LR_KMAX ? k_counts + (size_t)grp * 2 * LR_KMAX + i
                                                                        : cnt + (size_t)grp * 2 * (nb + 1) + (i - 2 * LR_KMAX));
        atomicAdd(dst, (unsigned long long)v);
    }
}

// shift frequency = histogram / n (get_r_plot: h[0] / float(res[5])); zero when the group sampled at most one shift time
// in all (get_r_plot :167-170 then histograms nothing).
__global__ void lr_rtt_freq_kernel(const long long* __restrict__ cnt, lr_rtt_geom g, double* __restrict__ freq) {
    const int nb = g.n_bins;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)g.G * 2 * nb) return;
    const long long gk = i / nb, b = i - gk * nb;
    const long long* c = cnt + gk * (nb + 1);
    freq[i] = c[nb] > 1 ? (double)c[b] / (double)g.n : 0.0;
}

// ---- 2. per-sample rates of a chunk of bins ------------------------------------------------------------------------
// One thread per sample.  Its shifts' bin indices go to LDS ([kind][k][thread], 16 bit: consecutive lanes share a dword or
// take the next one - no bank conflicts).  Bin i's rate is rates[c_i], c_i = #{shifts with bin index <= i}: the cumulative
// sum of np.histogram(shifts, edges) (get_marginal_rates :118-121), whatever order the shift times come in.
// vals[((kind * nb + ib) * G + grp) * n + j]: kind 0 birth, 1 death, 2 net = birth - death (plot_net_rate :236-240).
__global__ __launch_bounds__(LR_RTT_THREADS) void lr_rtt_expand_kernel(const double* __restrict__ trace, lr_rtt_geom g,
                                                                     int b0, int nb, double* __restrict__ vals) {
    __shared__ short s_idx[2][LR_KMAX - 1][LR_RTT_THREADS];
    const int grp = blockIdx.y, tid = threadIdx.x;
    const long long j = (long long)blockIdx.x * LR_RTT_THREADS + tid;
    if (j >= g.n) return;               // (no barrier below: each thread reads only its own LDS column)
    const double* row = lr_rtt_row(trace, g, grp, j);
    int K[2];
#pragma unroll
    for (int kind = 0; kind < 2; ++kind) {
        K[kind] = lr_rtt_k(row[6 + kind]);
        const double* t = row + (kind ? LR_RTT_TM : LR_RTT_TL);
        for (int k = 0; k < K[kind] - 1; ++k) s_idx[kind][k][tid] = (short)lr_rtt_bin(g, t[k]);
    }
    const size_t col = (size_t)g.G * g.n;                 // distance between the columns of two consecutive bins
    double* out = vals + (size_t)grp * g.n + j;
    int c_prev[2] = {0, 0};
    double v[2] = {row[LR_RTT_L], row[LR_RTT_M]};
    for (int ib = 0; ib < nb; ++ib) {
        const int i = b0 + ib;
#pragma unroll
        for (int kind = 0; kind < 2; ++kind) {
            int c = 0;
            for (int k = 0; k < K[kind] - 1; ++k) c += s_idx[kind][k][tid] <= i;
            if (c != c_prev[kind]) {
                c_prev[kind] = c;
                v[kind] = row[(kind ? LR_RTT_M : LR_RTT_L) + c];
            }
        }
        out[(size_t)(0 * nb + ib) * col] = v[0];
        out[(size_t)(1 * nb + ib) * col] = v[1];
        out[(size_t)(2 * nb + ib) * col] = v[0] - v[1];
    }
}

__global__ void lr_rtt_offsets_kernel(unsigned int* __restrict__ off, int n_off, unsigned int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_off) off[i] = (unsigned int)i * n;
}

// ---- 4. mean and HPD of each sorted column ---------------------------------------------------------------------------
// Sum: thread t adds d[t], d[t + 256], d[t + 512], ... in that order, then the 256 partial sums are added pairwise in LDS
// (s[t] += s[t + w] for w = 128, 64, ..., 1): one fixed order per column length, on sorted values, so the same bits on
// every call and for every chunking.  HPD (calcHPD): widths w_k = d[k + n_in - 1] - d[k], k = 0 .. n - n_in; the first k
// of minimum width (the reference's strict `rk < r` scan) - each thread keeps its first minimum, the tree keeps the
// smaller width and, on a tie, the smaller k.
// out: [G][3 kinds][mean, lo, hi][n_bins]
__global__ __launch_bounds__(LR_RTT_THREADS) void lr_rtt_hpd_kernel(const double* __restrict__ sorted, lr_rtt_geom g,
                                                                  int b0, int nb, double* __restrict__ out) {
    __shared__ double s_sum[LR_RTT_THREADS];
    __shared__ double s_w[LR_RTT_THREADS];
    __shared__ long long s_k[LR_RTT_THREADS];
    const int seg = blockIdx.x, tid = threadIdx.x;
    const int grp = seg % g.G, kb = seg / g.G, ib = kb % nb, kind = kb / nb;
    const long long n = g.n, n_in = g.n_in;
    const double* d = sorted + (size_t)seg * n;
    double sum = 0.0;
    for (long long i = tid; i < n; i += LR_RTT_THREADS) sum += d[i];
    double bw = INFINITY;
    long long bk = -1;
    for (long long k = tid; k <= n - n_in; k += LR_RTT_THREADS) {
        const double w = d[k + n_in - 1] - d[k];
        if (bk < 0 || w < bw) bw = w, bk = k;
    }
    s_sum[tid] = sum, s_w[tid] = bw, s_k[tid] = bk;
    __syncthreads();
    for (int w = LR_RTT_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_sum[tid] += s_sum[tid + w];
            const long long ok = s_k[tid + w];
            if (ok >= 0 && (s_k[tid] < 0 || s_w[tid + w] < s_w[tid] || (s_w[tid + w] == s_w[tid] && ok < s_k[tid])))
                s_w[tid] = s_w[tid + w], s_k[tid] = ok;
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* o = out + ((size_t)grp * 3 + kind) * 3 * g.n_bins + b0 + ib;
        const long long k = s_k[0];
        o[0] = s_sum[0] / (double)n;
        o[g.n_bins] = d[k];
        o[2 * g.n_bins] = d[k + n_in - 1];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int lr_rtt_setup(int32_t n_samples, int32_t n_chains, double start_age, double end_age, double burnin, int32_t pooled,
                        lr_rtt_geom* g) {
    if (n_samples < 1 || n_chains < 1 || n_chains > 65535) return LR_ERR_SIZE;   // (groups are grid.y)
    if (!(burnin >= 0.0 && burnin < 1.0)) return LR_ERR_SIZE;
    const int rc = lr_rtt_span(start_age, end_age, g);          // (lr_rtt.h: the span rules, n_bins, a, delta)
    if (rc != LR_OK) return rc;
    const long long S = n_samples;
    // burn-in: int(burnin * S), Python's truncation of the fp64 product; per chain capped at int(0.9 * S) (get_marginal_rates
    // :104-105); pooled (combine_logs :310-334, then burnin = 0) without the cap
    long long burn = (long long)(burnin * (double)S);
    if (!pooled) burn = std::min(burn, (long long)(0.9 * (double)S));
    g->S = n_samples, g->C = n_chains, g->G = pooled ? 1 : n_chains;
    g->burn = (int)burn, g->per = (int)(S - burn);
    g->n = pooled ? (long long)n_chains * g->per : g->per;
    // calcHPD: nIn = int(round(0.95 * n)), round half to even (the default rounding mode of nearbyint)
    g->n_in = (long long)std::nearbyint(0.95 * (double)g->n);
    if (g->n_in < 2) return LR_ERR_SIZE;
    return LR_OK;
}

struct lr_rtt_ws {
    size_t cnt, off, vals, sorted, tmp, total, tmp_bytes;
};

static const size_t LR_RTT_ALIGN = 256;

static size_t lr_rtt_up(size_t x) { return (x + LR_RTT_ALIGN - 1) / LR_RTT_ALIGN * LR_RTT_ALIGN; }

// workspace of a chunk of nb bins: counters | column offsets | values | sorted values | sort temporaries
static int lr_rtt_layout(const lr_rtt_geom& g, int nb, lr_rtt_ws* w) {
    const size_t segs = (size_t)3 * nb * g.G, elems = segs * (size_t)g.n;
    if (elems > 0x7FFFFFFFull) return LR_ERR_SIZE;      // rocprim's sizes are 32 bit
    size_t tmp = 0;
    hipError_t he = rocprim::segmented_radix_sort_keys(nullptr, tmp, (const double*)nullptr, (double*)nullptr,
                                                       (unsigned int)elems, (unsigned int)segs, (const unsigned int*)nullptr,
                                                       (const unsigned int*)nullptr);
    if (he != hipSuccess) return (int)he;
    w->tmp_bytes = tmp;
    w->cnt = 0;
    w->off = w->cnt + lr_rtt_up(sizeof(long long) * (size_t)g.G * 2 * (g.n_bins + 1));
    w->vals = w->off + lr_rtt_up(sizeof(unsigned int) * (segs + 1));
    w->sorted = w->vals + lr_rtt_up(sizeof(double) * elems);
    w->tmp = w->sorted + lr_rtt_up(sizeof(double) * elems);
    w->total = w->tmp + lr_rtt_up(tmp);
    return LR_OK;
}

// *chunk = the largest number of bins per pass whose workspace fits `cap` bytes (and rocprim's 32-bit sizes), 0 when not
// even one bin does; returns a hipError_t when the sort's size query fails (it asks the current device)
static int lr_rtt_chunk(const lr_rtt_geom& g, int64_t cap, lr_rtt_ws* w, int* chunk) {
    int lo = 0, hi = g.n_bins;
    lr_rtt_ws t;
    while (lo < hi) {               // the workspace grows with nb: bisect for the last nb that fits
        const int mid = (lo + hi + 1) / 2;
        const int rc = lr_rtt_layout(g, mid, &t);
        if (rc > 0) return rc;
        if (rc == LR_OK && (int64_t)t.total <= cap) lo = mid;
        else hi = mid - 1;
    }
    *chunk = lo;
    return lo > 0 ? lr_rtt_layout(g, lo, w) : LR_OK;
}

extern "C" int64_t lr_rtt_summary_workspace_bytes(int32_t n_samples, int32_t n_chains, double start_age, double end_age,
                                                  double burnin, int32_t pooled) {
    lr_rtt_geom g;
    int rc = lr_rtt_setup(n_samples, n_chains, start_age, end_age, burnin, pooled, &g);
    if (rc != LR_OK) return rc;
    lr_rtt_ws w;
    int chunk = 0;
    if ((rc = lr_rtt_chunk(g, INT64_MAX, &w, &chunk)) != LR_OK) return rc > 0 ? LR_ERR_STATE : rc;
    if (chunk < 1) return LR_ERR_SIZE;
    return (int64_t)w.total;
}

extern "C" int lr_rtt_summary(const double* trace, int32_t n_samples, int32_t n_chains, double start_age, double end_age,
                              double burnin, int32_t pooled, double* rates, double* shift_freq, int64_t* k_counts,
                              void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!trace || !rates || !shift_freq || !k_counts || !workspace) return LR_ERR_NULL;
    lr_rtt_geom g;
    int rc = lr_rtt_setup(n_samples, n_chains, start_age, end_age, burnin, pooled, &g);
    if (rc != LR_OK) return rc;
    lr_rtt_ws w;
    int chunk = 0;
    if ((rc = lr_rtt_chunk(g, workspace_bytes, &w, &chunk)) != LR_OK) return rc;
    if (chunk < 1) return LR_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    long long* cnt = (long long*)(ws + w.cnt);
    unsigned int* off = (unsigned int*)(ws + w.off);
    double* vals = (double*)(ws + w.vals);
    double* sorted = (double*)(ws + w.sorted);

    // counters (once)
    hipError_t he = hipMemsetAsync(cnt, 0, sizeof(long long) * (size_t)g.G * 2 * (g.n_bins + 1), stream);
    if (he == hipSuccess) he = hipMemsetAsync(k_counts, 0, sizeof(int64_t) * (size_t)g.G * 2 * LR_KMAX, stream);
    if (he != hipSuccess) return (int)he;
    {
        // enough slices for ~4 blocks per CU in all, each over at least 1024 samples
        const long long want = std::max(1LL, std::min((1024LL + g.G - 1) / g.G, (g.n + 1023) / 1024));
        const size_t lds = sizeof(int) * (2 * LR_KMAX + 2 * (g.n_bins + 1));
        hipLaunchKernelGGL(lr_rtt_count_kernel, dim3((unsigned)want, (unsigned)g.G), dim3(LR_RTT_THREADS), lds, stream,
                           trace, g, (long long*)k_counts, cnt);
        if ((rc = (int)hipGetLastError()) != 0) return rc;
        const long long nf = (long long)g.G * 2 * g.n_bins;
        hipLaunchKernelGGL(lr_rtt_freq_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, stream, cnt, g, shift_freq);
        if ((rc = (int)hipGetLastError()) != 0) return rc;
    }
    for (int b0 = 0; b0 < g.n_bins; b0 += chunk) {
        const int nb = std::min(chunk, g.n_bins - b0);
        const unsigned segs = (unsigned)(3 * nb * g.G);
        const unsigned elems = (unsigned)((size_t)segs * g.n);
        hipLaunchKernelGGL(lr_rtt_offsets_kernel, dim3((segs + 1 + 255) / 256), dim3(256), 0, stream, off, (int)segs + 1,
                           (unsigned)g.n);
        if ((rc = (int)hipGetLastError()) != 0) return rc;
        hipLaunchKernelGGL(lr_rtt_expand_kernel, dim3((unsigned)((g.n + LR_RTT_THREADS - 1) / LR_RTT_THREADS), (unsigned)g.G),
                           dim3(LR_RTT_THREADS), 0, stream, trace, g, b0, nb, vals);
        if ((rc = (int)hipGetLastError()) != 0) return rc;
        size_t tmp = w.tmp_bytes;
        he = rocprim::segmented_radix_sort_keys(ws + w.tmp, tmp, (const double*)vals, sorted, elems, segs,
                                                (const unsigned int*)off, (const unsigned int*)off + 1, 0, 64, stream);
        if (he != hipSuccess) return (int)he;
        hipLaunchKernelGGL(lr_rtt_hpd_kernel, dim3(segs), dim3(LR_RTT_THREADS), 0, stream, (const double*)sorted, g, b0, nb,
                           rates);
        if ((rc = (int)hipGetLastError()) != 0) return rc;
    }
    return LR_OK;
}
