// lr_score.hip - the grouped summary of the RJ trace and its score against known rates (lr_rtt_score,
// include/literate_hip_score.h): lr_rtt_summary(pooled = 1) for every group of chains_per_group chains in one launch, with no
// workspace, and over the groups the coverage of the HPD band and the error of the posterior mean.
//   1. lr_score_group_kernel  one workgroup per (bin, group), bins fastest: the group's n rows -> the bin's birth, death and
//                             net columns in LDS, sorted there by a bitonic network on the next power of two (padded with
//                             +inf), then lr_rtt_hpd_kernel's sum and window scan on the LDS columns; the bin's shift counts
//                             and (bin 0) the K histograms as integer counters in LDS; with truth, covered;
//   2. lr_score_table_kernel  one workgroup per (kind, bin): the six columns of score, summed over the groups in a fixed
//                             order.
// A sorted column holds the same values whatever sorted it (the trace has no -0.0: rates are positive and x - x = +0.0), so
// every value is lr_rtt_summary's bit for bit.  No floating-point atomics; every output element is written by exactly one
// thread, so the buffers need no clearing and a group's outputs depend on its own rows and truth alone.
#include <algorithm>
#include <cmath>

#include "../../include/literate_hip_score.h"
#include "lr_rtt.h"

#define LR_SCORE_MAX_BLOCKS (1 << 20)      // grid of kernel 1; a block walks items blockIdx.x, + gridDim.x, ... (G * n_bins
                                           // may exceed what one grid dimension of 256-thread blocks holds)

// sample j of group `grp` -> its trace row: the group's chains one after the other (lr_rtt_row's pooled order on the slice)
__device__ __forceinline__ const double* lr_score_row(const double* trace, const lr_rtt_geom& g, int cpg, long long grp, int j) {
    const int c = j / g.per, s = g.burn + (j - c * g.per);
    return trace + ((size_t)s * g.C + (size_t)grp * cpg + c) * LR_TRACE_W;
}

// ---- 1. one (bin, group) -------------------------------------------------------------------------------------------------
// LDS: s_col [3][P] doubles (dynamic; P = the power of two >= n), and the reduction's 256-entry arrays.  Consecutive threads
// take consecutive doubles in every phase but the network's strides below 32, where a half-wave's ds_read_b64 lands two deep
// on a bank (stride 2 doubles and up: 2-way, 5 of the log2(P) strides).
__global__ __launch_bounds__(LR_RTT_THREADS) void lr_score_group_kernel(const double* __restrict__ trace, lr_rtt_geom g, int cpg,
                                                                      int P, const double* __restrict__ truth,
                                                                      double* __restrict__ rates, double* __restrict__ freq,
                                                                      long long* __restrict__ k_counts,
                                                                      int* __restrict__ covered) {
    extern __shared__ double s_col[];
    __shared__ double s_sum[LR_RTT_THREADS];
    __shared__ double s_w[LR_RTT_THREADS];
    __shared__ int s_k[LR_RTT_THREADS];
    __shared__ int s_cnt[4];                 // shifts of the group in this bin [2 kinds], shift times of the group in all [2]
    __shared__ int s_kh[2 * LR_KMAX];
    const int tid = threadIdx.x, nb = g.n_bins, n = (int)g.n, n_in = (int)g.n_in;
    const long long items = (long long)g.G * nb;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long grp = item / nb;
        const int bin = (int)(item - grp * nb);
        if (tid < 4) s_cnt[tid] = 0;
        if (tid < 2 * LR_KMAX) s_kh[tid] = 0;
        __syncthreads();
        int here[2] = {0, 0}, all[2] = {0, 0};
        for (int j = tid; j < P; j += LR_RTT_THREADS) {
            double v[2] = {INFINITY, INFINITY};
            if (j < n) {
                const double* row = lr_score_row(trace, g, cpg, grp, j);
#pragma unroll
                for (int kind = 0; kind < 2; ++kind) {
                    const int K = lr_rtt_k(row[6 + kind]);
                    const double* t = row + (kind ? LR_RTT_TM : LR_RTT_TL);
                    int c = 0;                  // shifts with bin index <= bin: the sample's rate index (lr_rtt_expand_kernel)
                    for (int k = 0; k < K - 1; ++k) {
                        const int b = lr_rtt_bin(g, t[k]);
                        c += b <= bin;
                        here[kind] += b == bin;
                    }
                    all[kind] += K - 1;
                    v[kind] = row[(kind ? LR_RTT_M : LR_RTT_L) + c];
                    if (bin == 0) atomicAdd(&s_kh[kind * LR_KMAX + K - 1], 1);
                }
            }
            s_col[j] = v[0];
            s_col[P + j] = v[1];
            s_col[2 * P + j] = j < n ? v[0] - v[1] : INFINITY;
        }
#pragma unroll
        for (int kind = 0; kind < 2; ++kind) {
            if (here[kind]) atomicAdd(&s_cnt[kind], here[kind]);
            if (all[kind]) atomicAdd(&s_cnt[2 + kind], all[kind]);
        }
        __syncthreads();
        // bitonic network, the three columns side by side
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += LR_RTT_THREADS) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                    const bool up = (i & k) == 0;
#pragma unroll
                    for (int col = 0; col < 3; ++col) {
                        double* d = s_col + col * P;
                        const double x = d[i], y = d[p];
                        if ((x > y) == up) d[i] = y, d[p] = x;
                    }
                }
                __syncthreads();
            }
        }
        // mean and HPD of each column: lr_rtt_hpd_kernel's sum order and strict first-minimum scan
        for (int kind = 0; kind < 3; ++kind) {
            const double* d = s_col + kind * P;
            double sum = 0.0;
            for (int i = tid; i < n; i += LR_RTT_THREADS) sum += d[i];
            double bw = INFINITY;
            int bk = -1;
            for (int k = tid; k <= n - n_in; k += LR_RTT_THREADS) {
                const double w = d[k + n_in - 1] - d[k];
                if (bk < 0 || w < bw) bw = w, bk = k;
            }
            s_sum[tid] = sum, s_w[tid] = bw, s_k[tid] = bk;
            __syncthreads();
            for (int w = LR_RTT_THREADS / 2; w > 0; w >>= 1) {
                if (tid < w) {
                    s_sum[tid] += s_sum[tid + w];
                    const int ok = s_k[tid + w];
                    if (ok >= 0 && (s_k[tid] < 0 || s_w[tid + w] < s_w[tid] || (s_w[tid + w] == s_w[tid] && ok < s_k[tid])))
                        s_w[tid] = s_w[tid + w], s_k[tid] = ok;
                }
                __syncthreads();
            }
            if (tid == 0) {
                double* o = rates + ((size_t)grp * 3 + kind) * 3 * nb + bin;
                const int k = s_k[0];
                const double lo = d[k], hi = d[k + n_in - 1];
                o[0] = s_sum[0] / (double)n;
                o[nb] = lo;
                o[2 * nb] = hi;
                if (truth) {
                    const double* tr = truth + (size_t)grp * 2 * nb + bin;
                    const double t = kind == 2 ? __dsub_rn(tr[0], tr[nb]) : tr[kind * nb];
                    covered[((size_t)grp * 3 + kind) * nb + bin] = (lo <= t && t <= hi) ? 1 : 0;
                }
            }
            __syncthreads();
        }
        // shift frequency = histogram / n, zero when the group sampled at most one shift time in all (lr_rtt_freq_kernel)
        if (tid < 2) freq[((size_t)grp * 2 + tid) * nb + bin] = s_cnt[2 + tid] > 1 ? (double)s_cnt[tid] / (double)n : 0.0;
        if (bin == 0 && tid < 2 * LR_KMAX) k_counts[(size_t)grp * 2 * LR_KMAX + tid] = (long long)s_kh[tid];
        __syncthreads();
    }
}

// ---- 2. the table over the groups ----------------------------------------------------------------------------------------
// grid 3 * n_bins.  Thread t adds groups t, t + 256, ... in that order, then the 256 partial sums are added pairwise in LDS
// (s[t] += s[t + w], w = 128 .. 1).  Products and sums are rounded one at a time (no fused multiply-add).
__global__ __launch_bounds__(LR_RTT_THREADS) void lr_score_table_kernel(const double* __restrict__ rates,
                                                                      const double* __restrict__ truth,
                                                                      const int* __restrict__ covered, int G, int nb,
                                                                      double* __restrict__ score) {
    __shared__ double s_acc[5][LR_RTT_THREADS];
    const int tid = threadIdx.x, kind = blockIdx.x / nb, bin = blockIdx.x - kind * nb;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int grp = tid; grp < G; grp += LR_RTT_THREADS) {
        const double* o = rates + ((size_t)grp * 3 + kind) * 3 * nb + bin;
        const double* tr = truth + (size_t)grp * 2 * nb + bin;
        const double t = kind == 2 ? __dsub_rn(tr[0], tr[nb]) : tr[kind * nb];
        const double err = __dsub_rn(o[0], t);
        acc[0] = __dadd_rn(acc[0], (double)covered[((size_t)grp * 3 + kind) * nb + bin]);
        acc[1] = __dadd_rn(acc[1], err);
        acc[2] = __dadd_rn(acc[2], fabs(err));
        acc[3] = __dadd_rn(acc[3], __dmul_rn(err, err));
        acc[4] = __dadd_rn(acc[4], __dsub_rn(o[2 * nb], o[nb]));
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) s_acc[q][tid] = acc[q];
    __syncthreads();
    for (int w = LR_RTT_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < 5; ++q) s_acc[q][tid] = __dadd_rn(s_acc[q][tid], s_acc[q][tid + w]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* out = score + (size_t)blockIdx.x * LR_SCORE_COLS;
        const double Gd = (double)G;
        out[0] = Gd;
        out[1] = s_acc[0][0] / Gd;
        out[2] = s_acc[1][0] / Gd;
        out[3] = s_acc[2][0] / Gd;
        out[4] = sqrt(s_acc[3][0] / Gd);
        out[5] = s_acc[4][0] / Gd;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
extern "C" int lr_rtt_score(const lr_rtt_score_problem* p) {
    if (!p || !p->trace || !p->rates || !p->shift_freq || !p->k_counts) return LR_ERR_NULL;
    if (p->truth && (!p->covered || !p->score)) return LR_ERR_NULL;
    if (p->n_samples < 1 || p->n_chains < 1 || p->chains_per_group < 1) return LR_ERR_SIZE;
    if (p->n_chains % p->chains_per_group) return LR_ERR_SIZE;
    if (!(p->burnin >= 0.0 && p->burnin < 1.0)) return LR_ERR_SIZE;
    lr_rtt_geom g;
    int rc = lr_rtt_span(p->start_age, p->end_age, &g);
    if (rc != LR_OK) return rc;
    const long long S = p->n_samples;
    const long long burn = (long long)(p->burnin * (double)S);          // int(burnin * S), no cap: the pooled rule
    g.S = p->n_samples, g.C = p->n_chains, g.G = p->n_chains / p->chains_per_group;
    g.burn = (int)burn, g.per = (int)(S - burn);
    g.n = (long long)p->chains_per_group * g.per;
    g.n_in = (long long)std::nearbyint(0.95 * (double)g.n);
    if (g.n_in < 2) return LR_ERR_SIZE;
    if (g.n > LR_SCORE_MAX_SAMPLES) return LR_ERR_SIZE;
    int P = 2;
    while (P < (int)g.n) P <<= 1;
    const size_t lds = sizeof(double) * 3 * (size_t)P;
    hipStream_t stream = (hipStream_t)p->stream;
    {
        // always the cap, never this call's own size: the attribute belongs to the process, and a value that depended on the
        // call would let two host threads with different n undo each other's between the set and the launch
        const hipError_t he = hipFuncSetAttribute(reinterpret_cast<const void*>(&lr_score_group_kernel),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  (int)(sizeof(double) * 3 * LR_SCORE_MAX_SAMPLES));
        if (he != hipSuccess) return (int)he;
    }
    const long long items = (long long)g.G * g.n_bins;
    const unsigned blocks = (unsigned)std::min<long long>(items, LR_SCORE_MAX_BLOCKS);
    hipLaunchKernelGGL(lr_score_group_kernel, dim3(blocks), dim3(LR_RTT_THREADS), lds, stream, p->trace, g, (int)p->chains_per_group,
                       P, p->truth, p->rates, p->shift_freq, (long long*)p->k_counts, (int*)p->covered);
    if ((rc = (int)hipGetLastError()) != 0) return rc;
    if (p->truth) {
        hipLaunchKernelGGL(lr_score_table_kernel, dim3((unsigned)(3 * g.n_bins)), dim3(LR_RTT_THREADS), 0, stream,
                           (const double*)p->rates, p->truth, (const int*)p->covered, g.G, g.n_bins, p->score);
        if ((rc = (int)hipGetLastError()) != 0) return rc;
    }
    return LR_OK;
}
