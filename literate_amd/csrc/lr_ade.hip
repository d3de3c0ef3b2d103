// lr_ade.hip - age-dependent extinction (include/literate_hip_ade.h): the lineages counted per (birth bin, age at death)
// class, and for every (posterior draw of the per-bin death rates, Weibull shape) pair the multiplier c that maximises the
// interval-censored likelihood, with the value there.
//
//   lr_ade_classes_kernel  one pass over the lineages: the class counts, the censored per birth bin, the two totals.  Counters
//                          in LDS (the [A, A] table too while it fits: A <= LR_ADE_LDS_BINS), flushed with 64-bit integer
//                          atomics; above that the table's cells take the atomics directly.
//   lr_ade_prep_kernel     one block: the classes with a count, in the table's own order (a ballot scan, so the list - and
//                          with it every later sum - has one order), the bins that hold a death, the header
//   lr_ade_risk_kernel     R[jb][j] = cens[jb] + sum_{a > j} dead[jb][a]: the lineages of birth bin jb that live past age j
//                          (these two write the tables of lr_ade_tables.h, for the joint sampler of lr_adej.hip as well)
//   lr_ade_draw_kernel     one block per draw: its flag, and M_s[j] = sum_jb R[jb][j] mu[s, jb + j], added in the order of jb
//   lr_ade_profile_kernel  one block per (draw, shape)
//
// The likelihood of the header, rearranged: with d_i = mu[je_i] w_k[a_i] the hazard step of class i = (jb, a), je = jb + a,
//   l(c) = -c E + sum_i n_i log(-expm1(-c d_i)),   E = sum_i n_i H[jb_i][a_i] + sum_jb cens[jb] H[jb][A - jb]
//                                                    = sum_j w_k[j] M_s[j]
// (every lineage of birth bin jb that lives past age j pays mu[jb + j] w_k[j]).  M_s does not depend on the shape and R not
// on the draw, so a (draw, shape) pair costs A multiplications for E and one pass over the classes per Newton step, whatever
// the number of lineages.  The score in log c, phi(u) = -c E + sum_i n_i x_i / expm1(x_i) with x_i = c d_i, falls strictly
// from D (the deaths) to -inf: one root, bracketed as the iteration goes, Newton steps inside the bracket and bisection when
// a step leaves it.  Every block-wide sum is a fixed tree (lr_ade_sum2): no floating-point atomics.
#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

#include "lr_ade_tables.h"

#define LR_ADE_THREADS 256
#define LR_ADE_WAVES (LR_ADE_THREADS / 64)
#define LR_ADE_LDS_BINS 64                               /* the [A, A] class table is counted in LDS up to here (16 KiB) */
#define LR_ADE_LPT 4                                     /* lineages per thread and trip of lr_ade_classes_kernel */
#define LR_ADE_TILE (LR_ADE_THREADS * LR_ADE_LPT)
#define LR_ADE_CLASS_BLOCKS 1024
#define LR_ADE_FLUSH_TRIPS (1 << 20)                     /* a block flushes its 32-bit counters at least this often */
#define LR_ADE_PREP_THREADS 1024
#define LR_ADE_REG_CLASSES 4                             /* classes a thread keeps in registers across the Newton steps */
#define LR_ADE_MAX_STEPS 60

// ------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------
// dynamic LDS: [A: censored per birth bin | 2: used, unused | A A: the class table, when lds_table]
__global__ __launch_bounds__(LR_ADE_THREADS) void lr_ade_classes_kernel(
    const double* __restrict__ ts, const double* __restrict__ te, long long n, long long tiles, double t0, double t_end,
    int A, int lds_table, long long* __restrict__ out_dead, long long* __restrict__ out_cens,
    long long* __restrict__ out_totals) {
    extern __shared__ int s_cnt[];
    const int tid = threadIdx.x;
    const int n_cnt = A + 2 + (lds_table ? A * A : 0);
    int* s_tab = s_cnt + A + 2;
    const double nb = (double)A;
    long long tile = blockIdx.x;
    while (tile < tiles) {
        for (int i = tid; i < n_cnt; i += LR_ADE_THREADS) s_cnt[i] = 0;
        __syncthreads();
        for (int trip = 0; trip < LR_ADE_FLUSH_TRIPS && tile < tiles; ++trip, tile += gridDim.x) {
#pragma unroll
            for (int k = 0; k < LR_ADE_LPT; ++k) {
                const long long i = tile * LR_ADE_TILE + k * LR_ADE_THREADS + tid;
                if (i >= n) continue;
                const double s = ts[i], e = te[i];
                const double x = s - t0;
                if (!(x >= 0.0 && x < nb && e > s)) {
                    atomicAdd(&s_cnt[A + 1], 1);
                    continue;
                }
                atomicAdd(&s_cnt[A], 1);
                const int jb = min((int)floor(x), A - 1);
                if (e <= t_end) {
                    const int je = (int)fmin(fmax(floor(e - t0), 0.0), nb - 1.0);
                    const int cell = jb * A + max(je - jb, 0);
                    if (lds_table) atomicAdd(&s_tab[cell], 1);
                    else atomicAdd((unsigned long long*)(out_dead + cell), 1ull);
                } else {
                    atomicAdd(&s_cnt[jb], 1);
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < n_cnt; i += LR_ADE_THREADS) {
            const int v = s_cnt[i];
            if (!v) continue;
            long long* dst = i < A ? out_cens + i : i < A + 2 ? out_totals + (i - A) : out_dead + (i - A - 2);
            atomicAdd((unsigned long long*)dst, (unsigned long long)v);
        }
        __syncthreads();
    }
}

// one block.  The cells (jb, a) with jb + a < A and a count > 0, in the order of the table: cls_cell[p] = je | a << 16,
// cls_n[p] / cls_n32[p] = the count; death_bin[je] = 1 where a death was observed; hdr = {classes, deaths, FITS32}
__global__ __launch_bounds__(LR_ADE_PREP_THREADS) void lr_ade_prep_kernel(const long long* __restrict__ dead,
                                                                          const long long* __restrict__ cens, int A,
                                                                          int* __restrict__ cls_cell,
                                                                          double* __restrict__ cls_n,
                                                                          int* __restrict__ cls_n32,
                                                                          int* __restrict__ death_bin,
                                                                          long long* __restrict__ hdr) {
    __shared__ int s_wave[LR_ADE_PREP_THREADS / 64];
    __shared__ int s_bin[LR_ADE_MAX_BINS];
    __shared__ unsigned long long s_deaths;
    __shared__ unsigned long long s_most;                  // the largest number of lineages of one birth bin
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < A; i += LR_ADE_PREP_THREADS) s_bin[i] = 0;
    if (tid == 0) s_deaths = 0ull, s_most = 0ull;
    __syncthreads();
    const int cells = A * A;
    int base_pos = 0;
    unsigned long long mine = 0ull;
    for (int base = 0; base < cells; base += LR_ADE_PREP_THREADS) {
        const int e = base + tid;
        long long v = 0;
        int jb = 0, a = 0;
        if (e < cells) {
            jb = e / A, a = e - jb * A;
            if (jb + a < A) v = dead[e];
        }
        const bool is = v > 0;
        const unsigned long long votes = __ballot(is);
        if (lane == 0) s_wave[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < LR_ADE_PREP_THREADS / 64; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (is) {
            const int p = base_pos + before + __popcll(votes & ((1ull << lane) - 1ull));
            cls_cell[p] = (jb + a) | (a << 16);
            cls_n[p] = (double)v;
            cls_n32[p] = (int)(v < INT_MAX ? v : INT_MAX);
            s_bin[jb + a] = 1;
            mine += (unsigned long long)v;
        }
        base_pos += all;
        __syncthreads();
    }
    if (mine) atomicAdd(&s_deaths, mine);
    // a birth bin's lineages: R[jb][0] plus its deaths at age 0, the largest number any R or class count can reach
    for (int jb = tid; jb < A; jb += LR_ADE_PREP_THREADS) {
        unsigned long long tot = (unsigned long long)(cens[jb] > 0 ? cens[jb] : 0);
        for (int a = 0; a < A - jb; ++a) {
            const long long v = dead[(size_t)jb * A + a];
            tot += (unsigned long long)(v > 0 ? v : 0);
        }
        atomicMax(&s_most, tot);
    }
    __syncthreads();
    for (int i = tid; i < A; i += LR_ADE_PREP_THREADS) death_bin[i] = s_bin[i];
    if (tid == 0) {
        hdr[LR_ADE_HDR_CLASSES] = base_pos, hdr[LR_ADE_HDR_DEATHS] = (long long)s_deaths;
        hdr[LR_ADE_HDR_FITS32] = s_most < (unsigned long long)INT_MAX ? 1 : 0;
    }
}

// R and R32, row jb by thread jb (a negative count is read as 0)
__global__ __launch_bounds__(LR_ADE_THREADS) void lr_ade_risk_kernel(const long long* __restrict__ dead,
                                                                     const long long* __restrict__ cens, int A,
                                                                     double* __restrict__ R, int* __restrict__ R32) {
    const int jb = blockIdx.x * LR_ADE_THREADS + threadIdx.x;
    if (jb >= A) return;
    long long run = cens[jb] > 0 ? cens[jb] : 0;
    const int row = lr_ade_row(jb, A);
    for (int j = A - jb - 1; j >= 0; --j) {
        R[row + j] = (double)run;
        R32[row + j] = (int)(run < INT_MAX ? run : INT_MAX);
        const long long v = dead[(size_t)jb * A + j];
        run += v > 0 ? v : 0;
    }
}

// block s: out_flag[s]; unless flagged, M[s * A + j] = sum_{jb = 0}^{A - 1 - j} R[jb][j] mu[s, jb + j]
__global__ __launch_bounds__(LR_ADE_THREADS) void lr_ade_draw_kernel(const double* __restrict__ mu_bins, int A,
                                                                     const double* __restrict__ R,
                                                                     const int* __restrict__ death_bin,
                                                                     double* __restrict__ M, int* __restrict__ out_flag) {
    __shared__ double s_mu[LR_ADE_MAX_BINS];
    const int s = blockIdx.x, tid = threadIdx.x;
    const double* mu = mu_bins + (size_t)s * A;
    int bad = 0;
    for (int b = tid; b < A; b += LR_ADE_THREADS) {
        const double m = mu[b];
        s_mu[b] = m;
        bad |= lr_ade_bad_rate(m, death_bin, b);
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) out_flag[s] = bad ? 1 : 0;
    if (bad) return;
    for (int j = tid; j < A; j += LR_ADE_THREADS) {
        double acc = 0.0;
        for (int jb = 0, row = 0; jb + j < A; row += A - jb, ++jb) acc = fma(R[row + j], s_mu[jb + j], acc);   // row = lr_ade_row(jb, A)
        M[(size_t)s * A + j] = acc;
    }
}

// (a, b) summed over the block, the same in every thread: lanes by shuffles, the waves one after the other
// (not lr_adej_block_sum: that one adds the lanes in the order of a DPP scan, and the bits would differ)
__device__ __forceinline__ void lr_ade_sum2(double& a, double& b, double* s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_red[2 * wave] = a, s_red[2 * wave + 1] = b;
    __syncthreads();
    a = s_red[0], b = s_red[1];
#pragma unroll
    for (int w = 1; w < LR_ADE_WAVES; ++w) a += s_red[2 * w], b += s_red[2 * w + 1];
    __syncthreads();
}

// n g(x) and n x g'(x) of a class at x = c d, g(x) = x / expm1(x)
__device__ __forceinline__ void lr_ade_score(double n, double x, double& p, double& q) {
    if (x == 0.0) {
        p += n;
        return;
    }
    const double em = expm1(x);
    if (!(em < __builtin_inf())) return;                    // g = 0 and x g' = 0 to every digit
    const double g = x / em;
    p += n * g;
    q += n * g * (1.0 - x / -expm1(-x));
}

__global__ __launch_bounds__(LR_ADE_THREADS) void lr_ade_profile_kernel(
    const double* __restrict__ mu_bins, int A, const double* __restrict__ shapes, int G, lr_ade_data d,
    const double* __restrict__ M, const int* __restrict__ flag, double* __restrict__ out_ll, double* __restrict__ out_c) {
    const int* __restrict__ cls_cell = d.cls_cell;
    const double* __restrict__ cls_n = d.cls_n;
    __shared__ double s_mu[LR_ADE_MAX_BINS];
    __shared__ double s_w[LR_ADE_MAX_BINS];
    __shared__ double s_red[2 * LR_ADE_WAVES];
    const int tid = threadIdx.x;
    const int s = blockIdx.x / G, g = blockIdx.x - s * G;
    const size_t o = (size_t)s * G + g;
    const double k = shapes[g];
    const double nan = __builtin_nan("");
    // (everything the block branches on below is the same in all its threads)
    if (flag[s] || !(k > 0.0) || !(k < __builtin_inf())) {
        if (tid == 0) out_ll[o] = nan, out_c[o] = nan;
        return;
    }
    const double D = (double)d.hdr[LR_ADE_HDR_DEATHS];
    const int n_cls = lr_ade_class_count(d, A);
    if (D == 0.0) {
        if (tid == 0) out_ll[o] = 0.0, out_c[o] = 0.0;
        return;
    }
    double e_part = 0.0, zero = 0.0;
    for (int j = tid; j < A; j += LR_ADE_THREADS) {
        // (not lr_adej_weight: exp(k log j) from logs kept across iterations rounds differently from pow(j, k))
        const double w = j == 0 ? 1.0 : pow((double)j, k) * expm1(k * log1p(1.0 / (double)j));
        s_w[j] = w;
        s_mu[j] = mu_bins[(size_t)s * A + j];
        e_part = fma(w, M[(size_t)s * A + j], e_part);
    }
    lr_ade_sum2(e_part, zero, s_red);                         // (its first barrier also publishes s_w and s_mu)
    const double E = e_part;
    if (!(E > 0.0)) {
        if (tid == 0) out_ll[o] = 0.0, out_c[o] = __builtin_inf();
        return;
    }
    // the thread's first classes stay in registers; what is beyond them (more than 1024 classes) is read again each step
    double dr[LR_ADE_REG_CLASSES], nr[LR_ADE_REG_CLASSES];
    double nd = 0.0;
#pragma unroll
    for (int r = 0; r < LR_ADE_REG_CLASSES; ++r) {
        const int i = r * LR_ADE_THREADS + tid;
        dr[r] = 0.0, nr[r] = 0.0;
        if (i < n_cls) {
            const int cell = cls_cell[i];
            dr[r] = s_mu[cell & 0xFFFF] * s_w[cell >> 16], nr[r] = cls_n[i];
            nd = fma(nr[r], dr[r], nd);
        }
    }
    for (int i = LR_ADE_REG_CLASSES * LR_ADE_THREADS + tid; i < n_cls; i += LR_ADE_THREADS) {
        const int cell = cls_cell[i];
        nd = fma(cls_n[i], s_mu[cell & 0xFFFF] * s_w[cell >> 16], nd);
    }
    lr_ade_sum2(nd, zero, s_red);
    // the start: g(x) ~ 1 - x / 2, so phi ~ D - c (E + sum n d / 2): every death at the midpoint of its bin
    double u = log(D / (E + 0.5 * nd));
    double lo = -__builtin_inf(), hi = __builtin_inf();
    for (int it = 0; it < LR_ADE_MAX_STEPS; ++it) {
        const double c = exp(u);
        double p = 0.0, q = 0.0;
#pragma unroll
        for (int r = 0; r < LR_ADE_REG_CLASSES; ++r)
            if (nr[r] > 0.0) lr_ade_score(nr[r], c * dr[r], p, q);
        for (int i = LR_ADE_REG_CLASSES * LR_ADE_THREADS + tid; i < n_cls; i += LR_ADE_THREADS) {
            const int cell = cls_cell[i];
            lr_ade_score(cls_n[i], c * (s_mu[cell & 0xFFFF] * s_w[cell >> 16]), p, q);
        }
        lr_ade_sum2(p, q, s_red);
        const double phi = p - c * E, dphi = q - c * E;      // dphi < 0
        if (phi == 0.0) break;
        if (phi > 0.0) lo = u;
        else hi = u;
        double next = u - fmin(fmax(phi / dphi, -3.0), 3.0);
        if (!(next > lo && next < hi)) {
            if (lo > -__builtin_inf() && hi < __builtin_inf()) next = 0.5 * (lo + hi);
            else next = phi > 0.0 ? u + 3.0 : u - 3.0;
        }
        const double moved = fabs(next - u);
        u = next;
        if (moved <= 1e-14 || !(hi - lo > 1e-15)) break;
    }
    const double c = exp(u);
    double ll = 0.0;
#pragma unroll
    for (int r = 0; r < LR_ADE_REG_CLASSES; ++r)
        if (nr[r] > 0.0) ll += lr_ade_term(nr[r], c * dr[r]);
    for (int i = LR_ADE_REG_CLASSES * LR_ADE_THREADS + tid; i < n_cls; i += LR_ADE_THREADS) {
        const int cell = cls_cell[i];
        ll += lr_ade_term(cls_n[i], c * (s_mu[cell & 0xFFFF] * s_w[cell >> 16]));
    }
    lr_ade_sum2(ll, zero, s_red);
    if (tid == 0) out_ll[o] = ll - c * E, out_c[o] = c;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int lr_ade_sizes(int n_bins, int S, int G) {
    if (S < 1 || G < 1 || n_bins < 1 || n_bins > LR_ADE_MAX_BINS) return LR_ERR_SIZE;
    if ((long long)S * G >= (1ll << 31)) return LR_ERR_SIZE;
    return LR_OK;
}

int lr_ade_prepare_tables(const int64_t* dead, const int64_t* cens, int A, void* tables, hipStream_t stream) {
    const lr_ade_ws w = lr_ade_layout(A);
    char* base = (char*)tables;
    hipLaunchKernelGGL(lr_ade_prep_kernel, dim3(1), dim3(LR_ADE_PREP_THREADS), 0, stream, (const long long*)dead,
                       (const long long*)cens, A, (int*)(base + w.cls_cell), (double*)(base + w.cls_n), (int*)(base + w.cls_n32),
                       (int*)(base + w.death_bin), (long long*)(base + w.hdr));
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(lr_ade_risk_kernel, dim3((A + LR_ADE_THREADS - 1) / LR_ADE_THREADS), dim3(LR_ADE_THREADS), 0, stream,
                       (const long long*)dead, (const long long*)cens, A, (double*)(base + w.R), (int*)(base + w.R32));
    return (int)hipGetLastError();
}

extern "C" int lr_ade_classes(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins, int64_t* out_dead,
                              int64_t* out_cens, int64_t* out_totals, void* stream_) {
    if (!ts || !te || !out_dead || !out_cens || !out_totals) return LR_ERR_NULL;
    if (n < 1 || n_bins < 1 || n_bins > LR_ADE_MAX_BINS) return LR_ERR_SIZE;
    if (!std::isfinite(t0) || t0 != std::floor(t0)) return LR_ERR_T0;
    hipStream_t stream = (hipStream_t)stream_;
    const int A = n_bins;
    hipError_t e = hipMemsetAsync(out_dead, 0, (size_t)A * A * sizeof(int64_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(out_cens, 0, (size_t)A * sizeof(int64_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(out_totals, 0, 2 * sizeof(int64_t), stream);
    if (e != hipSuccess) return (int)e;
    const long long tiles = (n + LR_ADE_TILE - 1) / LR_ADE_TILE;
    const int lds_table = A <= LR_ADE_LDS_BINS;
    const size_t lds = (size_t)(A + 2 + (lds_table ? A * A : 0)) * sizeof(int);
    hipLaunchKernelGGL(lr_ade_classes_kernel, dim3((unsigned)(tiles < LR_ADE_CLASS_BLOCKS ? tiles : LR_ADE_CLASS_BLOCKS)),
                       dim3(LR_ADE_THREADS), lds, stream, ts, te, (long long)n, tiles, t0, t0 + (double)n_bins, A, lds_table,
                       (long long*)out_dead, (long long*)out_cens, (long long*)out_totals);
    return (int)hipGetLastError();
}

// workspace: [the tables (lr_ade_tables.h) | M [S, A]]
static int64_t lr_ade_profile_bytes(int A, int S) {
    return (int64_t)lr_ade_layout(A).total + lr_align_up64((long long)S * A * sizeof(double), 256);
}

extern "C" int64_t lr_ade_profile_workspace_bytes(int32_t n_bins, int32_t S, int32_t G) {
    const int rc = lr_ade_sizes(n_bins, S, G);
    if (rc != LR_OK) return rc;
    return lr_ade_profile_bytes(n_bins, S);
}

extern "C" int lr_ade_profile(const int64_t* dead, const int64_t* cens, int32_t n_bins, const double* mu_bins, int32_t S,
                              const double* shapes, int32_t G, double* out_ll, double* out_c, int32_t* out_flag,
                              void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!dead || !cens || !mu_bins || !shapes || !out_ll || !out_c || !out_flag || !workspace) return LR_ERR_NULL;
    int rc = lr_ade_sizes(n_bins, S, G);
    if (rc != LR_OK) return rc;
    const int A = n_bins;
    if (lr_ade_profile_bytes(A, S) > workspace_bytes) return LR_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const lr_ade_data d = lr_ade_view(workspace, A);
    double* M = (double*)((char*)workspace + lr_ade_layout(A).total);
    rc = lr_ade_prepare_tables(dead, cens, A, workspace, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(lr_ade_draw_kernel, dim3(S), dim3(LR_ADE_THREADS), 0, stream, mu_bins, A, d.R, d.death_bin, M,
                       (int*)out_flag);
    rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(lr_ade_profile_kernel, dim3((unsigned)((long long)S * G)), dim3(LR_ADE_THREADS), 0, stream, mu_bins, A,
                       shapes, G, d, (const double*)M, (const int*)out_flag, out_ll, out_c);
    return (int)hipGetLastError();
}
