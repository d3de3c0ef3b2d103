// lr_prior.hip - the prior on the times of rate shifts by Monte Carlo (lr_shift_prior): what plotRJforward.v3.py
// get_prior_shift (:58-89) estimates in a Python loop of 100 000 replicates, so that the sampled frequency of shifts per
// bin (lr_rtt_summary's shift_freq) can be read as a Bayes factor against the prior (calcBF :54-56, get_r_plot :182-195).
//
// One thread per replicate, grid-stride.  Replicate i draws from the Philox block (counter (i, LR_P_SHIFT_PRIOR, idx), key =
// the two halves of the seed), so what it does depends on (a, b, seed, i, poi_lambda) alone:
//   idx 0        hyper-prior mode: lambda ~ Gamma(2, 1) as -log((1 - u_a)(1 - u_b)); p0 = e^-lambda is the product itself
//   idx 1, u_a   K ~ zero-truncated Poisson(lambda) by inversion of the CDF, capped at LR_SHIFT_PRIOR_KCAP
//   idx 2 + j/2  shift time j < K - 1 (member a for even j, b for odd j): x_j = (a - 1) + ((b + 1) - (a - 1)) u
// A replicate is rejected when two of the K + 1 points {a, b, x_j} are closer than 1 (the script's
// min(np.diff(np.sort(...))) < 1: a rounded fp64 difference is monotone in its operands, so the smallest difference over
// all pairs is the smallest between neighbours).  No shift time is stored: the generator is addressed, so the pairwise
// check and the histogram recompute x_j instead of keeping 63 doubles per thread in scratch.  Every point is tested
// against the two ends first, which is where most replicates with many shifts die.
// Every product and sum that numpy would round on its own is rounded on its own here (__dmul_rn / __dadd_rn: hipcc
// contracts a * b + c into an FMA by default).
//
// Counters: per block in LDS as 32-bit integers (shift histogram, the two K histograms, the four totals), flushed into
// the int64 outputs with 64-bit integer atomics - exact in any order, so the outputs depend on the arguments only, not on
// the grid or the schedule.  No floating-point atomics.
// No 32-bit count can overflow: a block adds the replicates of at most LR_SP_FLUSH_TRIPS trips of its grid-stride loop
// (LR_SP_THREADS replicates per trip) between two flushes, 2^12 * 2^8 = 2^20 replicates, and one replicate adds at most
// LR_SHIFT_PRIOR_KCAP - 1 = 63 to any counter (its shifts, all in one bin; or K - 1 to the shift total): < 2^26.
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip.h"
#include "lr_device.h"

#define LR_P_SHIFT_PRIOR 40
#define LR_SP_THREADS 256
#define LR_SP_FLUSH_TRIPS 4096
#define LR_SP_MAX_REPS (1ll << 40)
#define LR_SP_NONE (-1)
// LDS counters: [n_bins] shift histogram | [KCAP] K drawn | [KCAP] K accepted | [4] totals
#define LR_SP_COUNTERS(nb) ((nb) + 2 * LR_SHIFT_PRIOR_KCAP + 4)

struct lr_sp_args {
    double a, b;              // the two ends (root_age, death_age)
    double lo, w;             // shift times are lo + w u: lo = a - 1, w = (b + 1) - (a - 1), formed on the host
    double delta;             // e_j = a + j * delta (j >= 2): numpy's arange fill, as lr_summary.hip
    double lambda, p0;        // fixed mode: the Poisson rate and exp(-rate)
    unsigned long long rep0;
    long long n_reps;
    uint32_t k0, k1;
    int n_bins;
    int fixed;
    long long* totals;
    long long* shift_hist;
    long long* k_drawn;
    long long* k_accepted;
};

// np.arange(a, b)'s edges and np.histogram's bin rule on them, as lr_summary.hip's shift histogram (lr_rtt_edge /
// lr_rtt_bin): bin i holds e_i <= t < e_{i+1}, the last bin also t == e_nbins; anything else is in no bin.
__device__ __forceinline__ double lr_sp_edge(const lr_sp_args& g, int j) {
    if (j == 0) return g.a;
    if (j == 1) return __dadd_rn(g.a, 1.0);
    return __dadd_rn(g.a, __dmul_rn((double)j, g.delta));
}
__device__ __forceinline__ int lr_sp_bin(const lr_sp_args& g, double t) {
    const int nb = g.n_bins;
    if (!(t >= g.a) || !(t <= lr_sp_edge(g, nb))) return LR_SP_NONE;
    const double f = floor(t - g.a);
    int j = (int)fmin(fmax(f, 0.0), (double)nb);
    while (j > 0 && t < lr_sp_edge(g, j)) --j;
    while (j < nb && t >= lr_sp_edge(g, j + 1)) ++j;
    return j == nb ? nb - 1 : j;
}

// the two shift times of the pair at idx 2 + q: x_{2q} and x_{2q+1}
__device__ __forceinline__ lr_u2 lr_sp_times(const lr_sp_args& g, const lr_stream& s, uint64_t it, int q) {
    const lr_u2 u = lr_pair(s, it, LR_P_SHIFT_PRIOR, 2u + (uint32_t)q);
    lr_u2 x;
    x.a = __dadd_rn(g.lo, __dmul_rn(g.w, u.a));
    x.b = __dadd_rn(g.lo, __dmul_rn(g.w, u.b));
    return x;
}

// is |p - q| < 1 in rounded fp64 (the larger minus the smaller, as np.diff of the sorted points forms it)?
__device__ __forceinline__ bool lr_sp_close(double p, double q) { return fabs(__dadd_rn(p, -q)) < 1.0; }

// K of replicate `it`; *capped = the cap stopped the inversion
__device__ __forceinline__ int lr_sp_draw_k(const lr_sp_args& g, const lr_stream& s, uint64_t it, bool* capped) {
    double lambda = g.lambda, p0 = g.p0;
    if (!g.fixed) {
        const lr_u2 u = lr_pair(s, it, LR_P_SHIFT_PRIOR, 0);
        p0 = __dmul_rn(1.0 - u.a, 1.0 - u.b);
        lambda = -lr_log(p0);
    }
    const double ua = lr_pair(s, it, LR_P_SHIFT_PRIOR, 1).a;
    const double t = __dadd_rn(p0, __dmul_rn(ua, 1.0 - p0));
    int k = 0;
    double p = p0, cum = p0;
    do {
        ++k;
        p = __ddiv_rn(__dmul_rn(p, lambda), (double)k);
        cum = __dadd_rn(cum, p);
    } while (cum <= t && k < LR_SHIFT_PRIOR_KCAP);
    *capped = cum <= t;
    return k;
}

// does replicate `it` with its n = K - 1 shift times keep every pair of points at least 1 apart?
__device__ __forceinline__ bool lr_sp_accept(const lr_sp_args& g, const lr_stream& s, uint64_t it, int n) {
    // every shift time against the two ends
    for (int q = 0; 2 * q < n; ++q) {
        const lr_u2 x = lr_sp_times(g, s, it, q);
        if (lr_sp_close(x.a, g.a) || lr_sp_close(x.a, g.b)) return false;
        if (2 * q + 1 < n && (lr_sp_close(x.b, g.a) || lr_sp_close(x.b, g.b))) return false;
    }
    // every two shift times: the members of each whole pair against each other and against the pairs before it
    for (int q = 0; 2 * q + 1 < n; ++q) {
        const lr_u2 x = lr_sp_times(g, s, it, q);
        if (lr_sp_close(x.a, x.b)) return false;
        for (int r = 0; r < q; ++r) {
            const lr_u2 y = lr_sp_times(g, s, it, r);
            if (lr_sp_close(x.a, y.a) || lr_sp_close(x.a, y.b)) return false;
            if (lr_sp_close(x.b, y.a) || lr_sp_close(x.b, y.b)) return false;
        }
    }
    // n odd: the last shift time is the a member of a pair the loop above did not reach
    if (n & 1) {
        const double xl = lr_sp_times(g, s, it, n >> 1).a;
        for (int r = 0; 2 * r + 1 < n; ++r) {
            const lr_u2 y = lr_sp_times(g, s, it, r);
            if (lr_sp_close(xl, y.a) || lr_sp_close(xl, y.b)) return false;
        }
    }
    return true;
}

__device__ __forceinline__ void lr_sp_flush(const lr_sp_args& g, int* s_cnt) {
    const int nb = g.n_bins, n_cnt = LR_SP_COUNTERS(nb);
    __syncthreads();
    for (int i = threadIdx.x; i < n_cnt; i += LR_SP_THREADS) {
        const int v = s_cnt[i];
        if (v == 0) continue;
        s_cnt[i] = 0;
        long long* dst = i < nb ? g.shift_hist + i
                                : (i < nb + LR_SHIFT_PRIOR_KCAP ? g.k_drawn + (i - nb)
                                                                : (i < nb + 2 * LR_SHIFT_PRIOR_KCAP
                                                                       ? g.k_accepted + (i - nb - LR_SHIFT_PRIOR_KCAP)
                                                                       : g.totals + (i - nb - 2 * LR_SHIFT_PRIOR_KCAP)));
        atomicAdd((unsigned long long*)dst, (unsigned long long)v);
    }
    __syncthreads();
}

__global__ __launch_bounds__(LR_SP_THREADS) void lr_shift_prior_kernel(lr_sp_args g) {
    extern __shared__ int s_cnt[];
    const int nb = g.n_bins;
    int* s_drawn = s_cnt + nb;
    int* s_acc = s_drawn + LR_SHIFT_PRIOR_KCAP;
    int* s_tot = s_acc + LR_SHIFT_PRIOR_KCAP;
    for (int i = threadIdx.x; i < LR_SP_COUNTERS(nb); i += LR_SP_THREADS) s_cnt[i] = 0;
    __syncthreads();
    const lr_stream s{g.k0, g.k1};
    const long long stride = (long long)gridDim.x * LR_SP_THREADS;
    const long long trips = (g.n_reps + stride - 1) / stride;          // the same for every thread: the flush has barriers
    long long j = (long long)blockIdx.x * LR_SP_THREADS + threadIdx.x;
    for (long long trip = 0; trip < trips; ++trip, j += stride) {
        if (j < g.n_reps) {
            const uint64_t it = g.rep0 + (unsigned long long)j;
            bool capped;
            const int K = lr_sp_draw_k(g, s, it, &capped);
            atomicAdd(&s_drawn[K - 1], 1);
            if (capped) atomicAdd(&s_tot[2], 1);
            const int n = K - 1;
            if (lr_sp_accept(g, s, it, n)) {
                atomicAdd(&s_tot[0], 1);
                atomicAdd(&s_acc[K - 1], 1);
                int in_bins = 0;
                for (int q = 0; 2 * q < n; ++q) {
                    const lr_u2 x = lr_sp_times(g, s, it, q);
                    const int ba = lr_sp_bin(g, x.a);
                    if (ba != LR_SP_NONE) atomicAdd(&s_cnt[ba], 1), ++in_bins;
                    if (2 * q + 1 < n) {
                        const int bb = lr_sp_bin(g, x.b);
                        if (bb != LR_SP_NONE) atomicAdd(&s_cnt[bb], 1), ++in_bins;
                    }
                }
                if (n > 0) atomicAdd(&s_tot[3], n);
                if (in_bins > 0) atomicAdd(&s_tot[1], in_bins);
            }
        }
        if ((trip + 1) % LR_SP_FLUSH_TRIPS == 0) lr_sp_flush(g, s_cnt);
    }
    lr_sp_flush(g, s_cnt);
}

extern "C" int lr_shift_prior(double start_age, double end_age, int64_t rep0, int64_t n_reps, uint64_t seed,
                              double poi_lambda, int32_t accumulate, int64_t* totals, int64_t* shift_hist,
                              int64_t* k_drawn, int64_t* k_accepted, void* stream_) {
    if (!totals || !shift_hist || !k_drawn || !k_accepted) return LR_ERR_NULL;
    if (!(std::isfinite(start_age) && std::isfinite(end_age) && end_age > start_age)) return LR_ERR_SIZE;
    // the bins of lr_rtt_summary: np.arange(a, b) has ceil(b - a) edges, the reference takes int(b - a) bins
    const double span = end_age - start_age;
    if (span > (double)LR_MAX_BINS + 1.0) return LR_ERR_SIZE;
    const long long n_bins = (long long)std::ceil(span) - 1;
    if (n_bins < 1 || n_bins > LR_MAX_BINS || n_bins != (long long)span) return LR_ERR_SIZE;
    if (n_reps < 1 || n_reps > LR_SP_MAX_REPS || rep0 < 0 || rep0 > INT64_MAX - n_reps) return LR_ERR_SIZE;
    if (std::isnan(poi_lambda) || poi_lambda > 700.0) return LR_ERR_SIZE;
    hipStream_t stream = (hipStream_t)stream_;
    lr_sp_args g;
    g.a = start_age, g.b = end_age;
    g.lo = start_age - 1.0, g.w = (end_age + 1.0) - (start_age - 1.0);
    g.delta = (start_age + 1.0) - start_age;
    g.fixed = poi_lambda > 0.0;
    g.lambda = g.fixed ? poi_lambda : 0.0, g.p0 = g.fixed ? std::exp(-poi_lambda) : 0.0;
    g.rep0 = (unsigned long long)rep0, g.n_reps = n_reps;
    g.k0 = (uint32_t)seed, g.k1 = (uint32_t)(seed >> 32);
    g.n_bins = (int)n_bins;
    g.totals = (long long*)totals, g.shift_hist = (long long*)shift_hist;
    g.k_drawn = (long long*)k_drawn, g.k_accepted = (long long*)k_accepted;
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(totals, 0, 4 * sizeof(int64_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(shift_hist, 0, (size_t)n_bins * sizeof(int64_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(k_drawn, 0, LR_SHIFT_PRIOR_KCAP * sizeof(int64_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(k_accepted, 0, LR_SHIFT_PRIOR_KCAP * sizeof(int64_t), stream);
        if (e != hipSuccess) return (int)e;
    }
    const long long want = (n_reps + LR_SP_THREADS - 1) / LR_SP_THREADS;
    const unsigned blocks = (unsigned)(want < LR_SHIFT_PRIOR_BLOCKS ? want : LR_SHIFT_PRIOR_BLOCKS);
    const size_t lds = sizeof(int) * (size_t)LR_SP_COUNTERS(n_bins);        // at most 16.9 KiB
    hipLaunchKernelGGL(lr_shift_prior_kernel, dim3(blocks), dim3(LR_SP_THREADS), lds, stream, g);
    return (int)hipGetLastError();
}
