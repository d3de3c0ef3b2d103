// lr_ess.hip - convergence summary of sampled trace rows (lr_ess_summary): per chain and log column the effective
// sample size with Tracer's estimator (BEAST TraceCorrelation), and per column the split R-hat across chains (BDA3 11.4).
//
//   1. lr_ess_series_kernel  one work-group per (chain, column) series: stages the kept rows (LDS, or a centred copy in
//                            the workspace past LR_ESS_LDS_ROWS), forms the mean and the two half-chain means and
//                            variances, centres the series, then computes the autocovariances a tile of 256 lags at a
//                            time (one lag per lane, j summed in increasing order).  Wave 0 applies the pairwise stop
//                            rule in lag order after each tile; the loop ends at the tile that holds the stop.
//   2. lr_ess_pool_kernel    one work-group per column: pooled mean and ESS, and R-hat from the 2C half-chain sequences,
//                            all in a fixed order over the chains.
// Every sum runs in an order fixed by the shape alone (no floating-point atomics): two calls on the same rows write the
// same bits.  A sequence whose values are all equal has that value as its mean (the sum of n equal values over n need
// not give it back), so a constant column has exactly zero variance.
#include <algorithm>
#include <cmath>

#include "lr_device.h"
#include "lr_internal.h"

#define LR_ESS_THREADS 256
#define LR_ESS_COLS_PER_LAUNCH 32

struct lr_ess_geom {
    int S, C, W;          // rows, chains, row width (doubles)
    int burn, n;          // rows dropped per chain, rows kept per chain
    int L;                // min(n - 1, max_lag)
    int h;                // floor(n / 2): length of the two R-hat sequences of a chain
    int K;                // columns
};

struct lr_ess_cols {      // the columns of one launch (by value: no host-to-device copy of the column list)
    int k0, nk;
    int col[LR_ESS_COLS_PER_LAUNCH];
};

// LDS carve (doubles; all of it dynamic, so the series stays 16-byte aligned): reduction scratch [3][T] | tile of
// autocovariances [T + 1] and the stop word | series [n] (LDS path)
#define LR_ESS_RED 0
#define LR_ESS_G (3 * LR_ESS_THREADS)
#define LR_ESS_X (LR_ESS_G + LR_ESS_THREADS + 2)

// s[0..T) -> s[0]: s[t] += s[t + w] for w = T/2, T/4, ..., 1 (fixed pairwise tree).  Ends with a barrier.
__device__ __forceinline__ void lr_ess_tree(double* s, int tid) {
    for (int w = LR_ESS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
}

// sum over the 64 lanes of a wave, fixed butterfly order
__device__ __forceinline__ double lr_ess_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <bool LDS>
__global__ __launch_bounds__(LR_ESS_THREADS) void lr_ess_series_kernel(const double* __restrict__ rows, lr_ess_geom g,
                                                                     lr_ess_cols cs, double* __restrict__ chain_stats,
                                                                     int32_t* __restrict__ stop_out,
                                                                     double* __restrict__ half,
                                                                     double* __restrict__ centred) {
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    double* s_red = s_mem + LR_ESS_RED;
    double* s_g = s_mem + LR_ESS_G;             // s_g[0] = g_{b-1} (carried from the previous tile), s_g[1 + i] = g_{b+i}
    int& s_stop = *reinterpret_cast<int*>(s_g + LR_ESS_THREADS + 1);
    int& s_same = s_stop;                       // (the same word, before the tile loop: which sequences are constant)
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = blockIdx.x, kk = blockIdx.y, k = cs.k0 + kk;
    const int n = g.n, h = g.h, L = g.L;
    const size_t series = (size_t)k * g.C + c;
    double* x = LDS ? s_mem + LR_ESS_X : centred + series * (size_t)n;

    // ---- stage the kept rows of the series; three fixed-order sums (whole, first half, second half) ----
    const size_t stride = (size_t)g.C * g.W;
    const double* src = rows + ((size_t)g.burn * g.C + c) * g.W + cs.col[kk];
    for (int j = tid; j < n; j += LR_ESS_THREADS) x[j] = src[(size_t)j * stride];
    if (tid == 0) s_same = 7;
    __syncthreads();
    const double x0 = x[0], xb = x[n - h];
    double s = 0.0, sa = 0.0, sb = 0.0;
    bool same = true, same_a = true, same_b = true;
    for (int j = tid; j < n; j += LR_ESS_THREADS) {
        const double v = x[j];
        s += v;
        same = same && v == x0;
        if (j < h) sa += v, same_a = same_a && v == x0;
        if (j >= n - h) sb += v, same_b = same_b && v == xb;
    }
    s_red[tid] = s, s_red[LR_ESS_THREADS + tid] = sa, s_red[2 * LR_ESS_THREADS + tid] = sb;
    const int fl = (int)same | (int)same_a << 1 | (int)same_b << 2;
    if (fl != 7) atomicAnd(&s_same, fl);        // (an integer AND: the same in any order)
    __syncthreads();
    for (int w = LR_ESS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_red[tid] += s_red[tid + w];
            s_red[LR_ESS_THREADS + tid] += s_red[LR_ESS_THREADS + tid + w];
            s_red[2 * LR_ESS_THREADS + tid] += s_red[2 * LR_ESS_THREADS + tid + w];
        }
        __syncthreads();
    }
    const int all = s_same;
    const double m = (all & 1) ? x0 : s_red[0] / (double)n;
    const double mu_a = (all & 2) ? x0 : s_red[LR_ESS_THREADS] / (double)h;
    const double mu_b = (all & 4) ? xb : s_red[2 * LR_ESS_THREADS] / (double)h;
    __syncthreads();

    // ---- half-chain variances (centred, second pass) and the centred series, in place ----
    double va = 0.0, vb = 0.0;
    for (int j = tid; j < n; j += LR_ESS_THREADS) {
        const double v = x[j];
        if (j < h) va += (v - mu_a) * (v - mu_a);
        if (j >= n - h) vb += (v - mu_b) * (v - mu_b);
        x[j] = v - m;
    }
    s_red[tid] = va, s_red[LR_ESS_THREADS + tid] = vb;
    __syncthreads();
    for (int w = LR_ESS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_red[tid] += s_red[tid + w];
            s_red[LR_ESS_THREADS + tid] += s_red[LR_ESS_THREADS + tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* o = half + series * 4;
        o[0] = mu_a, o[1] = s_red[0] / (double)(h - 1);
        o[2] = mu_b, o[3] = s_red[LR_ESS_THREADS] / (double)(h - 1);
    }

    // ---- autocovariances a tile at a time, stop rule in lag order ----
    // g_t = sum_{j < n - t} d_j d_{j+t} / (n - t).  Pairs (g_{t-1}, g_t), t = 2, 4, ... < L: V += 2 (g_{t-1} + g_t)
    // while the pair sum is positive; stop_lag = the first t whose pair sum is not (or L if none).  Only lags <= L - 1
    // (and lag 0) are ever read.
    double g0 = 0.0, V = 0.0;             // (wave 0)
    int stop_lag = -1;
    for (int b = 0;; b += LR_ESS_THREADS) {
        const int lag = b + tid;
        double acc = 0.0;
        if (lag == 0 || lag < L) {
            const double* xl = x + lag;
            const int nt = n - lag;
            for (int j = 0; j < nt; ++j) acc += x[j] * xl[j];
            acc /= (double)nt;
        }
        s_g[1 + tid] = acc;
        __syncthreads();
        if (tid < 64) {
            if (b == 0) g0 = s_g[1], V = g0;
            for (int r = 0; r < LR_ESS_THREADS / 128 && stop_lag < 0; ++r) {
                const int t = b + 2 * (r * 64 + lane);
                const double p = s_g[t - b] + s_g[t - b + 1];       // g_{t-1} + g_t
                const bool valid = t >= 2;
                const bool stop = valid && (t >= L || !(p > 0.0));
                const unsigned long long mask = __ballot(stop);
                const int first = mask ? __ffsll((long long)mask) - 1 : 64;
                V += 2.0 * lr_ess_wave_sum(valid && lane < first ? p : 0.0);
                if (mask) {
                    const int ts = b + 2 * (r * 64 + first);
                    stop_lag = ts >= L ? L : ts;
                }
            }
            if (stop_lag < 0 && b + LR_ESS_THREADS >= L) stop_lag = L;   // the next pair would be t >= L: ran out
            if (tid == 0) {
                s_stop = stop_lag;
                s_g[0] = s_g[LR_ESS_THREADS];                             // g_{b+T-1} for the next tile's first pair
            }
        }
        __syncthreads();
        if (s_stop >= 0) break;
    }
    if (tid == 0) {
        double* o = chain_stats + series * 4;
        o[0] = m;
        if (g0 == 0.0) {
            o[1] = o[2] = NAN;
            o[3] = 0.0;
            stop_out[series] = 0;
        } else {
            const double act = V / g0;
            o[1] = (double)n / act;
            o[2] = act;
            o[3] = sqrt(V / (double)n);
            stop_out[series] = stop_lag;
        }
    }
}

// one work-group per column: pooled mean and ESS; split R-hat over the M = 2C half-chain sequences q = (c, first half),
// (c, second half), c = 0 .. C - 1.  col_stats[k] = {pooled_mean, pooled_ess, rhat}.
__global__ __launch_bounds__(LR_ESS_THREADS) void lr_ess_pool_kernel(const double* __restrict__ chain_stats,
                                                                   const double* __restrict__ half, lr_ess_geom g,
                                                                   double* __restrict__ col_stats) {
    __shared__ double s_a[LR_ESS_THREADS], s_b[LR_ESS_THREADS], s_m[LR_ESS_THREADS], s_w[LR_ESS_THREADS];
    __shared__ int s_n[LR_ESS_THREADS];
    const int tid = threadIdx.x, k = blockIdx.x, C = g.C;
    const double* cs = chain_stats + (size_t)k * C * 4;
    const double* hs = half + (size_t)k * C * 4;
    double sm = 0.0, se = 0.0, smu = 0.0, sw = 0.0;
    int nf = 0;
    for (int c = tid; c < C; c += LR_ESS_THREADS) {
        sm += cs[c * 4 + 0];
        const double e = cs[c * 4 + 1];
        if (isfinite(e)) se += e, ++nf;
        smu += hs[c * 4 + 0];
        smu += hs[c * 4 + 2];
        sw += hs[c * 4 + 1];
        sw += hs[c * 4 + 3];
    }
    s_a[tid] = sm, s_b[tid] = se, s_m[tid] = smu, s_w[tid] = sw, s_n[tid] = nf;
    __syncthreads();
    for (int w = LR_ESS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_a[tid] += s_a[tid + w], s_b[tid] += s_b[tid + w], s_m[tid] += s_m[tid + w], s_w[tid] += s_w[tid + w];
            s_n[tid] += s_n[tid + w];
        }
        __syncthreads();
    }
    const double M = 2.0 * C;
    const double mu = s_m[0] / M, W = s_w[0] / M;
    __syncthreads();
    double sb = 0.0;
    for (int c = tid; c < C; c += LR_ESS_THREADS) {
        const double da = hs[c * 4 + 0] - mu, db = hs[c * 4 + 2] - mu;
        sb += da * da;
        sb += db * db;
    }
    s_m[tid] = sb;
    __syncthreads();
    lr_ess_tree(s_m, tid);
    if (tid == 0) {
        const double h = (double)g.h;
        const double B = h / (M - 1.0) * s_m[0];
        const double var_plus = (h - 1.0) / h * W + B / h;
        double* o = col_stats + (size_t)k * 3;
        o[0] = s_a[0] / (double)C;
        o[1] = s_n[0] > 0 ? s_b[0] : NAN;
        o[2] = W == 0.0 ? NAN : sqrt(var_plus / W);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int lr_ess_setup(int32_t n_samples, int32_t n_chains, int32_t row_width, const int32_t* cols, int32_t n_cols,
                        double burnin, int32_t max_lag, lr_ess_geom* g) {
    if (n_samples < 1 || n_chains < 1 || n_chains > (1 << 22) || row_width < 1 || n_cols < 1 || max_lag < 1)
        return LR_ERR_SIZE;
    if (!cols) return LR_ERR_NULL;
    if (!(burnin >= 0.0 && burnin < 1.0)) return LR_ERR_SIZE;
    for (int i = 0; i < n_cols; ++i)
        if (cols[i] < 0 || cols[i] >= row_width) return LR_ERR_SIZE;
    // burn-in: int(burnin * S), Python's truncation of the fp64 product
    const long long burn = (long long)(burnin * (double)n_samples);
    const long long n = (long long)n_samples - burn;
    if (n < 4) return LR_ERR_SIZE;
    g->S = n_samples, g->C = n_chains, g->W = row_width, g->K = n_cols;
    g->burn = (int)burn, g->n = (int)n;
    g->L = (int)std::min<long long>(n - 1, max_lag);
    g->h = (int)(n / 2);
    return LR_OK;
}

struct lr_ess_ws {
    size_t half, centred, total;
};

static size_t lr_ess_up(size_t x) { return (x + 255) / 256 * 256; }

static void lr_ess_layout(const lr_ess_geom& g, lr_ess_ws* w) {
    const size_t series = (size_t)g.K * g.C;
    w->half = 0;
    w->centred = lr_ess_up(sizeof(double) * 4 * series);
    w->total = w->centred + (g.n > LR_ESS_LDS_ROWS ? lr_ess_up(sizeof(double) * series * (size_t)g.n) : 0);
}

extern "C" int64_t lr_ess_summary_workspace_bytes(int32_t n_samples, int32_t n_chains, int32_t row_width,
                                                  const int32_t* cols, int32_t n_cols, double burnin, int32_t max_lag) {
    lr_ess_geom g;
    const int rc = lr_ess_setup(n_samples, n_chains, row_width, cols, n_cols, burnin, max_lag, &g);
    if (rc != LR_OK) return rc;
    lr_ess_ws w;
    lr_ess_layout(g, &w);
    return (int64_t)w.total;
}

extern "C" int lr_ess_summary(const double* rows, int32_t n_samples, int32_t n_chains, int32_t row_width, const int32_t* cols,
                              int32_t n_cols, double burnin, int32_t max_lag, double* chain_stats, int32_t* stop_lag,
                              double* col_stats, void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!rows || !chain_stats || !stop_lag || !col_stats || !workspace) return LR_ERR_NULL;
    lr_ess_geom g;
    int rc = lr_ess_setup(n_samples, n_chains, row_width, cols, n_cols, burnin, max_lag, &g);
    if (rc != LR_OK) return rc;
    lr_ess_ws w;
    lr_ess_layout(g, &w);
    if (workspace_bytes < (int64_t)w.total) return LR_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    double* half = (double*)(ws + w.half);
    double* centred = (double*)(ws + w.centred);
    const bool lds = g.n <= LR_ESS_LDS_ROWS;
    const size_t lds_bytes = sizeof(double) * (LR_ESS_X + (lds ? (size_t)g.n : 0));
    const void* fn = lds ? reinterpret_cast<const void*>(&lr_ess_series_kernel<true>)
                         : reinterpret_cast<const void*>(&lr_ess_series_kernel<false>);
    if (lds_bytes > 64 * 1024) {
        // (per call: the attribute belongs to the function on the CURRENT device)
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    for (int k0 = 0; k0 < g.K; k0 += LR_ESS_COLS_PER_LAUNCH) {
        lr_ess_cols cs;
        cs.k0 = k0;
        cs.nk = std::min(LR_ESS_COLS_PER_LAUNCH, g.K - k0);
        for (int i = 0; i < LR_ESS_COLS_PER_LAUNCH; ++i) cs.col[i] = i < cs.nk ? cols[k0 + i] : 0;
        const dim3 grid((unsigned)g.C, (unsigned)cs.nk);
        if (lds)
            hipLaunchKernelGGL(lr_ess_series_kernel<true>, grid, dim3(LR_ESS_THREADS), lds_bytes, stream, rows, g, cs,
                               chain_stats, stop_lag, half, centred);
        else
            hipLaunchKernelGGL(lr_ess_series_kernel<false>, grid, dim3(LR_ESS_THREADS), lds_bytes, stream, rows, g, cs,
                               chain_stats, stop_lag, half, centred);
        if ((rc = (int)hipGetLastError()) != 0) return rc;
    }
    hipLaunchKernelGGL(lr_ess_pool_kernel, dim3((unsigned)g.K), dim3(LR_ESS_THREADS), 0, stream, (const double*)chain_stats,
                       (const double*)half, g, col_stats);
    return (int)hipGetLastError();
}
