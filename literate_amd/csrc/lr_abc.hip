// lr_abc.hip - the count-level forward simulator of the niche-construction model with its distance to the observed per-bin
// statistics (lr_abc_simulate), and the binomial draw it is built on run on given uniforms (lr_abc_binomial):
// include/literate_hip_abc.h states the model, the draw, the draw addressing and the distance, and this file follows it
// operation by operation (tests/helpers/abc_ref.py restates it in numpy, bit for bit).
//
// One simulation per lane.  The batch simulators of lr_simbatch.hip follow every lineage and give a workgroup to a
// replicate, one block scan and barrier per step; ABC needs the per-bin counts alone, so the living lineages' uniforms
// collapse into B ~ Bin(n, pb) and D ~ Bin(n - B, pd / (1 - pb)) and a lane carries everything in registers: n, K, the
// bin's three running counters and the three row sums of the distance.  The loops over bins and steps are wave-uniform (a
// stopped lane idles under its predicate until the wave's last lane stops, then the wave skips the steps); only the chunk
// and search loops of the binomial diverge.  obs and weight are read once per bin by every lane at the same address: from
// LDS up to LR_ABC_LDS_BINS bins, from HBM above.  No atomics, no workspace; every output element is written by its lane.
//
// Every product, sum and quotient that numpy would round on its own is rounded on its own: written as __dmul_rn / __dadd_rn /
// __ddiv_rn, and this translation unit is compiled with -ffp-contract=off (build.TU_FLAGS) - in hipcc's headers the three
// are plain *, + and /, which the default contraction still fuses into an FMA where a product feeds a sum.
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_abc.h"
#include "lr_device.h"

#define LR_P_ABC 56          /* (lr_adej.hip holds 48-51) */
#define LR_ABC_THREADS 256

// where chunk c's uniform comes from: the Philox stream of a simulation, or a row of given uniforms
struct lr_abc_philox_src {
    lr_stream s;
    uint64_t it;             // step | (seed >> 32) << 32
    uint32_t odd;            // 0: births (idx 2 c), 1: deaths (idx 2 c + 1)
    __device__ __forceinline__ double operator()(uint32_t c) const { return lr_pair(s, it, LR_P_ABC, 2u * c + odd).a; }
};
struct lr_abc_array_src {
    const double* u;
    __device__ __forceinline__ double operator()(uint32_t c) const { return u[c]; }
};

// w^m by binary powering: at most 25 trips (m <= 2^24)
__device__ __forceinline__ double lr_abc_pow(double w, int m) {
    double f = 1.0, b = w;
    for (int e = m; e > 0;) {
        if (e & 1) f = __dmul_rn(f, b);
        e >>= 1;
        if (e > 0) b = __dmul_rn(b, b);
    }
    return f;
}

// the chunk length M of Bin(n, q), 0 < q <= 0.5, n >= 1
__device__ __forceinline__ int lr_abc_chunk(int n, double q) {
    const double len = __ddiv_rn(LR_ABC_CHUNK_MEAN, q);
    return len >= (double)n ? n : (int)len;
}

// Bin(n, p), 0 <= n <= LR_ABC_MAX_LIVING; *used = the uniforms consumed.  See the header for the scheme and its loop bounds.
template <class Src>
__device__ __forceinline__ int lr_abc_binom(int n, double p, const Src& src, int* used) {
    *used = 0;
    if (n <= 0 || !(p > 0.0)) return 0;
    if (p >= 1.0) return n;
    const bool flip = p > 0.5;
    const double q = flip ? __dadd_rn(1.0, -p) : p;
    const double w = __dadd_rn(1.0, -q), r = __ddiv_rn(q, w);
    const int M = lr_abc_chunk(n, q);
    const double fM = lr_abc_pow(w, M);
    int y = 0;
    uint32_t c = 0;
    for (int left = n; left > 0; left -= M, ++c) {
        const int m = left < M ? left : M;
        double f = m == M ? fM : lr_abc_pow(w, m);
        const int cap = m < LR_ABC_SEARCH_CAP ? m : LR_ABC_SEARCH_CAP;
        double u = src(c);
        int x = 0;
        while (u >= f && x < cap) {
            u = __dadd_rn(u, -f);
            ++x;
            f = __dmul_rn(f, __dmul_rn(r, __ddiv_rn((double)(m - x + 1), (double)x)));
        }
        y += x;
    }
    *used = (int)c;
    return flip ? n - y : y;
}

struct lr_abc_args {
    const double* theta;
    const int* n_start;
    const long long* sim_id;
    const double* obs;
    const double* weight;
    double* dist;
    int* flags;
    long long* counts;
    double* k_end;
    long long n_sims, id0;
    int n_bins, spb, max_living, lds;      // lds: the tables are staged in LDS
    uint32_t seed_lo, seed_hi;
};

__device__ __forceinline__ double lr_abc_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double lr_abc_min(double a, double b) { return b < a ? b : a; }

__global__ __launch_bounds__(LR_ABC_THREADS) void lr_abc_simulate_kernel(lr_abc_args g) {
    extern __shared__ double s_tab[];          // [2][3][n_bins] when g.lds
    const int nb = g.n_bins;
    if (g.lds) {
        for (int i = threadIdx.x; i < 3 * nb; i += LR_ABC_THREADS) s_tab[i] = g.obs[i], s_tab[3 * nb + i] = g.weight[i];
        __syncthreads();
    }
    const double* obs = g.lds ? s_tab : g.obs;
    const double* wgt = g.lds ? s_tab + 3 * nb : g.weight;
    const long long i = (long long)blockIdx.x * LR_ABC_THREADS + threadIdx.x;
    if (i >= g.n_sims) return;                 // (no barrier below)

    const double* th = g.theta + (size_t)i * LR_ABC_NPAR;
    const double l0 = th[0], m0 = th[1], K0 = th[2], Kmax = th[3], gg = th[4], hh = th[5];
    const int n0 = g.n_start[i];
    const long long id = g.sim_id ? g.sim_id[i] : g.id0 + i;
    int flags = 0;
    if (n0 < 1 || n0 > g.max_living || !(Kmax > 0.0) || id < 0 || id > 0xFFFFFFFFll) flags = LR_ABC_FLAG_REFUSED;
    if (!(isfinite(l0) && isfinite(m0) && isfinite(K0) && isfinite(Kmax) && isfinite(gg) && isfinite(hh))) flags = LR_ABC_FLAG_REFUSED;
    bool alive = flags == 0;

    const double spb = (double)g.spb, n0d = (double)n0, dl = __dadd_rn(l0, -m0);
    lr_abc_philox_src births, deaths;
    births.s = deaths.s = lr_stream{g.seed_lo, (uint32_t)id};
    births.odd = 0, deaths.odd = 1;
    int n = alive ? n0 : 0;
    double K = alive ? K0 : 0.0;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    const int last = nb * g.spb - 1;
    long long* cnt = g.counts ? g.counts + (size_t)i * 4 * nb : nullptr;

    for (int bin = 0; bin < nb; ++bin) {
        long long nB = 0, nD = 0, ls = 0;
        const int at_start = n;
        if (__any(alive)) {
            for (int s = 0; s < g.spb; ++s) {
                if (alive) {
                    const int t = bin * g.spb + s;
                    const double nd = (double)n;
                    // 1. the niche
                    const double grow = __dadd_rn(__dmul_rn(gg, __ddiv_rn(nd, Kmax)), hh);
                    const double room = __dadd_rn(1.0, -__ddiv_rn(K, Kmax));
                    const double dK = __ddiv_rn(__dmul_rn(__dmul_rn(grow, room), Kmax), spb);
                    K = lr_abc_max(n0d, __dadd_rn(K, dK));
                    // 2. the rates of this step
                    const double x = __ddiv_rn(__dmul_rn(dl, nd), K);
                    const double lt = __ddiv_rn(lr_abc_max(0.0, __dadd_rn(l0, -x)), spb);
                    const double mt = __ddiv_rn(lr_abc_max(0.0, __dadd_rn(m0, x)), spb);
                    // 3. the two draws
                    const double pb = lr_abc_min(1.0, lt);
                    const double pd = __dadd_rn(lr_abc_min(1.0, __dadd_rn(lt, mt)), -pb);
                    births.it = deaths.it = (uint64_t)(uint32_t)t | ((uint64_t)g.seed_hi << 32);
                    int used;
                    const int B = lr_abc_binom(n, pb, births, &used);
                    const int D = pb < 1.0 ? lr_abc_binom(n - B, __ddiv_rn(pd, __dadd_rn(1.0, -pb)), deaths, &used) : 0;
                    nB += B, nD += D, ls += n;
                    n = n + B - D;
                    if (n > g.max_living) flags |= LR_ABC_FLAG_OVERFLOW, alive = false;
                    else if (n == 0 && t < last) flags |= LR_ABC_FLAG_EXTINCT, alive = false;
                }
            }
        }
        const bool whole = flags == 0;          // the bin was simulated to its end
        if (cnt) {
            cnt[bin] = whole ? nB : 0;
            cnt[nb + bin] = whole ? nD : 0;
            cnt[2 * nb + bin] = whole ? (long long)at_start : 0;
            cnt[3 * nb + bin] = whole ? ls : 0;
        }
        if (whole) {
            const double w0 = wgt[bin], w1 = wgt[nb + bin], w2 = wgt[2 * nb + bin];
            const double time = __ddiv_rn((double)ls, spb);
            if (w0 != 0.0) d0 = __dadd_rn(d0, __dmul_rn(w0, fabs(__dadd_rn(__ddiv_rn((double)nB, time), -obs[bin]))));
            if (w1 != 0.0) d1 = __dadd_rn(d1, __dmul_rn(w1, fabs(__dadd_rn(__ddiv_rn((double)nD, time), -obs[nb + bin]))));
            if (w2 != 0.0) d2 = __dadd_rn(d2, __dmul_rn(w2, fabs(__dadd_rn((double)at_start, -obs[2 * nb + bin]))));
        }
    }
    g.dist[i] = flags ? INFINITY : __dadd_rn(__dadd_rn(d0, d1), d2);
    g.flags[i] = flags;
    if (g.k_end) g.k_end[i] = K;
}

struct lr_abc_binomial_args {
    const int* n;
    const double* p;
    const double* u;
    int* x;
    int* used;
    long long N;
    int n_u;
};

__global__ __launch_bounds__(LR_ABC_THREADS) void lr_abc_binomial_kernel(lr_abc_binomial_args g) {
    const long long i = (long long)blockIdx.x * LR_ABC_THREADS + threadIdx.x;
    if (i >= g.N) return;
    const int n = g.n[i];
    const double p = g.p[i];
    int x = -1, used = 0;
    if (n >= 0 && n <= LR_ABC_MAX_LIVING && !isnan(p)) {
        // the uniforms the draw will consume, before it reads any: its chunks
        long long need = 0;
        if (n > 0 && p > 0.0 && p < 1.0) {
            const int M = lr_abc_chunk(n, p > 0.5 ? __dadd_rn(1.0, -p) : p);
            need = ((long long)n + M - 1) / M;
        }
        if (need > g.n_u) {
            used = (int)need;
        } else {
            lr_abc_array_src src;
            src.u = g.u + (size_t)i * g.n_u;
            x = lr_abc_binom(n, p, src, &used);
        }
    }
    g.x[i] = x;
    g.used[i] = used;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
extern "C" int lr_abc_simulate(const lr_abc_problem* p) {
    if (!p || !p->theta || !p->n_start || !p->obs || !p->weight || !p->dist || !p->flags) return LR_ERR_NULL;
    if (p->n_sims < 1 || p->n_sims >= (1ll << 31)) return LR_ERR_SIZE;
    if (p->n_bins < 1 || p->n_bins > LR_MAX_BINS || p->steps_per_bin < 1) return LR_ERR_SIZE;
    if ((long long)p->n_bins * p->steps_per_bin >= (1ll << 31)) return LR_ERR_SIZE;
    if (p->max_living < 1 || p->max_living > LR_ABC_MAX_LIVING) return LR_ERR_SIZE;
    if (!p->sim_id && (p->id0 < 0 || p->id0 > (1ll << 32) - p->n_sims)) return LR_ERR_SIZE;
    lr_abc_args g;
    g.theta = p->theta, g.n_start = p->n_start, g.sim_id = (const long long*)p->sim_id, g.obs = p->obs, g.weight = p->weight;
    g.dist = p->dist, g.flags = p->flags, g.counts = (long long*)p->counts, g.k_end = p->k_end;
    g.n_sims = p->n_sims, g.id0 = p->id0;
    g.n_bins = p->n_bins, g.spb = p->steps_per_bin, g.max_living = p->max_living;
    g.lds = p->n_bins <= LR_ABC_LDS_BINS;
    g.seed_lo = (uint32_t)p->seed, g.seed_hi = (uint32_t)(p->seed >> 32);
    const size_t lds = g.lds ? sizeof(double) * 6 * (size_t)p->n_bins : 0;          // at most 48 KB
    const unsigned blocks = (unsigned)((p->n_sims + LR_ABC_THREADS - 1) / LR_ABC_THREADS);
    hipLaunchKernelGGL(lr_abc_simulate_kernel, dim3(blocks), dim3(LR_ABC_THREADS), lds, (hipStream_t)p->stream, g);
    return (int)hipGetLastError();
}

extern "C" int lr_abc_binomial(const lr_abc_binomial_problem* p) {
    if (!p || !p->n || !p->p || !p->u || !p->x || !p->used) return LR_ERR_NULL;
    if (p->N < 1 || p->N >= (1ll << 31) || p->n_u < 1 || p->N * (long long)p->n_u >= (1ll << 40)) return LR_ERR_SIZE;
    lr_abc_binomial_args g;
    g.n = p->n, g.p = p->p, g.u = p->u, g.x = p->x, g.used = p->used, g.N = p->N, g.n_u = p->n_u;
    const unsigned blocks = (unsigned)((p->N + LR_ABC_THREADS - 1) / LR_ABC_THREADS);
    hipLaunchKernelGGL(lr_abc_binomial_kernel, dim3(blocks), dim3(LR_ABC_THREADS), 0, (hipStream_t)p->stream, g);
    return (int)hipGetLastError();
}
