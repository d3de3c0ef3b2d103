// lr_trait.hip - trait-dependent rates (include/literate_hip_trait.h): every lineage's birth and death rate is the RJ skyline's
// times a logistic function of its trait.
//
//   lr_trait_weights_kernel   the streaming pass: block = (group of LR_TRAIT_CB states, lineage tile); a lineage is loaded
//                             once per block and scored under the group's states: one exponential, one division and one
//                             log1p per (lineage, state), at most four 64-bit LDS adds
//   lr_trait_final_kernel     one wave per state: the exact prefix sum of the difference array, the one rounding to fp64, and
//                             the tiles' Slog partials in a fixed tree
//   lr_trait_chain_kernel<BPL> one wave per chain: settles the pending trait proposal, runs lr_rjbin's iterations up to the
//                             next trait move (lr_rjbin_iter.h, unchanged) and proposes
//
// W is accumulated in integers (terms rounded once to 2^-LR_TRAIT_F), so it does not depend on the order of the atomics; the
// LDS accumulators exist in R copies (lane l uses copy l % R, the copies of an entry side by side in different banks) so
// that the lanes of a wave that hit the same bin - the normal case on input sorted by birth - do not serialise.  No
// floating-point atomics anywhere.
#include <hip/hip_runtime.h>

#include "../../include/literate_hip_trait.h"
#include "lr_chain.h"
#include "lr_internal.h"
#include "lr_rjbin_iter.h"

#define LR_TW_THREADS 256
#define LR_TW_WAVES (LR_TW_THREADS / LR_WAVE)
#define LR_TW_LDS_TARGET (40 * 1024)      /* LDS bytes per block the copies may fill, the Slog scratch included: four blocks fit a CU's 160 KiB */
#define LR_TRAIT_MAX_C (1 << 20)

struct lr_tw_shape {
    int tiles, groups, rshift;
    long long chunk;
    size_t lds_bytes;
};

// the tiles are a function of n alone: a state's Slog bits do not depend on n_bins, C or the device
static lr_tw_shape lr_tw_plan(long long n, int n_bins, int C) {
    lr_tw_shape p;
    long long t = (n + LR_TRAIT_TILE - 1) / LR_TRAIT_TILE;
    if (t > LR_TRAIT_MAX_TILES) t = LR_TRAIT_MAX_TILES;
    if (t < 1) t = 1;
    p.chunk = lr_align_up64((n + t - 1) / t, LR_TW_THREADS);
    p.tiles = (int)((n + p.chunk - 1) / p.chunk);
    p.groups = (C + LR_TRAIT_CB - 1) / LR_TRAIT_CB;
    const size_t one = (size_t)LR_TRAIT_CB * 2 * n_bins * 8;
    p.rshift = 5;
    const size_t scratch = (size_t)LR_TW_WAVES * LR_TRAIT_CB * 2 * 8;
    while (p.rshift > 0 && (one << p.rshift) + scratch > LR_TW_LDS_TARGET) --p.rshift;
    p.lds_bytes = (one << p.rshift) + scratch;
    return p;
}

static inline size_t lr_tw_acc_bytes(int n_bins, int C) { return (size_t)lr_align_up64((long long)C * 2 * n_bins * 8, 256); }
static inline size_t lr_tw_ws_bytes(const lr_tw_shape& p, int n_bins, int C) {
    return lr_tw_acc_bytes(n_bins, C) + (size_t)lr_align_up64((long long)C * p.tiles * 2 * 8, 256);
}

__global__ __launch_bounds__(LR_TW_THREADS) void lr_trait_weights_kernel(
    const double* __restrict__ ts, const double* __restrict__ te, const double* __restrict__ x, long long n, double t0, int W,
    const double* __restrict__ params, int C, long long chunk, int tiles, int rshift, long long* __restrict__ acc,
    double* __restrict__ slog_part) {
    extern __shared__ unsigned long long tw_lds[];          // [CB][2 W] << rshift accumulators, then [waves][CB][2] doubles
    const int tid = threadIdx.x, tile = blockIdx.y, c0 = blockIdx.x * LR_TRAIT_CB;      // (up to 2^17 groups: in x)
    const int n_acc = LR_TRAIT_CB * 2 * W;
    double* s_sl = reinterpret_cast<double*>(tw_lds + ((size_t)n_acc << rshift));
    for (int k = tid; k < (n_acc << rshift); k += LR_TW_THREADS) tw_lds[k] = 0ull;
    double px0[LR_TRAIT_CB], pk[LR_TRAIT_CB], ab[LR_TRAIT_CB], ad[LR_TRAIT_CB];
#pragma unroll
    for (int c = 0; c < LR_TRAIT_CB; ++c) {
        const bool ok = c0 + c < C;
        px0[c] = ok ? params[(size_t)(c0 + c) * 2] : 0.0, pk[c] = ok ? params[(size_t)(c0 + c) * 2 + 1] : 0.0;
        ab[c] = 0.0, ad[c] = 0.0;
    }
    __syncthreads();
    const int copy = tid & ((1 << rshift) - 1);
    const long long start = (long long)tile * chunk, end = min(start + chunk, n);
    for (long long i = start + tid; i < end; i += LR_TW_THREADS) {
        const double s = ts[i], e = te[i], xv = x[i];
        const double fl = floor(s), ce = ceil(e);
        // entry index = bin + 1; 0 = before the first bin, W + 1 = past the last (lr_bin_unit_events' own)
        int ia = min(max(__double2int_rz(fl - t0), -1), W) + 1;
        int ib = min(max(__double2int_rz(ce - t0), 0), W + 1);
        if (s != s) ia = W + 1;
        if (e != e) ib = W + 1;
        const bool born = ia >= 1 && ia <= W, died = ib >= 1 && ib <= W;       // counted in sp / ex
        const int bs = ia - 1, be = ib - 1;
        // the lineage's geometry, the same under every state: two partial bins (k1, k2) and the interior [da, db)
        int k1 = -1, k2 = -1, da = -1, db = -1;
        double t1 = 0.0, t2 = 0.0;
        if (s < e) {
            if (bs == be) {
                if (bs >= 0 && bs < W) k1 = bs, t1 = e - s;                    // born and dead in one bin
            } else {
                if (bs >= 0) k1 = bs, t1 = (fl + 1.0) - s;                     // (bs < be <= W)
                if (be < W) k2 = be, t2 = e - (ce - 1.0);                      // (be > bs >= -1)
                if (bs + 1 < be) da = bs + 1, db = be < W ? be : -1;           // born before t0: da = 0; alive past: no end
            }
        }
#pragma unroll
        for (int c = 0; c < LR_TRAIT_CB; ++c) {
            if (c0 + c >= C) continue;                                         // (uniform)
            const double z = pk[c] * (xv - px0[c]);
            const double u = exp(-fabs(z));                                    // in [0, 1]: no overflow for any finite z
            const double sg = (z >= 0.0 ? 1.0 : u) / (1.0 + u);
            const double ls = (z >= 0.0 ? 0.0 : z) - log1p(u);                 // log s = -softplus(-z)
            ab[c] += born ? ls : 0.0, ad[c] += died ? ls : 0.0;
            const int base = c * 2 * W;
            if (k1 >= 0) atomicAdd(tw_lds + (((size_t)(base + k1) << rshift) | copy), (unsigned long long)__double2ll_rn(sg * t1 * 0x1p38));
            if (k2 >= 0) atomicAdd(tw_lds + (((size_t)(base + k2) << rshift) | copy), (unsigned long long)__double2ll_rn(sg * t2 * 0x1p38));
            if (da >= 0) {
                const long long q = __double2ll_rn(sg * 0x1p38);
                atomicAdd(tw_lds + (((size_t)(base + W + da) << rshift) | copy), (unsigned long long)q);
                if (db >= 0) atomicAdd(tw_lds + (((size_t)(base + W + db) << rshift) | copy), (unsigned long long)(-q));
            }
        }
    }
    const int lane = tid & (LR_WAVE - 1), wave = tid / LR_WAVE;
#pragma unroll
    for (int c = 0; c < LR_TRAIT_CB; ++c) {
        const double a = lr_wave_sum(ab[c]), b = lr_wave_sum(ad[c]);
        if (lane == 0) s_sl[(wave * LR_TRAIT_CB + c) * 2] = a, s_sl[(wave * LR_TRAIT_CB + c) * 2 + 1] = b;
    }
    __syncthreads();
    // fold the copies and add the block's sums into the call's 64-bit accumulators: integer adds, order-free; the reader is
    // the next kernel on the stream
    const int R = 1 << rshift;
    for (int j = tid; j < n_acc; j += LR_TW_THREADS) {
        const int c = j / (2 * W);
        if (c0 + c >= C) continue;
        const unsigned long long* h = tw_lds + ((size_t)j << rshift);
        long long v = 0;
        for (int r = 0; r < R; ++r) v += (long long)h[(r + j) & (R - 1)];
        if (v) __hip_atomic_fetch_add(acc + (size_t)c0 * 2 * W + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid < 2 * LR_TRAIT_CB && c0 + (tid >> 1) < C) {
        double v = 0.0;
        for (int w = 0; w < LR_TW_WAVES; ++w) v += s_sl[w * LR_TRAIT_CB * 2 + tid];
        slog_part[((size_t)(c0 + (tid >> 1)) * tiles + tile) * 2 + (tid & 1)] = v;
    }
}

__global__ __launch_bounds__(LR_WAVE) void lr_trait_final_kernel(const long long* __restrict__ acc, const double* __restrict__ slog_part,
                                                                 int W, int tiles, double* __restrict__ Wout,
                                                                 double* __restrict__ slog_b, double* __restrict__ slog_d) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const long long* direct = acc + (size_t)c * 2 * W;
    const long long* diff = direct + W;
    // lane l owns the bins [l per, (l + 1) per)
    const int per = (W + LR_WAVE - 1) / LR_WAVE;
    const int b0 = min(lane * per, W), b1 = min(b0 + per, W);
    long long local = 0;
    for (int b = b0; b < b1; ++b) local += diff[b];
    long long incl = local;
    for (int d = 1; d < LR_WAVE; d <<= 1) {
        const long long up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    long long run = incl - local;
    for (int b = b0; b < b1; ++b) {
        run += diff[b];
        Wout[(size_t)c * W + b] = (double)(direct[b] + run) * 0x1p-38;          // the one rounding
    }
    double sb = 0.0, sd = 0.0;
    for (int t = lane; t < tiles; t += LR_WAVE) {
        sb += slog_part[((size_t)c * tiles + t) * 2], sd += slog_part[((size_t)c * tiles + t) * 2 + 1];
    }
    sb = lr_wave_sum(sb), sd = lr_wave_sum(sd);
    if (lane == 0) slog_b[c] = sb, slog_d[c] = sd;
}

static_assert(LR_TRAIT_F == 38, "the kernels scale by 0x1p38");

// the three enqueues of a pass; the arguments are checked by the callers
static int lr_tw_launch(const double* ts, const double* te, const double* x, long long n, double t0, int n_bins, const double* params,
                        int C, double* W, double* slog_b, double* slog_d, void* workspace, hipStream_t stream) {
    const lr_tw_shape p = lr_tw_plan(n, n_bins, C);
    char* ws = (char*)workspace;
    const size_t acc_bytes = lr_tw_acc_bytes(n_bins, C);
    hipError_t e = hipMemsetAsync(ws, 0, acc_bytes, stream);
    if (e != hipSuccess) return (int)e;
    if (p.lds_bytes > 64 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&lr_trait_weights_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)p.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(lr_trait_weights_kernel, dim3(p.groups, p.tiles), dim3(LR_TW_THREADS), p.lds_bytes, stream, ts, te, x, n, t0,
                       n_bins, params, C, p.chunk, p.tiles, p.rshift, (long long*)ws, (double*)(ws + acc_bytes));
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(lr_trait_final_kernel, dim3(C), dim3(LR_WAVE), 0, stream, (const long long*)ws, (const double*)(ws + acc_bytes),
                       n_bins, p.tiles, W, slog_b, slog_d);
    return (int)hipGetLastError();
}

static inline bool lr_trait_sizes_ok(int64_t n, int32_t n_bins, int32_t C) {
    return n >= 1 && n <= LR_TRAIT_MAX_N && n_bins >= 1 && n_bins <= LR_RJBIN_MAX_BINS && C >= 1 && C <= LR_TRAIT_MAX_C;
}

extern "C" int64_t lr_trait_weights_workspace_bytes(int64_t n, int32_t n_bins, int32_t C) {
    if (!lr_trait_sizes_ok(n, n_bins, C)) return LR_ERR_SIZE;
    return (int64_t)lr_tw_ws_bytes(lr_tw_plan(n, n_bins, C), n_bins, C);
}

extern "C" int lr_trait_weights_plan(int64_t n, int32_t n_bins, int32_t C, int32_t* out) {
    if (!out) return LR_ERR_NULL;
    if (!lr_trait_sizes_ok(n, n_bins, C)) return LR_ERR_SIZE;
    const lr_tw_shape p = lr_tw_plan(n, n_bins, C);
    out[0] = LR_TRAIT_CB, out[1] = p.tiles, out[2] = p.groups, out[3] = 1 << p.rshift;
    return LR_OK;
}

extern "C" int lr_trait_weights(const lr_trait_weights_problem* p) {
    if (!p) return LR_ERR_NULL;
    if (!p->ts || !p->te || !p->x || !p->params || !p->W || !p->Slog_birth || !p->Slog_death || !p->workspace) return LR_ERR_NULL;
    if (!lr_trait_sizes_ok(p->n, p->n_bins, p->C)) return LR_ERR_SIZE;
    if (!(p->t0 == floor(p->t0)) || fabs(p->t0) > 1e9) return LR_ERR_T0;
    if ((int64_t)lr_tw_ws_bytes(lr_tw_plan(p->n, p->n_bins, p->C), p->n_bins, p->C) > p->workspace_bytes) return LR_ERR_WORKSPACE;
    return lr_tw_launch(p->ts, p->te, p->x, p->n, p->t0, p->n_bins, p->params, p->C, p->W, p->Slog_birth, p->Slog_death, p->workspace,
                        (hipStream_t)p->stream);
}

// ---- the sampler --------------------------------------------------------------------------------------------------------
#define LR_TC_THREADS 256
#define LR_TC_WAVES (LR_TC_THREADS / LR_WAVE)

struct lr_trait_cfg {
    double win_x0[2], win_kappa[2], x0_lo, x0_hi, t_start, t_end;
};

// the trait scalars of a chain, wave-uniform
struct lr_trait_chain {
    double x0[2], kappa[2], slog[2], n_prop[2], n_acc[2];
};

// the workspace of the sampler: prop [C, 2] | Wp [C, n_bins] | slog_b [C] | slog_d [C] | the weights pass's own
struct lr_trait_ws {
    double *prop, *Wp, *slog_b, *slog_d;
    void* tw;
    size_t bytes;
};

static lr_trait_ws lr_trait_ws_of(void* workspace, long long n, int n_bins, int C) {
    lr_trait_ws w;
    char* p = (char*)workspace;
    size_t o = 0;
    w.prop = (double*)(p + o), o += (size_t)lr_align_up64((long long)C * 2 * 8, 256);
    w.Wp = (double*)(p + o), o += (size_t)lr_align_up64((long long)C * n_bins * 8, 256);
    w.slog_b = (double*)(p + o), o += (size_t)lr_align_up64((long long)C * 8, 256);
    w.slog_d = (double*)(p + o), o += (size_t)lr_align_up64((long long)C * 8, 256);
    w.tw = p + o, o += lr_tw_ws_bytes(lr_tw_plan(n, n_bins, C), n_bins, C);
    w.bytes = o;
    return w;
}

__device__ __forceinline__ void lr_trait_load(lr_trait_chain& T, const double* __restrict__ st, int lane) {
    const double sc = st[LR_TRAIT_ROW_SCALARS + lane];
    T.x0[0] = lr_bcast(sc, LR_TRAIT_S_X0_L), T.kappa[0] = lr_bcast(sc, LR_TRAIT_S_KAPPA_L);
    T.x0[1] = lr_bcast(sc, LR_TRAIT_S_X0_M), T.kappa[1] = lr_bcast(sc, LR_TRAIT_S_KAPPA_M);
    T.slog[0] = lr_bcast(sc, LR_TRAIT_S_SLOG_L), T.slog[1] = lr_bcast(sc, LR_TRAIT_S_SLOG_M);
    T.n_prop[0] = lr_bcast(sc, LR_TRAIT_S_PROPOSED_L), T.n_acc[0] = lr_bcast(sc, LR_TRAIT_S_ACCEPTED_L);
    T.n_prop[1] = lr_bcast(sc, LR_TRAIT_S_PROPOSED_M), T.n_acc[1] = lr_bcast(sc, LR_TRAIT_S_ACCEPTED_M);
}

__device__ __forceinline__ void lr_trait_store(const lr_trait_chain& T, double* __restrict__ st, int lane) {
    double so = 0.0;
    so = (lane == LR_TRAIT_S_X0_L) ? T.x0[0] : so, so = (lane == LR_TRAIT_S_KAPPA_L) ? T.kappa[0] : so;
    so = (lane == LR_TRAIT_S_X0_M) ? T.x0[1] : so, so = (lane == LR_TRAIT_S_KAPPA_M) ? T.kappa[1] : so;
    so = (lane == LR_TRAIT_S_SLOG_L) ? T.slog[0] : so, so = (lane == LR_TRAIT_S_SLOG_M) ? T.slog[1] : so;
    so = (lane == LR_TRAIT_S_PROPOSED_L) ? T.n_prop[0] : so, so = (lane == LR_TRAIT_S_ACCEPTED_L) ? T.n_acc[0] : so;
    so = (lane == LR_TRAIT_S_PROPOSED_M) ? T.n_prop[1] : so, so = (lane == LR_TRAIT_S_ACCEPTED_M) ? T.n_acc[1] : so;
    st[LR_TRAIT_ROW_SCALARS + lane] = so;
}

// a row of W in the state: the bins behind n_bins are written as 0
template <int BPL>
__device__ __forceinline__ void lr_trait_store_w(const double (&w)[BPL], double* __restrict__ row, int lane) {
#pragma unroll
    for (int i = 0; i < BPL; ++i) row[lane + LR_WAVE * i] = w[i];
    for (int b = lane + LR_WAVE * BPL; b < LR_RJBIN_MAX_BINS; b += LR_WAVE) row[b] = 0.0;
}

// the proposal of trait iteration `it`: the side and the (x0', kappa') of that side
__device__ __forceinline__ int lr_trait_propose(const lr_trait_chain& T, const lr_trait_cfg& tc, const lr_stream& rng, long long it,
                                                double* x0p, double* kp) {
#pragma clang fp contract(off)          // a product and a sum, each rounded: the restatement's bits, not an FMA's
    const int side = lr_pair(rng, (uint64_t)it, LR_P_TRAIT_MOVE, 0).a < 0.5 ? 0 : 1;
    const lr_u2 u = lr_pair(rng, (uint64_t)it, LR_P_TRAIT_MOVE, 1);
    *x0p = T.x0[side] + (u.a - 0.5) * tc.win_x0[side];
    *kp = T.kappa[side] + (u.b - 0.5) * tc.win_kappa[side];
    return side;
}

// the trace row: the engines' row with Slog in the likelihood and the kappas' Normal(0, 1) log densities in the prior
__device__ __forceinline__ void lr_trait_trace_row(const lr_rjbin_chain& S, const lr_trait_chain& T, const lr_rjbin_run& run, long long it,
                                                   double* __restrict__ row, int lane) {
    lr_rjbin_chain S2 = S;
    S2.likA = S.likA + (T.slog[0] + T.slog[1]);
    S2.priorA = S.priorA + ((-0.5 * T.kappa[0] * T.kappa[0] - 0.5 * T.kappa[1] * T.kappa[1]) - 1.8378770664093453 /* log 2 pi */);
    lr_rjbin_trace_row(S2, run, it, row, lane);
    double h = 0.0;
    h = (lane == 0) ? T.x0[0] : h, h = (lane == 1) ? T.kappa[0] : h, h = (lane == 2) ? T.x0[1] : h, h = (lane == 3) ? T.kappa[1] : h;
    h = (lane == 4) ? T.slog[0] : h, h = (lane == 5) ? T.slog[1] : h, h = (lane == 6) ? T.n_acc[0] : h, h = (lane == 7) ? T.n_acc[1] : h;
    if (lane < 8) row[LR_TRACE_W + lane] = h;
}

// mode 0: init, the birth side's W and Slog (the pass ran on the birth parameters) -> state
// mode 1: init, the death side's -> state, then the baseline's start
// mode 2: settle trait iteration `settle_it` (< 0: none), the baseline iterations [it_begin, it_end), propose trait iteration
//         `propose_it` (< 0: none) -> prop
template <int BPL>
__global__ __launch_bounds__(LR_TC_THREADS) void lr_trait_chain_kernel(
    const double* __restrict__ sp, const double* __restrict__ ex, lr_rjbin_cfg cfg, lr_trait_cfg tc, int mode, double* __restrict__ state,
    unsigned int* __restrict__ warn, double* __restrict__ prop, const double* __restrict__ Wp, const double* __restrict__ slog_b,
    const double* __restrict__ slog_d, long long settle_it, long long it_begin, long long it_end, long long propose_it,
    long long slot, double* __restrict__ rows) {
    const int lane = threadIdx.x & (LR_WAVE - 1), wave = threadIdx.x / LR_WAVE;
    const int c = blockIdx.x * LR_TC_WAVES + wave;
    if (c >= cfg.n_chains) return;          // the whole wave: no barrier anywhere below
    const int n_bins = cfg.n_bins;
    const lr_stream rng{cfg.seed, (uint32_t)(cfg.chain0 + c)};
    const lr_rjbin_run run = lr_rjbin_run_of(cfg, tc.t_start, tc.t_end);
    double* st = state + (size_t)c * LR_TRAIT_STATE_W;
    lr_trait_chain T;
    double wp[BPL];
#pragma unroll
    for (int i = 0; i < BPL; ++i) wp[i] = (mode != 2 || settle_it >= 0) && lane + LR_WAVE * i < n_bins ? Wp[(size_t)c * n_bins + lane + LR_WAVE * i] : 0.0;
    if (mode == 0) {
        T.x0[0] = prop[2 * c], T.kappa[0] = prop[2 * c + 1], T.slog[0] = slog_b[c];
        T.x0[1] = T.kappa[1] = T.slog[1] = 0.0, T.n_prop[0] = T.n_prop[1] = T.n_acc[0] = T.n_acc[1] = 0.0;
        lr_trait_store(T, st, lane);
        lr_trait_store_w<BPL>(wp, st + LR_TRAIT_ROW_WL, lane);
        return;
    }
    lr_trait_load(T, st, lane);
    // the bins: sp, br = WL, d_ex = ex, d_br = WM; model 2 keeps the two exposures apart and needs no log br
    lr_rjbin_bins<BPL> B;
#pragma unroll
    for (int i = 0; i < BPL; ++i) {
        const int b = lane + LR_WAVE * i;
        const bool in = b < n_bins;
        B.sp[i] = in ? sp[b] : 0.0, B.d_ex[i] = in ? ex[b] : 0.0, B.lk[i] = 0.0;
        B.br[i] = in ? st[LR_TRAIT_ROW_WL + b] : 0.0;
        B.d_br[i] = (in && mode == 2) ? st[LR_TRAIT_ROW_WM + b] : 0.0;
    }
    lr_rjbin_chain S;
    if (mode == 1) {
        T.x0[1] = prop[2 * c], T.kappa[1] = prop[2 * c + 1], T.slog[1] = slog_d[c];
#pragma unroll
        for (int i = 0; i < BPL; ++i) B.d_br[i] = wp[i];
        lr_trait_store_w<BPL>(wp, st + LR_TRAIT_ROW_WM, lane);
        lr_rjbin_start<BPL>(S, B, cfg, run, rng, (size_t)c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, lane);
        lr_rjbin_store(S, st, lane);
        lr_trait_store(T, st, lane);
        return;
    }
    lr_rjbin_load(S, st, lane);
    long long until_row = (cfg.s_freq - (settle_it >= 0 ? settle_it : it_begin) % cfg.s_freq) % cfg.s_freq;
    if (settle_it >= 0) {
        double x0p, kp;
        const int side = lr_trait_propose(T, tc, rng, settle_it, &x0p, &kp);
        const double log_u = lr_log(lr_pair(rng, (uint64_t)settle_it, LR_P_TRAIT_ACCEPT, 0).a);
        // the baseline likelihood of the proposed bins: recomputed by the same fixed tree, not updated
        lr_rjbin_bins<BPL> Bp = B;
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            if (side == 0) Bp.br[i] = wp[i];
            else Bp.d_br[i] = wp[i];
        }
        double logL, logM;
        lr_rjbin_log_rates(S.L, S.M, lane, &logL, &logM);
        const double lik = lr_rjbin_loglik<BPL>(Bp, cfg.model, n_bins, S.L, logL, S.eL, S.KL, S.M, logM, S.eM, S.KM, lane);
        const double slog_p = side == 0 ? slog_b[c] : slog_d[c];
        const double dprior = -0.5 * kp * kp + 0.5 * T.kappa[side] * T.kappa[side];
        const double delta = (lik + slog_p) - (S.likA + T.slog[side]) + dprior;
        const bool in_range = x0p >= tc.x0_lo && x0p <= tc.x0_hi;
        T.n_prop[side] += 1.0;
        if (in_range && delta >= log_u) {
            T.x0[side] = x0p, T.kappa[side] = kp, T.slog[side] = slog_p, T.n_acc[side] += 1.0;
            S.likA = lik, B = Bp;
            lr_trait_store_w<BPL>(wp, st + (side == 0 ? LR_TRAIT_ROW_WL : LR_TRAIT_ROW_WM), lane);
        }
        const bool sample = until_row == 0;
        until_row = sample ? cfg.s_freq - 1 : until_row - 1;
        if (sample) {
            lr_trait_trace_row(S, T, run, settle_it, rows + ((size_t)slot * cfg.n_chains + c) * LR_TRAIT_ROW_W, lane);
            slot += 1;
        }
    }
    for (long long it = it_begin; it < it_end; ++it) {
        lr_rjbin_iterate<BPL, false>(S, B, cfg, run, rng, it, 1.0, warn, lane);
        const bool sample = until_row == 0;
        until_row = sample ? cfg.s_freq - 1 : until_row - 1;
        if (sample) {
            lr_trait_trace_row(S, T, run, it, rows + ((size_t)slot * cfg.n_chains + c) * LR_TRAIT_ROW_W, lane);
            slot += 1;
        }
    }
    if (propose_it >= 0) {
        double x0p, kp;
        lr_trait_propose(T, tc, rng, propose_it, &x0p, &kp);
        if (lane == 0) prop[2 * c] = x0p, prop[2 * c + 1] = kp;
    }
    lr_rjbin_store(S, st, lane);
    lr_trait_store(T, st, lane);
}

// prop [C, 2] <- the side's pair of params0 [C, 4] (NULL: zeros)
__global__ void lr_trait_fill_kernel(const double* __restrict__ params0, int side, int C, double* __restrict__ prop) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2 * C) return;
    prop[j] = params0 ? params0[(size_t)(j >> 1) * 4 + 2 * side + (j & 1)] : 0.0;
}

struct lr_trait_launch_args {
    int mode;
    long long settle_it, it_begin, it_end, propose_it, slot;
    double* rows;
};

template <int BPL>
static void lr_trait_launch_bpl(const lr_trait_problem* p, const lr_rjbin_cfg& cfg, const lr_trait_cfg& tc, const lr_trait_ws& w,
                                const lr_trait_launch_args& a) {
    const unsigned blocks = (unsigned)((cfg.n_chains + LR_TC_WAVES - 1) / LR_TC_WAVES);
    hipLaunchKernelGGL(lr_trait_chain_kernel<BPL>, dim3(blocks), dim3(LR_TC_THREADS), 0, (hipStream_t)p->stream, p->sp, p->ex, cfg, tc,
                       a.mode, p->state, (unsigned int*)p->warn, w.prop, (const double*)w.Wp, (const double*)w.slog_b,
                       (const double*)w.slog_d, a.settle_it, a.it_begin, a.it_end, a.propose_it, a.slot, a.rows);
}

static int lr_trait_launch(const lr_trait_problem* p, const lr_rjbin_cfg& cfg, const lr_trait_cfg& tc, const lr_trait_ws& w,
                           const lr_trait_launch_args& a) {
    const int bpl = (cfg.n_bins + LR_WAVE - 1) / LR_WAVE;
    if (bpl <= 1) lr_trait_launch_bpl<1>(p, cfg, tc, w, a);
    else if (bpl <= 2) lr_trait_launch_bpl<2>(p, cfg, tc, w, a);
    else if (bpl <= 4) lr_trait_launch_bpl<4>(p, cfg, tc, w, a);
    else lr_trait_launch_bpl<8>(p, cfg, tc, w, a);
    return (int)hipGetLastError();
}

static int lr_trait_pass(const lr_trait_problem* p, const lr_trait_ws& w) {
    return lr_tw_launch(p->ts, p->te, p->x, p->n, p->t0, p->n_bins, w.prop, p->C, w.Wp, w.slog_b, w.slog_d, w.tw, (hipStream_t)p->stream);
}

// the checks of both entry points, in the header's order -> cfg, tc
static int lr_trait_args(const lr_trait_problem* p, bool steps, int64_t it0, int64_t n_iters, int32_t s_freq, const double* rows,
                         int64_t rows_cap, int64_t slot0, lr_rjbin_cfg* cfg, lr_trait_cfg* tc) {
    int64_t need = 0;
    const bool counts_ok = !steps || lr_rows_due(it0, n_iters, s_freq, &need);
    if (!p) return LR_ERR_NULL;
    if (!p->ts || !p->te || !p->x || !p->sp || !p->ex || !p->state || !p->warn || !p->workspace ||
        (steps && !rows && counts_ok && need > 0))
        return LR_ERR_NULL;
    if (!lr_trait_sizes_ok(p->n, p->n_bins, p->C) || p->trait_every < 0) return LR_ERR_SIZE;
    if (!(p->t0 == floor(p->t0)) || fabs(p->t0) > 1e9) return LR_ERR_T0;
    if (!(p->update_fraction >= 0.0 && p->update_fraction <= 1.0) || !(p->poisson_HP >= 0.0)) return LR_ERR_MODEL;
    if (!(p->win_x0[0] >= 0.0 && p->win_x0[1] >= 0.0 && p->win_kappa[0] >= 0.0 && p->win_kappa[1] >= 0.0) || !(p->x0_lo <= p->x0_hi) ||
        !(p->start_time < p->end_time))
        return LR_ERR_MODEL;
    if ((int64_t)lr_trait_ws_of(p->workspace, p->n, p->n_bins, p->C).bytes > p->workspace_bytes) return LR_ERR_WORKSPACE;
    if (steps && (!counts_ok || slot0 < 0 || rows_cap < 0 || rows_cap - slot0 < need)) return LR_ERR_SIZE;
    cfg->poisson_HP = p->poisson_HP, cfg->update_fraction = p->update_fraction, cfg->mult_l = 2.0 * std::log(LR_MULT_D);
    cfg->rows_cap = steps ? rows_cap : 0, cfg->slot0 = steps ? slot0 : 0, cfg->chain0 = p->chain0;
    cfg->n_bins = p->n_bins, cfg->n_chains = p->C, cfg->chains_per_rep = p->C;
    cfg->model = LR_MODEL_KEIDING, cfg->const_rates = p->const_rates ? 1 : 0, cfg->const_death_rate = p->const_death_rate ? 1 : 0;
    cfg->use_rate_HP = p->use_rate_HP ? 1 : 0, cfg->s_freq = steps ? s_freq : 1, cfg->seed = (uint32_t)p->seed;
    tc->win_x0[0] = p->win_x0[0], tc->win_x0[1] = p->win_x0[1], tc->win_kappa[0] = p->win_kappa[0], tc->win_kappa[1] = p->win_kappa[1];
    tc->x0_lo = p->x0_lo, tc->x0_hi = p->x0_hi, tc->t_start = p->start_time, tc->t_end = p->end_time;
    return LR_OK;
}

extern "C" int64_t lr_trait_workspace_bytes(int64_t n, int32_t n_bins, int32_t C) {
    if (!lr_trait_sizes_ok(n, n_bins, C)) return LR_ERR_SIZE;
    return (int64_t)lr_trait_ws_of(nullptr, n, n_bins, C).bytes;
}

extern "C" int lr_trait_init(const lr_trait_problem* p, const double* params0) {
    lr_rjbin_cfg cfg;
    lr_trait_cfg tc;
    int rc = lr_trait_args(p, false, 0, 0, 1, nullptr, 0, 0, &cfg, &tc);
    if (rc != LR_OK) return rc;
    const lr_trait_ws w = lr_trait_ws_of(p->workspace, p->n, p->n_bins, p->C);
    for (int side = 0; side < 2; ++side) {
        hipLaunchKernelGGL(lr_trait_fill_kernel, dim3((2 * p->C + 255) / 256), dim3(256), 0, (hipStream_t)p->stream, params0, side, p->C,
                           w.prop);
        if ((rc = (int)hipGetLastError())) return rc;
        if ((rc = lr_trait_pass(p, w))) return rc;
        const lr_trait_launch_args a{side, -1, 0, 0, -1, 0, nullptr};
        if ((rc = lr_trait_launch(p, cfg, tc, w, a))) return rc;
    }
    return LR_OK;
}

extern "C" int lr_trait_steps(const lr_trait_problem* p, int64_t it0, int64_t n_iters, int32_t s_freq, double* rows, int64_t rows_cap,
                              int64_t slot0) {
    lr_rjbin_cfg cfg;
    lr_trait_cfg tc;
    int rc = lr_trait_args(p, true, it0, n_iters, s_freq, rows, rows_cap, slot0, &cfg, &tc);
    if (rc != LR_OK) return rc;
    if (n_iters == 0) return LR_OK;
    const lr_trait_ws w = lr_trait_ws_of(p->workspace, p->n, p->n_bins, p->C);
    const long long end = it0 + n_iters, te = p->trait_every;
    // the slot of the row of iteration j, were one due: the rows due from it0 .. j - 1 come before it
    auto slot_of = [&](long long j) { return slot0 + ((j + s_freq - 1) / s_freq - (it0 + s_freq - 1) / s_freq); };
    long long it = it0, settle = -1;
    for (;;) {
        const long long next = te > 0 ? it + (te - 1 - it % te) : end;          // the first trait iteration >= it
        const long long b_end = next < end ? next : end;
        const long long propose = next < end ? next : -1;
        const lr_trait_launch_args a{2, settle, it, b_end, propose, slot_of(settle >= 0 ? settle : it), rows};
        if ((rc = lr_trait_launch(p, cfg, tc, w, a))) return rc;
        if (propose < 0) break;
        if ((rc = lr_trait_pass(p, w))) return rc;
        settle = propose, it = propose + 1;
    }
    return LR_OK;
}
