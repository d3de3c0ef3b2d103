// lr_waic.hip - pointwise WAIC over posterior draws: the lineage scan with the terms kept apart per lineage.
//
// A block owns a tile of lineages and walks the draws (lr_walk_draws, csrc/lr_drawwalk.h: the tables of a chunk of draws in
// LDS, the next chunk prefetched); the sink folds every term into the lineage's running state: one exponential (running
// maximum with a rescaled sum) and a Welford update.  Nothing of the [lineages, draws] matrix is ever stored.
//
//   lr_waic_kernel         grid (tiles, slices): per lineage and draw slice the state (max, rescaled sum, mean, M2, flag);
//                          with ONE slice it finishes the lineage and writes the tile's partial totals itself
//   lr_waic_merge_kernel   more than one slice: merges a lineage's slice states in slice order (Chan et al.), finishes
//   lr_waic_totals_kernel  one block: the tile partials in a fixed order (the pattern of lr_reduce_partials_kernel)
//
// Every reduction has a fixed order and the plan is a function of (n, n_bins, n_draws, model): results are bitwise
// reproducible.
#include <climits>
#include <cstdlib>

#include "lr_drawwalk.h"

#define LR_WAIC_NSTATE 5                                 /* max, sum, mean, M2, flag */
#define LR_WAIC_NPART 8                                  /* used, flagged, lppd, var, elpd, n(var > 0.4), max var, M2 of elpd */
#define LR_WAIC_VAR_WARN 0.4

struct lr_waic_shape {
    lr_draw_shape w;
    int slices;     // draw slices (grid.y)
    int dps;        // draws per slice
    int tiles;      // lineage tiles (grid.x)
};

struct lr_waic_state {
    double m, sum, mean, M2;
    int bad;
};

// one more draw: l = the lineage's term under it, inv = 1 / (draws so far, this one included)
__device__ __forceinline__ void lr_waic_update(lr_waic_state& st, double l, double inv) {
    st.bad |= !(fabs(l) < __builtin_inf());
    const double d = l - st.m;
    const double ed = exp(-fabs(d));
    if (d > 0.0) {
        st.sum = fma(st.sum, ed, 1.0);
        st.m = l;
    } else {
        st.sum += ed;
    }
    const double delta = l - st.mean;
    st.mean = fma(delta, inv, st.mean);
    st.M2 = fma(delta, l - st.mean, st.M2);
}

// b (nb draws) joins a (na draws), a's draws first
__device__ __forceinline__ void lr_waic_merge(lr_waic_state& a, double na, const lr_waic_state& b, double nb) {
    a.bad |= b.bad;
    const double m = fmax(a.m, b.m);
    a.sum = a.sum * exp(a.m - m) + b.sum * exp(b.m - m);
    a.m = m;
    const double nt = na + nb;
    const double delta = b.mean - a.mean;
    a.mean = a.mean + delta * (nb / nt);
    a.M2 = (a.M2 + b.M2) + (delta * delta) * (na * nb / nt);
}

// The finished lineages of a tile: the three outputs per lineage (NaN where flagged) and the tile's partial totals,
// tile_part[q * tiles + tile].  All threads of the block call.
__device__ __forceinline__ void lr_waic_emit(const lr_waic_state (&st)[LR_DRAW_LPT], const bool (&valid)[LR_DRAW_LPT],
                                             long long first, long long n, double n_draws, int tile, int tiles, int tid,
                                             double* __restrict__ out_pointwise, double* __restrict__ tile_part) {
    constexpr int NW = LR_DRAW_THREADS / LR_WAVE;
    __shared__ double red[NW];
    const double nan = __builtin_nan("");
    double used = 0.0, flagged = 0.0, s_lppd = 0.0, s_var = 0.0, s_elpd = 0.0, n_gt = 0.0, vmax = -__builtin_inf();
    double elpd[LR_DRAW_LPT];
    bool use[LR_DRAW_LPT];
#pragma unroll
    for (int k = 0; k < LR_DRAW_LPT; ++k) {
        const long long i = first + k * LR_DRAW_THREADS + tid;
        double lppd = st[k].m + lr_log(st[k].sum / n_draws);
        double mean = st[k].mean;
        double var = st[k].M2 / (n_draws - 1.0);
        use[k] = valid[k] && !st[k].bad;
        elpd[k] = 0.0;
        if (valid[k]) {
            if (st[k].bad) {
                lppd = mean = var = nan;
                flagged += 1.0;
            } else {
                elpd[k] = lppd - var;
                used += 1.0, s_lppd += lppd, s_var += var, s_elpd += elpd[k];
                n_gt += var > LR_WAIC_VAR_WARN ? 1.0 : 0.0;
                vmax = fmax(vmax, var);
            }
            out_pointwise[3 * i] = lppd, out_pointwise[3 * i + 1] = mean, out_pointwise[3 * i + 2] = var;
        }
    }
    (void)n;
    used = lr_block_sum(used, red, tid, NW);
    flagged = lr_block_sum(flagged, red, tid, NW);
    s_lppd = lr_block_sum(s_lppd, red, tid, NW);
    s_var = lr_block_sum(s_var, red, tid, NW);
    s_elpd = lr_block_sum(s_elpd, red, tid, NW);
    n_gt = lr_block_sum(n_gt, red, tid, NW);
    // the tile's sum of squares about ITS mean: the totals kernel joins the tiles as Chan et al. join samples
    const double tmean = used > 0.0 ? s_elpd / used : 0.0;
    double m2 = 0.0;
#pragma unroll
    for (int k = 0; k < LR_DRAW_LPT; ++k)
        if (use[k]) m2 += (elpd[k] - tmean) * (elpd[k] - tmean);
    m2 = lr_block_sum(m2, red, tid, NW);
    vmax = lr_block_max(vmax, red, tid, NW);
    if (tid == 0) {
        const size_t T = (size_t)tiles;
        tile_part[0 * T + tile] = used, tile_part[1 * T + tile] = flagged, tile_part[2 * T + tile] = s_lppd;
        tile_part[3 * T + tile] = s_var, tile_part[4 * T + tile] = s_elpd, tile_part[5 * T + tile] = n_gt;
        tile_part[6 * T + tile] = vmax, tile_part[7 * T + tile] = m2;
    }
}

// the walk's sink: draw d of the slice that starts at d0 is the (d - d0 + 1)-th of the lineage's state.  The state is
// updated in a copy: updated in place through the reference, the allocator keeps the running maximum twice in the draw
// loop (112 VGPRs for 108, three more instructions per draw in the loop that ends a chunk).
struct lr_waic_sink {
    lr_waic_state (&st)[LR_DRAW_LPT];
    int d0;
    __device__ __forceinline__ void operator()(int k, int d, double l) const {
        lr_waic_state t = st[k];
        lr_waic_update(t, l, 1.0 / (double)(d - d0 + 1));
        st[k] = t;
    }
};

// state[(q * slices + slice) * n + i]: field q of lineage i in draw slice `slice`
__global__ __launch_bounds__(LR_DRAW_THREADS) void lr_waic_kernel(
    const double* __restrict__ ts, const double* __restrict__ te, long long n, double t0, int n_bins, int n_cls, int H,
    double end_time, const double2* __restrict__ tables, int tab_stride, int n_draws, int chunk, int nbuf, int dps, int slices,
    double* __restrict__ out_pointwise, double* __restrict__ state, double* __restrict__ tile_part) {
    const int tid = threadIdx.x, tile = blockIdx.x, slice = blockIdx.y;
    const int d0 = slice * dps, d1 = min(d0 + dps, n_draws);
    const long long first = (long long)tile * LR_DRAW_TILE;

    bool valid[LR_DRAW_LPT];
    lr_waic_state st[LR_DRAW_LPT];
#pragma unroll
    for (int k = 0; k < LR_DRAW_LPT; ++k) {
        valid[k] = first + k * LR_DRAW_THREADS + tid < n;
        st[k].m = -__builtin_inf(), st[k].sum = 0.0, st[k].mean = 0.0, st[k].M2 = 0.0, st[k].bad = 0;
    }
    lr_walk_draws(ts, te, n, first, t0, n_bins, n_cls, H, end_time, tables, tab_stride, d0, d1, chunk, nbuf,
                  lr_waic_sink{st, d0});

    if (slices == 1) {
        lr_waic_emit(st, valid, first, n, (double)n_draws, tile, gridDim.x, tid, out_pointwise, tile_part);
        return;
    }
#pragma unroll
    for (int k = 0; k < LR_DRAW_LPT; ++k) {
        const long long i = first + k * LR_DRAW_THREADS + tid;
        if (!valid[k]) continue;
        const size_t plane = (size_t)slices * n, o = (size_t)slice * n + i;
        state[o] = st[k].m, state[plane + o] = st[k].sum, state[2 * plane + o] = st[k].mean, state[3 * plane + o] = st[k].M2;
        state[4 * plane + o] = st[k].bad ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(LR_DRAW_THREADS) void lr_waic_merge_kernel(const double* __restrict__ state, long long n,
                                                                        int n_draws, int dps, int slices,
                                                                        double* __restrict__ out_pointwise,
                                                                        double* __restrict__ tile_part) {
    const int tid = threadIdx.x, tile = blockIdx.x;
    const long long first = (long long)tile * LR_DRAW_TILE;
    const size_t plane = (size_t)slices * n;
    bool valid[LR_DRAW_LPT];
    lr_waic_state st[LR_DRAW_LPT];
#pragma unroll
    for (int k = 0; k < LR_DRAW_LPT; ++k) {
        const long long i = first + k * LR_DRAW_THREADS + tid;
        valid[k] = i < n;
        st[k].m = 0.0, st[k].sum = 1.0, st[k].mean = 0.0, st[k].M2 = 0.0, st[k].bad = 0;
        if (!valid[k]) continue;
        double na = 0.0;
        for (int sl = 0; sl < slices; ++sl) {
            const size_t o = (size_t)sl * n + i;
            lr_waic_state b;
            b.m = state[o], b.sum = state[plane + o], b.mean = state[2 * plane + o], b.M2 = state[3 * plane + o];
            b.bad = state[4 * plane + o] != 0.0;
            const double nb = (double)(min(dps, n_draws - sl * dps));
            if (sl == 0) st[k] = b;
            else lr_waic_merge(st[k], na, b, nb);
            na += nb;
        }
    }
    lr_waic_emit(st, valid, first, n, (double)n_draws, tile, gridDim.x, tid, out_pointwise, tile_part);
}

// out_totals[8] from the tile partials: thread j adds tiles j, j + 256, ... in ascending order, the 256 sums are then
// added by lr_ordered_sum
__global__ __launch_bounds__(256) void lr_waic_totals_kernel(const double* __restrict__ tile_part, int tiles,
                                                             double* __restrict__ out_totals) {
    __shared__ double red[256 + 16];
    const int j = threadIdx.x;
    const size_t T = (size_t)tiles;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double vmax = -__builtin_inf();
    for (int k = j; k < tiles; k += 256) {
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] += tile_part[q * T + k];
        vmax = fmax(vmax, tile_part[6 * T + k]);
    }
    double tot[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) tot[q] = lr_ordered_sum<256>(acc[q], red, j);
    __syncthreads();
    red[j] = vmax;
    __syncthreads();
    if (j == 0)
        for (int q = 1; q < 256; ++q) vmax = fmax(vmax, red[q]);
    const double used = tot[0];
    const double mean_all = used > 0.0 ? tot[4] / used : 0.0;
    double m2 = 0.0;
    for (int k = j; k < tiles; k += 256) {
        const double u = tile_part[k];
        if (u > 0.0) {
            const double dm = tile_part[4 * T + k] / u - mean_all;
            m2 += tile_part[7 * T + k] + u * (dm * dm);
        }
    }
    m2 = lr_ordered_sum<256>(m2, red, j);
    if (j == 0) {
        const double nan = __builtin_nan("");
        out_totals[0] = used, out_totals[1] = tot[1], out_totals[2] = tot[2], out_totals[3] = tot[3], out_totals[4] = tot[4];
        out_totals[5] = used >= 2.0 ? sqrt(used * (m2 / (used - 1.0))) : nan;
        out_totals[6] = tot[5];
        out_totals[7] = used > 0.0 ? vmax : nan;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int lr_waic_shape_of(long long n, int n_bins, int n_draws, int model, lr_waic_shape* p) {
    if (n < 1 || n_draws < 2) return LR_ERR_SIZE;
    const int rc = lr_draw_shape_of(n, n_bins, n_draws, model, &p->w);
    if (rc != LR_OK) return rc;
    const long long tiles = (n + LR_DRAW_TILE - 1) / LR_DRAW_TILE;
    if (tiles > INT_MAX) return LR_ERR_SIZE;
    p->tiles = (int)tiles;
    const char* env = getenv("LR_WAIC_SLICES");
    lr_draw_slices(tiles, n_draws, p->w.chunk, env ? atoi(env) : 0, &p->slices, &p->dps);
    return LR_OK;
}

// workspace: [tables | consts | tile partials | slice states], each 256-byte aligned
static void lr_waic_ws(const lr_waic_shape& p, long long n, int n_draws, size_t* o_tab, size_t* o_cst, size_t* o_part,
                       size_t* o_state, size_t* total) {
    size_t o = 0;
    *o_tab = o, o += lr_align_up64((long long)n_draws * p.w.tab_stride * sizeof(double2), 256);
    *o_cst = o, o += lr_align_up64((long long)n_draws * sizeof(double), 256);
    *o_part = o, o += lr_align_up64((long long)p.tiles * LR_WAIC_NPART * sizeof(double), 256);
    *o_state = o;
    if (p.slices > 1) o += lr_align_up64((long long)p.slices * n * LR_WAIC_NSTATE * sizeof(double), 256);
    *total = o;
}

extern "C" int64_t lr_waic_workspace_bytes(int64_t n, int32_t n_bins, int32_t n_draws, int32_t model) {
    lr_waic_shape p;
    const int rc = lr_waic_shape_of(n, n_bins, n_draws, model, &p);
    if (rc != LR_OK) return rc;
    size_t a, b, c, d, total;
    lr_waic_ws(p, n, n_draws, &a, &b, &c, &d, &total);
    return (int64_t)total;
}

extern "C" int lr_waic_plan(int64_t n, int32_t n_bins, int32_t n_draws, int32_t model, int32_t* out) {
    if (!out) return LR_ERR_NULL;
    lr_waic_shape p;
    const int rc = lr_waic_shape_of(n, n_bins, n_draws, model, &p);
    if (rc != LR_OK) return rc;
    out[0] = LR_DRAW_TILE, out[1] = p.w.chunk, out[2] = p.slices, out[3] = p.tiles;
    return LR_OK;
}

extern "C" int lr_waic_pointwise(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins,
                                 const double* lam_bins, const double* mu_bins, int32_t n_draws, int32_t model,
                                 const double* br_length, double end_time, double* out_pointwise, double* out_totals,
                                 void* workspace, int64_t workspace_bytes, void* stream_) {
    if (!ts || !te || !lam_bins || !mu_bins || !out_pointwise || !out_totals || !workspace) return LR_ERR_NULL;
    lr_waic_shape p;
    int rc = lr_waic_shape_of(n, n_bins, n_draws, model, &p);
    if (rc != LR_OK) return rc;
    size_t o_tab, o_cst, o_part, o_state, total;
    lr_waic_ws(p, n, n_draws, &o_tab, &o_cst, &o_part, &o_state, &total);
    hipStream_t stream = (hipStream_t)stream_;
    rc = lr_draw_begin(p.w, model, br_length, t0, total, workspace, workspace_bytes, o_tab, o_cst, lam_bins, mu_bins, n_bins,
                       n_draws, reinterpret_cast<const void*>(&lr_waic_kernel), stream);
    if (rc) return rc;
    char* ws = (char*)workspace;
    const double2* tables = (const double2*)(ws + o_tab);
    double* tile_part = (double*)(ws + o_part);
    double* state = (double*)(ws + o_state);
    hipLaunchKernelGGL(lr_waic_kernel, dim3(p.tiles, p.slices), dim3(LR_DRAW_THREADS), p.w.lds_bytes, stream, ts, te,
                       (long long)n, t0, n_bins, p.w.n_cls, p.w.H, end_time, tables, p.w.tab_stride, n_draws, p.w.chunk,
                       p.w.nbuf, p.dps, p.slices, out_pointwise, state, tile_part);
    rc = (int)hipGetLastError();
    if (rc) return rc;
    if (p.slices > 1) {
        hipLaunchKernelGGL(lr_waic_merge_kernel, dim3(p.tiles), dim3(LR_DRAW_THREADS), 0, stream, state, (long long)n, n_draws,
                           p.dps, p.slices, out_pointwise, tile_part);
        rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(lr_waic_totals_kernel, dim3(1), dim3(256), 0, stream, tile_part, p.tiles, out_totals);
    return (int)hipGetLastError();
}
