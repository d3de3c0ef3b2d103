// lr_rtt.h - what the two summaries of the RJ trace share (lr_summary.hip: lr_rtt_summary; lr_score.hip: lr_rtt_score): the
// geometry of a call, the bin edges np.arange(a, b) writes, np.histogram's bin of a shift time, the K column's clamp and the
// span rules.  One definition, so the two units cannot drift apart: lr_rtt_score's values are lr_rtt_summary's bit for bit.
#pragma once
#include <cmath>

#include "lr_device.h"
#include "lr_internal.h"

#define LR_RTT_THREADS 256
#define LR_RTT_NONE 0x7FFF                       // bin index of a shift outside [e_0, e_nbins]: never counted
#define LR_RTT_L (LR_TRACE_HEAD)                 // trace row: birth rates ...
#define LR_RTT_TL (LR_TRACE_HEAD + LR_KMAX)      // ... interior birth shift times ...
#define LR_RTT_M (LR_TRACE_HEAD + 2 * LR_KMAX - 1)
#define LR_RTT_TM (LR_RTT_M + LR_KMAX)

struct lr_rtt_geom {
    int S, C, G;          // trace rows per chain, chains, groups (lr_rtt_summary: 1 pooled, C per chain)
    int burn;             // rows dropped at the start of every chain
    int per;              // rows kept per chain = S - burn
    long long n;          // samples per group
    long long n_in;       // samples inside the HPD window
    int n_bins;
    double a, delta;      // e_0 = a, e_1 = a + 1, e_j = a + j * delta (j >= 2): numpy's arange fill
};

// ---- edges and bins ------------------------------------------------------------------------------------------------
// np.arange(a, b) writes e_0 = a, e_1 = a + 1 and then e_j = a + j * delta with delta = e_1 - e_0 (numpy's DOUBLE_fill);
// the products and sums are rounded one at a time, as numpy's loop does (no fused multiply-add).
__device__ __forceinline__ double lr_rtt_edge(const lr_rtt_geom& g, int j) {
    if (j == 0) return g.a;
    if (j == 1) return __dadd_rn(g.a, 1.0);
    return __dadd_rn(g.a, __dmul_rn((double)j, g.delta));
}

// np.histogram(t, edges) with edges given as an array (the reference's call): bin i holds e_i <= t < e_{i+1}, the last bin
// also t == e_nbins; anything else (and NaN) is in no bin.
__device__ __forceinline__ int lr_rtt_bin(const lr_rtt_geom& g, double t) {
    const int nb = g.n_bins;
    if (!(t >= g.a) || !(t <= lr_rtt_edge(g, nb))) return LR_RTT_NONE;
    double f = floor(t - g.a);
    int j = (int)fmin(fmax(f, 0.0), (double)nb);
    while (j > 0 && t < lr_rtt_edge(g, j)) --j;
    while (j < nb && t >= lr_rtt_edge(g, j + 1)) ++j;
    return j == nb ? nb - 1 : j;
}

__device__ __forceinline__ int lr_rtt_k(double v) {   // K column -> 1..LR_KMAX (a row outside the range is clamped)
    int k = (int)v;
    return k < 1 ? 1 : (k > LR_KMAX ? LR_KMAX : k);
}

// ---- host: the span ------------------------------------------------------------------------------------------------
// bins: np.arange(a, b) has ceil(b - a) edges; the reference takes nbins = int(b - a) and indexes that many columns of a
// matrix with ceil(b - a) - 1: it breaks unless the two agree (b - a not integer valued).  Sets n_bins, a, delta.
static inline int lr_rtt_span(double start_age, double end_age, lr_rtt_geom* g) {
    if (!(std::isfinite(start_age) && std::isfinite(end_age) && end_age > start_age)) return LR_ERR_SIZE;
    const double span = end_age - start_age;
    if (span > (double)LR_MAX_BINS + 1.0) return LR_ERR_SIZE;
    const long long n_bins = (long long)std::ceil(span) - 1;
    if (n_bins < 1 || n_bins != (long long)span) return LR_ERR_SIZE;
    g->n_bins = (int)n_bins;
    g->a = start_age;
    g->delta = (start_age + 1.0) - start_age;
    return LR_OK;
}
