/*
 * literate_hip_abc.h - C ABI of libliterate_hip.so, approximate Bayesian computation around a count-level forward simulator
 * (literate_amd/csrc/lr_abc.hip): many simulations of the niche-construction model in one launch, one simulation per lane,
 * each scored against the observed per-bin statistics.  The model has no closed-form likelihood (the carrying capacity is a
 * state that grows with the diversity it carries, simulateRateABC.v2.py:92-97, 147-148), so it is fitted by simulation
 * (literate_amd/abc.py).  Nothing is kept per lineage: the per-lineage uniforms of lr_simulate_bd_batch are replaced by two
 * binomial draws per step.  The conventions and status codes are literate_hip.h's: device pointers unless marked "host", the
 * caller owns every buffer, asynchronous on the stream, 0 = ok, < 0 = LR_ERR_*, > 0 = a hipError_t; buffers may hold
 * anything on entry, an argument error has touched nothing, and the library keeps no state between calls.
 *
 * The stream rides in the descriptor (a hipStream_t, NULL = default stream), not in a last parameter of the entry point, as
 * in literate_hip_score.h: the call is asynchronous on that stream and returns after enqueueing.  Neither entry point takes
 * a workspace: a simulation lives in the registers of its lane.
 */
#ifndef LITERATE_HIP_ABC_H
#define LITERATE_HIP_ABC_H

#include "literate_hip.h"

#define LR_ABC_NPAR 6                /* theta = [l0, m0, K0, Kmax, g, h] */
#define LR_ABC_MAX_LIVING (1 << 24)  /* the largest max_living */
#define LR_ABC_CHUNK_MEAN 16.0       /* a binomial is cut into chunks of mean <= 16 */
#define LR_ABC_SEARCH_CAP 200        /* most steps of one chunk's sequential search */
#define LR_ABC_LDS_BINS 1024         /* obs and weight are staged in LDS up to this many bins (48 KB), read from HBM above */
#define LR_ABC_FLAG_OVERFLOW 1       /* the living count exceeded max_living */
#define LR_ABC_FLAG_EXTINCT 2        /* no lineage left before the last step */
#define LR_ABC_FLAG_REFUSED 4        /* n_start < 1 or > max_living, a parameter that is not finite, Kmax <= 0, an id outside
                                        [0, 2^32) */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The binomial draw ---------------------------------------------------------------------------------------------------
 * X ~ Bin(n, p) from uniforms u_0, u_1, ... in [0, 1), exact in distribution up to the fp64 rounding of the probabilities and
 * the search cap below.  Only IEEE add, multiply, divide and compare, each rounded on its own (no fused multiply-add, no exp,
 * log or pow), so numpy arithmetic on the same uniforms returns the same integer (tests/helpers/abc_ref.py):
 *   n <= 0 or not p > 0:  X = 0;   p >= 1:  X = n;   neither consumes a uniform.
 *   q = p > 0.5 ? 1 - p : p,  w = 1 - q,  r = q / w,  M = 16 / q >= n ? n : (int) (16 / q)        (32 <= 16 / q)
 *   chunk c = 0, 1, ... covers m = min(M, what is left of n) trials and consumes u_c:
 *     f = w^m by binary powering:  f = 1, b = w, e = m;  while e > 0 { if (e & 1) f = f * b;  e >>= 1;  if (e > 0) b = b * b; }
 *     x = 0, u = u_c;  while (u >= f && x < min(m, LR_ABC_SEARCH_CAP)) { u = u - f;  x = x + 1;  f = f * (r * ((m - x + 1) / x)); }
 *   Y = the sum of the chunks' x;   X = p > 0.5 ? n - Y : Y.
 * A chunk's count has mean m q <= 16, so the cap of 200 cuts off a tail below 1e-130; without it a uniform next to 1 would
 * walk to m, since the rounded pmf terms sum to less than 1.
 * Loop bounds as functions of the arguments: chunks = ceil(n / M) <= n q / 16 + 2 <= n / 32 + 2; the powering loop runs
 * floor(log2 m) + 1 <= 25 times per distinct chunk length (two lengths per draw: M and the remainder); the search runs at
 * most min(m, 200) times per chunk.
 *
 * ---- One simulation ---------------------------------------------------------------------------------------------------------
 * Simulation i has the id id0 + i, or sim_id[i] when that array is given, theta = theta[i, :] and starts with n = n_start[i]
 * living lineages and K = K0.  With spb = steps_per_bin, step t = 0 .. n_bins spb - 1 belongs to bin t / spb; with n living
 * at its start, every product, sum and quotient rounded on its own, in this order (max(a, b) = b > a ? b : a and min(a, b) =
 * b < a ? b : a, so a NaN second operand gives the first):
 *   1. K  = max((double) n_start, K + ((g (n / Kmax) + h) (1 - K / Kmax) Kmax) / spb)
 *   2. x  = ((l0 - m0) n) / K;   lt = max(0, l0 - x) / spb;   mt = max(0, m0 + x) / spb      (simulateRateABC.v2.py:156-164)
 *   3. pb = min(1, lt);  pd = min(1, lt + mt) - pb;  B ~ Bin(n, pb);  D ~ Bin(n - B, pd / (1 - pb)) when pb < 1, else 0;
 *      n = n + B - D
 * which is the script's "u < lt spawns, lt <= u < lt + mt kills" summed over the living lineages.  g = h = 0 is the fixed
 * niche the script runs (lr_simulate_bd mode 2).
 * Draws: Philox4x32-10 with the key (the low word of seed, id) and the counter (t, the high word of seed, LR_P_ABC = 56,
 * idx): chunk c of B reads member a of idx 2 c, chunk c of D member a of idx 2 c + 1 - oracle.philox.Stream(seed, id).pair(t
 * | (seed >> 32) << 32, 56, idx)[0].  A simulation therefore depends on (seed, id, theta, n_start, n_bins, steps_per_bin,
 * max_living) and the observed table alone, not on its position, the batch size or the grid.
 * After a step, n > max_living sets flag 1 and n = 0 before the last step sets flag 2; either stops the simulation.
 *
 * Per bin four integers, lr_simulate_bd_batch's counts: 0 births, 1 deaths, 2 living at the start of the bin, 3 lineage-steps
 * (the sum over the bin's steps of n at the start of the step).
 *
 * ---- The distance -----------------------------------------------------------------------------------------------------------
 * obs [3, n_bins]: birth rate, death rate, diversity at the start of the bin; weight [3, n_bins], 0 = the entry does not
 * count and is not evaluated (obs may hold anything there).  The simulated statistics of a bin: s_0 = births / (lineage-steps
 * / spb), s_1 = deaths / (lineage-steps / spb), s_2 = living at the start.  d_row = sum over the bins, ascending, of weight
 * |s - obs| (d_row = d_row + weight * |s - obs|, each operation rounded on its own, starting from 0), and
 *   dist = (d_0 + d_1) + d_2.
 * (One lane walks the bins in time order and keeps nothing per bin, so each row is summed on its own and the three sums are
 * added at the end, rather than all 3 n_bins terms in one running sum.)  With weight = 1 / (obs x the number of counted
 * entries) this is the script's mean relative deviation (simulateRateABC.v2.py:426-430).
 *
 * ---- Outputs ------------------------------------------------------------------------------------------------------------------
 *   dist   [n_sims] double;  +inf for a flagged simulation
 *   flags  [n_sims] int32, a set of LR_ABC_FLAG_*; a refused simulation (4) draws nothing
 *   counts [n_sims, 4, n_bins] int64, or NULL: zero from the bin in which a flagged simulation stopped (that bin included),
 *          all zero for a refused one
 *   k_end  [n_sims] double, or NULL: K after the last step taken; 0 for a refused simulation
 * Every element of every given output is written; dist and flags do not depend on whether counts or k_end is given.  No
 * floating-point atomics (no atomics at all): one lane writes the outputs of its simulation.
 */
typedef struct lr_abc_problem {
    const double* theta;      /* [n_sims, LR_ABC_NPAR] */
    const int32_t* n_start;   /* [n_sims] */
    const int64_t* sim_id;    /* [n_sims], or NULL for id0 + i */
    const double* obs;        /* [3, n_bins] */
    const double* weight;     /* [3, n_bins] */
    double* dist;             /* [n_sims] */
    int32_t* flags;           /* [n_sims] */
    int64_t* counts;          /* [n_sims, 4, n_bins], or NULL */
    double* k_end;            /* [n_sims], or NULL */
    int64_t n_sims, id0;
    int32_t n_bins, steps_per_bin, max_living, reserved;
    uint64_t seed;
    void* stream;             /* hipStream_t; NULL = default stream */
} lr_abc_problem;

/* lr_abc_simulate: one lane per simulation, 256 lanes per workgroup, every lane of a wave at the same step; obs and weight in
 *   LDS (n_bins <= LR_ABC_LDS_BINS), the bin's counters in registers, stored once per bin.
 *   Errors before any launch, in this order: LR_ERR_NULL: the descriptor, theta, n_start, obs, weight, dist or flags;
 *   LR_ERR_SIZE: n_sims < 1 or >= 2^31, n_bins < 1 or > LR_MAX_BINS, steps_per_bin < 1, n_bins steps_per_bin >= 2^31,
 *   max_living < 1 or > LR_ABC_MAX_LIVING, and without sim_id: id0 < 0 or id0 + n_sims > 2^32.                            */
int lr_abc_simulate(const lr_abc_problem* problem /* host */);

/* The device binomial on GIVEN uniforms, so that tests reach the branches Philox will not visit on demand: draw i is Bin(n[i],
 * p[i]) with u_c = u[i, c].  x[i] = the draw, used[i] = the uniforms it consumed (its chunks).  A draw that needs more than
 * n_u uniforms reads none: x[i] = -1, used[i] = the number it needs; n[i] < 0, n[i] > LR_ABC_MAX_LIVING or a NaN p[i]: x[i]
 * = -1, used[i] = 0.  Every element of x and used is written. */
typedef struct lr_abc_binomial_problem {
    const int32_t* n;         /* [N] */
    const double* p;          /* [N] */
    const double* u;          /* [N, n_u] */
    int32_t* x;               /* [N] */
    int32_t* used;            /* [N] */
    int64_t N;
    int32_t n_u, reserved;
    void* stream;             /* hipStream_t; NULL = default stream */
} lr_abc_binomial_problem;

/* lr_abc_binomial: one lane per draw.  Errors before any launch: LR_ERR_NULL: the descriptor or any of its five arrays;
 *   LR_ERR_SIZE: N < 1 or >= 2^31, n_u < 1 or N n_u >= 2^40.                                                               */
int lr_abc_binomial(const lr_abc_binomial_problem* problem /* host */);

#ifdef __cplusplus
}
#endif

#endif
