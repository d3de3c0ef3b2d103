/*
 * literate_hip_age.h - C ABI of libliterate_hip.so, the lifespan check: posterior predictive deaths and hazard by age
 * (literate_amd/csrc/lr_age.hip).  The conventions, status codes and LR_MAX_BINS are literate_hip.h's: device pointers
 * unless marked "host", the caller owns every buffer, asynchronous on `stream`, 0 = ok, < 0 = LR_ERR_*, > 0 = a
 * hipError_t; buffers may hold anything on entry, and an argument error has touched nothing.
 */
#ifndef LITERATE_HIP_AGE_H
#define LITERATE_HIP_AGE_H

#include "literate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Deaths by age under posterior draws of the death rates -----------------------------------------------------------------
 * The three samplers share one assumption none of their other checks tests: a lineage's chance of dying does not depend on
 * its age.  lr_ppc_age conditions on the observed birth times, draws a death time for each of the n lineages under each of
 * the n_draws rows of mu_bins [n_draws, n_bins] (per-bin death rates, bin b = [t0 + b, t0 + b + 1)), and counts deaths and
 * survivors per age class beside the observed ones.  A = n_bins age classes of width one bin; T_c = t0 + n_bins, the end of
 * the modelled window.  Every product, sum, difference and quotient below is rounded on its own (no fused multiply-add), so
 * that a numpy restatement gives the same doubles.
 *   Lineage i, from the data only:  x = ts_i - t0.  It is USED iff 0 <= x < n_bins and te_i > ts_i (NaN fails both).
 *     jb = floor(x), fs = x - jb.  It is observed DEAD iff te_i <= T_c (the rule by which ex_events counts a death), else
 *     CENSORED at T_c.  Observed class = min(floor((dead ? te_i : T_c) - ts_i), A - 1); censor class
 *     c_i = min(floor(T_c - ts_i), A - 1).
 *   out_obs [2, A]: out_obs[0][a] = observed dead of class a, out_obs[1][a] = censored of class a; used lineages only.
 *   Draw s:  C_s[0] = 0, C_s[b + 1] = C_s[b] + mu[s, b], added one after the other (np.cumsum, not a tree).  The draw is
 *     FLAGGED iff some mu[s, b] is not finite or < 0, or C_s[n_bins] is not finite; out_rep[s] is then all -1.
 *   Pair (i, s), used lineage and unflagged draw:  u = member a of Philox4x32-10 with key ((uint32) seed,
 *     (uint32) (seed >> 32)) and counter (i low, i high, purpose 41, s), u_a as everywhere in this library;
 *     E = -log(1 - u);  target = (C_s[jb] + mu[s, jb] fs) + E;  b = the smallest bin in [jb, n_bins) with C_s[b + 1] > target
 *     (strict: mu[s, b] > 0 there).  No such bin: the lineage survives, out_rep[s][1][c_i] += 1.  Otherwise
 *     t_in = (target - C_s[b]) / mu[s, b], l = ((double) b + t_in) - x, class = min(max(floor(l), 0), A - 1),
 *     out_rep[s][0][class] += 1.
 *   out_rep [n_draws, 2, A];  out_totals [4] = {lineages used, lineages unused, draws used, draws flagged}.
 * The lineage index of the Philox counter is the position in ts / te: the result is a function of (ts, te in their given
 * order, t0, n_bins, mu_bins, seed) alone.  All outputs are exact integers reached by integer atomics only, no
 * floating-point ones, so they do not depend on the plan; the one place where the device and a host restatement may part is
 * the logarithm (the device's is within 1.2 ulp), which matters only to a pair whose target lies within a few ulp of a
 * table step or whose lifespan lies within a few ulp of a class edge.
 * lr_ppc_age_plan: out (host int32[4]) = {lineages per tile, draws per slice, slices, tiles}, a function of the three sizes
 * alone (tiles capped at 2^31 - 1 in `out`): a workgroup owns a tile of lineages and walks the draws of one slice.
 * LR_PPC_AGE_SLICES=k in the environment (read at every call; for tests and measurements) asks for k slices instead, within
 * [1, min(n_draws, 65535)]: the same bits.
 * workspace: lr_ppc_age_workspace_bytes (the sequential C tables, one per draw, and the flags); < 0 = the LR_ERR_* of the
 * sizes.
 * Errors before any launch, in this order: LR_ERR_NULL; LR_ERR_SIZE: n < 1, n_draws < 1, n_bins < 1 or > LR_MAX_BINS, or
 * n n_draws >= 2^62; LR_ERR_T0: t0 not integer valued; LR_ERR_WORKSPACE.                                                   */
int64_t lr_ppc_age_workspace_bytes(int64_t n, int32_t n_bins, int32_t n_draws);
int lr_ppc_age_plan(int64_t n, int32_t n_bins, int32_t n_draws, int32_t* out /* host int32[4] */);
int lr_ppc_age(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins,
               const double* mu_bins /* [n_draws, n_bins] */, int32_t n_draws, uint64_t seed,
               int64_t* out_obs /* [2, A] */, int64_t* out_rep /* [n_draws, 2, A] */, int64_t* out_totals /* [4] */,
               void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
