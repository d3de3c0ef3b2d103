/*
 * literate_hip_ade.h - C ABI of libliterate_hip.so, age-dependent extinction: the Weibull shape of the lineages' hazard, fitted
 * conditional on posterior draws of the per-bin death rates (literate_amd/csrc/lr_ade.hip).  The conventions and status codes
 * are literate_hip.h's: device pointers unless marked "host", the caller owns every buffer, asynchronous on `stream`, 0 = ok,
 * < 0 = LR_ERR_*, > 0 = a hipError_t; buffers may hold anything on entry, and an argument error has touched nothing.
 */
#ifndef LITERATE_HIP_ADE_H
#define LITERATE_HIP_ADE_H

#include "literate_hip.h"

#define LR_ADE_MAX_BINS 512

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The model, at the resolution of the bins -------------------------------------------------------------------------------
 * A = n_bins bins, bin b = [t0 + b, t0 + b + 1); T_c = t0 + n_bins, the end of the modelled window.  A lineage is born at the
 * start of its birth bin jb; with its age a counted from there in bins, its hazard in bin b is  c mu[b] k a^(k - 1):  mu one
 * draw of per-bin death rates, k > 0 the shape, c > 0 a multiplier (k = 1, c = 1: the samplers' own death process; mu = 1
 * throughout: a Weibull of scale c^(-1/k)).  A death is known to its bin only, so the likelihood is interval-censored:
 *   w_k[0] = 1, w_k[j] = j^k expm1(k log1p(1 / j))           (= (j + 1)^k - j^k without the cancellation)
 *   H[jb][m] = sum_{j < m} mu[jb + j] w_k[j],  m = 0 .. A - jb
 *   a CLASS is (jb, a), a = je - jb, je the death bin
 *   l(c) = sum_{dead[jb][a] > 0} dead[jb][a] (-c H[jb][a] + log(-expm1(-c (H[jb][a + 1] - H[jb][a]))))
 *          - c sum_jb cens[jb] H[jb][A - jb]
 * l is concave in c; lr_ade_profile returns the profile maximum l(c^) and c^ for every (draw, shape).
 *
 * lr_ade_classes: one pass over the n lineages, from the data only.  Lineage i is USED iff 0 <= ts_i - t0 < n_bins and
 *   te_i > ts_i (NaN fails both: lr_ppc_age's rule); jb = floor(ts_i - t0).  It is DEAD iff te_i <= T_c, and then
 *   je = min(floor(te_i - t0), A - 1) and out_dead[jb][je - jb] += 1; any other used lineage: out_cens[jb] += 1.
 *   out_dead [A, A], out_cens [A], out_totals [2] = {lineages used, lineages unused}: every element is written, zeros included
 *   (out_dead[jb][a] with jb + a >= A is always 0).  Integer atomics only: exact, and independent of the launch shape.
 *   Errors before any launch, in this order: LR_ERR_NULL; LR_ERR_SIZE: n < 1, n_bins < 1 or > LR_ADE_MAX_BINS; LR_ERR_T0: t0
 *   not integer valued.                                                                                                      */
int lr_ade_classes(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins,
                   int64_t* out_dead /* [A, A] */, int64_t* out_cens /* [A] */, int64_t* out_totals /* [2] */, void* stream);

/* lr_ade_profile: for each of the S rows of mu_bins [S, A] and each of the G shapes, c^ = argmax_c l(c) and l(c^).  dead [A, A]
 *   and cens [A] as lr_ade_classes writes them; of dead only the cells with jb + a < A and a count > 0 are classes (a negative
 *   count is read as 0).
 *   Draw s is FLAGGED iff some mu[s, b] is not finite or < 0, or mu[s, je] == 0 for a bin je that holds an observed death:
 *   out_flag[s] = 1 (else 0) and the rows out_ll[s, .], out_c[s, .] are NaN.  A shape that is not finite or <= 0: its column is
 *   NaN.  No observed death: out_c = 0, out_ll = 0.  No finite maximiser (the coefficient of -c, sum of dead H[jb][a] and
 *   cens H[jb][A - jb], is 0: every death in class a = 0 and nothing censored): out_c = +inf, out_ll = 0.
 *   Otherwise c^ is the root of the score, found by a safeguarded Newton iteration on log c; only c^, l(c^) and the flags are
 *   contract, not the path.  out_ll, out_c [S, G], out_flag int32 [S].
 *   The sums are formed in an order that depends on the arguments' sizes alone and there are no floating-point atomics: a
 *   result is a function of (dead, cens, mu[s, .], shapes[g]) alone - the same bits from a second call, on dirty buffers,
 *   beside other draws or without them.
 *   workspace: lr_ade_profile_workspace_bytes (the tables lr_adej_prepare writes too - the class list and the numbers at risk
 *   as a packed triangle, as doubles and as 32-bit integers - and one row of A sums per draw); < 0 = the LR_ERR_* of the
 *   sizes.
 *   Errors before any launch, in this order: LR_ERR_NULL; LR_ERR_SIZE: S < 1, G < 1, n_bins < 1 or > LR_ADE_MAX_BINS, or
 *   S G >= 2^31; LR_ERR_WORKSPACE.                                                                                          */
int64_t lr_ade_profile_workspace_bytes(int32_t n_bins, int32_t S, int32_t G);
int lr_ade_profile(const int64_t* dead /* [A, A] */, const int64_t* cens /* [A] */, int32_t n_bins,
                   const double* mu_bins /* [S, A] */, int32_t S, const double* shapes /* [G] */, int32_t G,
                   double* out_ll /* [S, G] */, double* out_c /* [S, G] */, int32_t* out_flag /* [S] */,
                   void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
