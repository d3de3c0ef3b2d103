/*
 * literate_hip_adej.h - C ABI of libliterate_hip.so, age-dependent extinction sampled jointly: one Metropolis-Hastings sampler
 * over (the death-rate skyline, the Weibull shape of the hazard by lineage age), many independent chains, one workgroup per
 * chain (literate_amd/csrc/lr_adej.hip).  The conventions and status codes are literate_hip.h's: device pointers unless marked
 * "host", the caller owns every buffer, asynchronous on `stream`, 0 = ok, < 0 = LR_ERR_*, > 0 = a hipError_t; buffers may hold
 * anything on entry, an argument error has touched nothing, and the library keeps no state between calls.
 */
#ifndef LITERATE_HIP_ADEJ_H
#define LITERATE_HIP_ADEJ_H

#include "literate_hip.h"

#define LR_ADEJ_MAX_BINS 128  /* the table of the numbers at risk stays in a workgroup's LDS, several workgroups per CU */
#define LR_ADEJ_MOVES 5       /* move kinds: 0 multiplier, 1 shape window, 2 add a shift, 3 remove a shift, 4 Gibbs */
#define LR_ADEJ_STATE_W 96    /* doubles per chain of the state buffer */
#define LR_ADEJ_ROW_W 73      /* doubles per sampled row: 10 + LR_KMAX + LR_KMAX - 1 */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The model ----------------------------------------------------------------------------------------------------------
 * literate_hip_ade.h's, with the multiplier c = 1 (it is absorbed into the rates): A = n_bins bins, classes (jb, a) counted by
 * lr_ade_classes in dead [A, A] and cens [A]; w_k[0] = 1, w_k[j] = j^k expm1(k log1p(1 / j)).  Given per-bin baseline rates mu
 * and the shape k,
 *   R[jb][j] = cens[jb] + sum_{a > j, jb + a < A} dead[jb][a]            (the lineages of birth bin jb that live past age j)
 *   M[j]     = sum_{jb < A - j} R[jb][j] mu[jb + j]
 *   l(mu, k) = -sum_j w_k[j] M[j] + sum_{classes} dead[jb][a] log(-expm1(-mu[jb + a] w_k[a]))
 * which is the cumulative-hazard form of literate_hip_ade.h at c = 1, rearranged.
 *
 * A chain's state: K rates m[0 .. K), 1 <= K <= LR_KMAX, on the segments of times t[0 .. K], t[0] = t0, t[K] = t0 + A (bin b
 * takes the rate of the segment that holds it by floor(t), as the RJ engines expand theirs); g = log k; the hyper-parameters
 * rate_hp, poi_hp.  Priors: Gamma(2, rate rate_hp) on each rate, -log(A) (K - 1) on the shift times, the Poisson prior of the
 * engines on K with rate poi_hp, g flat on [-log 8, log 8] (a constant, left out of the prior column).  Iteration `it` of
 * chain c draws from the Philox stream of key (seed, chain0 + c) at counter (it, purpose, index):
 *   (r0, r1) = pair(it, LR_P_MOVE, 0)
 *   r0 < 0.30                        move 0: every rate times exp(2 log 1.1 (u - 0.5)) with probability 0.75 (LR_P_MULT, index j)
 *   r0 < 0.60                        move 1: g' = g + (u - 0.5) win (purpose 48, index 0); outside the bounds: rejected
 *   r0 < 0.999 and not const_rates   r1 > 0.5: move 2, add a shift (the engines' add_shift_RJ_weighted_mean; LR_P_RJ index 1,
 *                                    LR_P_BETA_A / _B), rejected at K = LR_KMAX; else move 3, remove a shift, and at K = 1 the
 *                                    unchanged state is scored
 *   else                             move 4: poi_hp = Gamma(2 + K) / 2 (purpose 50) unless poisson_prior > 0 fixes it, rate_hp =
 *                                    Gamma(1.2 + 2 K) / (0.1 + sum m) (purpose 51) if use_rate_hp; always accepted, and the
 *                                    prior is recomputed under the new hyper-parameters
 * A proposal with min |t[j + 1] - t[j]| <= 1 is rejected; any other is accepted iff
 *   lik' - lik + prior' - prior + hastings >= log(pair(it, LR_P_ACCEPT, 0).a).
 * The initial state (lr_adej_init): K = 1, m[0] = 0.2 Gamma(2) (counter (0, 49, attempts from 0)), g = (pair(0, 49, 64).a - 0.5)
 * 2 log 4, rate_hp = 1, poi_hp = poisson_prior > 0 ? poisson_prior : 1.
 *
 * ---- The buffers ----------------------------------------------------------------------------------------------------------
 * workspace: lr_adej_workspace_bytes(n_bins) bytes (< 0: LR_ERR_SIZE), written by lr_adej_prepare and only read by the others:
 *   a header, the classes with a count in the table's own order (so every sum over them has one order), the bins that hold a
 *   death, and R as a packed triangle - the tables lr_ade_profile starts its own workspace with, written by the same two
 *   kernels.  Integer arithmetic on the counts; from the data only.
 * state [n_chains, LR_ADEJ_STATE_W]: 0 K, 1 g, 2 rate_hp, 3 poi_hp, 4 log-likelihood, 5 log prior, 6 .. 10 proposals made per
 *   move kind, 11 .. 15 proposals accepted per move kind, 16 .. 47 the rates, 48 .. 80 the times; every unused slot (rates and
 *   times beyond K, 81 .. 95) is 0.
 * rows [n_rows, n_chains, LR_ADEJ_ROW_W], one per chain and sampled iteration: 0 it, 1 posterior (2 + 3), 2 log-likelihood,
 *   3 log prior, 4 shape, 5 log shape, 6 K, 7 mean rate, 8 rate_hp, 9 poi_hp, 10 .. 41 the K rates, 42 .. 72 the K - 1 shift
 *   times; every unused slot is NaN.
 */
int64_t lr_adej_workspace_bytes(int32_t n_bins);

/* lr_adej_prepare: (dead [A, A], cens [A]) as lr_ade_classes writes them -> workspace.  Of dead only the cells with jb + a < A
 *   and a count > 0 are classes.
 *   Errors before any launch, in this order: LR_ERR_NULL; LR_ERR_SIZE: n_bins < 1 or > LR_ADEJ_MAX_BINS; LR_ERR_WORKSPACE.   */
int lr_adej_prepare(const int64_t* dead /* [A, A] */, const int64_t* cens /* [A] */, int32_t n_bins, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* lr_adej_loglik: out_ll[s] = l(mu_bins[s, .], shapes[s]) for the S rows of mu_bins [S, A] and shapes [S].  out_flag[s]: bit 0 -
 *   some mu[s, b] is not finite or < 0, or mu[s, je] == 0 for a bin je that holds an observed death; bit 1 - shapes[s] is not
 *   finite or <= 0; a flagged row's out_ll is NaN.  Fixed reduction trees, no floating-point atomics: a row's bits are a
 *   function of the workspace and its own inputs alone.
 *   Errors before any launch, in this order: LR_ERR_NULL; LR_ERR_SIZE: S < 1, n_bins < 1 or > LR_ADEJ_MAX_BINS;
 *   LR_ERR_WORKSPACE.                                                                                                          */
int lr_adej_loglik(const void* workspace, int64_t workspace_bytes, int32_t n_bins, const double* mu_bins /* [S, A] */,
                   const double* shapes /* [S] */, int32_t S, double* out_ll /* [S] */, int32_t* out_flag /* [S] */, void* stream);

/* lr_adej_init: the initial state of chains chain0 .. chain0 + n_chains - 1, with its likelihood and prior -> state.
 * lr_adej_steps: iterations it0 .. it0 + n_iters - 1 of every chain, from `state` and back into it; a row is written after
 *   every iteration with it % s_freq == 0, the first of the launch into rows[0]: n_rows must be at least
 *   ceil((it0 + n_iters) / s_freq) - ceil(it0 / s_freq) (rows may be NULL where that is 0).  A chain's draws depend on (seed, its global index, it) alone, and the
 *   state holds everything a launch starts from: a run cut into launches, or into groups of chains, is the same run bit for bit.
 *   Errors before any launch, in this order: LR_ERR_NULL; LR_ERR_SIZE: n_bins < 1 or > LR_ADEJ_MAX_BINS, n_chains < 1,
 *   chain0 < 0, (steps) it0 < 0, n_iters < 0, s_freq < 1, n_rows too small; LR_ERR_MODEL: win or poisson_prior not finite,
 *   win <= 0, poisson_prior < 0; LR_ERR_T0: t0 not integer valued; LR_ERR_WORKSPACE.  n_iters = 0 launches nothing.          */
int lr_adej_init(const void* workspace, int64_t workspace_bytes, int32_t n_bins, double t0, int32_t const_rates,
                 int32_t use_rate_hp, double poisson_prior, double win, uint64_t seed, int32_t chain0, int32_t n_chains,
                 double* state /* [n_chains, LR_ADEJ_STATE_W] */, void* stream);
int lr_adej_steps(const void* workspace, int64_t workspace_bytes, int32_t n_bins, double t0, int32_t const_rates,
                  int32_t use_rate_hp, double poisson_prior, double win, uint64_t seed, int32_t chain0, int32_t n_chains,
                  double* state /* [n_chains, LR_ADEJ_STATE_W] */, int64_t it0, int64_t n_iters, int32_t s_freq,
                  double* rows /* [n_rows, n_chains, LR_ADEJ_ROW_W] */, int64_t n_rows, void* stream);

#ifdef __cplusplus
}
#endif

#endif
