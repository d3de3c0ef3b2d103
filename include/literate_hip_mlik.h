/*
 * literate_hip_mlik.h - C ABI of libliterate_hip.so, marginal likelihoods of the DDRate models: many independent chains of
 * DDRate.py's sampler on power posteriors L(theta)^beta p(theta), one wave per chain, and the stepping-stone and thermodynamic
 * integration estimates from their rows (literate_amd/csrc/lr_mlik.hip).  The conventions and status codes are
 * literate_hip.h's: device pointers unless marked "host", the caller owns every buffer, asynchronous on `stream`, 0 = ok,
 * < 0 = LR_ERR_*, > 0 = a hipError_t; buffers may hold anything on entry, an argument error has touched nothing, and the
 * library keeps no state between calls.
 */
#ifndef LITERATE_HIP_MLIK_H
#define LITERATE_HIP_MLIK_H

#include "literate_hip.h"

#define LR_MLIK_MAX_BINS 512   /* a lane keeps at most 8 bins' statistics in registers for the whole launch */
#define LR_MLIK_MAX_TEMPS 128  /* betas and scales travel in the kernel arguments */
#define LR_MLIK_MOVES 2        /* move kinds: 0 vector multiplier, 1 sliding window on the midpoint */
#define LR_MLIK_STATE_W 16     /* doubles per chain of the state buffer */
#define LR_MLIK_ROW_W 12       /* doubles per sampled row */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The model ----------------------------------------------------------------------------------------------------------
 * DDRate.py's: parameters [l_max, k, x0, div_0, L, m_max, nuB, nuD], per-bin statistics N_SPEC, N_EXTI, DT [n_bins] (as
 * doubles), bin b at x = b; rates by likelihood_function (DD:71-100) under (m_birth in {0, 1, 2}, m_death in {-2, -1, 0, 1, 2}),
 *   lik = sum_b log(birth_b) N_SPEC_b - birth_b DT_b + log(death_b) N_EXTI_b - death_b DT_b     (a NaN counts as -inf)
 * and calc_prior (DD:110-122) with PRIOR_K0_L = max DT.  The initial state is [0.5, 1.5, present - (origin + present) / 2, 10,
 * 20000, init_death, 1, 1].
 *
 * Chain (replicate r, temperature j), c = r T + j, targets L^betas[j] p and draws from the Philox stream of key
 * (seed, (rep0 + r) T + j) at counter (it, purpose, index), purposes 16-19 as the DD engine uses them:
 *   (r0, r1) = pair(it, 16, 0)
 *   r1 < 0.1 and (m_birth == 2 or m_death == 2)   move 1: x0' = |reflect at present of x0 + (pair(it, 17, 0).a - 0.5) 1.5 s|, and
 *                                                  under m_death == -1 k' = k + normal(it, 17, 1) 0.2 s
 *   else                                           move 0: parameter i with pair(it, 18, i).a < f_i (the model's update
 *                                                  probabilities, DD:166-181) times exp(2 s log 1.1 (pair(it, 18, i).b - 0.5));
 *                                                  hastings = the sum of the exponents
 * with s = scales[j].  The proposal is accepted iff
 *   betas[j] (lik' - lik) + (prior' - prior) + hastings > log(pair(it, 19, 0).a)        or it == 0;
 * at betas[j] == 0 the likelihood term is left out (it is still evaluated and stored).  At betas[j] == 1 and s == 1 the chain
 * is DDRate.py's own.
 *
 * betas, scales: host [T], 2 <= T <= LR_MLIK_MAX_TEMPS; betas[0] == 0, betas[T - 1] == 1, strictly ascending; scales finite
 * and > 0.
 *
 * ---- The buffers ----------------------------------------------------------------------------------------------------------
 * state [n_reps, T, LR_MLIK_STATE_W]: 0 .. 7 the parameters, 8 log-likelihood, 9 log prior, 10, 11 proposals made per move
 *   kind, 12, 13 proposals accepted per move kind, 14 beta, 15 scale.
 * rows [n_rows, n_reps, T, LR_MLIK_ROW_W], one per chain and sampled iteration: 0 it, 1 beta, 2 log-likelihood, 3 log prior,
 *   4 .. 11 the parameters.
 */

/* lr_mlik_init: the initial state of replicates rep0 .. rep0 + n_reps - 1 at every temperature, with its likelihood and
 *   prior -> state.
 * lr_mlik_steps: iterations it0 .. it0 + n_iters - 1 of every chain, from `state` and back into it; a row is written after
 *   every iteration with it % s_freq == 0, the first of the launch into rows[0]: n_rows must be at least
 *   ceil((it0 + n_iters) / s_freq) - ceil(it0 / s_freq) (rows may be NULL where that is 0).  A chain's draws depend on (seed, its
 *   global index, it) alone, and the state holds everything a launch starts from: a run cut into launches, or into groups of
 *   replicates, is the same run bit for bit.
 *   Errors before any launch, in this order: LR_ERR_NULL; LR_ERR_SIZE: n_bins < 1 or > LR_MLIK_MAX_BINS, T < 2 or >
 *   LR_MLIK_MAX_TEMPS, n_reps < 1, rep0 < 0, (rep0 + n_reps) T beyond 2^31 - 1; LR_ERR_MODEL: m_birth or m_death out of range,
 *   origin, present or init_death not finite, betas[0] != 0, betas[T - 1] != 1, betas not strictly ascending, a scale not finite
 *   or <= 0; then (steps) LR_ERR_SIZE: it0 < 0, n_iters < 0, s_freq < 1, n_rows too small.  n_iters = 0 launches nothing.       */
int lr_mlik_init(const double* n_spec /* [n_bins] */, const double* n_exti /* [n_bins] */, const double* DT /* [n_bins] */,
                 int32_t n_bins, double origin, double present, int32_t m_birth, int32_t m_death, double init_death,
                 const double* betas /* host [T] */, const double* scales /* host [T] */, int32_t T, uint64_t seed, int32_t rep0,
                 int32_t n_reps, double* state /* [n_reps, T, LR_MLIK_STATE_W] */, void* stream);
int lr_mlik_steps(const double* n_spec /* [n_bins] */, const double* n_exti /* [n_bins] */, const double* DT /* [n_bins] */,
                  int32_t n_bins, double origin, double present, int32_t m_birth, int32_t m_death, double init_death,
                  const double* betas /* host [T] */, const double* scales /* host [T] */, int32_t T, uint64_t seed, int32_t rep0,
                  int32_t n_reps, double* state /* [n_reps, T, LR_MLIK_STATE_W] */, int64_t it0, int64_t n_iters, int32_t s_freq,
                  double* rows /* [n_rows, n_reps, T, LR_MLIK_ROW_W] */, int64_t n_rows, void* stream);

/* lr_mlik_estimate: from rows row0 .. n_rows - 1 (n = n_rows - row0 samples per chain, lik_i(r, j) = column 2), with
 *   d_j = betas[j + 1] - betas[j]:
 *   stone [n_reps, T - 1]  log mean_i exp(d_j lik_i(r, j)), shifted by the largest lik; a -inf lik contributes 0, all -inf: -inf
 *   ss [n_reps]            sum_j stone[r, j]: the stepping-stone estimate of log Z of replicate r
 *   lik_mean, lik_var [n_reps, T]   mean and sample variance (n - 1; NaN at n = 1) of lik per chain
 *   ti [n_reps]            sum_j d_j (lik_mean[r, j] + lik_mean[r, j + 1]) / 2: thermodynamic integration by the trapezoid rule
 *   pooled [T]             0 .. T - 2 the stones over all replicates' samples of a temperature, T - 1 their sum
 *   Fixed reduction trees, no floating-point atomics: a value is a function of its own inputs alone.
 *   Errors before any launch, in this order: LR_ERR_NULL; LR_ERR_SIZE: n_rows < 1, n_reps < 1, T < 2 or > LR_MLIK_MAX_TEMPS,
 *   row0 < 0 or >= n_rows; LR_ERR_MODEL: betas as above.                                                                        */
int lr_mlik_estimate(const double* rows /* [n_rows, n_reps, T, LR_MLIK_ROW_W] */, int64_t n_rows, int32_t n_reps, int32_t T,
                     int64_t row0, const double* betas /* host [T] */, double* stone /* [n_reps, T - 1] */,
                     double* ss /* [n_reps] */, double* lik_mean /* [n_reps, T] */, double* lik_var /* [n_reps, T] */,
                     double* ti /* [n_reps] */, double* pooled /* [T] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif
