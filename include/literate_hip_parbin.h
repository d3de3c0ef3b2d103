/*
 * literate_hip_parbin.h - C ABI of libliterate_hip.so, the parametric samplers on binned statistics: DDRate.py's
 * (DD:124-241) and trend_rate.py's (trend_rate.py:102-196) Metropolis-Hastings loops for many chains that do NOT share
 * their data, one wave per chain, all of them in one launch (literate_amd/csrc/lr_parbin.hip).  Both likelihoods are
 * functions of create_bins' per-bin statistics alone, so chain c carries the statistics of its own replicate - one
 * stochastic imputation of the death times, say - and an iteration costs O(n_bins) whatever the number of lineages.  The
 * conventions and status codes are literate_hip.h's: device pointers unless marked "host", the caller owns every buffer,
 * asynchronous on the stream, 0 = ok, < 0 = LR_ERR_*, > 0 = a hipError_t; buffers may hold anything on entry, an argument
 * error has touched nothing, and the library keeps no state between calls.
 *
 * The stream rides in the descriptor (lr_parbin_problem.stream, a hipStream_t, NULL = default stream), not in a last
 * parameter of the entry points, as in literate_hip_rjbin.h: every call is asynchronous on that stream and returns after
 * enqueueing (tests/test_hip_parbin.py holds both entry points to it on a busy side stream).
 */
#ifndef LITERATE_HIP_PARBIN_H
#define LITERATE_HIP_PARBIN_H

#include "literate_hip.h"

#define LR_PARBIN_MAX_BINS 512 /* a lane keeps at most 8 bins' statistics in registers */
#define LR_PARBIN_STATE_W 16   /* doubles per chain of the state buffer */

/* elements of a chain's state */
#define LR_PARBIN_S_ARGS 0     /* the accepted parameters: 8 of sampler 1, 6 of sampler 2 (then two zeros) */
#define LR_PARBIN_S_LIK 8      /* their log-likelihood                                                    */
#define LR_PARBIN_S_PRIOR 9    /* their log prior                                                         */
#define LR_PARBIN_S_PROPOSED 10 /* proposals made: [multiplier, window] (sampler 2: a window step whose mask fires
                                  for no slope is not counted)                                            */
#define LR_PARBIN_S_ACCEPTED 12 /* proposals accepted, likewise; elements 14, 15 are 0                     */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The model ----------------------------------------------------------------------------------------------------------
 * Replicate r has create_bins' statistics n_spec, n_exti, DT [n_bins] (births, deaths, lineage-time per bin, as doubles)
 * and its own origin, present (create_bins' values, after -rm_first_bin).  Chain c belongs to replicate c /
 * chains_per_rep, C = R chains_per_rep.  With lam_b, mu_b the rates of bin b under the chain's parameters:
 *   lik = sum_b (log(lam_b) n_spec_b - lam_b DT_b) + (log(mu_b) n_exti_b - mu_b DT_b);   a NaN counts as -inf
 * sampler 1 (DDRate.py): parameters [l_max, k, x0, div_0, L, m_max, nuB, nuD]; lam_b, mu_b are lr_dd_rates' at x = b and
 *   the replicate's DT_b, m_birth 0 .. 2, m_death -2 .. 2 as lr_dd_rates takes them; the prior is calc_prior's
 *   (DD:110-122) with PRIOR_K0_L = the maximum of the replicate's own DT and its own origin, present; the initial state is
 *   [0.5, 1.5, present - (origin + present) / 2, 10, 20000, init_death, 1, 1] (DD:151-161).
 * sampler 2 (trend_rate.py): parameters [l_min, m_min, alpha, beta, delta, gamma]; lam_b, mu_b are lr_trend_rates' at
 *   trend_b, the normalised covariate all replicates share; m_birth, m_death are the -const_B / -const_D flags (0 or 1), as
 *   lr_curve_summary takes them; the additive window on the slopes is the reference's 0.001; a window step whose mask fires
 *   for no slope proposes the state itself.  The initial state is [.1, .1, 0, 0, 1, 1].
 * Both are the engines' samplers 1 and 2 (lr_mcmc_config.sampler) and the beta = 1, scale = 1 chains of lr_mlik_* /
 * lr_tmlik_* (window 0.001), whose iteration they share (csrc/lr_par_iter.h): chain c draws from the Philox stream of key
 * (seed, chain0 + c) at counter (it, purpose, index), purposes 16 .. 19 / 32 .. 35 (oracle/dd_mcmc_oracle.py,
 * oracle/trend_mcmc_oracle.py); `>` in the acceptance test; iteration 0 is always accepted.
 * Every sum: a lane's bins in ascending order (bin b sits in lane b % 64), then a fixed tree over the lanes; no
 * floating-point atomics: a chain's bits depend on its own arguments alone.
 *
 * ---- The buffers --------------------------------------------------------------------------------------------------------
 * state [C, LR_PARBIN_STATE_W]: see above; everything a launch starts from.
 * rows  [rows_cap, C, LR_TRACE_W]: the engines' trace rows of that sampler (literate_hip.h), one per chain and sampled
 *   iteration: [it, posterior = likelihood + prior, likelihood, prior, args[8]] for sampler 1, [.., args[6]] for sampler 2,
 *   the rest of the row 0.
 */
typedef struct lr_parbin_problem {
    const double* n_spec;      /* [R, n_bins] */
    const double* n_exti;      /* [R, n_bins] */
    const double* DT;          /* [R, n_bins] */
    const double* origin;      /* [R] */
    const double* present;     /* [R] */
    const double* trend;       /* [n_bins]; sampler 2, otherwise NULL */
    double* state;             /* [C, LR_PARBIN_STATE_W] */
    int32_t n_bins, R, chains_per_rep;
    int32_t sampler;           /* 1 = DDRate, 2 = trend_rate: the engines' numbering */
    int32_t m_birth, m_death;
    double init_death;         /* sampler 1: the initial (with m_death < 0: the fixed) death rate, -fix_death */
    /* The Philox key of chain c is ((uint32) seed, (uint32) (chain0 + c)): both wrap modulo 2^32. */
    int64_t chain0;            /* Philox key of chain 0 */
    uint64_t seed;
    void* stream;              /* hipStream_t; NULL = default stream */
} lr_parbin_problem;

/* lr_parbin_init: the initial state of every chain with its likelihood and prior, the counters 0 -> state.
 * lr_parbin_steps: iterations it0 .. it0 + n_iters - 1 of every chain, from `state` and back into it; a row is written
 *   after every iteration with it % s_freq == 0, the first of the launch into slot slot0: rows_cap - slot0 must be at
 *   least ceil((it0 + n_iters) / s_freq) - ceil(it0 / s_freq) (rows may be NULL where that is 0); the other slots are not
 *   touched.  A chain's draws depend on (seed, chain0 + c, it) alone and the state holds everything a launch starts from:
 *   a run cut into launches - in iterations, or into groups of replicates with chain0 advanced - is the same run bit for
 *   bit.
 *   Errors before any launch, in this order: LR_ERR_NULL: the descriptor, n_spec, n_exti, DT, origin, present, state,
 *   trend (sampler 2), rows (where the step arguments are valid and a row is due); LR_ERR_SIZE: n_bins < 1 or >
 *   LR_PARBIN_MAX_BINS, R < 1, chains_per_rep < 1, R chains_per_rep beyond 2^31 - 1; LR_ERR_MODEL: sampler other than 1 or
 *   2, sampler 1: m_birth outside 0 .. 2, m_death outside -2 .. 2, init_death not finite, sampler 2: m_birth or m_death
 *   outside 0 .. 1; then (steps) LR_ERR_SIZE: it0 < 0, n_iters < 0, s_freq < 1, slot0 < 0, rows_cap - slot0 too small.
 *   n_iters = 0 launches nothing.                                                                                         */
int lr_parbin_init(const lr_parbin_problem* problem /* host */);
int lr_parbin_steps(const lr_parbin_problem* problem /* host */, int64_t it0, int64_t n_iters, int32_t s_freq,
                    double* rows /* [rows_cap, C, LR_TRACE_W] */, int64_t rows_cap, int64_t slot0);

#ifdef __cplusplus
}
#endif

#endif
