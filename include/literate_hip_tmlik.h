/*
 * literate_hip_tmlik.h - C ABI of libliterate_hip.so, marginal likelihoods of the trend_rate.py models: many independent
 * chains of trend_rate.py's sampler on power posteriors L(theta)^beta p(theta), one wave per chain, for a whole grid of
 * (model, replicate, temperature) in one launch (literate_amd/csrc/lr_tmlik.hip).  Their rows are what lr_mlik_estimate
 * (literate_hip_mlik.h) reads: there is no second estimator.  The conventions and status codes are literate_hip.h's: device
 * pointers unless marked "host", the caller owns every buffer, asynchronous on the stream, 0 = ok, < 0 = LR_ERR_*, > 0 = a
 * hipError_t; buffers may hold anything on entry, an argument error has touched nothing, and the library keeps no state
 * between calls.
 *
 * The stream rides in the descriptor (lr_tmlik_problem.stream, a hipStream_t, NULL = default stream), not in a last
 * parameter of the entry points: both take one descriptor, and the functions whose last parameter is the stream are a
 * counted set (tests/test_stream_contract_host.py); the contract is the same - every call is asynchronous on that stream and
 * returns after enqueueing - and tests/test_hip_tmlik.py holds both entry points to it on a busy side stream.
 */
#ifndef LITERATE_HIP_TMLIK_H
#define LITERATE_HIP_TMLIK_H

#include "literate_hip.h"

#define LR_TMLIK_MAX_BINS 512   /* a lane keeps at most 8 bins' statistics and covariate logarithms in registers */
#define LR_TMLIK_MAX_TEMPS 128  /* betas and scales travel in the kernel arguments */
#define LR_TMLIK_MAX_MODELS 64  /* per call: col, flags and key0 travel in the kernel arguments */
#define LR_TMLIK_MOVES 2        /* move kinds: 0 vector multiplier, 1 additive normal step on the slopes */
#define LR_TMLIK_STATE_W 16     /* doubles per chain of the state buffer */
#define LR_TMLIK_ROW_W 12       /* doubles per sampled row (= LR_MLIK_ROW_W, the likelihood in column 2) */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The model ----------------------------------------------------------------------------------------------------------
 * trend_rate.py's: parameters [l_min, m_min, alpha, beta, delta, gamma], per-bin statistics N_SPEC, N_EXTI, DT [n_bins] (as
 * doubles) and a covariate t [n_bins], normalised into (0, 1] (zeros floored to 1e-15); rates by likelihood_function
 * (trend_rate.py:73-88), t ** d evaluated as exp(d log t) with the logarithm taken once per launch,
 *   birth_b = l_min + alpha t_b ** delta (l_min alone under const_B), death_b = m_min + beta t_b ** gamma (m_min alone under
 *   const_D), a rate <= 0 floored to 1e-15,
 *   lik = sum_b log(birth_b) N_SPEC_b - birth_b DT_b + log(death_b) N_EXTI_b - death_b DT_b     (a NaN counts as -inf)
 * and calc_prior (trend_rate.py:93-100).  The initial state is [0.1, 0.1, 0, 0, 1, 1].
 *
 * Model m of a call is (col[m]: its covariate is row col[m] of `trends`; flags[m]: bit 0 const_B, bit 1 const_D; key0[m]).
 * Chain (model m, replicate r, temperature j), c = (m n_reps + r) T + j, targets L^betas[j] p and draws from the Philox
 * stream of key (seed, (key0[m] + r) T + j) at counter (it, purpose, index), purposes 32-35 as the trend engine uses them:
 *   pair(it, 32, 0).a < 0.33   move 1: slope i in {alpha, beta} with pair(it, 34, i).a < f_i (the additive mask's
 *                              probabilities, trend_rate.py:122-135) plus normal(it, 33, i) wins[m, j]
 *   else                       move 0: parameter i with pair(it, 34, i).a < g_i (the multiplier mask's probabilities) times
 *                              exp(2 s log 1.1 (pair(it, 34, i).b - 0.5)), s = scales[j]; hastings = the sum of the exponents
 * An empty mask gives NaN probabilities that never fire, as in the reference.  The proposal is accepted iff
 *   betas[j] (lik' - lik) + (prior' - prior) + hastings > log(pair(it, 35, 0).a)        or it == 0;
 * at betas[j] == 0 the likelihood term is left out (it is still evaluated and stored).  At betas[j] == 1, s == 1 and
 * wins[m, j] == 0.001 the chain is trend_rate.py's own.
 *
 * ---- The buffers ----------------------------------------------------------------------------------------------------------
 * state [n_models, n_reps, T, LR_TMLIK_STATE_W]: 0 .. 5 the parameters, 6 log-likelihood, 7 log prior, 8, 9 proposals made
 *   per move kind, 10, 11 proposals accepted per move kind, 12 beta, 13 scale, 14 the window of the launch that wrote it,
 *   15 m.  A move 1 whose mask fires for no slope proposes the state itself: it is carried out (and always accepted) but
 *   counted in neither 9 nor 11 - the windows are tuned from these counters, and such a step says nothing about a window.
 * rows [n_models, rows_cap, n_reps, T, LR_TMLIK_ROW_W], one per chain and sampled iteration: 0 it, 1 beta, 2 log-likelihood,
 *   3 log prior, 4 .. 9 the parameters, 10 the window, 11 m.  Models are outermost: rows + m rows_cap n_reps T LR_TMLIK_ROW_W
 *   is a [rows_cap, n_reps, T, LR_MLIK_ROW_W] buffer as lr_mlik_estimate reads it.
 */
typedef struct lr_tmlik_problem {
    const double* n_spec;  /* [n_bins] */
    const double* n_exti;  /* [n_bins] */
    const double* DT;      /* [n_bins] */
    const double* trends;  /* [n_cols, n_bins], normalised: every entry in (0, 1] */
    const double* wins;    /* [n_models, T]: additive windows; device data, NOT checked: must be finite and >= 0 */
    double* state;         /* [n_models, n_reps, T, LR_TMLIK_STATE_W] */
    const double* betas;   /* host [T]: betas[0] == 0, betas[T - 1] == 1, strictly ascending */
    const double* scales;  /* host [T]: finite and > 0 */
    const int32_t* col;    /* host [n_models]: 0 .. n_cols - 1 */
    const int32_t* flags;  /* host [n_models]: 0 .. 3 */
    const int64_t* key0;   /* host [n_models]: >= 0, (key0[m] + n_reps) T <= 2^31 - 1 */
    int32_t n_bins, n_cols, n_models, n_reps, T;
    uint64_t seed;
    void* stream;          /* hipStream_t; NULL = default stream */
} lr_tmlik_problem;

/* lr_tmlik_init: the initial state of every chain of the grid, with its likelihood and prior -> state.
 * lr_tmlik_steps: iterations it0 .. it0 + n_iters - 1 of every chain, from `state` and back into it; a row is written after
 *   every iteration with it % s_freq == 0, the first of the launch into slot slot0 of every model: rows_cap - slot0 must be
 *   at least ceil((it0 + n_iters) / s_freq) - ceil(it0 / s_freq) (rows may be NULL where that is 0); the other slots are not
 *   touched.  A chain's draws depend on (seed, its key, it) alone, the host tables are copied into the kernel arguments
 *   (nothing is uploaded) and the state holds everything a launch starts from: a run cut into launches, into groups of
 *   replicates (key0[m] + first replicate of the group) or into groups of models is the same run bit for bit.
 *   Errors before any launch, in this order: LR_ERR_NULL: the descriptor or one of its pointers (rows: where the step arguments are valid and a row is due);
 *   LR_ERR_SIZE: n_bins < 1 or > LR_TMLIK_MAX_BINS, n_cols < 1, T < 2 or > LR_TMLIK_MAX_TEMPS, n_models < 1 or >
 *   LR_TMLIK_MAX_MODELS, n_reps < 1, n_models n_reps T beyond 2^31 - 1; LR_ERR_MODEL: a col out of range, flags outside 0 .. 3,
 *   key0 < 0 or (key0 + n_reps) T beyond 2^31 - 1, betas[0] != 0, betas[T - 1] != 1, betas not strictly ascending, a scale not
 *   finite or <= 0; then (steps) LR_ERR_SIZE: it0 < 0, n_iters < 0, s_freq < 1, slot0 < 0, rows_cap - slot0 too small.
 *   n_iters = 0 launches nothing.                                                                                              */
int lr_tmlik_init(const lr_tmlik_problem* problem /* host */);
int lr_tmlik_steps(const lr_tmlik_problem* problem /* host */, int64_t it0, int64_t n_iters, int32_t s_freq,
                   double* rows /* [n_models, rows_cap, n_reps, T, LR_TMLIK_ROW_W] */, int64_t rows_cap, int64_t slot0);

#ifdef __cplusplus
}
#endif

#endif
