/*
 * literate_hip_mtrend.h - C ABI of libliterate_hip.so, the joint covariate model: birth and death rates that are log-linear
 * in several covariates at once, with a selection indicator per covariate and side (Bayesian variable selection, Kuo-Mallick),
 * for many chains on one data set in one launch, one wave per chain (literate_amd/csrc/lr_mtrend.hip).  The likelihood is a
 * function of create_bins' per-bin statistics and the covariate matrix alone, so an iteration costs O(n_bins x included
 * covariates) whatever the number of lineages.  The conventions and status codes are literate_hip.h's: device pointers
 * unless marked "host", the caller owns every buffer, asynchronous on the stream, 0 = ok, < 0 = LR_ERR_*, > 0 = a
 * hipError_t; buffers may hold anything on entry, an argument error has touched nothing, and the library keeps no state
 * between calls.  No floating-point atomics, no scratch, no workspace.
 *
 * The stream rides in the descriptor (lr_mtrend_problem.stream, a hipStream_t, NULL = default stream), not in a last
 * parameter of the entry points, as in literate_hip_parbin.h and literate_hip_mte.h: every call is asynchronous on that
 * stream and returns after enqueueing (tests/test_hip_mtrend.py holds both entry points to it on a busy side stream).
 */
#ifndef LITERATE_HIP_MTREND_H
#define LITERATE_HIP_MTREND_H

#include "literate_hip.h"

#define LR_MTREND_MAX_BINS 512 /* a lane keeps at most 8 bins' statistics in registers */
#define LR_MTREND_MAX_COVS 16  /* P: X is at most 16 x 512 doubles = 64 KiB of LDS */
#define LR_MTREND_STATE_W 96   /* doubles per chain of the state buffer */
#define LR_MTREND_ROW_W 72     /* doubles per row: 8 + 4 P in use */
#define LR_MTREND_MOVES 6      /* counters per kind: see LR_MTREND_S_PROPOSED */

/* elements of a chain's state; what lies behind P in a block of 16, and every element not named here, is written as 0 */
#define LR_MTREND_S_L0 0        /* the base birth rate l0                                                          */
#define LR_MTREND_S_M0 1        /* the base death rate m0                                                          */
#define LR_MTREND_S_LIK_B 2     /* the birth side's log-likelihood of the accepted parameters                      */
#define LR_MTREND_S_LIK_D 3     /* the death side's (0 with no_death)                                              */
#define LR_MTREND_S_PRIOR 4     /* their log prior                                                                 */
#define LR_MTREND_S_E_B 5       /* E = sum_b DT_b exp(eta_b) of the accepted birth side                            */
#define LR_MTREND_S_E_D 6       /* ... of the death side (0 with no_death)                                         */
#define LR_MTREND_S_PROPOSED 8  /* proposals made: [multiplier, coefficient birth, coefficient death, flip, coefficient
                                   birth where I_j = 1, coefficient death where I_j = 1]; a rejected proposal counts as
                                   proposed.  The last two are what a window is tuned from: a move of an excluded
                                   coefficient is judged by its prior alone and says nothing about the window on the
                                   posterior                                                                       */
#define LR_MTREND_S_ACCEPTED 16 /* proposals accepted, likewise                                                    */
#define LR_MTREND_S_IL 32       /* I_j of the birth side, 0.0 or 1.0 [LR_MTREND_MAX_COVS]                          */
#define LR_MTREND_S_A 48        /* a_j [LR_MTREND_MAX_COVS]                                                        */
#define LR_MTREND_S_IM 64       /* I_j of the death side [LR_MTREND_MAX_COVS]                                      */
#define LR_MTREND_S_B 80        /* b_j [LR_MTREND_MAX_COVS]                                                        */

/* elements of a row */
#define LR_MTREND_R_IT 0
#define LR_MTREND_R_POST 1
#define LR_MTREND_R_LIK 2
#define LR_MTREND_R_LIK_B 3
#define LR_MTREND_R_LIK_D 4
#define LR_MTREND_R_PRIOR 5
#define LR_MTREND_R_L0 6
#define LR_MTREND_R_M0 7
#define LR_MTREND_R_IL 8        /* I_l[P], then a[P], I_m[P], b[P]; the rest of the row 0 */

/* Philox purposes (csrc/lr_device.h) with every index used; the counter is (it, purpose, index) */
#define LR_P_MTREND_MOVE 72     /* 0: a = the move selector r, b = the target (side, covariate) of a coefficient move or
                                   a flip; 1: a < 0.5 = the multiplier moves l0 (else m0), b = the multiplier's uniform */
#define LR_P_MTREND_NORM 73     /* 0: the Normal(0, 1) of a coefficient's step (lr_normal)                             */
#define LR_P_MTREND_ACCEPT 74   /* 0: a = the acceptance uniform                                                       */
#define LR_P_MTREND_INIT 75     /* index (it = 0): the Normal(0, 1) of an initial coefficient; birth j: j, death j: P + j */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The model ----------------------------------------------------------------------------------------------------------
 * Data: create_bins' statistics n_spec, n_exti, DT [n_bins] (births, deaths, lineage-time per bin, as doubles) and a
 * covariate matrix X [P, n_bins], 1 <= P <= 16, 1 <= n_bins <= 512 (the command line standardises every row to mean 0,
 * population sd 1; the library takes X as it is).  All C chains run on the one data set.
 * A side is birth (l) or death (m).  Each side has a base rate (l0, m0), coefficients a_j (birth) or b_j (death) and
 * indicators I_j in {0, 1}, j < P:
 *   eta_b = sum over j ascending with I_j = 1 of coef_j X[j, b]   (one fma chain starting from 0.0)
 *   rate_b = base exp(eta_b)
 * A side declared constant (m_birth / m_death = 1) has no coefficients: all its coefficients and indicators are 0 - also
 * where the caller's state (given = 1) says otherwise - and it is never picked.  With no_death the death side adds nothing
 * to the likelihood (its term and its E are 0), is constant, and m0 never moves; m0 keeps its prior term, a constant.
 * Likelihood, per side, with n = n_spec (birth) or n_exti (death):
 *   lik_side = N log(base) + sum_j I_j coef_j SX_j - base E,   N = sum_b n_b,  SX_j = sum_b n_b X[j, b],
 *   E = sum_b DT_b exp(eta_b)
 * which is sum_b log(rate_b) n_b - rate_b DT_b (trend_rate.py:82).  lik = lik_birth + lik_death; a NaN counts as -inf.
 * SX (sx_spec, sx_exti [P]) is the caller's, computed once on the host.  The accepted E of each side lives in the state: a
 * move touches only its own side and the other side's term is not recomputed.  The sum over j of the second term runs over
 * j ascending as an fma chain from 0.0.  Every sum over bins takes a lane's bins in ascending order (bin b sits in lane
 * b % 64) and then a fixed tree over the lanes; no floating-point atomics: a chain's bits depend on its own arguments alone.
 * Prior (log densities): l0 and m0: Gamma(shape 1, scale 10, loc .001), -inf below 0.001 (trend_rate.py:94-95); every
 * coefficient of a free side, included or not: Normal(0, slab_sd) - an excluded coefficient stays in the state and moves
 * under its prior alone (Kuo-Mallick); every free indicator: log(pI) when 1, log(1 - pI) when 0.
 * One iteration, selector r = MOVE[0].a against the thresholds (0.10, 0.60) where flips are allowed (bvs = 1 and it >=
 * bvs_from), (0.10, 1.0) otherwise, (1.0, 1.0) when both sides are constant.  F = free sides x P; the target is k =
 * min(floor(MOVE[0].b F), F - 1), its side k / P over the free sides in the order birth, death, its covariate j = k % P:
 *   r < first:   l0 (MOVE[1].a < 0.5, or no_death) or m0: x' = x exp(2 log(1.1) (MOVE[1].b - 0.5)), the exponent is the
 *                Hastings term
 *   r < second:  coef' = coef + win[side] NORM[0]; where I_j = 0 the likelihood is the accepted one (no sum is taken)
 *   otherwise:   I_j flips
 * A proposal is accepted where (lik' - lik) + (prior' - prior) + Hastings > log ACCEPT[0].a; iteration 0 always is.
 * The initial state (given = 0): l0 = sum n_spec / sum DT and m0 = sum n_exti / sum DT, 0.1 where that is not finite and
 * positive; every free coefficient 0.1 INIT[index]; I = 0 with bvs, 1 on free sides without it.
 * Chain c draws from the Philox stream of key ((uint32) seed, (uint32) (chain0 + c)).
 *
 * ---- The buffers --------------------------------------------------------------------------------------------------------
 * state [C, LR_MTREND_STATE_W]: see above; everything a launch starts from.
 * rows  [rows_cap, C, LR_MTREND_ROW_W]: one per chain and sampled iteration: [it, posterior = likelihood + prior,
 *   likelihood, likelihood_birth, likelihood_death, prior, l0, m0, I_l[P], a[P], I_m[P], b[P]], the rest of the row 0.
 */
typedef struct lr_mtrend_problem {
    const double* n_spec;   /* [n_bins] */
    const double* n_exti;   /* [n_bins] */
    const double* DT;       /* [n_bins] */
    const double* X;        /* [P, n_bins] */
    const double* sx_spec;  /* [P], host: SX of the birth side; the launch carries it, no call waits for the device */
    const double* sx_exti;  /* [P], host: SX of the death side */
    double* state;          /* [C, LR_MTREND_STATE_W] */
    int32_t n_bins, P, C;
    int32_t m_birth, m_death; /* 1 = the side is constant (-const_B / -const_D), as lr_parbin's sampler 2 takes them */
    int32_t no_death;       /* 0 / 1 */
    int32_t bvs;            /* 0 / 1: the indicators flip */
    int32_t reserved;       /* 0 */
    int64_t bvs_from;       /* the first iteration an indicator may flip at */
    double pI;              /* the prior probability of an indicator */
    double slab_sd;         /* the sd of the Normal prior on every coefficient */
    double win[2];          /* the sd of a coefficient's step: birth, death; may change between launches */
    /* The Philox key of chain c is ((uint32) seed, (uint32) (chain0 + c)): both wrap modulo 2^32. */
    int64_t chain0;         /* Philox key of chain 0 */
    uint64_t seed;
    void* stream;           /* hipStream_t; NULL = default stream */
} lr_mtrend_problem;

/* lr_mtrend_init: given = 0: the initial state of every chain; given = 1: l0, m0, the coefficients and the indicators are
 *   taken from `state` as the caller wrote them (I_j != 0 reads as 1; those of a constant side read as 0).  Either way E,
 *   the likelihoods, the prior and zeroed counters -> state.
 * lr_mtrend_steps: iterations it0 .. it0 + n_iters - 1 of every chain, from `state` and back into it; a row is written
 *   after every iteration with it % s_freq == 0, the first of the launch into slot slot0: rows_cap - slot0 must be at least
 *   ceil((it0 + n_iters) / s_freq) - ceil(it0 / s_freq) (rows may be NULL where that is 0); the other slots are not
 *   touched.  A chain's draws depend on (seed, chain0 + c, it) alone and the state holds everything a launch starts from:
 *   a run cut into launches - in iterations, or into groups of chains with chain0 advanced, also with win changed between
 *   the launches - is the same run bit for bit.
 *   Errors before any launch, in this order: LR_ERR_NULL: the descriptor, n_spec, n_exti, DT, X, sx_spec, sx_exti, state,
 *   rows (where the step arguments are valid and a row is due); LR_ERR_SIZE: n_bins < 1 or > LR_MTREND_MAX_BINS, P < 1 or >
 *   LR_MTREND_MAX_COVS, C < 1, (init) given not 0 or 1; LR_ERR_MODEL: m_birth, m_death, no_death or bvs not 0 / 1, pI not
 *   inside (0, 1), slab_sd not finite and positive, a win not finite or negative, bvs_from < 0; then (steps) LR_ERR_SIZE:
 *   it0 < 0, n_iters < 0, s_freq < 1, slot0 < 0, rows_cap - slot0 too small.  n_iters = 0 launches nothing.               */
int lr_mtrend_init(const lr_mtrend_problem* problem /* host */, int32_t given);
int lr_mtrend_steps(const lr_mtrend_problem* problem /* host */, int64_t it0, int64_t n_iters, int32_t s_freq,
                    double* rows /* [rows_cap, C, LR_MTREND_ROW_W] */, int64_t rows_cap, int64_t slot0);

#ifdef __cplusplus
}
#endif

#endif
