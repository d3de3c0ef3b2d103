/*
 * literate_hip_mte.h - C ABI of libliterate_hip.so, the multi-trait extinction (MTE) model: the Metropolis-Hastings loop of
 * the reference's other/MTEmodel.py (MTE:287-366) with Bayesian variable selection over several categorical traits, for
 * many chains on many problems (time slices) in one launch, one wave per chain (literate_amd/csrc/lr_mte.hip).  The
 * likelihood depends on a lineage only through its combination of trait states, so a problem is the table of combinations
 * with three statistics per combination, and an iteration costs O(combinations x traits) whatever the number of lineages.
 * The conventions and status codes are literate_hip.h's: device pointers unless marked "host", the caller owns every
 * buffer, asynchronous on the stream, 0 = ok, < 0 = LR_ERR_*, > 0 = a hipError_t; buffers may hold anything on entry, an
 * argument error has touched nothing, and the library keeps no state between calls.  No floating-point atomics, no scratch,
 * no workspace.
 *
 * The stream rides in the descriptor (lr_mte_problem.stream, a hipStream_t, NULL = default stream), not in a last
 * parameter of the entry points, as in literate_hip_parbin.h: every call is asynchronous on that stream and returns after
 * enqueueing (tests/test_hip_mte.py holds both entry points to it on a busy side stream).
 */
#ifndef LITERATE_HIP_MTE_H
#define LITERATE_HIP_MTE_H

#include "literate_hip.h"

#define LR_MTE_MAX_TRAITS 16
#define LR_MTE_MAX_STATES 16   /* per trait: a code fits four bits */
#define LR_MTE_MAX_CATS 128    /* sum of the traits' states: two categories to a lane at most */
#define LR_MTE_MAX_COMBOS 1024 /* a lane keeps at most 16 combinations' statistics in registers */
#define LR_MTE_STATE_W 176     /* doubles per chain of the state buffer */
#define LR_MTE_ROW_W 192       /* doubles per row: 5 + 2 T + sum S_t + 1 <= 166 in use, three stores of a wave */

/* elements of a chain's state; what lies behind T or sum S_t in a block is written as 0 */
#define LR_MTE_S_M 0           /* the mean rate m                                                             */
#define LR_MTE_S_BETA 1        /* beta_hp                                                                     */
#define LR_MTE_S_LIK 2         /* the log-likelihood of the accepted parameters                               */
#define LR_MTE_S_PRIOR 3       /* their log prior                                                             */
#define LR_MTE_S_PROPOSED 4    /* proposals made: [Y, m, indicator]; a rejected proposal counts as proposed   */
#define LR_MTE_S_ACCEPTED 7    /* proposals accepted, likewise; elements 10 .. 15 are 0                        */
#define LR_MTE_S_I 16          /* I_t, 0.0 or 1.0 [LR_MTE_MAX_TRAITS]                                          */
#define LR_MTE_S_SD 32         /* sd_t [LR_MTE_MAX_TRAITS]                                                     */
#define LR_MTE_S_Y 48          /* Y of every trait concatenated [LR_MTE_MAX_CATS]                              */

/* elements of a row */
#define LR_MTE_R_IT 0
#define LR_MTE_R_POST 1
#define LR_MTE_R_LIK 2
#define LR_MTE_R_PRIOR 3
#define LR_MTE_R_M 4
#define LR_MTE_R_I 5           /* I[T], then softmax(Y_t) of every trait concatenated [sum S_t], sd[T], beta_hp */

/* Philox purposes (csrc/lr_device.h) with every index used; the counter is (it, purpose, index), it = 0 for the initial
 * state.  k is a category's index in the concatenation of the traits, t a trait. */
#define LR_P_MTE_MOVE 64       /* 0: a = the move selector, b = the trait of a Y move or of an indicator flip;
                                  1: a = the coin of the Gibbs step, b = the uniform of the multiplier on m     */
#define LR_P_MTE_YMASK 65      /* k: a < 0.5 = category k of the picked trait moves                             */
#define LR_P_MTE_YNORM 66      /* k: the Normal(0, 1) of category k's step (lr_normal)                          */
#define LR_P_MTE_ACCEPT 67     /* 0: a = the acceptance uniform                                                 */
#define LR_P_MTE_GIBBS_BETA 68 /* lr_gamma at base 0: beta_hp                                                   */
#define LR_P_MTE_GIBBS_TAU 69  /* lr_gamma at base 64 t: tau_t                                                  */
#define LR_P_MTE_INIT_Y 70     /* k: the Normal(0, 1) of the initial Y of category k (it = 0)                   */
#define LR_P_MTE_INIT_HP 71    /* lr_gamma at base 64 t: the initial tau_t; at base 1024: the initial beta_hp   */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The model ----------------------------------------------------------------------------------------------------------
 * T categorical traits, trait t with S_t states 0 .. S_t - 1; G combinations of states, code[g, t] the state of trait t in
 * combination g; P problems (time slices) on that one table, problem p with n[p, g] lineages, E[p, g] extinctions and
 * B[p, g] lineage-time in combination g, N_p = sum_g n, E_tot = sum_g E.  Chain c belongs to problem c /
 * chains_per_problem, C = P chains_per_problem.  A chain holds m, Y_t[s], I_t in {0, 1}, sd_t, beta_hp:
 *   q_t = softmax(Y_t) where I_t = 1, 1 / S_t otherwise;  w_g = sum_t q_t[code[g, t]];  Z = sum_g n_g w_g / N_p
 *   lik = sum_g E_g log(m w_g / Z) - B_g m w_g / Z = E_tot log(m / Z) + sum_g E_g log w_g - (m / Z) sum_g B_g w_g
 *   (a combination with E_g = 0 adds nothing to the second sum whatever w_g is; a NaN counts as -inf)
 *   prior = sum_ts Normal(Y_t[s]; 0, sd_t) + sum_t Gamma(1 / sd_t^2; 1.5, rate beta_hp) + Gamma(beta_hp; 1, rate 0.1)
 *           + Gamma(m; 1, rate 1) + log(pI) sum_t I_t                                                   (log densities)
 * One iteration (MTE:305-364), selector r = MOVE[0].a against the thresholds (0.45, 0.46, 0.91) with bvs, (0.90, 0.95,
 * 0.95) without, (0, 1, 1) with `constant`:
 *   r < first:   the trait t = floor(MOVE[0].b T) is picked; every state s >= 1 of it with YMASK[k].a < 0.5 moves by
 *                0.5 YNORM[k]
 *   r < second:  m' = m exp(2 log(1.1) (MOVE[1].b - 0.5)), the exponent is the Hastings term
 *   r < third and it >= bvs_from: the indicator of trait floor(MOVE[0].b T) flips
 *   otherwise:   Gibbs, always accepted: MOVE[1].a > 0.5: beta_hp = Gamma(1 + 1.5 T) / (0.1 + sum_t 1 / sd_t^2); else
 *                every sd_t = 1 / sqrt(tau_t), tau_t = Gamma(1.5 + S_t / 2) / (beta_hp + sum_s Y_t[s]^2 / 2)
 * A proposal is accepted where (lik' - lik) + (prior' - prior) + Hastings >= log ACCEPT[0].a; iteration 0 always is.
 * The initial state (given = 0): m = E_tot / sum_g B_g of the chain's problem, Y_t[0] = 0 and Y_t[s] = 0.1 INIT_Y[k],
 * I_t = 1 without bvs and 0 with it or with `constant`, sd_t = 1 / sqrt(Gamma(1.5 + S_t / 2) / (1 + sum_s Y_t[s]^2 / 2)),
 * beta_hp as in the Gibbs step.
 * Chain c draws from the Philox stream of key ((uint32) seed, (uint32) (chain0 + c)).
 * Every sum over g: a lane's combinations in ascending order (combination g sits in lane g % 64), then a fixed tree over
 * the lanes; every sum over the states of a trait in ascending order: a chain's bits depend on its own arguments alone.
 *
 * ---- The buffers --------------------------------------------------------------------------------------------------------
 * state [C, LR_MTE_STATE_W]: see above; everything a launch starts from.
 * rows  [rows_cap, C, LR_MTE_ROW_W]: one per chain and sampled iteration: [it, posterior = likelihood + prior, likelihood,
 *   prior, m, I[T], softmax(Y_t) of every trait concatenated - whatever I_t is, as MTE:392 logs it -, sd[T], beta_hp], the
 *   rest of the row 0.
 */
typedef struct lr_mte_problem {
    const uint8_t* code;          /* [G, T]; a code >= S_t is the caller's error (the kernel reads it as S_t - 1) */
    const int32_t* n_states;      /* [T] */
    const int32_t* n_states_host; /* [T], host: the same values; the checks and the launch read this copy, so that no call
                                     waits for the device */
    const double* n;              /* [P, G] */
    const double* E;              /* [P, G] */
    const double* B;              /* [P, G] */
    double* state;                /* [C, LR_MTE_STATE_W] */
    int32_t G, T, P, chains_per_problem;
    int32_t bvs, constant;        /* 0 / 1 */
    int64_t bvs_from;             /* the first iteration an indicator may flip at (the reference: 1001) */
    double pI;
    /* The Philox key of chain c is ((uint32) seed, (uint32) (chain0 + c)): both wrap modulo 2^32. */
    int64_t chain0;               /* Philox key of chain 0 */
    uint64_t seed;
    void* stream;                 /* hipStream_t; NULL = default stream */
} lr_mte_problem;

/* lr_mte_init: given = 0: the initial state of every chain; given = 1: m, beta_hp, I, sd and Y are taken from `state` as
 *   the caller wrote them (I_t != 0 reads as 1).  Either way the likelihood, the prior and zeroed counters -> state.
 * lr_mte_steps: iterations it0 .. it0 + n_iters - 1 of every chain, from `state` and back into it; a row is written after
 *   every iteration with it % s_freq == 0, the first of the launch into slot slot0: rows_cap - slot0 must be at least
 *   ceil((it0 + n_iters) / s_freq) - ceil(it0 / s_freq) (rows may be NULL where that is 0); the other slots are not
 *   touched.  A chain's draws depend on (seed, chain0 + c, it) alone and the state holds everything a launch starts from:
 *   a run cut into launches - in iterations, or into groups of problems with chain0 advanced - is the same run bit for bit.
 *   Errors before any launch, in this order: LR_ERR_NULL: the descriptor, code, n_states, n_states_host, n, E, B, state,
 *   rows (where the step arguments are valid and a row is due); LR_ERR_SIZE: G, T, P or chains_per_problem < 1, G >
 *   LR_MTE_MAX_COMBOS, T > LR_MTE_MAX_TRAITS, P chains_per_problem beyond 2^31 - 1, an n_states_host[t] outside 1 ..
 *   LR_MTE_MAX_STATES, their sum beyond LR_MTE_MAX_CATS, (init) given not 0 or 1; LR_ERR_MODEL: bvs or constant not 0 / 1, pI
 *   not inside (0, 1), bvs_from < 0; then (steps) LR_ERR_SIZE: it0 < 0, n_iters < 0, s_freq < 1, slot0 < 0, rows_cap - slot0
 *   too small.  n_iters = 0 launches nothing.                                                                              */
int lr_mte_init(const lr_mte_problem* problem /* host */, int32_t given);
int lr_mte_steps(const lr_mte_problem* problem /* host */, int64_t it0, int64_t n_iters, int32_t s_freq,
                 double* rows /* [rows_cap, C, LR_MTE_ROW_W] */, int64_t rows_cap, int64_t slot0);

#ifdef __cplusplus
}
#endif

#endif
