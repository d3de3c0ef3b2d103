/*
 * literate_hip_rjbin.h - C ABI of libliterate_hip.so, the RJ sampler on binned statistics: runMCMC (LRF:216-373) for many
 * chains that do NOT share their data, one wave per chain, all of them in one launch (literate_amd/csrc/lr_rjbin.hip).  The
 * likelihood of runMCMC is a function of the per-bin statistics alone (shift times are floored to unit bins), so chain c
 * carries the statistics of its own replicate - one stochastic imputation of the death times, say - and an iteration costs
 * O(n_bins) whatever the number of lineages.  The conventions and status codes are literate_hip.h's: device pointers unless
 * marked "host", the caller owns every buffer, asynchronous on the stream, 0 = ok, < 0 = LR_ERR_*, > 0 = a hipError_t;
 * buffers may hold anything on entry, an argument error has touched nothing, and the library keeps no state between calls.
 *
 * The stream rides in the descriptor (lr_rjbin_problem.stream, a hipStream_t, NULL = default stream), not in a last
 * parameter of the entry points, as in literate_hip_tmlik.h: every call is asynchronous on that stream and returns after
 * enqueueing (tests/test_hip_replicates.py holds both entry points to it on a busy side stream).
 */
#ifndef LITERATE_HIP_RJBIN_H
#define LITERATE_HIP_RJBIN_H

#include "literate_hip.h"

#define LR_RJBIN_MAX_BINS 512  /* a lane keeps at most 8 bins' statistics in registers */
#define LR_RJBIN_STATE_W 448   /* doubles per chain of the state buffer: 7 rows of LR_ROW */

/* rows of a chain's state, LR_ROW doubles each (element j of a row belongs to lane j) */
#define LR_RJBIN_ROW_L 0       /* birth rates, K_l of them (the rest 0)                                  */
#define LR_RJBIN_ROW_M 1       /* death rates, K_m                                                       */
#define LR_RJBIN_ROW_TL 2      /* birth shift times, K_l + 1: start_time, the shifts, end_time           */
#define LR_RJBIN_ROW_TM 3      /* death shift times, K_m + 1                                             */
#define LR_RJBIN_ROW_EL 4      /* integer bin edge of every birth shift time relative to the first one   */
#define LR_RJBIN_ROW_EM 5      /* the same for the death process                                         */
#define LR_RJBIN_ROW_SCALARS 6
/* elements of the scalar row */
#define LR_RJBIN_S_LIKA 0      /* log-likelihood of the accepted state                                   */
#define LR_RJBIN_S_PRIORA 1    /* its log prior                                                          */
#define LR_RJBIN_S_PRIORPOIA 2 /* the Poisson term cached with it (stale after a Gibbs step, LRF:300-304) */
#define LR_RJBIN_S_GRATE_L 3   /* Gamma_rate[0]                                                          */
#define LR_RJBIN_S_GRATE_M 4   /* Gamma_rate[1]                                                          */
#define LR_RJBIN_S_POI 5       /* Poi_lambda_rjHP                                                        */
#define LR_RJBIN_S_KL 6        /* number of birth rates                                                  */
#define LR_RJBIN_S_KM 7        /* number of death rates                                                  */
#define LR_RJBIN_S_ACCEPTED 8  /* proposals accepted so far (Gibbs steps included)                       */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The model ----------------------------------------------------------------------------------------------------------
 * Replicate r has statistics sp, ex, br [n_bins] (births, deaths, lineage-time per unit bin, as doubles), for model 3 also
 * ex_dead, br_dead (those of the lineages that died before end_time), and its own start_time, end_time, which enter the
 * prior on the shift times, the add move, the guard on short segments and columns 8, 9 of the rows.  Chain c belongs to
 * replicate c / chains_per_rep, C = R chains_per_rep.  Bin b takes the rate of segment j, edge[j] <= b < edge[j + 1] (bins
 * behind the last edge: the last segment); the edges are the shift times floored (rounded for the initial state, LRF:129)
 * minus the first one.  With lam_b, mu_b the rates of bin b:
 *   model 2:     lik = sum_b log(lam_b) sp_b - lam_b br_b + log(mu_b) ex_b - mu_b br_b
 *   model 3:     the death half on ex_dead, br_dead
 *   model 0, 1:  bins with br_b > 0 only, k = br_b:
 *                0: sp_b (log k + log lam_b) + ex_b (log mu_b + log k) - k (lam_b + mu_b)
 *                1: sp_b log lam_b + ex_b (log mu_b + log k) - (k mu_b + lam_b)                     (immigration)
 * Every sum: a lane's bins in ascending order (bin b sits in lane b % 64), then a fixed tree over the lanes; no
 * floating-point atomics: a chain's bits depend on its own arguments alone.
 *
 * The sampler is runMCMC's with the engines' randomness: chain c draws from the Philox stream of key (seed, chain0 + c) at
 * counter (it, purpose, index), purposes 0 .. 10 as the engines use them (oracle/philox.py P_MOVE .. P_INIT); its
 * quirks are kept: the time move that changes nothing but consumes its draws (and re-floors the edges), the Poisson term
 * that goes stale after a Gibbs step, `>=` in the acceptance test, and - the device's own - an add move from LR_KMAX rates
 * is rejected and sets LR_WARN_KCAP in *warn.
 *
 * ---- The buffers --------------------------------------------------------------------------------------------------------
 * state [C, LR_RJBIN_STATE_W]: see the rows above; everything a launch starts from.
 * rows  [rows_cap, C, LR_TRACE_W]: the engines' trace rows (literate_hip.h), one per chain and sampled iteration.
 */
typedef struct lr_rjbin_problem {
    const double* sp;          /* [R, n_bins] */
    const double* ex;          /* [R, n_bins] */
    const double* br;          /* [R, n_bins] */
    const double* ex_dead;     /* [R, n_bins]; model 3, otherwise NULL */
    const double* br_dead;     /* [R, n_bins]; model 3, otherwise NULL */
    const double* start_time;  /* [R] */
    const double* end_time;    /* [R] */
    double* state;             /* [C, LR_RJBIN_STATE_W] */
    uint32_t* warn;            /* one word; bits are OR-ed in, never cleared */
    int32_t n_bins, R, chains_per_rep, model, const_rates, const_death_rate, use_rate_HP;
    /* The Philox key of chain c is ((uint32) seed, (uint32) (chain0 + c)): both wrap modulo 2^32 (tests/test_hip_long_run.py). */
    int64_t chain0;            /* Philox key of chain 0 */
    double poisson_HP;         /* 0: the Poisson rate is sampled, starting at 1 */
    double update_fraction;
    uint64_t seed;
    void* stream;              /* hipStream_t; NULL = default stream */
} lr_rjbin_problem;

/* lr_rjbin_init: the initial state of every chain, with likA, priorA (Gamma rate 2, LRF:227), priorPoiA, both Gamma_rates
 *   (1) and Poi_lambda -> state.  L, M [C, LR_KMAX], tL, tM [C, LR_KMAX + 1], K_l, K_m [C] (1 .. LR_KMAX; device data, NOT
 *   checked, clamped): the initial rates and times of every chain; all six NULL = the CLI's start (LRF:580-583): one
 *   Gamma(2, 2) rate each, drawn at purpose P_INIT, and times [start_time, end_time].
 * lr_rjbin_steps: iterations it0 .. it0 + n_iters - 1 of every chain, from `state` and back into it; a row is written after
 *   every iteration with it % s_freq == 0, the first of the launch into slot slot0: rows_cap - slot0 must be at least
 *   ceil((it0 + n_iters) / s_freq) - ceil(it0 / s_freq) (rows may be NULL where that is 0); the other slots are not
 *   touched.  A chain's draws depend on (seed, chain0 + c, it) alone and the state holds everything a launch starts
 *   from: a run cut into launches is the same run bit for bit.
 *   Errors before any launch, in this order: LR_ERR_NULL: the descriptor, sp, ex, br, start_time, end_time, state, warn,
 *   some but not all of the six initial arrays, rows (where the step arguments are valid and a row is due); LR_ERR_SIZE:
 *   n_bins < 1 or > LR_RJBIN_MAX_BINS, R < 1, chains_per_rep < 1, R chains_per_rep beyond 2^31 - 1; LR_ERR_MODEL: model
 *   outside 0 .. 3, model 3 without ex_dead and br_dead, update_fraction outside [0, 1], poisson_HP < 0 (or either not a
 *   number); then (steps) LR_ERR_SIZE: it0 < 0, n_iters < 0, s_freq < 1, slot0 < 0, rows_cap - slot0 too small.
 *   n_iters = 0 launches nothing.                                                                                         */
int lr_rjbin_init(const lr_rjbin_problem* problem /* host */, const double* L, const double* M, const double* tL,
                  const double* tM, const int32_t* K_l, const int32_t* K_m);
int lr_rjbin_steps(const lr_rjbin_problem* problem /* host */, int64_t it0, int64_t n_iters, int32_t s_freq,
                   double* rows /* [rows_cap, C, LR_TRACE_W] */, int64_t rows_cap, int64_t slot0);

#ifdef __cplusplus
}
#endif

#endif
