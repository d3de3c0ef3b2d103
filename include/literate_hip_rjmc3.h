/*
 * literate_hip_rjmc3.h - C ABI of libliterate_hip.so, the Metropolis-coupled RJ sampler (MC3): the sampler of
 * literate_hip_rjbin.h with a ladder of heated chains beside every cold one, which hand their states down by swaps
 * (literate_amd/csrc/lr_rjmc3.hip).  In runMCMC the number and the position of the rate shifts change through the
 * reversible-jump moves alone; a chain on L^beta * prior, beta < 1, crosses between shift configurations more easily.  The
 * conventions and status codes are literate_hip.h's: device pointers unless marked "host", the caller owns every buffer,
 * asynchronous on the stream, 0 = ok, < 0 = LR_ERR_*, > 0 = a hipError_t; buffers may hold anything on entry, an argument
 * error has touched nothing, and the library keeps no state between calls.
 *
 * The stream rides in the descriptor (lr_rjmc3_problem.stream, a hipStream_t, NULL = default stream), not in a last
 * parameter of the entry points, as in literate_hip_rjbin.h (tests/test_hip_mc3.py holds both entry points to the stream
 * contract on a busy side stream).
 */
#ifndef LITERATE_HIP_RJMC3_H
#define LITERATE_HIP_RJMC3_H

#include "literate_hip_rjbin.h"

#define LR_RJMC3_MAX_TEMPS 8   /* temperatures per ladder: the waves of one workgroup */
#define LR_RJMC3_S_POS 9       /* element of the state's scalar row: the replica's position on the ladder (lr_rjbin_* write 0) */
#define LR_RJMC3_LADDER_W 4    /* doubles per position of the ladder buffer: replica, likA, K_l, K_m */
#define LR_RJMC3_WIDE_MAX_BINS 256 /* most bins of a ladder of more than 4 temperatures */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The ladders --------------------------------------------------------------------------------------------------------
 * A ladder is one chain of literate_hip_rjbin.h's sense: there are G = R chains_per_rep of them, ladder g samples replicate
 * g / chains_per_rep.  It holds T replicas; replica (g, w), w = 0 .. T - 1, is wave w of workgroup g, its state sits at
 * state[(g T + w) LR_RJBIN_STATE_W] in lr_rjbin's layout and its Philox key is (seed, chain0 + g T + w).  A replica keeps its
 * key, its state and its hyper-parameters for the whole run; what moves between the replicas of a ladder is the POSITION j,
 * element LR_RJMC3_S_POS of the scalar row, and with it the temperature beta = betas[j].  betas[0] is exactly 1, the betas
 * decrease strictly and are all > 0 (no prior-only rung: with the Gibbs hyper-priors it can run off to overflow).
 *
 * Iteration `it` of the replica at position j is lr_rjbin's with one change: it accepts iff
 *     beta (lik - likA) + priorP - priorA + hasting >= log u.
 * Invalid proposals (a short segment, the cap on the rates) are rejected before the multiply, Gibbs steps are accepted as
 * before; all draws are the engines', purposes 0 .. 10 at counter (it, purpose, index).  Then the trace row (it % s_freq ==
 * 0), then the swap round (swap_every > 0 and (it + 1) % swap_every == 0), round n = (it + 1) / swap_every:
 *   the candidate pairs are the positions (j, j + 1), j = n % 2, n % 2 + 2, ... while j + 1 < T; with a the replica at
 *   position j and b the one at j + 1, u the first uniform of the Philox stream of the ladder's replica 0, key (seed, chain0
 *   + g T), at counter (it, 11, j) - purpose LR_P_SWAP = 11, beside the sampler's 0 .. 10 -: the two exchange their positions iff
 *     (betas[j] - betas[j + 1]) (likA_b - likA_a) >= log u.
 * The waves of a workgroup publish (likA, position) in LDS and meet at a barrier in swap iterations only; every wave
 * evaluates the round from the published values; between rounds no wave waits for another.  No floating-point atomics, no
 * waits between workgroups: a ladder's bits depend on its own arguments alone.
 *
 * ---- The buffers --------------------------------------------------------------------------------------------------------
 * state  [G T, LR_RJBIN_STATE_W]
 * rows   [rows_cap, G, LR_TRACE_W]: the engines' trace row of the replica that holds position 0 in that iteration: column 2
 *        is the likelihood itself, column 1 likA + priorA.
 * ladder [rows_cap, G, T, LR_RJMC3_LADDER_W], may be NULL: for every position of a sampled iteration the replica index w
 *        there, its likA, its K_l and its K_m.
 * swaps  [G, T - 1, 2] int64: (proposed, accepted) of every adjacent pair of positions; zeroed by init, accumulated and never
 *        cleared by steps.  May be NULL at T = 1.
 */
typedef struct lr_rjmc3_problem {
    const double* sp;          /* [R, n_bins] */
    const double* ex;          /* [R, n_bins] */
    const double* br;          /* [R, n_bins] */
    const double* ex_dead;     /* [R, n_bins]; model 3, otherwise NULL */
    const double* br_dead;     /* [R, n_bins]; model 3, otherwise NULL */
    const double* start_time;  /* [R] */
    const double* end_time;    /* [R] */
    double* state;             /* [G T, LR_RJBIN_STATE_W] */
    uint32_t* warn;            /* one word; bits are OR-ed in, never cleared */
    int32_t n_bins, R, chains_per_rep, model, const_rates, const_death_rate, use_rate_HP;
    /* The Philox key of replica (g, w) is ((uint32) seed, (uint32) (chain0 + g T + w)), the swap uniforms' ((uint32) seed,
     * (uint32) (chain0 + g T)): both wrap modulo 2^32, also inside a ladder (tests/test_hip_long_run.py). */
    int64_t chain0;            /* Philox key of replica 0 of ladder 0 */
    double poisson_HP;         /* 0: the Poisson rate is sampled, starting at 1 */
    double update_fraction;
    uint64_t seed;
    const double* betas;       /* host [T]; travels in the kernel arguments */
    int64_t* swaps;            /* [G, T - 1, 2] */
    int32_t T;                 /* temperatures per ladder, 1 .. LR_RJMC3_MAX_TEMPS */
    int32_t swap_every;        /* a swap round after every swap_every iterations; 0: never */
    void* stream;              /* hipStream_t; NULL = default stream */
} lr_rjmc3_problem;

/* lr_rjmc3_init: lr_rjbin_init for every replica (the six arrays [G T, ...], all or none), position = w, swaps zeroed.
 * lr_rjmc3_steps: iterations it0 .. it0 + n_iters - 1 of every replica; rows and ladder are written after every iteration
 *   with it % s_freq == 0, the first of the launch into slot slot0, by lr_rjbin_steps' arithmetic (rows_cap counts the slots
 *   of both).  The draws depend on (seed, key, it) alone and state and swaps hold everything a launch starts from: a run cut
 *   into launches at any iteration, swap iterations included, is the same run bit for bit.
 *   Errors before any launch, in this order: first lr_rjbin_init's / lr_rjbin_steps' own, in their order, on the fields the
 *   two descriptors share (with C = G); then LR_ERR_SIZE: T < 1 or T > LR_RJMC3_MAX_TEMPS; LR_ERR_NULL: betas, or swaps with
 *   T > 1; LR_ERR_MODEL: betas[0] != 1, betas not strictly decreasing in (0, 1] (or not numbers), swap_every < 0;
 *   LR_ERR_SIZE: G T beyond 2^31 - 1, or n_bins > LR_RJMC3_WIDE_MAX_BINS with T > 4: eight bins to a lane do not fit into
 *   the 256 registers that a workgroup of more than four waves leaves each of them.  n_iters = 0 launches nothing.        */
int lr_rjmc3_init(const lr_rjmc3_problem* problem /* host */, const double* L, const double* M, const double* tL,
                  const double* tM, const int32_t* K_l, const int32_t* K_m);
int lr_rjmc3_steps(const lr_rjmc3_problem* problem /* host */, int64_t it0, int64_t n_iters, int32_t s_freq,
                   double* rows /* [rows_cap, G, LR_TRACE_W] */, double* ladder /* [rows_cap, G, T, 4] or NULL */,
                   int64_t rows_cap, int64_t slot0);

#ifdef __cplusplus
}
#endif

#endif
