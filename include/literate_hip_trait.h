/*
 * literate_hip_trait.h - C ABI of libliterate_hip.so, trait-dependent rates: the RJ skyline sampler of LiteRateForward.py
 * whose rates are multiplied, per lineage, by a logistic function of one static real trait (the model of the reference's
 * other/LiteTraitRate.py, transform_rate_logistic :209-213; literate_amd/csrc/lr_trait.hip).  The conventions and status
 * codes are literate_hip.h's: device pointers unless marked "host", the caller owns every buffer, asynchronous on the stream,
 * 0 = ok, < 0 = LR_ERR_*, > 0 = a hipError_t; buffers may hold anything on entry, an argument error has touched nothing, and
 * the library keeps no state between calls.  The stream rides in the descriptors (a hipStream_t, NULL = default stream), as
 * in literate_hip_rjbin.h.
 *
 * ---- The model ----------------------------------------------------------------------------------------------------------
 * Lineage i has ts_i, te_i and a trait x_i.  s^L_i = 1 / (1 + exp(-kappa_L (x_i - x0_L))), s^M_i likewise with (x0_M,
 * kappa_M).  In unit bin b = [t0 + b, t0 + b + 1] it is born at rate lambda_b s^L_i and dies at rate mu_b s^M_i; lambda and mu
 * are RJ skylines.  With e_ib = max(0, min(te_i, hi_b) - max(ts_i, lo_b)) (lr_bin_unit_events' overlap; a lineage with
 * te <= ts or a NaN carries no time):
 *   log lik = sum_b [ log(lambda_b) sp_b - lambda_b WL_b + log(mu_b) ex_b - mu_b WM_b ] + SlogL + SlogM
 *   WL_b = sum_i s^L_i e_ib,   SlogL = sum of log s^L_i over the births lr_bin_unit_events counts in sp (ts in the window),
 *   WM_b, SlogM: the same with s^M and the deaths counted in ex.
 * Priors: runMCMC's on the baseline; kappa ~ Normal(0, 1) on each side; x0 uniform on [x0_lo, x0_hi] (-inf outside).
 *
 * ---- The fixed point ----------------------------------------------------------------------------------------------------
 * Every term s e of a W_b lies in [0, 1] and is rounded ONCE, to nearest, to a multiple of 2^-F, F = LR_TRAIT_F = 38; the terms
 * are then summed as 64-bit integers (in LDS per (state, bin), then with integer atomics into the workspace), the bins a
 * lineage covers completely through an integer difference array that is prefix-summed exactly: a lineage costs at most four
 * adds per state however many bins it spans, and W_b = the exact integer sum, rounded to fp64 once.  The result does not
 * depend on the order of the adds, on the launch shape or on the other states of the call.  |W_b - the real sum| <=
 * (lineages overlapping bin b) 2^-(F + 1), beside the error of s itself.  No accumulator can overflow while n 2^F < 2^62:
 * n <= LR_TRAIT_MAX_N = 2^24; a larger n is LR_ERR_SIZE.  At kappa = 0 (s = 1/2) and times that are multiples of 2^-32, every
 * term is exact and 2 W_b is lr_bin_unit_events' br_length bit for bit.
 * Slog is a floating-point sum: a thread adds its lineages of a tile in order, a tile is reduced in a fixed tree, and the
 * tiles of a state - a function of n alone - are added in a fixed tree: a state's bits depend on (ts, te, x, its own
 * parameters) alone.  log s = -softplus(-z), z = kappa (x - x0), from u = exp(-|z|): finite for every finite z.
 */
#ifndef LITERATE_HIP_TRAIT_H
#define LITERATE_HIP_TRAIT_H

#include "literate_hip_rjbin.h"

#define LR_TRAIT_F 38                       /* W terms are multiples of 2^-38 */
#define LR_TRAIT_MAX_N (1ll << 24)          /* most lineages: n 2^F < 2^62 */
#define LR_TRAIT_CB 8                       /* states one pass over the lineages scores */
#define LR_TRAIT_TILE 2048                  /* least lineages per tile (but for the last) */
#define LR_TRAIT_MAX_TILES 1024

/* the Philox purposes of the trait move (beside lr_device.h's) */
#define LR_P_TRAIT_MOVE 60                  /* index 0: .a picks the side (< 0.5: birth); index 1: (u_x0, u_kappa) */
#define LR_P_TRAIT_ACCEPT 61                /* index 0: .a the acceptance uniform */

/* a chain's state: lr_rjbin's rows, then the trait row */
#define LR_TRAIT_ROW_SCALARS LR_RJBIN_STATE_W                        /* LR_ROW doubles */
#define LR_TRAIT_ROW_WL (LR_TRAIT_ROW_SCALARS + LR_ROW)              /* LR_RJBIN_MAX_BINS doubles, n_bins used, the rest 0 */
#define LR_TRAIT_ROW_WM (LR_TRAIT_ROW_WL + LR_RJBIN_MAX_BINS)
#define LR_TRAIT_STATE_W (LR_TRAIT_ROW_WM + LR_RJBIN_MAX_BINS)       /* 1536 */
/* elements of the trait scalars */
#define LR_TRAIT_S_X0_L 0
#define LR_TRAIT_S_KAPPA_L 1
#define LR_TRAIT_S_X0_M 2
#define LR_TRAIT_S_KAPPA_M 3
#define LR_TRAIT_S_SLOG_L 4
#define LR_TRAIT_S_SLOG_M 5
#define LR_TRAIT_S_PROPOSED_L 6             /* trait proposals made on the birth side */
#define LR_TRAIT_S_ACCEPTED_L 7
#define LR_TRAIT_S_PROPOSED_M 8
#define LR_TRAIT_S_ACCEPTED_M 9

/* a trace row: the engines' row (literate_hip.h) whose `likelihood` and `posterior` include SlogL + SlogM and whose `prior`
 * and `posterior` include the Normal(0, 1) log densities of both kappa; then x0_l, kappa_l, x0_m, kappa_m, SlogL, SlogM and
 * the trait proposals accepted so far on the birth and on the death side */
#define LR_TRAIT_ROW_W (LR_TRACE_W + 8)

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lr_trait_weights ---------------------------------------------------------------------------------------------------
 * params [C, 2] = (x0, kappa) of C states -> W [C, n_bins], Slog_birth [C], Slog_death [C] (the caller takes the Slog of the
 * side its parameters are for).  One pass over ts, te, x scores a group of LR_TRAIT_CB states: the input is read
 * ceil(C / LR_TRAIT_CB) times.  workspace: at least lr_trait_weights_workspace_bytes(n, n_bins, C) bytes, 256-byte aligned.
 * Errors before any launch, in this order: LR_ERR_NULL: the descriptor, ts, te, x, params, W, Slog_birth, Slog_death,
 * workspace; LR_ERR_SIZE: n < 1 or > LR_TRAIT_MAX_N, n_bins < 1 or > LR_RJBIN_MAX_BINS, C < 1 or > 2^20; LR_ERR_T0: t0 not
 * integer valued or beyond 1e9; LR_ERR_WORKSPACE: workspace_bytes too small.
 * lr_trait_weights_plan: out (host int32[4]) = Cb, lineage tiles, passes, copies of every LDS accumulator. */
typedef struct lr_trait_weights_problem {
    const double* ts;          /* [n] */
    const double* te;          /* [n] */
    const double* x;           /* [n] */
    const double* params;      /* [C, 2] */
    double* W;                 /* [C, n_bins] */
    double* Slog_birth;        /* [C] */
    double* Slog_death;        /* [C] */
    void* workspace;
    int64_t workspace_bytes;
    int64_t n;
    double t0;
    int32_t n_bins, C;
    void* stream;              /* hipStream_t; NULL = default stream */
} lr_trait_weights_problem;

int64_t lr_trait_weights_workspace_bytes(int64_t n, int32_t n_bins, int32_t C);
int lr_trait_weights_plan(int64_t n, int32_t n_bins, int32_t C, int32_t* out /* host */);
int lr_trait_weights(const lr_trait_weights_problem* problem /* host */);

/* ---- The sampler --------------------------------------------------------------------------------------------------------
 * C chains on one data set.  Iteration `it` is a TRAIT MOVE when trait_every > 0 and (it + 1) % trait_every == 0; otherwise
 * it is lr_rjbin's iteration (model 2 on sp, br = WL, ex, br of the death half = WM), unchanged, with its draws.  likA and
 * priorA of the state are the baseline's alone; SlogL + SlogM and the prior of the kappas are added in the trace row.
 * A trait move (after LiteTraitRate.py:399-404): u = pair(it, LR_P_TRAIT_MOVE, 0).a < 0.5 picks the birth side, otherwise
 * the death side; with (ux, uk) = pair(it, LR_P_TRAIT_MOVE, 1): x0' = x0 + (ux - 0.5) win_x0[side], kappa' = kappa +
 * (uk - 0.5) win_kappa[side].  The proposals of all chains go through one lr_trait_weights pass; then, per chain, the
 * baseline likelihood is recomputed from the proposed bins by lr_rjbin's fixed tree, delta = (lik' + Slog') - (likA + Slog)
 * - kappa'^2 / 2 + kappa^2 / 2, and the proposal is accepted when x0_lo <= x0' <= x0_hi and delta >= log
 * pair(it, LR_P_TRAIT_ACCEPT, 0).a: W, Slog and likA are replaced.  A rejected move changes nothing but the count of
 * proposals made.  Chain c draws from the Philox stream of key (seed, chain0 + c).
 *
 * state [C, LR_TRAIT_STATE_W]; rows [rows_cap, C, LR_TRAIT_ROW_W], slots as for lr_rjbin_steps.  workspace: at least
 * lr_trait_workspace_bytes(n, n_bins, C) bytes, 256-byte aligned; it carries nothing from one call to the next.
 * sp, ex [n_bins]: lr_bin_unit_events' counts as doubles.
 *
 * lr_trait_init: params0 [C, 4] = (x0_l, kappa_l, x0_m, kappa_m) of every chain, NULL = all 0; the baseline starts as
 *   lr_rjbin_init's CLI start (one Gamma(2, 2) rate each at purpose P_INIT, times [start_time, end_time]).
 * lr_trait_steps: iterations it0 .. it0 + n_iters - 1; the call loops over the cycles itself - a one-wave-per-chain kernel
 *   that settles the pending proposal, runs the baseline iterations up to the next trait move and proposes, then the weights
 *   pass - and returns with nothing pending: a run cut into calls at any iterations is the same run bit for bit.
 * Errors before any launch, in this order: LR_ERR_NULL: the descriptor, ts, te, x, sp, ex, state, warn, workspace, rows
 *   (where the step arguments are valid and a row is due); LR_ERR_SIZE: n < 1 or > LR_TRAIT_MAX_N, n_bins < 1 or >
 *   LR_RJBIN_MAX_BINS, C < 1 or > 2^20, trait_every < 0; LR_ERR_T0: t0; LR_ERR_MODEL: update_fraction outside [0, 1],
 *   poisson_HP < 0, a window < 0, x0_lo > x0_hi, start_time >= end_time (or any of them not a number); LR_ERR_WORKSPACE;
 *   then (steps) LR_ERR_SIZE: it0 < 0, n_iters < 0, s_freq < 1, slot0 < 0, rows_cap - slot0 too small.
 *   n_iters = 0 launches nothing. */
typedef struct lr_trait_problem {
    const double* ts;          /* [n] */
    const double* te;          /* [n] */
    const double* x;           /* [n] */
    const double* sp;          /* [n_bins] */
    const double* ex;          /* [n_bins] */
    double* state;             /* [C, LR_TRAIT_STATE_W] */
    uint32_t* warn;            /* one word; bits are OR-ed in, never cleared */
    void* workspace;
    int64_t workspace_bytes;
    int64_t n;
    int64_t chain0;            /* Philox key of chain 0 */
    double t0, start_time, end_time;
    double poisson_HP, update_fraction;
    double win_x0[2], win_kappa[2];      /* [0] birth side, [1] death side */
    double x0_lo, x0_hi;
    int32_t n_bins, C, const_rates, const_death_rate, use_rate_HP, trait_every;
    uint64_t seed;
    void* stream;              /* hipStream_t; NULL = default stream */
} lr_trait_problem;

int64_t lr_trait_workspace_bytes(int64_t n, int32_t n_bins, int32_t C);
int lr_trait_init(const lr_trait_problem* problem /* host */, const double* params0 /* [C, 4] or NULL */);
int lr_trait_steps(const lr_trait_problem* problem /* host */, int64_t it0, int64_t n_iters, int32_t s_freq,
                   double* rows /* [rows_cap, C, LR_TRAIT_ROW_W] */, int64_t rows_cap, int64_t slot0);

#ifdef __cplusplus
}
#endif

#endif
