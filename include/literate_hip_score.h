/*
 * literate_hip_score.h - C ABI of libliterate_hip.so, the grouped summary of the RJ trace and its score against known
 * rates (literate_amd/csrc/lr_score.hip): what a simulation study needs after ReplicateEngine has sampled many simulated
 * data sets in one launch - per replicate (a group of chains) the posterior rates through time with their 95 % HPD, the
 * shift frequencies and the K histograms, and over the replicates how often the band holds the truth and how far the
 * posterior mean lies from it.  The conventions and status codes are literate_hip.h's: device pointers unless marked
 * "host", the caller owns every buffer, asynchronous on the stream, 0 = ok, < 0 = LR_ERR_*, > 0 = a hipError_t; buffers
 * may hold anything on entry, an argument error has touched nothing, and the library keeps no state between calls.
 *
 * The stream rides in the descriptor (lr_rtt_score_problem.stream, a hipStream_t, NULL = default stream), not in a last
 * parameter of the entry point, as in literate_hip_rjbin.h: the call is asynchronous on that stream and returns after
 * enqueueing (tests/test_hip_score.py holds it to that on a busy side stream).  It takes no workspace: a group's columns
 * are sorted in LDS.
 */
#ifndef LITERATE_HIP_SCORE_H
#define LITERATE_HIP_SCORE_H

#include "literate_hip.h"

#define LR_SCORE_MAX_SAMPLES 4096 /* samples of a group after burn-in: three columns of doubles in LDS, 96 KB */
#define LR_SCORE_COLS 6           /* columns of `score`, below */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The summary ---------------------------------------------------------------------------------------------------------
 * G = n_chains / chains_per_group groups; group g is chains g chains_per_group .. (g + 1) chains_per_group - 1.  Bins, edges,
 * burn-in (int(burnin n_samples) rows dropped from every chain), the HPD count n_in = round-half-even(0.95 n), a sample's
 * rate in a bin, the shift histogram and the K histograms are lr_rtt_summary's (literate_hip.h) with pooled = 1, applied to
 * the group's chains alone: n = chains_per_group (n_samples - int(burnin n_samples)) samples per group, chain-major.
 *   rates      [G, 3 (birth, death, net), 3 (mean, HPD low, HPD high), n_bins]
 *   shift_freq [G, 2, n_bins]
 *   k_counts   [G, 2 (K_l, K_m), LR_KMAX] int64
 * Every value is bit for bit what lr_rtt_summary(pooled = 1) writes for the group's slice of the trace, the means included
 * (the sorted column summed in that function's order).  n_bins = int(end_age - start_age), under lr_rtt_summary's span
 * rules.
 *
 * ---- The score -----------------------------------------------------------------------------------------------------------
 * truth [G, 2 (birth, death), n_bins], or NULL for the summary alone; the net truth is birth - death.  With it:
 *   covered [G, 3, n_bins] int32: 1 where HPD low <= truth <= HPD high (ends included), else 0
 *   score   [3, n_bins, LR_SCORE_COLS]: over the groups, 0 the number of groups, 1 coverage (the mean of covered), 2 bias =
 *           mean of (posterior mean - truth), 3 mean absolute error, 4 root mean squared error, 5 mean HPD width.
 * Every sum over the groups: thread t adds groups t, t + 256, ... in that order, then a fixed pairwise tree.  No
 * floating-point atomics anywhere: a group's outputs depend on that group's rows and its truth alone, and every output
 * element is written (the buffers need no clearing).  covered and score may be NULL when truth is, and are then ignored.
 */
typedef struct lr_rtt_score_problem {
    const double* trace;       /* [n_samples, n_chains, LR_TRACE_W]: the engines' trace rows */
    const double* truth;       /* [G, 2, n_bins], or NULL */
    double* rates;             /* [G, 3, 3, n_bins] */
    double* shift_freq;        /* [G, 2, n_bins] */
    int64_t* k_counts;         /* [G, 2, LR_KMAX] */
    int32_t* covered;          /* [G, 3, n_bins]; with truth */
    double* score;             /* [3, n_bins, LR_SCORE_COLS]; with truth */
    int32_t n_samples, n_chains, chains_per_group, reserved;
    double start_age, end_age, burnin;
    void* stream;              /* hipStream_t; NULL = default stream */
} lr_rtt_score_problem;

/* lr_rtt_score: one workgroup per (bin, group) reads the group's n rows, sorts the bin's birth, death and net columns in LDS
 *   and writes their mean and HPD, the bin's shift frequencies, (bin 0) the K histograms and, with truth, covered; then one
 *   workgroup per (kind, bin) sums over the groups into score.
 *   Errors before any launch, in this order: LR_ERR_NULL: the descriptor, trace, rates, shift_freq, k_counts, covered or
 *   score while truth is given; LR_ERR_SIZE: n_samples, n_chains or chains_per_group < 1, n_chains not a multiple of
 *   chains_per_group, burnin outside [0, 1), lr_rtt_summary's span rules (a span that is not finite, not positive, integer
 *   valued or beyond LR_MAX_BINS + 1), n_in < 2, n > LR_SCORE_MAX_SAMPLES.                                                */
int lr_rtt_score(const lr_rtt_score_problem* problem /* host */);

#ifdef __cplusplus
}
#endif

#endif
