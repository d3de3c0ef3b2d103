/*
 * literate_hip.h - C ABI of libliterate_hip.so: the MI355X (gfx950) kernels behind the
 * LiteRate RJMCMC birth-death likelihood path.
 *
 * The reference (dsilvestro/LiteRate) is pure Python/numpy and has no FFI layer; the seams
 * this library plugs into are the Python call signatures listed per entry point below
 * (LRF = LiteRateForward.py, lib = literate_library.py, DD = DDRate.py, BDIx =
 * other/LiteRateBDI_ext.py).  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch tensor.data_ptr()) unless it is
 *     marked "host"; the caller owns every buffer, nothing is allocated behind its back;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is
 *     asynchronous on it and returns after enqueueing; the calls that wait for `stream` say "blocks" where they
 *     are declared (lr_mcmc_init / _restore on some engines, lr_mcmc_time_scan, _time_steps, _status, _warnings);
 *   - return value: 0 = ok, <0 = invalid argument (LR_ERR_*), >0 = a hipError_t;
 *   - arithmetic is IEEE fp64, counts are int64 (as numpy in the reference);
 *   - results are bitwise reproducible: all reductions run in a fixed order, no float atomics;
 *   - buffers may hold anything on entry: a workspace is uninitialised memory as far as the library is concerned (what a
 *     call needs cleared it clears itself, on `stream`), and no output is read before it is written - the two exceptions
 *     say so where they are declared (lr_shift_prior with accumulate = 1 adds to its outputs, lr_mcmc_restore resumes the
 *     run its workspace holds).  A call touches only the first *_workspace_bytes bytes of its workspace (lr_simulate_bd:
 *     64; the engine: lr_mcmc_layout.total_bytes) and the documented extents of its outputs, and after an argument
 *     error (LR_ERR_NULL, _SIZE, _MODEL, _WORKSPACE, _T0) it has touched nothing: every argument check comes before the
 *     first launch, copy or memset (tests/test_hip_abi_contract.py holds every entry point to this, on exact-size
 *     buffers between guards).
 */
#ifndef LITERATE_HIP_H
#define LITERATE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LR_OK 0
#define LR_ERR_NULL (-1)      /* a required pointer is NULL                              */
#define LR_ERR_SIZE (-2)      /* a size / count is out of range                          */
#define LR_ERR_MODEL (-3)     /* unknown model id or missing model input                 */
#define LR_ERR_WORKSPACE (-4) /* workspace too small                                     */
#define LR_ERR_T0 (-5)        /* bin origin must be integer valued                       */
#define LR_ERR_STATE (-6)     /* engine used before lr_mcmc_init / after destroy         */
#define LR_ERR_ORDER (-7)     /* persistent engines: lineages not grouped by birth bin (sort them by ts) */

#define LR_KMAX 32     /* max number of rates per process held on the device (reference: unbounded) */
#define LR_ROW 64      /* padded row length of per-chain state arrays                                 */
#define LR_MAX_BINS 4094

/* model ids = the reference's -model_BDI (LRF:388, 421-431) */
#define LR_MODEL_BD 0       /* BDI_partial_lik, birth-death      (LRF:150-162) */
#define LR_MODEL_ID 1       /* BDI_partial_lik, immigration-death               */
#define LR_MODEL_KEIDING 2  /* BD_lik_Keiding                     (LRF:137-148) */
#define LR_MODEL_KEIDING_DEAD 3 /* Keiding, death half on te<end_time (LRF:141-142, 529-546) */

int lr_version(void);

/* ---- A1/A2: sufficient statistics ---------------------------------------------------------
 * Replaces precompute_events + get_br (lib:74-85; LRF:111-123) evaluated for n_windows windows
 * at once (the loop LRF:519-523 / lib create_bins:231-245).  Window w is [win_lo[w], win_hi[w]]:
 *   sp_events[w] = #{ts >= lo && ts <  hi}
 *   ex_events[w] = #{te >  lo && te <= hi}
 *   br_length[w] = sum_i max(0, min(te_i,hi) - max(ts_i,lo))
 * Counts are exact; br_length is summed in a fixed order.                                    */
int64_t lr_bin_events_workspace_bytes(int64_t n, int32_t n_windows);
int lr_bin_events(const double* ts, const double* te, int64_t n,
                  const double* win_lo, const double* win_hi, int32_t n_windows,
                  int64_t* sp_events, int64_t* ex_events, double* br_length,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* The same statistics for the n_bins UNIT windows [t0 + w, t0 + w + 1] the reference always bins into (LRF:519-523:
 * `for i in range(int(min(ts)), int(max(te)))`; lib create_bins:231-245), t0 integer valued: ONE pass over ts / te,
 * 16 bytes per lineage - SURVEY 8(b)'s lr_bin_events(ts, te, n, t0, n_bins, ...).  Counts are exact; br_length[w] is the
 * EXACT sum of the per-lineage overlaps get_br forms (lib:74-79), rounded to fp64 once (integer accumulation: order
 * free, bitwise reproducible); on year-resolution input it equals the reference's value bit for bit.              */
int64_t lr_bin_unit_events_workspace_bytes(int64_t n, int32_t n_bins);
int lr_bin_unit_events(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins,
                       int64_t* sp_events, int64_t* ex_events, double* br_length,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ---- A3: rate index -----------------------------------------------------------------------
 * Replaces get_rate_index + fancy indexing L[indL] (LRF:125-135, 262, 306): expands K segment
 * rates to one rate per unit bin.  rates [C,kmax], times [C,kmax+1] ascending, K [C].
 * mode 0: floor(times) (LRF:262,272,277-278); mode 1: round-half-even (LRF:129, initial call
 * LRF:224-225).  Bin b of chain c gets segment j with e_j <= b < e_{j+1},
 * e_j = int(mode(times[j])) - int(mode(times[0])).                                            */
int lr_expand_rates(const double* rates, const double* times, const int32_t* K, int32_t kmax,
                    int32_t n_chains, int32_t n_bins, int32_t mode,
                    double* rate_bins /* [C,n_bins] */, void* stream);

/* ---- A4/A5/A6: batched per-lineage log-likelihood -----------------------------------------
 * Replaces calc_likelihood(L[indL], M[indM]) (LRF:226, 306, 430-431) for n_chains states at
 * once, in the per-lineage form of BD_partial_lik/get_BDlik (BDIx:124-146): one pass over
 * ts/te per group of chains, unit bins [t0+b, t0+b+1), b < n_bins, t0 integer valued
 * (= int(min ts), LRF:519).  lam_bins/mu_bins [C,n_bins] are the per-bin rates (the
 * L_acc_vec/M_acc_vec arguments).  br_length [n_bins] is required for models 0/1 (it is the
 * k = br_length_bin of LRF:154), end_time for model 3.  out_loglik [C].
 * Few states on few lineages (n <= 2^18, C <= 64, n * C <= 2^21: the reference's own use, one state per iteration) take
 * ONE launch - a block per state builds its table in LDS and walks all lineages (LR_LOGLIK_SMALL=0: never); lam_bins,
 * mu_bins and out_loglik may then as well be pinned HOST memory (device-accessible), which saves the caller two copies
 * and the synchronisation (literate_amd/ops.py LoglikSession).
 * n_bins: 1 .. LR_MAX_BINS for models 0 - 2.  Model 3 keeps two table classes per chain (dead and extant lineages), 64
 * bytes per table entry of n_bins + 2, and one chain's tables must fit the scan's 150 KiB of LDS: n_bins <= 2398.  Above
 * its cap the call and the size query return LR_ERR_SIZE.                                        */
int64_t lr_bd_loglik_workspace_bytes(int64_t n, int32_t n_bins, int32_t n_chains, int32_t model);
/* measurement hook: the launch shape lr_bd_loglik_batch uses for these sizes - out[0] = Cb, the chains one pass over
 * ts / te scores (the call makes ceil(n_chains / Cb) passes = 16 B x n x passes of algorithmic HBM reads), out[1] =
 * lineage tiles per pass, out[2] = table entries reserved per chain and side, out[3] = passes.  out: host int32[4]. */
int lr_bd_loglik_plan(int64_t n, int32_t n_bins, int32_t n_chains, int32_t model, int32_t* out /* host */);
int lr_bd_loglik_batch(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins,
                       const double* lam_bins, const double* mu_bins, int32_t n_chains,
                       int32_t model, const double* br_length, double end_time,
                       double* out_loglik, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- A7/A8: proposal scoring with explicit draws ------------------------------------------
 * Replaces update_multiplier_freq (LRF:165-176 == lib update_multiplier_proposal_vec:156-165),
 * add_shift_RJ_weighted_mean (LRF:29-47) and remove_shift_RJ_weighted_mean (LRF:49-69), one
 * move per chain, randomness supplied by the caller:
 *   move[c] = 0 multiplier: draws[c, 0:K) = binomial mask (0/1), draws[c, kmax:kmax+K) = uniforms
 *   move[c] = 1 add shift : index[c] = interval (0..K-1), draws[c,0] = offset in it, draws[c,1] = Beta(10,10) variate
 *   move[c] = 2 remove    : index[c] = shift (1..K-1)
 * out_score = Hastings term (multiplier) or log q + log Jacobian (RJ).                        */
int lr_rj_propose_score(const double* rates /* [C,kmax] */, const double* times /* [C,kmax+1] */,
                        const int32_t* K, int32_t kmax, int32_t n_chains,
                        const int32_t* move, const int32_t* index,
                        const double* draws /* [C,2*kmax] */, double mult_d,
                        double* out_rates, double* out_times, int32_t* out_K, double* out_score,
                        void* stream);

/* ---- A10: priors --------------------------------------------------------------------------
 * out[c] = prior_gamma(rates[c,:K], a=shape, b=gamma_rate[c]) (LRF:201-202)
 *        + Poisson_prior(K[c], poi_rate[c]) if poi_rate != NULL (LRF:198-199).               */
int lr_log_priors(const double* rates, const int32_t* K, int32_t kmax, int32_t n_chains,
                  double shape, const double* gamma_rate, const double* poi_rate,
                  double* out, void* stream);

/* ---- A12: DDRate rates --------------------------------------------------------------------
 * Replaces the rate half of likelihood_function (DD:71-100): args [C,8] =
 * [l_max,k,x0,div_0,L,m_max,nuB,nuD] -> per-bin birth/death rates, niche, niche fraction
 * (each [C,n_bins]); the likelihood half is lr_bd_loglik_batch(model 2) on those rates.
 * niche_frac ** nu is what numpy's power gives for every fraction >= 0, inf included, and every
 * exponent (x ** 0 = 1 for every x); a negative fraction gives nan (csrc/lr_dd.h).             */
int lr_dd_rates(const double* args, const double* DT, int32_t n_bins, int32_t n_chains,
                int32_t m_birth, int32_t m_death,
                double* birth_rates, double* death_rates, double* niche, double* niche_frac,
                void* stream);

/* ---- the reference's other rate maps onto the same per-bin likelihood ---------
 * lr_ddv2_rates replaces the rate half of DDRatev2.py likelihood_function (DDRatev2.py:73-104):
 * args [C,9] = [l_f,l_mul,k,x0,div_0,L,m_mul,nuB,nuD]; m_birth 0..2, m_death <=0 (rates of 1) / 1 / 2.
 * lr_trend_rates replaces trend_rate.py likelihood_function's rate half (trend_rate.py:73-88):
 * args [C,6] = [l_min,m_min,alpha,beta,delta,gamma], trend [n_bins] = the normalised covariate
 * (parse_trend_data, trend_rate.py:58-69).  Likelihood half: lr_bd_loglik_batch(model 2).     */
int lr_ddv2_rates(const double* args, const double* DT, int32_t n_bins, int32_t n_chains,
                  int32_t m_birth, int32_t m_death,
                  double* birth_rates, double* death_rates, double* niche, double* niche_frac,
                  void* stream);
int lr_trend_rates(const double* args, const double* trend, int32_t n_bins, int32_t n_chains,
                   int32_t const_birth, int32_t const_death,
                   double* birth_rates, double* death_rates, void* stream);

/* Binned Keiding halves of C per-bin rate vectors, out[c] = sum_b log(rate[c,b]) * events[b] - rate[c,b] * DT[b]
 * (DD:86, 101; trend_rate.py:82, 89; the same expression as BD_lik_Keiding LRF:137-148 on create_bins statistics):
 * the likelihood_birth / likelihood_death columns of the DDRate-family logs.                                       */
int lr_binned_keiding(const double* birth_rates, const double* death_rates, const int64_t* n_spec,
                      const int64_t* n_exti, const double* DT, int32_t n_bins, int32_t n_chains,
                      double* out_birth, double* out_death, void* stream);

/* ---- discrete-time birth-death lineage simulator ----------------------------------
 * The scheme of simulateRateABC.v2.py:103-234 and of notebook 4's Simulator / Population: n_start lineages born at
 * step 0; at every step t < n_steps each living lineage draws one uniform r (Philox keyed by (seed, lineage slot),
 * counter (t, 24, 0)): r < lambda_t spawns a lineage born at t, lambda_t <= r < lambda_t + mu_t kills it at t.
 * mode 0: lambda_t = lam_steps[t], mu_t = mu_steps[t] (per-step probabilities, i.e. rate / scale);
 * mode 1: notebook-4 diversity dependence, lambda = max(0, l0 - l0 D/K), mu = max(0, m0 + m0 D/K), both / scale;
 * mode 2: simulateRateABC.v2.py:153-154, lambda = max(0, l0 - (l0-m0) D/K), mu = max(0, m0 + (l0-m0) D/K), / scale;
 * D = living lineages at the start of the step.  Outputs: ts/te [capacity] = birth / death STEP of every lineage
 * (te = n_steps: extant), counters[0] = lineages, counters[1] = living at the end, counters[2] = 1 if `capacity`
 * was hit (later births were dropped); alive_trace[n_steps] (may be NULL) = D per step.  workspace: 64 bytes.   */
int lr_simulate_bd(const double* lam_steps, const double* mu_steps, int32_t n_steps, int32_t mode,
                   double l0, double m0, double K, double scale, int64_t n_start, int64_t capacity,
                   uint64_t seed, double* ts, double* te, int64_t* counters /* [4] */,
                   int64_t* alive_trace, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Batched simulator: many independent mode-0 runs of the scheme above in one launch (the replicates of a posterior
 * predictive check).  Replicate r < n_reps IS the run lr_simulate_bd(lam_steps, mu_steps, n_steps = n_bins * steps_per_bin,
 * mode 0, ..., n_start[r], capacity, seed + r) with lam_steps[t] = lam_bins[r, t / steps_per_bin] / (double) steps_per_bin
 * (likewise mu): the same draws at the same addresses - key ((uint32) (seed + r), lineage slot), counter (t, 24, 0), first
 * uniform - and the same thresholds, so its counts equal that run's bit for bit.  Outputs, exact integers (nothing per
 * lineage is written):
 *   counts [n_reps, 4, n_bins]: per bin b, 0 births during its steps (founders are not births), 1 deaths during its steps,
 *                               2 living at the start of its first step, 3 lineage-steps (the living count summed over its
 *                               steps; / steps_per_bin = branch length in time units);
 *   totals [n_reps, 4]:         lineages created incl. founders, living after the last step, overflow flag, the first step
 *                               at whose start nobody lived or -1.
 * capacity: the most lineages ONE replicate may create, 1 .. 2^31 - 1 (the slot is a 32-bit key).  A replicate that would
 * exceed it sets its overflow flag; its counts are then unspecified and no other replicate is affected.  n_start [n_reps]
 * lives on the device: a value < 1 or > capacity makes that replicate report overflow and nothing else.  An extinct
 * replicate carries zeros on.  The result of a replicate depends on (seed + r, its two rate rows, n_start[r], capacity)
 * only.  One workgroup per replicate at a time, at most LR_SIMBATCH_GROUPS workgroups; the living lineages are a list of
 * slot numbers whose first LR_SIMBATCH_LDS_SLOTS positions sit in LDS, the rest in the workgroup's slice of the workspace.
 * LR_ERR_SIZE: n_reps / n_bins / steps_per_bin < 1, n_bins > LR_MAX_BINS, n_bins * steps_per_bin >= 2^31, capacity outside
 * its range.  The size query is host arithmetic (no device); a smaller workspace is LR_ERR_WORKSPACE.                    */
#define LR_SIMBATCH_GROUPS 512
#define LR_SIMBATCH_LDS_SLOTS 16384
int64_t lr_simulate_bd_batch_workspace_bytes(int32_t n_reps, int32_t n_bins, int32_t steps_per_bin, int64_t capacity);
int lr_simulate_bd_batch(const double* lam_bins /* [n_reps, n_bins] */, const double* mu_bins /* [n_reps, n_bins] */,
                         int32_t n_reps, int32_t n_bins, int32_t steps_per_bin,
                         const int64_t* n_start /* [n_reps] */, int64_t capacity, uint64_t seed,
                         int64_t* counts /* [n_reps, 4, n_bins] */, int64_t* totals /* [n_reps, 4] */,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Batched diversity-dependent simulator: lr_simulate_bd_batch's replicate under DDRate's rate map (the replicates of
 * DDRate.py's posterior predictive check).  Replicate r is lr_simulate_bd_batch's replicate with ONE change: the thresholds
 * of step t are recomputed from the count n_t living at the start of that step,
 *   (br, dr) = the DDRate rates (DD:71-100, csrc/lr_dd.h lr_dd_bin_rates: the function lr_dd_rates and the engine evaluate)
 *              of params[r] = [l_max, k, x0, div_0, L, m_max, nuB, nuD] as the trace holds them (x0 and L unshifted), at
 *              x = x_bins[r, t / steps_per_bin] (the TIME_RANGE value of the simulated bin) with (double) n_t in the place of
 *              DT[b]; the 1e-15 floor and x ** nu = exp(nu * lr_log x) as there;
 *   lt = br / (double) steps_per_bin, mt = dr / (double) steps_per_bin.
 * The living count stands in for DT[b]: the model's DT[b] is the lineage-time lived in bin b, unknown until the bin is
 * over, and the reference's own simulators (simulateRateABC.v2.py:142-166, notebook 4's
 * Diversity_Dependence_Rate_Generator) feed back the count living at the step.  The draws - key ((uint32) (seed + r),
 * lineage slot), counter (t, 24, 0) - and the comparisons - u < lt births, otherwise !(u < lt + mt) survives - are
 * lr_simulate_bd_batch's, so a nan rate means "no event"; counts, totals, capacity, n_start, the workspace and its size
 * have that function's layout and meaning, and with m_birth = 0, m_death = 0 the results equal its results on the
 * constant rates l_max, m_max bit for bit.  m_birth 0..2, m_death -2..2 as lr_dd_rates; anything else is LR_ERR_MODEL.
 * LR_ERR_NULL / LR_ERR_SIZE / LR_ERR_WORKSPACE as lr_simulate_bd_batch; every error is returned before any launch.     */
int64_t lr_simulate_dd_batch_workspace_bytes(int32_t n_reps, int32_t n_bins, int32_t steps_per_bin, int64_t capacity);
int lr_simulate_dd_batch(const double* params /* [n_reps, 8]: l_max, k, x0, div_0, L, m_max, nuB, nuD, as the trace holds them */,
                         const double* x_bins /* [n_reps, n_bins]: TIME_RANGE value of each simulated bin */,
                         int32_t m_birth, int32_t m_death, int32_t n_reps, int32_t n_bins, int32_t steps_per_bin,
                         const int64_t* n_start, int64_t capacity, uint64_t seed,
                         int64_t* counts /* [n_reps, 4, n_bins] */, int64_t* totals /* [n_reps, 4] */,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the text form of the logs (host only, no GPU) ---------------------------------
 * The reference writes every number through Python's csv module (LRF:334-359, DD:236-238): str(float), the shortest
 * decimal string that reads back to the same double, "24.0" / "1e-05" / "1.5e+16" by Python's rules.  lr_format_rows
 * writes n_rows tab-separated lines into `out`: row i = vals[row_start[i] .. row_start[i + 1]); a value in column
 * c < 64 of its row whose bit is set in int_cols is written as an integer; lines end "\n", or "\r\n" with
 * LR_FORMAT_CRLF in flags (csv.writer's default, which DDRate.py and trend_rate.py write).  cap must be at least
 * 26 * (number of values) + 2 * n_rows.  Returns the number of bytes written (>= 0) or LR_ERR_*.  Thread-safe.       */
#define LR_FORMAT_CRLF 1
int64_t lr_format_rows(const double* vals, const int64_t* row_start, int64_t n_rows, uint64_t int_cols, int32_t flags,
                       char* out, int64_t cap);

/* ---- Posterior rates through time: the summary of a run (plotRJforward.v3.py get_marginal_rates :92-139,
 * plot_net_rate :234-270, the shift histogram of get_r_plot :166-178, get_K_values :292-305, calcHPD :12-28) --------------
 * trace: rows [n_chains x n_samples] in the trace layout below, row (sample s, chain c) at trace + (s * n_chains + c) *
 * LR_TRACE_W - the engine's resident trace (its first n_samples slots) or rows a caller assembled.  start_age / end_age =
 * a / b, the root_age / death_age columns.  Bins: edges np.arange(a, b), n_bins = ceil(b - a) - 1, which must equal
 * int(b - a) (else LR_ERR_SIZE: b - a integer valued, where the reference breaks).  Burn-in (0 <= burnin < 1):
 *   pooled = 0: one group per chain, each dropping its first min(int(burnin S), int(0.9 S)) rows (the script's default);
 *   pooled = 1: one group, int(burnin S) rows dropped from every chain, the rest pooled chain after chain (-combine 1).
 * A group of n samples needs n_in = round-half-even(0.95 n) >= 2 (else LR_ERR_SIZE; the reference raises).
 * Outputs (G = 1 pooled, n_chains per chain; bins in ascending time, bin i ending at e_{i+1}):
 *   rates      [G, 3 kinds (birth, death, net = birth - death), 3 (mean, HPD low, HPD high), n_bins] doubles;
 *   shift_freq [G, 2 (birth, death), n_bins]: shift times in the bin / n (0 where the group sampled <= 1 shift time);
 *   k_counts   [G, 2 (K_l, K_m), LR_KMAX] int64: rows with K = 1 .. LR_KMAX.
 * The HPD ends are sample values; means are fixed-order sums over the sorted column / n; counts are exact.  A workspace
 * smaller than lr_rtt_summary_workspace_bytes (the whole problem in one pass) makes the call work through the bins in
 * chunks, down to one bin per chunk (LR_ERR_WORKSPACE below that), with the same results bit for bit.  The size query
 * asks the current device (the sort's temporary storage depends on it): LR_ERR_STATE when there is none.               */
int64_t lr_rtt_summary_workspace_bytes(int32_t n_samples, int32_t n_chains, double start_age, double end_age,
                                       double burnin, int32_t pooled);
int lr_rtt_summary(const double* trace, int32_t n_samples, int32_t n_chains, double start_age, double end_age,
                   double burnin, int32_t pooled, double* rates, double* shift_freq, int64_t* k_counts,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The prior on the times of rate shifts, by Monte Carlo: what the shift frequencies of lr_rtt_summary are read against
 * (plotRJforward.v3.py get_prior_shift :58-89; calcBF :54-56 and get_r_plot :182-195 turn the result into the 2 ln BF = 2
 * and = 6 thresholds, literate_amd/shift_bf.py) -----------------------------------------------------------------------------
 * start_age / end_age = a / b and the bins as lr_rtt_summary: edges np.arange(a, b), n_bins = ceil(b - a) - 1 = int(b - a).
 * Replicates rep0 .. rep0 + n_reps - 1; replicate i draws from Philox4x32-10 with key ((uint32) seed, (uint32) (seed >> 32))
 * and counter (i, purpose 40, idx), u_a / u_b as everywhere in this library; every product and sum below is rounded on its
 * own (no fused multiply-add), so that a numpy restatement gives the same doubles:
 *   idx 0 (poi_lambda <= 0, the reference's Gamma(2, 1) hyper-prior): p0 = (1 - u_a) (1 - u_b), lambda = -log p0;
 *         poi_lambda > 0 (a run with a fixed -Poisson_prior): lambda = poi_lambda, p0 = exp(-lambda);
 *   idx 1: K ~ zero-truncated Poisson(lambda) by inversion: t = p0 + u_a (1 - p0); k = 0, p = cum = p0; repeat { k++;
 *         p = (p lambda) / k; cum = cum + p } while cum <= t and k < LR_SHIFT_PRIOR_KCAP; K = k.  A replicate the cap stopped
 *         (cum <= t still holds) counts in totals[2] and goes on as K = LR_SHIFT_PRIOR_KCAP;
 *   idx 2 + (j >> 1), member a for even j, b for odd j: shift time x_j = (a - 1) + ((b + 1) - (a - 1)) u, j < K - 1.
 * A replicate is rejected when two of the K + 1 points {a, b, x_j} differ by less than 1 (the rounded fp64 difference:
 * min(np.diff(np.sort(points))) < 1).  (The reference takes K as the first positive of 1000 Poisson draws and silently
 * skips the replicate when there is none, probability 1 / 1001^2; here K is always drawn.)  Outputs, exact integers:
 *   totals [4]: accepted replicates, shift times of accepted replicates that fall in a bin, replicates the cap stopped,
 *               shift times of accepted replicates (sum of K - 1);
 *   shift_hist [n_bins]: those shift times per bin (np.histogram on the edges: e_i <= x < e_{i+1}, the last bin closed);
 *   k_drawn / k_accepted [LR_SHIFT_PRIOR_KCAP]: replicates / accepted replicates with K = 1 .. LR_SHIFT_PRIOR_KCAP.
 * accumulate = 0: the outputs are zeroed on the stream first; 1: added to (a replicate range sharded over calls).  The
 * result depends on (a, b, seed, the replicate range, poi_lambda) only: integer atomics, no floating-point ones; at most
 * LR_SHIFT_PRIOR_BLOCKS workgroups stride over the replicates.  No workspace.
 * LR_ERR_SIZE: n_bins < 1 or > LR_MAX_BINS or != int(b - a), n_reps < 1 or > 2^40, rep0 < 0, poi_lambda > 700 or NaN.      */
#define LR_SHIFT_PRIOR_KCAP 64
#define LR_SHIFT_PRIOR_BLOCKS 768
int lr_shift_prior(double start_age, double end_age, int64_t rep0, int64_t n_reps, uint64_t seed, double poi_lambda,
                   int32_t accumulate, int64_t* totals /* [4] */, int64_t* shift_hist /* [n_bins] */,
                   int64_t* k_drawn /* [LR_SHIFT_PRIOR_KCAP] */, int64_t* k_accepted /* [LR_SHIFT_PRIOR_KCAP] */,
                   void* stream);

/* ---- Convergence summary: per-chain ESS and split R-hat (the check the reference's tutorial does in Tracer) ------------
 * rows: [n_samples, n_chains, row_width] doubles, row (sample s, chain c) at rows + (s * n_chains + c) * row_width - the
 * engine's trace (its first n_samples slots) or rows a caller assembled.  cols (host): the n_cols column indices to
 * diagnose.  Every chain drops its first burn = int(burnin * n_samples) rows and keeps n = n_samples - burn.  Needs
 * n >= 4, 0 <= burnin < 1, n_cols >= 1, every column in [0, row_width), max_lag >= 1 (else LR_ERR_SIZE).
 * Per chain c and column k, on the kept series x (Tracer's estimator, BEAST TraceCorrelation):
 *   m = sum x_j / n, d_j = x_j - m;  L = min(n - 1, max_lag);  g_t = sum_{j < n - t} d_j d_{j+t} / (n - t);
 *   V = g_0, then for t = 2, 4, ... while t < L: V += 2 (g_{t-1} + g_t) while that pair sum is > 0, else stop_lag = t;
 *   stop_lag = L if the loop runs out.  ACT = V / g_0 (samples), ESS = n / ACT, SE_mean = sqrt(V / n).
 *   g_0 == 0 (constant after burn-in): mean = the value, SE_mean = 0, stop_lag = 0, ACT = ESS = NaN.
 *   (A sequence of equal values has that value as its mean, here and for the R-hat halves below.)
 * Per column: pooled_mean = the mean of the chain means; pooled_ess = the sum of the finite chain ESS (NaN if none);
 *   rhat = split R-hat (BDA3 11.4): h = n / 2, chain c gives its kept rows [0, h) and [n - h, n); M = 2C sequences of
 *   means mu_q and variances s2_q (divisor h - 1); B = h / (M - 1) sum (mu_q - mu)^2, W = mean s2_q;
 *   rhat = sqrt(((h - 1) / h W + B / h) / W), NaN when W == 0.
 * Outputs: chain_stats [n_cols, n_chains, 4] = (mean, ess, act, se_mean); stop_lag [n_cols, n_chains];
 *   col_stats [n_cols, 3] = (pooled_mean, pooled_ess, rhat).
 * Every sum has an order fixed by the shape alone (no floating-point atomics): the same rows give the same bits.  A
 * series of n <= LR_ESS_LDS_ROWS kept rows is held in LDS; a longer one is centred into the workspace and read from
 * there.  The size query validates the arguments on the host (no device); a smaller workspace is LR_ERR_WORKSPACE.     */
#define LR_ESS_LDS_ROWS 16384
int64_t lr_ess_summary_workspace_bytes(int32_t n_samples, int32_t n_chains, int32_t row_width, const int32_t* cols,
                                       int32_t n_cols, double burnin, int32_t max_lag);
int lr_ess_summary(const double* rows, int32_t n_samples, int32_t n_chains, int32_t row_width, const int32_t* cols,
                   int32_t n_cols, double burnin, int32_t max_lag, double* chain_stats, int32_t* stop_lag,
                   double* col_stats, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Posterior summary of the parametric samplers: mean and 95 % HPD of columns and of per-bin curves (plotDD.py
 * make_vec_dict :11-57, utilities/logAverager.py :18-51: np.mean and calcHPD lib:25-41 of a log's columns) ---------------
 * rows: [n_samples, n_chains, row_width] doubles, row (sample s, chain c) at rows + (s * n_chains + c) * row_width, as in
 * lr_ess_summary.  Every chain drops its first int(burnin * n_samples) rows (0 <= burnin < 1, no cap).  pooled = 0: one
 * group per chain (plotDD.py on one log), G = n_chains; pooled = 1: one group, the kept rows pooled chain after chain
 * (plotDD.py combine_logs :102-118), G = 1.  A group of n samples needs n_in = round-half-even(0.95 n) >= 2 and n < 2^31
 * (else LR_ERR_SIZE).  A value triple is (mean, HPD low, HPD high) by calcHPD's rule: the column sorted, the first window of
 * n_in values of minimum width (strict <), its two ends returned as sample values; mean = a fixed-order sum of the sorted
 * column / n (no floating-point atomics: the same rows give the same bits).  A column that holds a NaN reports NaN in all
 * three: the reference sorts a Python list, and a list sort of unordered values has no defined order, so its answer for
 * such a column depends on where the NaN stood.  (-0.0 sorts below 0.0 here; the two compare equal.)  Infinities are
 * values like any other: a window width inf - inf = NaN behaves as in calcHPD's scan (as the first width it is never
 * replaced: window 0; as a later one it never compares below the minimum), the mean is what the sum gives.
 *   lr_col_summary:   the triples of the n_cols columns cols[] (host, each in [0, row_width)) of any row table;
 *                     out [G, n_cols, 3].
 *   lr_curve_summary: per-bin curves derived on the device from the parameter vector rows[..., arg_col : arg_col + npar]
 *                     by the functions the log columns come from (lr_dd_rates / lr_trend_rates: the same doubles);
 *                     out [G, kinds, 3, n_bins], 1 <= n_bins <= LR_MAX_BINS.
 *                     sampler 1 (DDRate.py, npar 8, aux = DT [n_bins], m_birth / m_death as lr_dd_rates): kinds 0 birth,
 *                     1 death, 2 net = birth - death, 3 niche, 4 nicheFrac; sampler 2 (trend_rate.py, npar 6, aux = TREND
 *                     [n_bins], m_birth / m_death = the -const_B / -const_D flags): kinds 0 birth, 1 death, 2 net.
 *                     Another sampler (or DDRate model ids outside lr_dd_rates') is LR_ERR_MODEL.
 * Workspace: the size queries check the arguments on the host first; the size itself asks the current device (the sort's
 * temporary storage): LR_ERR_STATE when there is none.  per_pass = 0 asks for the whole problem in one pass, k > 0 for
 * passes of k columns / bins.  A workspace smaller than the whole problem's makes the call work through the columns / bins
 * in chunks - also where one pass would exceed the sort's 32-bit counts - down to one per pass (LR_ERR_WORKSPACE below
 * that), with the same results bit for bit.                                                                              */
int64_t lr_col_summary_workspace_bytes(int32_t n_samples, int32_t n_chains, int32_t row_width, const int32_t* cols,
                                       int32_t n_cols, double burnin, int32_t pooled, int32_t cols_per_pass);
int lr_col_summary(const double* rows, int32_t n_samples, int32_t n_chains, int32_t row_width, const int32_t* cols,
                   int32_t n_cols, double burnin, int32_t pooled, double* out, void* workspace, int64_t workspace_bytes,
                   void* stream);
int64_t lr_curve_summary_workspace_bytes(int32_t n_samples, int32_t n_chains, int32_t row_width, int32_t arg_col,
                                         int32_t sampler, int32_t n_bins, double burnin, int32_t pooled,
                                         int32_t bins_per_pass);
int lr_curve_summary(const double* rows, int32_t n_samples, int32_t n_chains, int32_t row_width, int32_t arg_col,
                     int32_t sampler, int32_t m_birth, int32_t m_death, const double* aux, int32_t n_bins, double burnin,
                     int32_t pooled, double* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Model comparison: pointwise WAIC over posterior draws (Watanabe 2010; Vehtari, Gelman & Gabry 2017) ------------
 * l[i, s] = the term lr_bd_loglik_batch adds for lineage i under draw s (lam_bins / mu_bins [n_draws, n_bins]), models 0, 2
 * and 3 (model 1 carries a per-bin constant that belongs to no lineage: LR_ERR_MODEL).  Per lineage, over the S draws:
 *   lppd_i = m_i + log(1/S sum_s exp(l[i, s] - m_i)), m_i = max_s l[i, s];  mean_i = 1/S sum_s l[i, s];
 *   var_i  = sum_s (l[i, s] - mean_i)^2 / (S - 1)      (running maximum with a rescaled sum; Welford / Chan moments)
 * out_pointwise [n, 3] = (lppd_i, mean_i, var_i) in input order.  A lineage with any non-finite l[i, s] (a zero rate gives
 * -inf, a nan rate nan) is FLAGGED: its three outputs are NaN and it is left out of the totals.
 * out_totals [8]: 0 lineages used, 1 lineages flagged, 2 lppd = sum lppd_i, 3 p_waic = sum var_i, 4 elpd_waic =
 *   sum (lppd_i - var_i), 5 se_elpd = sqrt(used * sample variance over i of (lppd_i - var_i)) (NaN when used < 2),
 *   6 the number of used lineages with var_i > 0.4, 7 max_i var_i (NaN when none is used).
 * The [n, S] matrix is never stored: a block owns plan[0] lineages and walks the draws, whose tables pass through
 * LDS plan[1] at a time; on few lineages the draws are split into plan[2] slices (grid.y) whose per-lineage states a
 * second kernel merges in slice order.  lr_waic_plan: out (host int32[4]) = {lineages per tile, draws per LDS chunk, draw
 * slices, tiles}, a function of (n, n_bins, n_draws, model) alone; every sum has a fixed order, so the same inputs give
 * the same bits.  LR_WAIC_SLICES=k in the environment (read at every call; for tests and measurements) asks for k slices
 * instead of the plan's own count (at most n_draws; slices of ceil(n_draws / k) draws).
 * Errors before any launch: n < 1 or n_draws < 2 or an n_bins lr_bd_loglik_batch refuses -> LR_ERR_SIZE; model 1 or
 * unknown, or model 0 without br_length -> LR_ERR_MODEL; t0 not integer valued -> LR_ERR_T0; LR_ERR_WORKSPACE.          */
int64_t lr_waic_workspace_bytes(int64_t n, int32_t n_bins, int32_t n_draws, int32_t model);
int lr_waic_plan(int64_t n, int32_t n_bins, int32_t n_draws, int32_t model, int32_t* out /* host int32[4] */);
int lr_waic_pointwise(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins,
                      const double* lam_bins /* [n_draws, n_bins] */, const double* mu_bins, int32_t n_draws,
                      int32_t model, const double* br_length, double end_time,
                      double* out_pointwise /* [n, 3] */, double* out_totals /* [8] */,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Model comparison: PSIS-LOO over posterior draws (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao &
 * Gabry, "Pareto smoothed importance sampling"; the fit: Zhang & Stephens 2009 as loo::gpdfit) --------------------------
 * Per row (a lineage) of S = n_draws log-likelihood terms l[s], with r = -l the log importance ratios, rmax = max r:
 *   M = min(floor(0.2 S), ceil(3 sqrt S)) (relative efficiency 1).  The draws sorted ascending by (r, draw index): the
 *   last M are the tail t_1 <= ... <= t_M, the one below them the cutoff c (M = 0: c = rmax).
 *   M < 5 or t_M == t_1: nothing is smoothed, pareto_k = +inf.  Otherwise x_j = exp(t_j - rmax) - exp(c - rmax) and the
 *   generalized Pareto fit on m = 30 + floor(sqrt M) grid points theta_j = 1/x_M + (1 - sqrt(m / (j - 1/2))) / (3 x_q),
 *   q = floor(M/4 + 1/2): k(theta) = mean log1p(-theta x), ell_j = M (log(-theta_j / k_j) - k_j - 1),
 *   w_j = 1 / sum_i exp(ell_i - ell_j), theta^ = sum theta_j w_j, k = k(theta^), sigma = -k / theta^.  The tail's log weights
 *   become min(log(sigma expm1(-k log1p(-p_j)) / k + exp(c - rmax)), 0), p_j = (j - 1/2) / M (k == 0: -sigma log1p(-p_j)),
 *   in the tail's sorted order; every other draw keeps r - rmax.  A k or sigma that is not finite leaves the raw weights
 *   and reports +inf.  Reported pareto_k = (M k + 5) / (M + 10).
 *   elpd_loo = logsumexp(l + lw) - logsumexp(lw), evaluated as (max(l + lw) - max lw) + log(sum / sum);
 *   lppd = max l + log(1/S sum exp(l - max l));  n_eff = 1 / sum of the squared normalised weights.
 * out_pointwise [n, 4] = (elpd_loo, pareto_k, lppd, n_eff) in input order; a row with any non-finite term is FLAGGED:
 * four NaN, left out of the totals.
 * out_totals [10]: 0 rows used, 1 flagged, 2 elpd_loo, 3 se_elpd = sqrt(used * sample variance of elpd_loo_i) (NaN when
 *   used < 2), 4 p_loo = sum (lppd_i - elpd_loo_i), 5 lppd, 6 rows with finite k > 0.5, 7 with finite k > 0.7, 8 unsmoothed
 *   rows (k = +inf), 9 the largest finite k (NaN when there is none); 2, 4 and 5 are NaN when no row is used.
 * lr_psis_rows takes any row-major matrix of pointwise log-likelihoods that lives on the device.  Its workspace receives
 * the tail's draw indices, int32 [n_rows, max(M, 1)] in the tail's sorted order (-1 in a flagged row).
 * lr_loo_pointwise computes the terms of lr_waic_pointwise for a batch of plan[2] lineages into a [batch, n_draws] slab at
 * the START of the workspace (at most 64 MiB; whole tiles of 512 when n does not fit one slab), smooths its rows, and goes
 * on to the next batch; lr_loo_plan: out (host int32[4]) = {M, m (0 without a fit), lineages per batch, batches}.
 * LR_LOO_BATCH=b in the environment (read at every call; for tests and measurements) forces min(b, n) lineages per batch.
 * One workgroup sorts one row in LDS (a bitonic network over n_draws padded to a power of two): 2 <= n_draws <= 8192.
 * Every sum has a fixed order; a row's outputs depend on the row alone, not on the batch or the other rows.
 * Errors before any launch, in the order of lr_waic_pointwise: LR_ERR_NULL; n < 1, n_draws outside [2, 8192] or an n_bins
 * lr_bd_loglik_batch refuses -> LR_ERR_SIZE; LR_ERR_MODEL; LR_ERR_T0; LR_ERR_WORKSPACE.                                */
int64_t lr_loo_workspace_bytes(int64_t n, int32_t n_bins, int32_t n_draws, int32_t model);
int lr_loo_plan(int64_t n, int32_t n_bins, int32_t n_draws, int32_t model, int32_t* out /* host int32[4] */);
int lr_loo_pointwise(const double* ts, const double* te, int64_t n, double t0, int32_t n_bins,
                     const double* lam_bins /* [n_draws, n_bins] */, const double* mu_bins, int32_t n_draws,
                     int32_t model, const double* br_length, double end_time,
                     double* out_pointwise /* [n, 4] */, double* out_totals /* [10] */,
                     void* workspace, int64_t workspace_bytes, void* stream);
int64_t lr_psis_rows_workspace_bytes(int64_t n_rows, int32_t n_draws);
int lr_psis_rows(const double* loglik /* device [n_rows, n_draws], row-major */, int64_t n_rows, int32_t n_draws,
                 double* out_pointwise /* [n_rows, 4] */, double* out_totals /* [10] */,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* ---- A11: fused multi-chain RJMCMC --------------------------------------------------------
 * Replaces runMCMC (LRF:216-373) for n_chains independent chains.  Per iteration: one scan of
 * the lineage arrays scoring every chain's proposal, then one chain-step kernel (reduce,
 * Metropolis-Hastings accept, trace write, next proposal, next tables).  Randomness: Philox4x32-10
 * addressed by (iteration, purpose, index), keyed by (seed, chain_offset + chain).            */
typedef struct lr_mcmc_config {
    int64_t n_lineages;
    int32_t n_bins;
    int32_t n_chains;
    int32_t model;            /* LR_MODEL_*                                         */
    int32_t const_rates;      /* -const_rates       (LRF:386, 274)                  */
    int32_t const_death_rate; /* -const_death_rate  (LRF:387, 243-252)              */
    int32_t use_rate_HP;      /* -use_rate_HP       (LRF:395, 285)                  */
    int32_t s_freq;           /* -s sampling frequency (LRF:382, 321)               */
    int32_t n_trace_slots;    /* capacity of the trace buffer in samples            */
    double poisson_HP;        /* -Poisson_prior     (LRF:396, 220-221)              */
    double update_fraction;   /* -update_fraction   (LRF:399)                       */
    double t0;                /* first bin edge = int(min ts)                       */
    double start_time;        /* min(ts)  (LRF:473)                                 */
    double end_time;          /* max(te)  (LRF:474)                                 */
    /* The Philox key of local chain c is ((uint32) seed, (uint32) (chain_offset + c)): both wrap modulo 2^32 (seed 2^32 + 5
     * is seed 5, chain_offset 2^32 - 2 gives chain 2 the key 0; tests/test_hip_long_run.py). */
    uint64_t seed;
    int64_t chain_offset;     /* global index of local chain 0 (multi-GPU sharding) */
    /* unit-resolution data: 1 asserts that EVERY lineage has ts - floor(ts) == frac_birth and
     * te - (ceil(te) - 1) == frac_death (true for year-resolution input + death_jitter, i.e. every
     * dataset the reference ships: 0 and 0.5).  The fractions are then folded into the lookup
     * tables (8-byte entries, half the LDS traffic per lineage).  0 = general times.
     * frac_birth in [0, 1), frac_death in (0, 1]: any shared pair is taken as it is (-death_jitter 0.25 gives
     * (0, 0.25)); frac_death == 1 is integer te (-death_jitter 0 or 1): a death ON a window edge belongs to the bin
     * it closes, and a lineage with te == ts gathers the death entry of the bin BEFORE its birth bin (entry 0, which
     * is 0, when born in the first bin).  The fractions never steer the choice of kernel; only the four-chain
     * kernel's specialised configuration words assume (+0.0, 0.5) and every other pair runs its generic one
     * (tests/test_hip_shared_fractions.py).                                                             */
    int32_t unit_resolution;
    int32_t engine_mode;      /* 0 = auto, 1 = launch-per-iteration engine (fused, pipelined), 2 = a persistent kernel
                               * (the library picks which), 3 = four chains per block, 4 = two chains per block,
                               * 5 = speculative team kernel, 6 = the launch-based plan with its iterations inside the
                               * resident streaming kernel where it applies, 7 = the launch-based engine scanning the
                               * PACKED lineages (lr_mcmc_layout.persistent / .streaming / .packed_scan tell what runs) */
    double frac_birth;
    double frac_death;
    /* ---- sampler 1: the DDRate.py Metropolis-Hastings loop (DD:124-241) on the same engine -------------
     * model must be LR_MODEL_KEIDING, br_length = DT of create_bins (lib:231-257), t0 = ORIGIN, n_bins =
     * N_TIME_BINS.  A chain's state is the parameter vector [l_max,k,x0,div_0,L,m_max,nuB,nuD] (DD:161) in
     * lanes 0..7 of the rate row; a trace row is [it, posterior, likelihood, prior, args[8]].               */
    int32_t sampler;          /* 0 = runMCMC (LRF), 1 = DDRate, 2 = trend_rate (below) */
    int32_t m_birth;          /* -m_birth (DD:25); sampler 2: -const_B flag          */
    int32_t m_death;          /* -m_death (DD:26); sampler 2: -const_D flag          */
    int32_t team_request;     /* speculative kernel: bits 0-7 blocks per team (1, 2, 4, 8), bits 8-15 chains per team (1 or
                               * 2); 0 in either field = the library chooses                                            */
    double dd_present;        /* PRESENT - as create_bins returns it (DD:36)        */
    double dd_init_death;     /* -fix_death (DD:27, 156)                            */
    /* sampler 2: the trend_rate.py loop (trend_rate.py:102-196): parameters [l_min,m_min,alpha,beta,delta,gamma],
     * br_length = the normalised covariate TREND[n_bins] (parse_trend_data, trend_rate.py:58-69), t0 / n_bins as
     * for sampler 1; a trace row is [it, posterior, likelihood, prior, args[6]].                              */
} lr_mcmc_config;

/* where things live inside the engine workspace (byte offsets), for zero-copy host views */
typedef struct lr_mcmc_layout {
    int64_t state_f64;    /* [C, LR_STATE_ROWS, LR_ROW] doubles  (rows: see LR_ROW_* below)  */
    int64_t state_i32;    /* [C, LR_ISTATE_ROWS, LR_ROW] int32                                */
    int64_t bin_consts;   /* [n_bins] doubles: log(br_length) (models 0/1)                    */
    int64_t lineage_idx;  /* [groups] 16 bytes: packed table entries of the lineages (persistent engines): a group = up to
                           * 14 consecutive lineages of one birth bin in 7 slots of one or two lineages: byte 0 birth
                           * index, byte 1 count, then seven 16-bit entry byte offsets (csrc/lr_pack.hip)                  */
    int64_t args_blob;    /* 1 KiB: kernel arguments of the persistent engine, kept in device memory          */
    int64_t tables;       /* [C, table_stride] double2                                        */
    int64_t partials;     /* [C, tiles rounded up to 16] doubles: a chain's tile partials are one row    */
    int64_t trace;        /* [n_trace_slots, C, LR_TRACE_W] doubles                           */
    int64_t total_bytes;
    int32_t table_stride; /* double2 entries per chain                                         */
    int32_t tiles;
    int32_t chains_per_block;
    int32_t trace_width;
    int32_t n_parts;      /* independent chain partitions, each on its own stream                  */
    int32_t pipelined;    /* 1: each partition runs the fused scan|step schedule over two halves   */
    int32_t persistent;   /* 0: launch-per-iteration engine; 1 / 2: persistent kernel, 2 / 4 chains per block;
                           * 3: speculative team kernel (a chain pair per team of team_blocks blocks)             */
    int32_t reserved1;    /* threads per block of the persistent kernel (512 / 1024), 0 for the launch-based engine */
    int64_t status;       /* engine status word (uint32): 0 ok, 1 = a team exchange of the speculative kernel timed out;
                           * the uint32 behind it is the warning word (lr_mcmc_warnings)                                */
    int64_t xchg;         /* partial-sum exchange granules of the speculative kernel's teams (team_blocks > 1); under the
                           * four-chain kernel (persistent == 2) the scan sums a launch leaves for the next one, 512 bytes
                           * per block - engine scratch either way: not part of a run, cleared by init / restore        */
    int32_t team_blocks;  /* blocks (= CUs) that share one chain pair, each scanning 1/team_blocks of the lineages     */
    int32_t table_mode;   /* 0 chain-major general tables, 1 unit-resolution pair tables, 2 pair-general tables (persistent
                           * engines on general lineage times: in-bin fractions packed as 32-bit fixed point)             */
    int64_t lineage_frac; /* [3][groups] uint4: fe' of the 7 slots + sum of fs (table_mode 2)                               */
    int64_t pack_tmp;     /* scratch of the lineage packing (two int32 per lineage + the scans' temporary storage)       */
    int32_t spec_chains_per_team; /* speculative kernel: chains a team of blocks owns - 2 (a pair) or 1; 0 for the other engines */
    int32_t streaming;    /* 1 (persistent == 0 only): too few chains for the pipelined schedule - the iterations run inside one
                           * RESIDENT kernel (csrc/lr_stream.hip: scanner blocks + a stepper wave per chain, the step taken
                           * ahead on the assumption that the pending proposal is rejected) wherever its grid fits the device
                           * at once; xchg then holds the launch's counters and the second table buffer                      */
    int32_t packed_scan;  /* 1 (persistent == 0 only): the launch-based engine scans the PACKED lineages (lineage_idx: 1.14 bytes
                           * per lineage at unit resolution) once per iteration for all its chains (csrc/lr_packscan.hip)
                           * instead of ts / te (16 bytes per lineage); unit-resolution data, too few chains for the
                           * pipelined schedule.  engine_mode 1 keeps the scan of ts / te                               */
    int32_t reserved3;
} lr_mcmc_layout;

/* rows of the fp64 state block (element j of a row lives in lane j of the chain's wave) */
#define LR_ROW_L 0      /* accepted birth rates       [K_l]   */
#define LR_ROW_M 1      /* accepted death rates       [K_m]   */
#define LR_ROW_TL 2     /* accepted birth shift times [K_l+1] */
#define LR_ROW_TM 3
#define LR_ROW_PL 4     /* proposed ... */
#define LR_ROW_PM 5
#define LR_ROW_PTL 6
#define LR_ROW_PTM 7
#define LR_ROW_SCALARS 8 /* see LR_S_* */
#define LR_STATE_ROWS 9
/* scalar slots inside LR_ROW_SCALARS */
#define LR_S_LIKA 0
#define LR_S_PRIORA 1
#define LR_S_PRIORPOIA 2
#define LR_S_GRATE_L 3   /* Gamma_rate[0] (LRF:222, 286) */
#define LR_S_GRATE_M 4
#define LR_S_POI 5       /* Poi_lambda_rjHP (LRF:220-221, 284) */
#define LR_S_HASTING 6   /* of the pending proposal */
#define LR_S_PRIOR_P 7
#define LR_S_PRIORPOI_P 8
#define LR_S_CONST_P 9   /* model constant of the pending proposal (model 1)   */
#define LR_S_CONST_A 10
#define LR_S_LIK_P 11    /* last evaluated proposal log-likelihood (diagnostic) */
#define LR_S_LOG_G0 12   /* cached log(Gamma_rate[0]), log(Gamma_rate[1]), log(Poi_lambda_rjHP) */
#define LR_S_LOG_G1 13
#define LR_S_LOG_POI 14
#define LR_S_LOG_U 15     /* log of the acceptance uniform of the pending proposal's iteration (drawn one step early) */
/* rows of the int32 state block */
#define LR_IROW_EL 0     /* accepted birth bin edges (ints, relative to bin 0) [K_l+1] */
#define LR_IROW_EM 1
#define LR_IROW_PEL 2
#define LR_IROW_PEM 3
#define LR_IROW_SCALARS 4 /* see LR_I_* */
#define LR_ISTATE_ROWS 5
#define LR_I_KL 0
#define LR_I_KM 1
#define LR_I_PKL 2
#define LR_I_PKM 3
#define LR_I_GIBBS 4     /* pending proposal is a Gibbs step (LRF:283-287)     */
#define LR_I_INVALID 5   /* pending proposal fails the LRF:290 guard or K cap  */
#define LR_I_IT_LO 6     /* next iteration number (64 bit)                      */
#define LR_I_IT_HI 7
#define LR_I_ACCEPTED 8  /* number of accepted proposals so far                 */
#define LR_I_MOVE 9      /* kind of the pending proposal: 0 L-mult 1 L-times 2 M-mult 3 M-times 4 RJ 5 Gibbs */
#define LR_I_NEXT_LO 10  /* next iteration number that writes a trace row (64 bit) and its slot     */
#define LR_I_NEXT_HI 11
#define LR_I_SLOT 12

/* trace row (one per chain per sample; columns 0..12 are the _mcmc.log columns LRF:496-502
 * without the adequacy triple, then the _sp_rates / _ex_rates rows LRF:354-359):
 *   [it, posterior, likelihood, prior, lambda_avg, mu_avg, K_l, K_m, root_age, death_age,
 *    gamma_rate_hp_BI, gamma_rate_hp_D, poisson_rate_hp,
 *    L[0..KMAX), tL interior [0..KMAX-1), M[0..KMAX), tM interior [0..KMAX-1)]               */
#define LR_TRACE_HEAD 13
#define LR_TRACE_W (LR_TRACE_HEAD + 2 * (2 * LR_KMAX - 1))

typedef struct lr_engine lr_engine;

int lr_mcmc_query_layout(const lr_mcmc_config* cfg /* host */, lr_mcmc_layout* out /* host */);
int lr_mcmc_create(const lr_mcmc_config* cfg /* host */, const double* ts, const double* te,
                   const double* br_length /* [n_bins], models 0/1, else NULL */,
                   void* workspace, int64_t workspace_bytes, lr_engine** out /* host */);
/* init_state: NULL = the CLI's initial state (K=1, Gamma(2,2) rates, LRF:580-583) drawn from the
 * chain's Philox stream; else device arrays L[C,kmax], M[C,kmax], tL[C,kmax+1], tM[C,kmax+1],
 * KL[C], KM[C] (the runMCMC argument, LRF:218).  Evaluates likA/priorA (LRF:224-230) and
 * prepares the proposal of iteration 0.
 * Not asynchronous everywhere: lr_mcmc_init and lr_mcmc_restore block until `stream` is idle on the persistent engines and on
 * the packed scan (lr_mcmc_layout.persistent != 0 or packed_scan != 0), where they pack the lineages and read the number of
 * packed groups back to the host; on the other engines they return after enqueueing.  Either way their work runs on
 * `stream`, behind what the caller enqueued there (tests/test_hip_stream_contract.py).                                    */
int lr_mcmc_init(lr_engine* e, const double* L, const double* M, const double* tL,
                 const double* tM, const int32_t* KL, const int32_t* KM, int32_t kmax, void* stream);
int lr_mcmc_steps(lr_engine* e, int64_t n_iters, void* stream);
/* Resume (no reference counterpart: the reference cannot resume).  Between two lr_mcmc_steps
 * calls the whole run - accepted states, pending proposals and their tables, iteration counters, trace rows -
 * is the workspace; the Philox draws are addressed by (seed, chain, iteration), so a run continued from a copy of
 * the workspace is bit-identical to an uninterrupted one.  The caller copies a workspace saved from an engine
 * with the SAME configuration (hence the same lr_mcmc_layout) into this engine's workspace, then calls this
 * instead of lr_mcmc_init: it rebuilds what holds device addresses or derives from the data (argument blob,
 * log(br_length), packed lineage indices), forgets what earlier launches left in the engine's scratch regions (status,
 * carried scan sums), keeps the warning word the restored workspace carries (the rows that raised it are still in
 * its trace) and leaves the chains alone.  Chain state written into the workspace from outside
 * must always be followed by this call.                                                                          */
int lr_mcmc_restore(lr_engine* e, void* stream);
/* measurement hook (bench.py roofline): average duration in ms of `reps` back-to-back launches of
 * the engine's lineage-scan kernel on `stream`, timed with HIP events recorded on that stream.
 * Blocks until the launches finish; re-scores the pending proposal, so chain state is unchanged. */
int lr_mcmc_time_scan(lr_engine* e, int32_t reps, float* avg_ms /* host */, void* stream);
/* lr_mcmc_steps(n_iters) bracketed by HIP events on `stream`; blocks; *total_ms = elapsed device time. */
int lr_mcmc_time_steps(lr_engine* e, int64_t n_iters, float* total_ms /* host */, void* stream);
/* Blocks until `stream` is idle and copies the engine status word to *status (host): 0 = ok, 1 = a team exchange of the
 * speculative kernel timed out (its blocks were not all resident within two seconds) and the run is void.          */
int lr_mcmc_status(lr_engine* e, int32_t* status /* host */, void* stream);
/* Blocks until `stream` is idle and copies the engine's warning word to *warnings (host): a bit set of LR_WARN_*.
 * LR_WARN_KCAP: at least one add-shift move (LRF:29-47) was proposed from a state that already holds LR_KMAX rates and
 * was rejected for that reason alone - the reference has no such cap, the posterior on the number of shifts is
 * truncated at LR_KMAX.  Cleared by lr_mcmc_init; lr_mcmc_restore keeps the word of the workspace it resumes.        */
#define LR_WARN_KCAP 2
int lr_mcmc_warnings(lr_engine* e, int32_t* warnings /* host */, void* stream);
/* measurement hook: name of the kernel lr_mcmc_steps spends its time in, as a kernel trace prints it (n >= 64). */
int lr_mcmc_describe(const lr_engine* e, char* buf /* host */, int32_t n);
/* measurement hook: the four-chain kernel with helper waves exists once per configuration word - 0 = generic (reads the
 * configuration at run time; also returned for every other kernel), 1 = models 0 / 1 and 2 = model 2 compiled in together
 * with the default switches (const_rates 0, use_rate_HP on, poisson_HP 0, fractions 0 / 0.5); the same results bit for
 * bit.  The environment variable LR_P4_GENERIC=1, read by lr_mcmc_init / lr_mcmc_restore, forces 0.  lr_mcmc_describe's name
 * carries no word. */
int lr_mcmc_p4_config(const lr_engine* e, int32_t* word /* host */);
/* measurement hook: the scanning lanes of the four-chain kernel with helper waves keep the decoded scan groups of their
 * first trips in registers for a whole launch instead of loading and decoding them in every scan; the same results bit for
 * bit.  out[0] = resident trips per scanner lane in use (the two scanner waves that also make the draws ahead keep fewer),
 * out[1] = resident trips per helper lane, out[2] = packed groups, out[3] = the helper lanes' trips; out[0] = out[1] = 0 for
 * every other kernel and under the environment variable LR_P4_RESIDENT=0, read by lr_mcmc_init / lr_mcmc_restore, which
 * sends every trip through the scan loop. */
int lr_mcmc_p4_resident(const lr_engine* e, int32_t out[4] /* host */);
/* measurement hook: a wave of that kernel that runs all its resident trips takes them as one block of straight-line code,
 * without the test and branch per trip (no gather is requested sooner than in the trip-by-trip form); the same results
 * bit for bit.  out[0] = 1 when that form runs, and the waves that take the block: out[1] of the ten scanner waves, out[2]
 * of the two scanner waves that also make the draws ahead, out[3] of the two helper waves; all zero for every other
 * kernel, without resident groups and under the environment variable LR_P4_PIPE=0, read where LR_P4_RESIDENT is, which
 * runs the resident trips one by one on every wave. */
int lr_mcmc_p4_pipe(const lr_engine* e, int32_t out[4] /* host */);
/* measurement hook: the two scanner waves of that kernel that make a chain's state-independent draws one step ahead run a
 * lean form of the duty - the logarithm of the acceptance uniform rides in a free lane of the step's packed logarithm, the
 * multiplier draws are made only for iterations that can read them; the same results bit for bit.  *out = 1 when the lean
 * form runs, 0 for every other kernel, without the one-block form and under the environment variable LR_P4_LEAN_DRAWS=0,
 * read where LR_P4_RESIDENT is, which runs the full duty. */
int lr_mcmc_p4_draws(const lr_engine* e, int32_t* out /* host */);
int lr_mcmc_destroy(lr_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* LITERATE_HIP_H */
