// lr_plan.hip - the engine planner: which kernel an RJMCMC engine runs, on which tables, in how many partitions and with how
// many threads per block (lr_plan.h: lr_engine_plan), and the workspace layout that follows from it.
//
// Host code only.  lr_plan_engine decides everything in one pass: the table class (lr_plan_scan's, or a pair class of its
// own where a persistent kernel or the packed scan takes the configuration), the kernel family on that class
// (lr_persist_family: the cost models of the persistent kernels against the launches), the packed scan and its partition
// mode, the partitioning and the streaming kernel, the launch shape of whatever scans, and the block width.
// lr_mcmc_query_layout and lr_mcmc_create both go through lr_plan_layout; the engine keeps the plan and nothing re-derives
// any part of it.  The measured numbers in the comments below are the reasons for the thresholds.
#include <cmath>
#include <cstdlib>

#include "lr_dd.h"
#include "lr_plan.h"

// The launch-based engine scans the PACKED lineages (lr_packscan.hip) where that applies and pays: always with too few chains
// for the pipelined schedule; with more, once a pass is long against the chain step it no longer hides (the packed scan runs
// at ~3e13 evals/s - the pipelined launches on ts / te at 7e12 - but serially before the step kernel)
// (p: the plan with the PAIR tables the packed scan reads - unit resolution: the launches' own; general times: the
// pair-general layout of the persistent engines, 32-bit fixed-point fractions)
static bool lr_packscan_planned(const lr_mcmc_config* cfg, const lr_scan_plan& p) {
    if (!lr_packscan_eligible(cfg, p)) return false;
    const bool general = p.unit == LR_TAB_PAIRGEN;
    const double evals = (double)cfg->n_lineages * (double)cfg->n_chains;
    // (chains that the launches on ts / te would not pipeline either: fewer than two blocks' worth - general times: up to the
    // sixteen of the wide scan)
    return cfg->engine_mode == 7 || cfg->n_chains < (general ? 17 : 32) || evals >= (general ? 1.5e8 : 3.0e8);
}

// 0: the launches scan ts / te; 1: the packed lineages in one partition; 2: ... in partitions (long scans)
static int lr_packed_mode(const lr_mcmc_config* cfg, const lr_scan_plan& p) {
    if (!lr_packscan_planned(cfg, p)) return 0;
    const char* env = getenv("LR_PACKED_PARTS");          // 1 / 2 force it (read per call: tests switch it)
    if (env && (atoi(env) == 1 || atoi(env) == 2)) return atoi(env);
    const double evals = (double)cfg->n_lineages * (double)cfg->n_chains;
    // (scratch/exp_packed_parts.py: a tie at n C = 3.2e8, two partitions 3-7 % ahead at 3.8e8 - 6.4e8, 8-16 % beyond; general
    // times cost twice the gathers per eval)
    return evals >= (p.unit == LR_TAB_PAIRGEN ? 1.75e8 : 3.5e8) ? 2 : 1;
}

// Partition layout of the engine.  LR_PARTS (default 2) independent partitions run on their own streams so
// that the ramp-up / drain of one partition's launches overlaps the other's; each partition with at least
// 2*cb chains is software-pipelined in two halves.  All boundaries are multiples of cb.
// packed (lr_packed_mode): the launches scan the packed lineages - never pipelined (one launch scores a group against all
// chains of its partition); 2: partitions on their own streams overlap one's step kernel with the other's scan, 1: one
// partition (short scans: two streams of 5-us kernels do not overlap well - 16 chains x 1e7 lineages 20.9 us per iteration in
// two partitions against 16.4 in one; x 1e8: 54.1 against 63.9)
static int lr_partition(int n_chains, int cb, bool fused_ok, int base[LR_MAX_PARTS + 1], int hA[LR_MAX_PARTS],
                        bool pipelined[LR_MAX_PARTS], int packed) {
    static const int want_parts = lr_env_int("LR_PARTS", 2);
    int parts = want_parts < 1 ? 1 : (want_parts > LR_MAX_PARTS ? LR_MAX_PARTS : want_parts);
    if (packed) fused_ok = false;
    if (packed == 1) parts = 1;
    const int groups = (n_chains + cb - 1) / cb;
    static const int pipeline = lr_env_int("LR_PIPELINE", 1);
    const bool pipe = pipeline && fused_ok;
    while (parts > 1 && groups < parts * (pipe ? 2 : 1)) --parts;
    base[0] = 0;
    for (int p = 0; p < parts; ++p) {
        const int g = groups / parts + (p < groups % parts ? 1 : 0);
        base[p + 1] = base[p] + g * cb < n_chains ? base[p] + g * cb : n_chains;
    }
    base[parts] = n_chains;
    for (int p = 0; p < parts; ++p) {
        const int count = base[p + 1] - base[p];
        pipelined[p] = pipe && count >= 2 * cb;
        hA[p] = pipelined[p] ? ((count / 2 + cb - 1) / cb) * cb : count;
    }
    return parts;
}

// Compute units of the CURRENT device (the engine is planned and created with its device current: literate_amd/engine.py),
// asked every time: a process may drive several devices.  LR_DEVICE_CUS overrides it (planner tests).  Without a device
// to ask (planning on a GPU-less host: the CPU tests) an MI355X is assumed - lr_mcmc_create cannot succeed there anyway.
static int lr_device_cus() {
    const char* v = getenv("LR_DEVICE_CUS");
    if (v && atoi(v) > 0) return atoi(v);
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) return n;
    return 256;
}

// Speculative team kernel (lr_spec.h): one block per CU, a chain pair - or a single chain - owned by a team of k blocks.
// Model of an iteration in microseconds, fitted to MI355X measurements over 1k..200k lineages x k = 1, 2, 4, 8 x chains per
// team (scratch/exp_teams.py, round 3: candidates with a column of their own, no-op moves copying it): with `trips` =
// groups / k / 512 scanner lanes,
//                        a team per PAIR                                  a team per CHAIN
//     unit resolution    k = 1: max(2.95, 2.93 + 0.180 trips)             k = 1: max(2.02, 1.68 + 0.135 trips)
//                        k > 1: max(3.40, 3.20 + 0.205 trips)             k > 1: max(2.78, 2.32 + 0.125 trips) + 0.05 log2(k / 2)
//     general times      k = 1: max(2.90, 2.85 + 0.434 trips)             k = 1: max(2.05, 1.53 + 0.30 trips)
//                        k > 1: max(3.45, 2.90 + 0.478 trips)             k > 1: max(2.63, 2.15 + 0.33 trips) + 0.05 log2(k / 2)
//     DDRate / trend     k = 1: max(2.60, 2.70 + 0.18 trips)              k = 1: max(2.05, 1.55 + 0.125 trips)
//                        k > 1: max(3.05, 2.70 + 0.21 trips)              k > 1: max(2.90, 2.25 + 0.112 trips)
// (a team per chain: refitted in round 4 to the one-chain form of the scan - 8-byte gathers, half the fp64 instructions -,
// scratch/exp_teams.py 1 unit | dd | general on 32 chains; LR_PLAN_CHECK=1 checks the choice on the device in use)
// (the floor is the candidate build - shorter with one chain per CU: the table is built by a helper wave on a SIMD of its
// own, a no-op move copies its table, and the scanners need no table build behind the barrier -; a team pays the exchange
// behind its last scanner; a team per chain scans for one chain what a team per pair scans for two, so it needs the CUs:
// chains x k <= CUs).  Returns the modelled time, the best team size in *k
// (0 = not applicable) and the chains per team.
static double lr_spec_model(const lr_mcmc_config* cfg, bool general, int* k_out, int* cpb_out) {
    const int cus = lr_device_cus();
    *k_out = 0;
    *cpb_out = 2;
    static const int k_env0 = lr_env_int("LR_SPEC_TEAM", 0);
    // (lr_check_cfg has refused a request that is not 1, 2, 4 or 8; a malformed LR_SPEC_TEAM is ignored)
    const int k_req = cfg->team_request & 0xff, cpb_req = (cfg->team_request >> 8) & 0xff;
    const int k_env = k_req > 0 ? k_req : ((k_env0 == 1 || k_env0 == 2 || k_env0 == 4 || k_env0 == 8) ? k_env0 : 0);
    static const int cpb_env0 = lr_env_int("LR_SPEC_CPB", 0);       // 1 / 2 force the chains per team (A/B runs)
    const int cpb_env = cpb_req > 0 ? cpb_req : cpb_env0;
    const double n8 = (double)((cfg->n_lineages + LR_GRP - 1) / LR_GRP);      // groups, for lineages sorted by birth time
    double best = 1e30;
    for (int cpb = 1; cpb <= 2; ++cpb) {
        if (cpb_env != 0 && cpb != cpb_env) continue;
        const int teams = (cfg->n_chains + cpb - 1) / cpb;
        if (teams > cus) continue;
        double best_c = 1e30;
        int k_c = 0;
        for (int k = 1; k <= LR_TEAM_MAX; k *= 2) {
            if (teams * k > cus) break;
            if (k_env > 0 && k != k_env) continue;
            // (groups beyond an XCD's 4 MB of L2 stream from HBM with one group of prefetch per lane: measured 0.32 instead of
            // 0.205 us per trip at 10M lineages; round-2 sweep)
            // (... setting in gradually: 1e6 lineages on general times - 4.6 MB of groups and fractions - ran 8.9 us per
            // iteration of 16 chains where the full penalty predicted 14.7 and the planner took the launches at 15.1: the
            // round-5 sweep, profiles/r05_packed_scan.txt)
            const double over = n8 * 16.0 * (general ? 1.0 + LR_FRAC_ARRAYS : 1.0) / 4.0e6 - 1.0;
            const double sfrac = over <= 0.0 ? 0.0 : (over >= 1.0 ? 1.0 : over);
            const bool streaming = sfrac >= 0.5;
            const double slow = 1.0 + 0.55 * sfrac;
            const double trips = slow * n8 / k / (double)((cpb == 1 ? LR_SPEC_THREADS_SINGLE : LR_SPEC_THREADS) - 256);
            // (a trip that waits for its group to arrive from HBM costs what the memory round trip costs: the one-chain form
            // of the scan, which made the L2-resident trips of a team per chain cheaper in round 4, does not shorten it -
            // the round-3 slopes stay for that regime)
            const double s1 = streaming ? 0.20 : 0.135, sk = streaming ? 0.165 : 0.125;          // unit resolution, a team per chain
            const double d1 = streaming ? 0.20 : 0.125, dk = streaming ? 0.16 : 0.112;           // parametric samplers
            const double g1 = streaming ? 0.46 : 0.30, gk = streaming ? 0.46 : 0.33;             // general times
            double t;
            if (cfg->sampler != 0) {
                if (cpb == 2) t = (k == 1) ? fmax(2.60, 2.70 + 0.18 * trips) : fmax(3.05, 2.70 + 0.21 * trips);
                else t = (k == 1) ? fmax(2.05, 1.55 + d1 * trips) : fmax(2.90, 2.25 + dk * trips);
                if (general) t += ((cpb == 1 && !streaming) ? 0.17 : 0.26) * trips;
            } else if (!general) {
                if (cpb == 2) t = (k == 1) ? fmax(2.95, 2.93 + 0.180 * trips) : fmax(3.40, 3.20 + 0.205 * trips);
                else t = (k == 1) ? fmax(2.02, 1.68 + s1 * trips) : fmax(2.78, 2.32 + sk * trips) + (k == 4 ? 0.05 : (k == 8 ? 0.10 : 0.0));
            } else {
                if (cpb == 2) t = (k == 1) ? fmax(2.90, 2.85 + 0.434 * trips) : fmax(3.45, 2.90 + 0.478 * trips);
                else t = (k == 1) ? fmax(2.05, 1.53 + g1 * trips) : fmax(2.63, 2.15 + gk * trips) + (k == 4 ? 0.05 : (k == 8 ? 0.10 : 0.0));
            }
            if (t < best_c - 0.05) best_c = t, k_c = k;
        }
        if (k_c > 0 && best_c < best) {
            best = best_c, *k_out = k_c;
            *cpb_out = cpb;
        }
    }
    return best;
}

// Persistent engine (lr_persist_kernel): needs unit-resolution tables with byte-sized indices and an
// instantiated table size.  cfg->engine_mode 1 / 2 / 3 force the launch-based / persistent / four-chain persistent
// engine (2 and 3 still need the prerequisites); auto picks the persistent kernel unless the chains are too few for the lineage count: a block
// scans ALL lineages for its two chains, so with few chains and very long inputs the tiled launch-based scan,
// which spreads one chain group over many CUs, is faster.
// Measured iteration times (us, MI355X, scratch/exp_p2_vs_p4.py: 3k..3M lineages x 768 / 1024 / 1536 chains; refitted at
// the end of round 3, the four-chain kernel with helper waves) of the two persistent kernels that take more than 256
// chain pairs, per round of 1024 chains:
//   two-chain kernel (512-thread blocks, two per CU)   f2 = 4.8 + 0.0355 per 1000 lineages
//   four-chain kernel                                  f4 = max(5.45, 3.13 + 0.0362 per 1000 lineages)
//                                                      (general times: max(8.0, 3.8 + 0.091 per 1000 lineages), round 2)
// and a remainder of at most 512 chains costs the two-chain kernel 0.62 of a round.
static double lr_model_two_chain(const lr_mcmc_config* cfg) {
    const double kn = (double)cfg->n_lineages * 1e-3;
    const int C = cfg->n_chains, rem = C % 1024;
    const double f2 = 4.8 + 0.0355 * kn;
    return f2 * ((double)(C / 1024) + (rem == 0 ? 0.0 : (rem <= 512 ? 0.62 : 1.0)));
}
static double lr_model_four_chain(const lr_mcmc_config* cfg, bool general) {
    const double kn = (double)cfg->n_lineages * 1e-3;
    const double f4 = general ? fmax(8.0, 3.8 + 0.091 * kn) : fmax(5.45, 3.13 + 0.0362 * kn);
    return f4 * (double)((cfg->n_chains + 1023) / 1024);
}

// Which persistent kernel runs the tables p, 0 for none (the launch-based engine): the prerequisites and the cost models
// above, evaluated once.  *team_k, *team_cpb: blocks and chains per team of the speculative kernel, else 0.
// Which persistent kernel: 1 = two chains per 512-thread block (lr_persist_kernel), 2 = four chains per 1024-thread
// block in ping-pong (lr_persist4_kernel), 3 = the speculative team kernel (at most 256 chain pairs).  The four-chain
// block hides the chain step under the other pair's scan, so beyond 256 pairs it wins while a scan is about as long as a
// step (from ~20k lineages up, whole rounds of 1024 chains); the two-chain kernel, two blocks per CU, is ahead on short
// scans (the step is all there is) and on remainders of at most 512 chains; on very long scans the two tie.
static int lr_persist_family(const lr_mcmc_config* cfg, const lr_scan_plan& p, int* team_k, int* team_cpb) {
    *team_k = 0, *team_cpb = 0;
    static const int env = lr_env_int("LR_PERSIST", -1);   // debugging override: 0 off, 1 on
    if (env == 0 || cfg->engine_mode == 1 || cfg->engine_mode == 6 || cfg->engine_mode == 7) return 0;
    if (!p.unit || cfg->n_bins + 2 > LR_H_WIDE || p.cb < 2) return 0;
    const bool general = p.unit == LR_TAB_PAIRGEN;   // general times: the speculative (H <= 136) and four-chain kernels only
    // the packing holds lineage indices as int32 and the scan loops address the groups by 32-bit byte offsets
    if (cfg->n_lineages >= (1ll << 31) - 1 || lr_groups_alloc(cfg->n_lineages) * 16 >= (1ll << 32)) return 0;
    if (p.H != 40 && p.H != 72 && p.H != 136 && p.H != 264 && p.H != LR_H_WIDE) return 0;
    int k = 0, cpb = 2;
    const double t_spec = (p.H > (general ? 136 : 264)) ? 1e30 : lr_spec_model(cfg, general, &k, &cpb);   // few chains: a team of CUs per pair
    if (env != 1 && cfg->engine_mode < 2) {
        const double n = (double)cfg->n_lineages, c = (double)cfg->n_chains;
        // the best persistent kernel for the shape (microseconds) against the tiled launches (measured: 7e12 evals/s at unit
        // resolution, 3e12 on general times, 15.5 us of launches per iteration + 1 us per 1024 chains of the step blocks:
        // scratch/exp_plan_small.py - with a flat 14 us, 4096 chains on short inputs went to the launches at 19.5 - 23 us
        // where the two-chain kernel runs 15.7 - 19.1)
        double t_persist = lr_model_four_chain(cfg, general);
        if (!general) t_persist = fmin(t_persist, lr_model_two_chain(cfg));
        if (k > 0 && t_spec < t_persist) t_persist = t_spec;
        double t_launch = n * c / (general ? 3e12 : 7e12) * 1e6 + 15.5 + c / 1024.0;
        // ... or, at unit resolution, one launch over the packed lineages for all chains + the step kernel (16 chains x 1e7 / 3e7 /
        // 1e8 lineages: 16.3 / 27.0 / 63.9 us per iteration, scan alone 9.6 / 19.7 / 55.8: round 5)
        // (general times: sixteen gathers per group and pair instead of eight)
        // (only where the launches WOULD scan the packed lineages: lr_packscan_planned)
        if (lr_packscan_planned(cfg, p)) t_launch = fmin(t_launch, 11.5 + 5.0 * c / 1024.0 + n * c / (general ? 1.5e13 : 3.1e13) * 1e6);
        if (t_persist > t_launch) return 0;
    }
    static const int p4_env = lr_env_int("LR_PERSIST4", -1);
    static const int spec_env = lr_env_int("LR_SPEC", -1);
    if (k > 0 && t_spec < 1e29 && cfg->engine_mode != 3 && cfg->engine_mode != 4 && spec_env != 0) {
        // the two-chain kernel with all 16 waves scanning wins only on long scans without room for a team
        // (measured at 256 pairs, 10k..1M lineages, scratch/exp_engines.py: 4.41 + 0.236 us per trip of its 1024 scanner
        // lanes, 4.1 at least; the speculative kernel is ahead up to ~200k lineages)
        const double t_wide = general ? 1e30 : fmax(4.1, 4.41 + 0.236 * (double)((cfg->n_lineages + LR_GRP - 1) / LR_GRP) / 1024.0);
        if (cfg->engine_mode == 5 || spec_env == 1 || t_spec <= t_wide) {
            *team_k = k, *team_cpb = cpb;
            return 3;
        }
    }
    if (cfg->engine_mode == 5) return 0;
    if (general) return (p.cb >= 4 && cfg->engine_mode != 4) ? 2 : 0;
    if (p.cb < 4) return 1;                 // tables are laid out per group of cb chains; a quad must not straddle
    if (cfg->engine_mode == 3) return 2;
    if (cfg->engine_mode == 4) return 1;
    if (p4_env >= 0) return p4_env ? 2 : 1;
    return lr_model_four_chain(cfg, false) < lr_model_two_chain(cfg) ? 2 : 1;
}

// threads per persistent block.  The two-chain kernel with one block per CU at most gets the whole CU (16 waves on the one
// pair); short scans keep 512: the 16-wave barrier costs more than it buys
static int lr_block_threads(const lr_mcmc_config* cfg, int family, int team_cpb) {
    static const int wide_env = lr_env_int("LR_PERSIST_WIDE", -1);
    const bool wide = wide_env >= 0 ? wide_env != 0 : ((cfg->n_chains + 1) / 2 <= 256 && cfg->n_lineages >= 20000);
    if (family == 3) return team_cpb == 1 ? LR_SPEC_THREADS_SINGLE : LR_SPEC_THREADS;
    return family == 2 ? 1024 : (family == 1 ? (wide ? 1024 : 512) : 0);
}

// The pair class of its own a configuration has beside the launch plan p, if any: tables only the persistent kernels and the
// packed scan read (outside the kernels: lr_pairscan_kernel).  At most one of the three applies:
static bool lr_pair_class(const lr_mcmc_config* cfg, const lr_scan_plan& p, lr_scan_plan* q) {
    int H = 0;
    bool general = !cfg->unit_resolution;
    if (cfg->model == LR_MODEL_KEIDING_DEAD && cfg->n_bins <= 258) {
        // model 3 on a persistent engine: one table class with an extant block behind the death-side entries (lr_step.h),
        // so the half-stride must hold 2 (n_bins + 2) entries
        // (... or, on the same tables, under the launch-based engine scanning the packed lineages: their death-side slots
        // point extant lineages at the extant block)
        static const int fast_H[] = {40, 72, 136, 264, LR_H_WIDE};
        for (int h : fast_H)
            if (2 * (cfg->n_bins + 2) <= h) {
                H = h;
                break;
            }
    } else if (!p.unit && p.fast && p.n_cls == 1) {
        // general lineage times: a persistent engine takes them in the pair-general table layout (LR_TAB_PAIRGEN) with the
        // in-bin fractions packed as 32-bit fixed point; if none applies the plan stays the launch-based engine's
        // (... or the launch-based engine scanning the packed lineages, on the same pair-general tables)
        // (a lone chain at unit resolution is here too: it cannot fill a pair entry, lr_plan_scan gave it general tables)
        H = p.H, general = true;
    } else if (!p.fast && cfg->model != LR_MODEL_KEIDING_DEAD && cfg->n_bins + 2 <= LR_H_WIDE && cfg->n_bins <= 64 * lr_bins_per_lane(LR_H_WIDE)) {
        // 255..512 bins: beyond the table sizes the launch-based scans are instantiated for, but the persistent kernels
        // (two- and four-chain; the packed groups address their entries with 16 bits) take one more class, H = 520;
        // the scans outside the kernels go through lr_pairscan_kernel as they do for pair-general tables
        // (... or the launch-based engine scanning the packed lineages: two pairs of H = 520 tables per block)
        H = LR_H_WIDE;
    }
    if (!H) return false;
    *q = p;
    q->n_cls = 1, q->fast = 1, q->H = H;
    q->unit = general ? LR_TAB_PAIRGEN : LR_TAB_UNIT;
    q->cb = general ? 4 : 16;
    while (!general && q->cb > 2 && q->cb / 2 >= cfg->n_chains) q->cb >>= 1;
    q->tab_stride = general ? 2 * H : H;
    q->groups = (cfg->n_chains + q->cb - 1) / q->cb;
    return true;
}

// Take the tables q with the kernel family that runs them.  A pair class of its own (lr_pair_class) is taken only where a
// persistent kernel runs on it or the launch-based engine scans the packed lineages on it; the launch plan is taken whatever
// runs on it.
static bool lr_take_class(const lr_mcmc_config* cfg, const lr_scan_plan& q, bool pair_only, lr_engine_plan* plan) {
    int team_k = 0, team_cpb = 0;
    const int family = lr_persist_family(cfg, q, &team_k, &team_cpb);
    if (pair_only && family == 0 && !lr_packscan_planned(cfg, q)) return false;
    plan->scan = q;
    plan->family = family, plan->team_blocks = team_k, plan->team_cpb = team_cpb;
    plan->pair_only = pair_only;
    return true;
}

int lr_plan_engine(const lr_mcmc_config* cfg, lr_engine_plan* plan) {
    // (general times, 9 to 16 chains: ONE pass of the sixteen-chain scan - lr_scan_wide_kernel - instead of two halves of eight)
    lr_scan_plan p, q;
    const int rc = lr_plan_scan(cfg->n_lineages, cfg->n_chains, cfg->n_bins, cfg->model, cfg->unit_resolution, &p,
                                (!cfg->unit_resolution && cfg->n_chains > 8 && cfg->n_chains <= 16 && lr_env_int("LR_ENGINE_WIDE", 1)) ? 1 : 0);
    if (rc) return rc;
    if (!lr_pair_class(cfg, p, &q) || !lr_take_class(cfg, q, true, plan)) lr_take_class(cfg, p, false, plan);
    lr_scan_plan& s = plan->scan;
    plan->threads = lr_block_threads(cfg, plan->family, plan->team_cpb);
    plan->packed_mode = lr_packed_mode(cfg, s);
    plan->packed_scan = plan->family == 0 && plan->packed_mode != 0;
    plan->streaming = false;
    // The launch plan gets the launch shape of the engine that would run it without a persistent kernel, whichever family
    // runs it; a pair class of its own under a persistent kernel keeps lr_plan_scan's tiles (lr_pairscan_kernel's grid).
    const bool shaped = !(plan->pair_only && plan->family != 0);
    // the scan over the packed lineages: its tiles sized to the device, eight chains per partition boundary
    if (shaped && plan->packed_mode) lr_packscan_plan(cfg, &s, lr_device_cus());
    plan->n_parts = lr_partition(cfg->n_chains, s.cb, lr_fused_supported(s), plan->base, plan->hA, plan->pipelined, plan->packed_mode);
    if (!shaped || plan->packed_mode) return LR_OK;
    if (!plan->pipelined[0]) {
        // too few chains for two halves, opt-in: the resident streaming kernel, its tiles sized to the device's block slots
        if (plan->n_parts == 1 && lr_stream_eligible(cfg, s)) {
            lr_stream_plan(cfg, &s, lr_device_cus());
            plan->streaming = plan->family == 0;
        }
        return LR_OK;
    }
    // launch shape of the pipelined schedule: as lr_plan_scan, but the lineage tiles are sized so that the fused launches that
    // run concurrently (one per partition: step blocks of one half + scan blocks of the other) fill the resident block
    // slots of the chip (256 CUs x 4 blocks) exactly once.
    const int count = plan->base[1] - plan->base[0];
    const int half = plan->hA[0] > count - plan->hA[0] ? plan->hA[0] : count - plan->hA[0];
    const int groups_half = (half + s.cb - 1) / s.cb;
    const int step_blocks = (half + (LR_SCAN_THREADS / LR_WAVE) - 1) / (LR_SCAN_THREADS / LR_WAVE);
    static const int slots = lr_env_int("LR_SLOTS", 256 * 4);
    long long tiles = (slots / plan->n_parts - step_blocks) / groups_half;
    const long long unit = 2 * LR_SCAN_THREADS;
    const long long max_tiles = (cfg->n_lineages + 4 * unit - 1) / (4 * unit);
    if (tiles > max_tiles) tiles = max_tiles;
    if (tiles < 1) tiles = 1;
    long long chunk = lr_align_up64((cfg->n_lineages + tiles - 1) / tiles, unit);
    tiles = (cfg->n_lineages + chunk - 1) / chunk;
    s.tiles = (int)tiles;
    s.chunk = chunk;
    return LR_OK;
}

static int lr_check_cfg(const lr_mcmc_config* cfg) {
    if (!cfg) return LR_ERR_NULL;
    if (cfg->n_lineages < 1 || cfg->n_chains < 1 || cfg->s_freq < 1 || cfg->n_trace_slots < 0) return LR_ERR_SIZE;
    if (cfg->n_bins < 1 || cfg->n_bins > LR_MAX_BINS) return LR_ERR_SIZE;
    if (cfg->model < 0 || cfg->model > 3) return LR_ERR_MODEL;
    if (cfg->t0 != floor(cfg->t0)) return LR_ERR_T0;
    if (!(cfg->end_time > cfg->start_time)) return LR_ERR_SIZE;
    if (cfg->sampler < 0 || cfg->sampler > 2) return LR_ERR_MODEL;
    {
        const int k_req = cfg->team_request & 0xff, cpb_req = (cfg->team_request >> 8) & 0xff;
        if (cfg->team_request < 0 || cfg->team_request > 0xffff) return LR_ERR_SIZE;
        if (k_req != 0 && k_req != 1 && k_req != 2 && k_req != 4 && k_req != 8) return LR_ERR_SIZE;   // a team is 1, 2, 4 or 8 blocks (LR_TEAM_MAX)
        if (cpb_req > 2) return LR_ERR_SIZE;                                                           // ... of one chain or a pair
    }
    if (cfg->sampler != 0) {
        if (cfg->model != LR_MODEL_KEIDING) return LR_ERR_MODEL;
        if (cfg->n_bins > LR_DD_MAXP * LR_WAVE) return LR_ERR_SIZE;
    }
    if (cfg->sampler == 1) {
        if (cfg->m_birth < 0 || cfg->m_birth > 2 || cfg->m_death < -2 || cfg->m_death > 2) return LR_ERR_MODEL;
        if (!(cfg->dd_present > cfg->t0)) return LR_ERR_SIZE;
    }
    return LR_OK;
}

int lr_plan_layout(const lr_mcmc_config* cfg, lr_engine_plan* plan, lr_mcmc_layout* out) {
    int rc = lr_check_cfg(cfg);
    if (rc) return rc;
    if (!out) return LR_ERR_NULL;
    rc = lr_plan_engine(cfg, plan);
    if (rc) return rc;
    const lr_scan_plan& p = plan->scan;
    const long long C = cfg->n_chains;
    const long long table_bytes = lr_align_up64((long long)lr_align_up64(C, p.cb < 2 ? 2 : p.cb) * p.tab_stride * 16, 256);
    long long o = 0;
    out->state_f64 = o, o += lr_align_up64(C * LR_STATE_ROWS * LR_ROW * 8, 256);
    out->state_i32 = o, o += lr_align_up64(C * LR_ISTATE_ROWS * LR_ROW * 4, 256);
    out->bin_consts = o, o += lr_align_up64((long long)(cfg->n_bins + 2) * 8, 256);   // log(br) + the DD constants
    // packed lineages of the persistent engines (lr_pack.hip): groups of LR_GRP lineages of one birth bin, 16 bytes of
    // table indices each; on general times LR_FRAC_ARRAYS more uint4 arrays with the in-bin fractions; scratch of the packing
    const long long n_alloc = lr_groups_alloc(cfg->n_lineages);
    out->lineage_idx = o, o += lr_align_up64(n_alloc * 16, 256);
    out->lineage_frac = o;
    if (p.unit == LR_TAB_PAIRGEN) o += lr_align_up64(n_alloc * 16 * LR_FRAC_ARRAYS, 256);
    out->pack_tmp = o, o += lr_align_up64(lr_pack_tmp_bytes(cfg->n_lineages), 256);
    out->args_blob = o, o += 1024;   // lr_step_args of the persistent kernel
    out->tables = o, o += table_bytes;
    out->partials = o, o += lr_align_up64((long long)lr_tile_stride(p.tiles) * C * 8, 256);
    out->trace = o, o += lr_align_up64((long long)cfg->n_trace_slots * C * LR_TRACE_W * 8, 256);
    out->status = o, o += 256;   // engine status word
    // team exchange granules of the speculative kernel: [2 parities][pairs][LR_TEAM_MAX][LR_SPEC_GRANULES] x 8 bytes
    // (four-chain kernel: the scan sums a launch leaves for the next one, LR_P4_CARRY_BYTES per block - lr_persist4_kernel)
    // (streaming engine: the counters of a launch and the second table buffer)
    out->xchg = o, o += (plan->team_blocks > 1) ? lr_align_up64(2ll * C * LR_TEAM_MAX * LR_SPEC_GRANULES * 8, 256)   // (room for a team per chain)
                                               : (plan->family == 2 ? lr_align_up64((C + 3) / 4 * LR_P4_CARRY_BYTES, 256)
                                                  : (plan->streaming ? LR_STREAM_SYNC_BYTES + table_bytes : 0));
    out->total_bytes = o;
    out->table_stride = p.tab_stride;
    out->tiles = p.tiles;
    out->chains_per_block = p.cb;
    out->trace_width = LR_TRACE_W;
    out->n_parts = plan->n_parts;
    out->pipelined = plan->pipelined[0] ? 1 : 0;
    out->persistent = plan->family;
    out->reserved1 = plan->threads;
    out->team_blocks = plan->team_blocks;
    out->spec_chains_per_team = plan->team_cpb;
    out->table_mode = p.unit;
    out->streaming = plan->streaming ? 1 : 0;
    out->packed_scan = plan->packed_scan ? 1 : 0;
    out->reserved3 = 0;
    return LR_OK;
}
