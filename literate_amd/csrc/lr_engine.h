// lr_engine.h - host-side engine object shared by the translation units of the RJMCMC engines
// (lr_mcmc.hip: launch-based and two- / four-chain persistent kernels, lr_spec.hip: speculative team kernel,
// lr_pack.hip: packing of the lineages for the persistent scans).  What an engine runs is decided by the planner
// (lr_plan.h / lr_plan.hip) and kept in lr_engine.plan.
#pragma once
#include <cmath>
#include "lr_internal.h"
#include "lr_plan.h"
#include "lr_scan.h"
#include "lr_step.h"

// a partition = a contiguous, independent block of chains with its own stream and captured graph; inside it
// the chains are software-pipelined in two halves (A = [base, base+hA), B = the rest)
struct lr_part {
    int base, count, hA;
    bool pipelined;
    hipStream_t stream;
    hipEvent_t done;
    hipGraphExec_t graph_exec;
    int graph_units;
};

// Four-chain kernel: delta[s] = trips scanner slot s (wave s + 2) scores beyond (+) or short of (-) the equal share
// k_tot; the deltas sum to zero.  The trips given up are stored, in slot / trip order, behind the takers' own shares.
struct lr_p4_shares {
    int delta[16];
    int n_slots;          // scanner waves striding over the groups: 14 (four-chain kernel; 12 with helper waves) or 8 (two-chain kernel)
    int help_trips;       // four-chain kernel with helper waves: trips of the scan each helper wave makes before its hand-over arrives
};

struct lr_engine {
    lr_mcmc_config cfg;
    lr_mcmc_layout lay;
    lr_engine_plan plan;      // what runs, as lr_plan_engine decided it for cfg (lr_mcmc_create plans once, through lr_plan_layout)
    const double* ts;
    const double* te;
    const double* br_length;
    char* ws;
    bool initialised;
    lr_part part[LR_MAX_PARTS];   // the plan's partitions with their streams and graphs: launch-based engines only (plan.family == 0)
    long long n8;             // 16-byte groups of packed lineage indices
    long long n8_alloc;       // ... allocated (zero-filled behind the data)
    lr_p4_shares p4;          // per scanner wave: trips more (+) or fewer (-) than the equal share (four-chain kernel)
    bool p4_help;             // four-chain kernel: the form with helper waves - latched by lr_set_shares (init / restore), so
                              // that the form, its shares and the sums carried between launches belong together for a whole run
    int p4_cfg;               // ... and its configuration word (LR_P4_CFG_*, lr_p4_cfg_choice), latched with p4_help
    bool p4_resident;         // ... and whether its scanning lanes keep decoded groups in registers (lr_p4_resident_choice), latched with p4_help
    bool p4_pipe;             // ... and whether a wave's full set of resident trips runs as one block (lr_p4_pipe_choice), latched with p4_help
    bool p4_lean;             // ... and whether waves 4, 5 run the lean draw duty (lr_p4_lean_choice), latched with p4_help
    bool packed_scan;         // launch-based engine whose scan kernel reads the PACKED lineages (lr_packscan.hip) instead of ts / te:
                              // planned (plan.packed_scan), dropped by init / restore if the packing
                              // refuses the input (unsorted beyond LR_MAX_RUNS runs)
    bool streaming;           // launch-based plan, but the iterations run inside ONE resident kernel (lr_stream.hip): wanted by the
                              // plan (plan.streaming), latched by lr_mcmc_create, which asks the device in use whether the whole grid fits it at once
    hipEvent_t fork;
    hipEvent_t ev0, ev1;      // timing events of lr_mcmc_time_steps / lr_mcmc_time_scan, created once
};


// ---- speculative team engine (lr_spec.h / lr_spec.hip) ----
#ifndef LR_SPEC_SCAN_UNROLL
#define LR_SPEC_SCAN_UNROLL 1
#endif
#ifndef LR_SPEC_SCAN_PRIO
#define LR_SPEC_SCAN_PRIO 2   /* s_setprio of the scanner waves of a team (0 = leave the default) */
#endif
#define LR_SPEC_TIMEOUT_TICKS 200000000ull   /* 2 s of the 100 MHz wall clock */

// Four-chain kernel: helper waves (lr_persist4_kernel's HELP) under the RJ sampler at unit resolution; LR_P4_HELP = 0: the
// form with fourteen scanner waves (A/B runs).  Evaluated ONLY by lr_set_shares, i.e. at lr_mcmc_init / lr_mcmc_restore
// (a test process that runs both forms re-initialises between them); everything else reads e->p4_help.
static inline bool lr_p4_help_choice(const lr_engine* e) {
    const char* env = getenv("LR_P4_HELP");
    if (e->lay.persistent != 2 || e->plan.scan.unit == LR_TAB_PAIRGEN || e->cfg.sampler != 0 || e->plan.scan.H > 264) return false;
    return env ? atoi(env) != 0 : true;
}

// Four-chain kernel with helper waves: the configuration word of the instantiation an engine runs (LR_P4_CFG_*, lr_step.h).
// A specialised word needs the default switches - const_rates == 0, use_rate_HP != 0, poisson_HP == 0, in-bin fractions
// (+0.0, 0.5) - and model 0, 1 (LR_P4_CFG_BDI) or 2 (LR_P4_CFG_KEIDING); model 3 and every other setting run the generic
// instantiation, and LR_P4_GENERIC = 1 forces it (A/B runs, the bit-equality test).  Evaluated where lr_p4_help_choice is.
static inline int lr_p4_cfg_choice(const lr_engine* e) {
    const char* env = getenv("LR_P4_GENERIC");
    if (!lr_p4_help_choice(e) || (env && atoi(env) != 0)) return LR_P4_CFG_GENERIC;
    const lr_mcmc_config& c = e->cfg;
    if (c.const_rates != 0 || c.use_rate_HP == 0 || c.poisson_HP != 0.0) return LR_P4_CFG_GENERIC;
    if (c.frac_birth != LR_P4_FRAC_BIRTH || std::signbit(c.frac_birth) || c.frac_death != LR_P4_FRAC_DEATH) return LR_P4_CFG_GENERIC;
    if (c.model == LR_MODEL_BD || c.model == LR_MODEL_ID) return LR_P4_CFG_BDI;
    return c.model == LR_MODEL_KEIDING ? LR_P4_CFG_KEIDING : LR_P4_CFG_GENERIC;
}

// Four-chain kernel with helper waves: the scanning lanes keep the decoded groups of their first trips in registers for a
// whole launch (lr_persist4_kernel's NR, lr_resident_groups in lr_scan.h); LR_P4_RESIDENT = 0: every trip goes through the
// scan loop (A/B runs, the bit-equality test).  Evaluated where lr_p4_help_choice is.
static inline bool lr_p4_resident_choice(const lr_engine* e) {
    const char* env = getenv("LR_P4_RESIDENT");
    return lr_p4_help_choice(e) && !(env && atoi(env) == 0);
}

// ... and a wave that runs all its resident trips takes them as one basic block, without the test and branch per trip
// (lr_persist4_kernel's PIPE, lr_resident_trips_block in lr_scan.h); LR_P4_PIPE = 0: trip by trip on every wave (A/B runs,
// the bit-equality test).  Evaluated where lr_p4_help_choice is.
static inline bool lr_p4_pipe_choice(const lr_engine* e) {
    const char* env = getenv("LR_P4_PIPE");
    return lr_p4_resident_choice(e) && !(env && atoi(env) == 0);
}

// ... and the draw duty of its waves 4, 5 is the lean one (lr_persist4_kernel's LEAN, lr_spec_draw_lean in lr_step.h);
// LR_P4_LEAN_DRAWS = 0: lr_spec_draw_both, the kernel without LEAN (A/B runs, the bit-equality test).  Evaluated where
// lr_p4_help_choice is.
static inline bool lr_p4_lean_choice(const lr_engine* e) {
    const char* env = getenv("LR_P4_LEAN_DRAWS");
    return lr_p4_pipe_choice(e) && !(env && atoi(env) == 0);
}

// Which instantiation of the speculative kernel an engine runs (lr_spec.h): 0 = a team per pair; a team per chain: 1 = in
// a team of several blocks, 2 = on its own CU with the pair planes of a candidate's table derived by the scanner waves for
// the ONE table that becomes pending (short scans - at most 3 trips per scanner lane -: the helper waves' build is the
// longer path of an iteration), 3 = on its own CU with the planes derived by the helper wave that builds the table (long
// scans: the scan is).  LR_SPEC_PLANES_BY_SCANNERS = 0 / 1 overrides the rule between 2 and 3.
static inline int lr_spec_mode(const lr_engine* e) {
    if (e->lay.spec_chains_per_team != 1) return 0;
    if (e->lay.team_blocks > 1) return 1;
    const double trips = (double)e->n8 / 64.0 / 8.0;
    const char* env = getenv("LR_SPEC_PLANES_BY_SCANNERS");
    const bool by_scanners = env ? atoi(env) != 0 : trips <= 3.0;
    return by_scanners ? 2 : 3;
}

// ---- resident streaming engine (lr_stream.hip) ----
#define LR_STEP_WAVES_PER_BLOCK (LR_SCAN_THREADS / LR_WAVE)
// counters of one launch, in the workspace at lr_mcmc_layout.xchg, each on a cache line of its own (LR_STREAM_COPIES,
// LR_STREAM_SYNC_BYTES: lr_plan.h)
#define LR_STREAM_MAX_CHAINS 16
struct lr_stream_sync {
    unsigned long long arrived;      // scanner blocks that have stored their tile's partial sums, over the launch's iterations
    unsigned long long pad0[15];
    // what the stepper wave of chain c has published, LR_STREAM_COPIES times - one 128-byte line per copy holds all chains'
    // words, and scanner block b polls copy b % LR_STREAM_COPIES (a thousand blocks polling ONE line kept the memory channel
    // that holds it so busy that the blocks still streaming took twice as long):
    //   bits 40-63  early: iterations whose early table stands (the step taken ahead)
    //   bits 16-39  ready: iterations decided - the next iteration's table is final
    //   bits  0-15  changed: +1 before and +1 behind every table written AGAIN (an accepted proposal); a scanner block
    //               that staged the early tables stages again if this moved since
    unsigned long long word[LR_STREAM_COPIES][LR_STREAM_MAX_CHAINS];
};
static_assert(sizeof(lr_stream_sync) + 128 == LR_STREAM_SYNC_BYTES && LR_STREAM_SYNC_BYTES % 256 == 0, "counter line + a line per copy");
// n_iters iterations in launches of at most 4096; query = true only asks whether the grid fits the current device at once
int lr_launch_stream(lr_engine* e, const lr_step_args& a, int64_t n_iters, bool query, hipStream_t stream);

// ---- packed scan of the launch-based engine (lr_packscan.hip) ----
int lr_packscan_pairs(const lr_scan_plan& p, int n_chains);
int lr_launch_packscan(const lr_engine* e, int base, int count, hipStream_t stream);

// lr_mcmc.hip
lr_step_args lr_make_args(const lr_engine* e);
// lr_pack.hip: (re)builds the packed lineages in the workspace and the scanner-wave shares; blocks on `stream` once
int lr_pack_lineages(lr_engine* e, hipStream_t stream);
// lr_spec.hip: n_iters iterations of the speculative team kernel
int lr_launch_spec(lr_engine* e, const lr_step_args& a, const lr_packed_lineages& pk, int64_t n_iters, hipStream_t stream);
