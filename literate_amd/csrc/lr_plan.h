// lr_plan.h - the engine planner (lr_plan.hip): which kernel an RJMCMC engine runs, on which tables, in how many partitions
// and with how many threads per block, decided ONCE per configuration as one lr_engine_plan.  lr_mcmc_query_layout turns
// the plan into workspace offsets; lr_mcmc_create stores it in the engine, and everything that launches reads it there.
// Host only; the constants below are the ones the planner and the layout share with the kernels' translation units.
#pragma once
#include "lr_internal.h"
#include "lr_scan.h"

#define LR_MAX_PARTS 4

// spare zero-filled 16-byte groups behind the packed lineages (group 0 bytes = sentinel table entries, contribution 0):
// room for the trips the four-chain kernel moves between waves and for its prefetch past the end
#define LR_P4_MAX_GIVE 64
// sized for the widest stride (16 scanner waves x 64 lanes): the takers' extra trips reach group (k_tot + give) * stride
#define LR_IDX_SPARE ((LR_P4_MAX_GIVE + 2) * 1024)
// the packing keeps the caller's order and starts a new group wherever the birth bin changes: lineages sorted by birth
// time give at most n_bins + 2 such runs; more than LR_MAX_RUNS of them (unsorted input) are refused
#define LR_MAX_RUNS (1ll << 20)

static inline long long lr_groups_alloc(long long n_lineages) {
    const long long runs = n_lineages < LR_MAX_RUNS ? n_lineages : LR_MAX_RUNS;
    // (unit resolution: LR_SLOTS slots of one or two lineages per group - all singles in the worst case)
    return (n_lineages + LR_SLOTS - 1) / LR_SLOTS + runs + LR_IDX_SPARE;
}

// four-chain kernel: bytes per block of the sums a launch leaves for the next ([16 waves][2] doubles + a valid word)
#define LR_P4_CARRY_BYTES 512

// widest table class of the persistent kernels (the launch-based scans are instantiated up to H = 264)
#define LR_H_WIDE 520

// ---- speculative team engine (lr_spec.h / lr_spec.hip) ----
#ifndef LR_SPEC_THREADS
#define LR_SPEC_THREADS 768   /* a team per pair: 12 waves = 4 candidate + 8 scanner waves, 3 per SIMD = 168 VGPRs each */
#endif
#ifndef LR_SPEC_THREADS_SINGLE
#define LR_SPEC_THREADS_SINGLE 768    /* a team per chain: 12 waves = 2 candidate + 2 helper + 8 scanner waves.  (1024 threads = 12
                                         scanner waves fit without spills - with the table build on the helper waves no role needs
                                         more than ~105 VGPRs - and take 5 % off a 100k-lineage scan on one CU, but every team
                                         exchange and every short scan got 3-8 % slower: measured round 3, not used) */
#endif
#define LR_TEAM_MAX 8
#define LR_SPEC_GRANULES 16      /* 8-byte granules reserved per block and parity: one 128-byte line */

// ---- resident streaming engine (lr_stream.hip) ----
// counters of one launch, in the workspace at lr_mcmc_layout.xchg, each on a cache line of its own (lr_stream_sync,
// lr_engine.h); the second table buffer follows LR_STREAM_SYNC_BYTES behind
#define LR_STREAM_COPIES 64
#define LR_STREAM_SYNC_BYTES (128 + LR_STREAM_COPIES * 128 + 128)

// What runs a configuration.  Filled in one pass by lr_plan_engine; nothing else decides any of it.
struct lr_engine_plan {
    lr_scan_plan scan;        // table class and launch shape
    int family;               // 0: the launch-based engine; 1 = two chains per block (lr_persist_kernel), 2 = four chains per
                              // 1024-thread block (lr_persist4_kernel), 3 = the speculative team kernel (lr_mcmc_layout.persistent)
    int team_blocks;          // family 3: blocks per team ...
    int team_cpb;             // ... and chains per team (1 or 2)
    int threads;              // threads per persistent block, 0 for family 0 (lr_mcmc_layout.reserved1)
    bool packed_scan;         // family 0 and its scan reads the PACKED lineages (lr_packscan.hip) instead of ts / te
    int packed_mode;          // lr_packed_mode of the tables: 0 = no packed scan planned on them, 1 = one partition, 2 = partitions
    bool streaming;           // family 0 and the resident streaming kernel is wanted (lr_mcmc_create asks the device whether it fits)
    bool pair_only;           // the tables are a pair class of their own - pair-general, the extant block of model 3, H = 520 -:
                              // only lr_pairscan_kernel and the packed scan read them, the scans of ts / te cannot
    int n_parts;              // partitions of the chains (lr_partition): [base[p], base[p + 1]), first half hA[p] chains
    int base[LR_MAX_PARTS + 1], hA[LR_MAX_PARTS];
    bool pipelined[LR_MAX_PARTS];
};

// the plan of a configuration lr_check_cfg has passed; LR_OK or the error of lr_plan_scan
int lr_plan_engine(const lr_mcmc_config* cfg, lr_engine_plan* plan);
// lr_mcmc_query_layout: check the configuration, plan it, turn the plan into workspace offsets
int lr_plan_layout(const lr_mcmc_config* cfg, lr_engine_plan* plan, lr_mcmc_layout* out);

// what the planner asks the engines' translation units
// lr_stream.hip
bool lr_stream_eligible(const lr_mcmc_config* cfg, const lr_scan_plan& p);
void lr_stream_plan(const lr_mcmc_config* cfg, lr_scan_plan* p, int cus);
// lr_packscan.hip
bool lr_packscan_eligible(const lr_mcmc_config* cfg, const lr_scan_plan& p);
void lr_packscan_plan(const lr_mcmc_config* cfg, lr_scan_plan* p, int cus);
// lr_pack.hip
long long lr_pack_tmp_bytes(long long n_lineages);
