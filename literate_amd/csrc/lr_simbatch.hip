// lr_simbatch.hip - many independent runs of lr_sim.hip's discrete-time birth-death scheme in ONE launch.
//
// Replicate r is, by definition, lr_simulate_bd(mode 0) with seed + r and the per-step probabilities
// lam_bins[r, t / steps_per_bin] / steps_per_bin: the same draws at the same addresses (Philox key ((uint32) (seed + r),
// lineage slot), counter (step, 24, 0)), the same thresholds (one fp64 division, lt and lt + mt), so every count it
// reports equals what that run's (ts, te, alive_trace) give.  Nothing per lineage is written out.
//
// One workgroup works on one replicate at a time and takes the next from an integer ticket; workgroups never wait on
// one another.  The state of a replicate is the list of living slot numbers (4 bytes each) and a handful of counters
// that every thread carries as the same value.  Per step the block walks the list in chunks of THREADS * ITEMS
// positions: every thread draws for its positions, one block scan (wave DPP scan + eight wave totals in LDS, one
// barrier) gives the survivors their offsets, and they are written back IN PLACE - the write cursor never passes the
// chunk that was just read, so the list needs no second copy.  The newborns of a step take the next unused slot
// numbers, a contiguous range, which is appended behind the survivors once the walk is over (which newborn gets which
// number does not matter, see lr_sim.hip).  Position p of the list lives in LDS while p < lds_slots and in the
// workgroup's slice of the workspace beyond: a list that outgrows LDS in mid-run just continues there, and the
// result does not depend on where a position lived.  Per-bin counters are registers, stored once per bin by one
// thread with ordinary stores.  No floating-point atomics; the only atomic is the integer ticket.
//
// Where the two thresholds of a step come from is a parameter of the walk (SRC below), and there are two sources.
// lr_sb_fixed (lr_simulate_bd_batch): per-bin rates given before the launch, one division per bin.  lr_sb_dd
// (lr_simulate_dd_batch): DDRate's diversity-dependent rates, recomputed at EVERY step from the count n_t living at its
// start by lr_dd_bin_rates of lr_dd.h - the function the engine and lr_dd_rates use, with n_t in the place of DT[b].  The
// model's DT[b] is the lineage-time lived in bin b, which is not known until the bin is over; the reference's own
// simulators (simulateRateABC.v2.py:142-166, notebook 4's Diversity_Dependence_Rate_Generator) feed back the count living
// at the step, and so does this one.  n_t is the same value in every thread, so every thread evaluates the map itself
// (one lr_log, two exp per step): nothing is broadcast, and the parameters of the replicate sit in scalar registers.
#include <hip/hip_runtime.h>

#include "../../include/literate_hip.h"
#include "lr_device.h"
#include "lr_dd.h"

#define LR_P_SIM 24
#define LR_SB_THREADS 512
#define LR_SB_WAVES (LR_SB_THREADS / LR_WAVE)
#define LR_SB_ITEMS 4
#define LR_SB_CHUNK (LR_SB_THREADS * LR_SB_ITEMS)
#define LR_SB_HEAD 256                      // bytes at the head of the workspace: the ticket
#define LR_SB_MAX_CAPACITY 2147483647ll

// list positions held in LDS for this capacity (host and device agree on it through the launch argument)
static inline long long lr_sb_lds_slots(long long capacity) {
    return capacity < LR_SIMBATCH_LDS_SLOTS ? capacity : (long long)LR_SIMBATCH_LDS_SLOTS;
}
// slots of one workgroup's slice of the workspace: the positions beyond LDS, padded to 64 slots (256 bytes)
static inline long long lr_sb_slice_slots(long long capacity) {
    const long long over = capacity - lr_sb_lds_slots(capacity);
    return (over + 63) / 64 * 64;
}

// The threshold sources.  A source makes a per-replicate object with bin(b, spb), called by every thread when bin b
// begins, and step(n, spb, &lt, &ltmt), called at every step with the living count: the birth threshold lt and the
// death threshold lt + mt.
struct lr_sb_fixed {
    const double* lam_bins;
    const double* mu_bins;
    struct rep {
        const double* lam;
        const double* mu;
        double lt, ltmt;
        __device__ __forceinline__ void bin(int b, int spb) {
            lt = lam[b] / (double)spb;
            const double mt = mu[b] / (double)spb;
            ltmt = lt + mt;
        }
        __device__ __forceinline__ void step(long long, int, double* lt_, double* ltmt_) const { *lt_ = lt, *ltmt_ = ltmt; }
    };
    __device__ __forceinline__ rep replicate(int r, int nb) const {
        return rep{lam_bins + (long long)r * nb, mu_bins + (long long)r * nb, 0.0, 0.0};
    }
};

struct lr_sb_dd {
    const double* params;                   // [n_reps, LR_DD_NPAR]
    const double* x_bins;                   // [n_reps, n_bins]
    int m_birth, m_death;
    struct rep {
        lr_dd_params p;
        const double* xs;
        double x;
        int m_birth, m_death;
        __device__ __forceinline__ void bin(int b, int) { x = xs[b]; }
        __device__ __forceinline__ void step(long long n, int spb, double* lt_, double* ltmt_) const {
            double br, dr, niche, frac;
            lr_dd_bin_rates(p, x, (double)n, m_birth, m_death, &br, &dr, &niche, &frac);
            const double lt = br / (double)spb, mt = dr / (double)spb;
            *lt_ = lt, *ltmt_ = lt + mt;
        }
    };
    __device__ __forceinline__ rep replicate(int r, int nb) const {
        // r is the same in every thread of the block: say so, and the eight parameters are scalar loads
        const int ru = __builtin_amdgcn_readfirstlane(r);
        const double* a = params + (long long)ru * LR_DD_NPAR;
        rep q;
        q.p.l_max = a[0], q.p.k = a[1], q.p.x0 = a[2], q.p.div_0 = a[3];
        q.p.L = a[4], q.p.m_max = a[5], q.p.nuB = a[6], q.p.nuD = a[7];
        q.xs = x_bins + (long long)ru * nb, q.x = 0.0;
        q.m_birth = m_birth, q.m_death = m_death;
        return q;
    }
};

// the kernel argument: the threshold source first, then what every source shares
template <class SRC>
struct lr_sb_args {
    SRC src;
    const long long* n_start;
    long long* counts;
    long long* totals;
    unsigned int* ticket;
    unsigned int* slices;
    long long slice_slots;
    long long capacity;
    unsigned long long seed;
    int n_reps, n_bins, steps_per_bin, lds_slots;
};

__device__ __forceinline__ unsigned int lr_sb_get(const unsigned int* s_list, const unsigned int* g_list, int L, long long p) {
    return p < L ? s_list[p] : g_list[p - L];
}
__device__ __forceinline__ void lr_sb_put(unsigned int* s_list, unsigned int* g_list, int L, long long p, unsigned int v) {
    if (p < L) s_list[p] = v;
    else g_list[p - L] = v;
}

// One replicate.  n, created and the per-bin sums hold the same value in every thread (they come from block totals).
template <class SRC>
__device__ void lr_sb_run(const lr_sb_args<SRC>& a, int r, unsigned int* s_list, unsigned int* g_list, int (*s_wtot)[LR_SB_WAVES],
                          int& parity) {
    const int tid = threadIdx.x, lane = tid & (LR_WAVE - 1), wave = tid / LR_WAVE;
    const int L = a.lds_slots, nb = a.n_bins, spb = a.steps_per_bin;
    const long long n0 = a.n_start[r];
    long long* tot = a.totals + 4ll * r;
    if (n0 < 1 || n0 > a.capacity) {
        if (tid == 0) tot[0] = 0, tot[1] = 0, tot[2] = 1, tot[3] = -1;
        return;
    }
    for (long long p = tid; p < n0; p += LR_SB_THREADS) lr_sb_put(s_list, g_list, L, p, (unsigned int)p);
    __syncthreads();
    const uint32_t key = (uint32_t)(a.seed + (unsigned long long)r);
    typename SRC::rep rates = a.src.replicate(r, nb);
    long long* cnt = a.counts + 4ll * r * nb;
    long long n = n0, created = n0, first_empty = -1;
    int overflow = 0;
    for (int b = 0; b < nb && !overflow; ++b) {
        if (n == 0) {                       // extinct: the remaining bins keep the zeros the host wrote
            if (first_empty < 0) first_empty = (long long)b * spb;
            break;
        }
        rates.bin(b, spb);
        const long long at_start = n;
        long long births_b = 0, deaths_b = 0, steps_b = 0;
        for (int s = 0; s < spb; ++s) {
            const long long t = (long long)b * spb + s;
            if (n == 0) {
                if (first_empty < 0) first_empty = t;
                break;
            }
            double lt, ltmt;                // the thresholds of this step
            rates.step(n, spb, &lt, &ltmt);
            steps_b += n;
            long long w = 0;                // survivors written so far
            int born = 0;                   // births of this step
            for (long long base = 0; base < n; base += LR_SB_CHUNK) {
                unsigned int slot[LR_SB_ITEMS];
                int keep = 0, nbirth = 0;   // keep: bit k set = item k survives
#pragma unroll
                for (int k = 0; k < LR_SB_ITEMS; ++k) {
                    const long long p = base + (long long)k * LR_SB_THREADS + tid;
                    slot[k] = 0u;
                    if (p < n) {
                        slot[k] = lr_sb_get(s_list, g_list, L, p);
                        const lr_stream rng{key, slot[k]};
                        const double u = lr_pair(rng, (uint64_t)t, LR_P_SIM, 0).a;
                        if (u < lt) nbirth += 1, keep |= 1 << k;
                        else if (!(u < ltmt)) keep |= 1 << k;
                    }
                }
                // block scan of (survivors | births << 16): a chunk holds at most 2048 of either
                const int v = __popc(keep) | (nbirth << 16);
                const int excl = lr_wave_exclusive_scan_i32(v);
                const int wtot = __builtin_amdgcn_readlane(excl + v, LR_WAVE - 1);
                if (lane == 0) s_wtot[parity][wave] = wtot;
                __syncthreads();            // also: every read of this chunk is done before any write below
                int before = 0, total = 0;
#pragma unroll
                for (int q = 0; q < LR_SB_WAVES; ++q) {
                    const int x = s_wtot[parity][q];
                    if (q < wave) before += x;
                    total += x;
                }
                parity ^= 1;                // the next scan writes the other row: no second barrier per chunk
                long long dst = w + ((before + excl) & 0xffff);
#pragma unroll
                for (int k = 0; k < LR_SB_ITEMS; ++k)
                    if (keep >> k & 1) lr_sb_put(s_list, g_list, L, dst++, slot[k]);
                w += total & 0xffff, born += total >> 16;
            }
            if (created + born > a.capacity) {
                overflow = 1;
                break;
            }
            // the newborn range goes behind the survivors: positions the walk did not write, and every read of
            // the walk lies before its last barrier
            for (int i = tid; i < born; i += LR_SB_THREADS) lr_sb_put(s_list, g_list, L, w + i, (unsigned int)(created + i));
            __syncthreads();
            births_b += born, deaths_b += n - w;
            n = w + born, created += born;
        }
        if (overflow) break;
        if (tid == 0) cnt[b] = births_b, cnt[nb + b] = deaths_b, cnt[2ll * nb + b] = at_start, cnt[3ll * nb + b] = steps_b;
    }
    if (tid == 0) tot[0] = created, tot[1] = overflow ? 0 : n, tot[2] = overflow, tot[3] = first_empty;
}

template <class SRC>
__device__ __forceinline__ void lr_sb_block(const lr_sb_args<SRC>& a) {
    extern __shared__ unsigned int s_list[];
    __shared__ int s_wtot[2][LR_SB_WAVES];
    __shared__ int s_next;
    unsigned int* g_list = a.slices + (long long)blockIdx.x * a.slice_slots;
    int parity = 0;
    int r = blockIdx.x;
    while (r < a.n_reps) {
        lr_sb_run(a, r, s_list, g_list, s_wtot, parity);
        __syncthreads();                    // the list and s_next are free again
        if (threadIdx.x == 0) {
            // (a ticket beyond n_reps ends the block; 2^32 tickets cannot be reached, n_reps is 32-bit)
            const unsigned int k = atomicAdd(a.ticket, 1u);
            const long long next = (long long)gridDim.x + k;
            s_next = next < a.n_reps ? (int)next : a.n_reps;
        }
        __syncthreads();
        r = s_next;
    }
}

__global__ __launch_bounds__(LR_SB_THREADS) void lr_simbatch_kernel(lr_sb_args<lr_sb_fixed> a) { lr_sb_block(a); }
__global__ __launch_bounds__(LR_SB_THREADS) void lr_simbatch_dd_kernel(lr_sb_args<lr_sb_dd> a) { lr_sb_block(a); }

static int lr_sb_check_sizes(int32_t n_reps, int32_t n_bins, int32_t steps_per_bin, int64_t capacity) {
    if (n_reps < 1 || n_bins < 1 || steps_per_bin < 1 || n_bins > LR_MAX_BINS) return LR_ERR_SIZE;
    if (capacity < 1 || capacity > LR_SB_MAX_CAPACITY) return LR_ERR_SIZE;
    if ((int64_t)n_bins * steps_per_bin > 2147483647ll) return LR_ERR_SIZE;      // the step is a 32-bit counter word
    return LR_OK;
}

extern "C" int64_t lr_simulate_bd_batch_workspace_bytes(int32_t n_reps, int32_t n_bins, int32_t steps_per_bin,
                                                        int64_t capacity) {
    const int rc = lr_sb_check_sizes(n_reps, n_bins, steps_per_bin, capacity);
    if (rc != LR_OK) return rc;
    const int64_t groups = n_reps < LR_SIMBATCH_GROUPS ? n_reps : LR_SIMBATCH_GROUPS;
    return LR_SB_HEAD + groups * lr_sb_slice_slots(capacity) * 4;
}

// the checks that do not depend on the threshold source, then the two memsets and the launch
template <class SRC, class KERNEL>
static int lr_sb_launch(KERNEL kernel, const SRC& src, int32_t n_reps, int32_t n_bins, int32_t steps_per_bin,
                        const int64_t* n_start, int64_t capacity, uint64_t seed, int64_t* counts, int64_t* totals,
                        void* workspace, int64_t workspace_bytes, void* stream_) {
    if (workspace_bytes < lr_simulate_bd_batch_workspace_bytes(n_reps, n_bins, steps_per_bin, capacity))
        return LR_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    lr_sb_args<SRC> a;
    a.src = src;
    a.n_start = (const long long*)n_start;
    a.counts = (long long*)counts, a.totals = (long long*)totals;
    a.ticket = (unsigned int*)workspace;
    a.slices = (unsigned int*)((char*)workspace + LR_SB_HEAD);
    a.slice_slots = lr_sb_slice_slots(capacity);
    a.capacity = capacity, a.seed = seed;
    a.n_reps = n_reps, a.n_bins = n_bins, a.steps_per_bin = steps_per_bin, a.lds_slots = (int)lr_sb_lds_slots(capacity);
    hipError_t e = hipMemsetAsync(workspace, 0, LR_SB_HEAD, stream);
    if (e != hipSuccess) return (int)e;
    // bins a replicate does not reach (extinct, overflowed, refused start) read zero
    e = hipMemsetAsync(counts, 0, (size_t)n_reps * 4 * n_bins * sizeof(int64_t), stream);
    if (e != hipSuccess) return (int)e;
    // (LR_SIMBATCH_LDS_SLOTS * 4 = 64 KiB: two workgroups per CU, and no attribute to raise)
    const size_t lds_bytes = (size_t)a.lds_slots * 4;
    const int groups = n_reps < LR_SIMBATCH_GROUPS ? n_reps : LR_SIMBATCH_GROUPS;
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(LR_SB_THREADS), lds_bytes, stream, a);
    return (int)hipGetLastError();
}

extern "C" int lr_simulate_bd_batch(const double* lam_bins, const double* mu_bins, int32_t n_reps, int32_t n_bins,
                                    int32_t steps_per_bin, const int64_t* n_start, int64_t capacity, uint64_t seed,
                                    int64_t* counts, int64_t* totals, void* workspace, int64_t workspace_bytes,
                                    void* stream_) {
    if (!lam_bins || !mu_bins || !n_start || !counts || !totals || !workspace) return LR_ERR_NULL;
    const int rc = lr_sb_check_sizes(n_reps, n_bins, steps_per_bin, capacity);
    if (rc != LR_OK) return rc;
    return lr_sb_launch(lr_simbatch_kernel, lr_sb_fixed{lam_bins, mu_bins}, n_reps, n_bins, steps_per_bin, n_start, capacity,
                        seed, counts, totals, workspace, workspace_bytes, stream_);
}

extern "C" int64_t lr_simulate_dd_batch_workspace_bytes(int32_t n_reps, int32_t n_bins, int32_t steps_per_bin,
                                                        int64_t capacity) {
    return lr_simulate_bd_batch_workspace_bytes(n_reps, n_bins, steps_per_bin, capacity);
}

extern "C" int lr_simulate_dd_batch(const double* params, const double* x_bins, int32_t m_birth, int32_t m_death,
                                    int32_t n_reps, int32_t n_bins, int32_t steps_per_bin, const int64_t* n_start,
                                    int64_t capacity, uint64_t seed, int64_t* counts, int64_t* totals, void* workspace,
                                    int64_t workspace_bytes, void* stream_) {
    if (!params || !x_bins || !n_start || !counts || !totals || !workspace) return LR_ERR_NULL;
    const int rc = lr_sb_check_sizes(n_reps, n_bins, steps_per_bin, capacity);
    if (rc != LR_OK) return rc;
    if (m_birth < 0 || m_birth > 2 || m_death < -2 || m_death > 2) return LR_ERR_MODEL;      // lr_curve_setup's ranges
    return lr_sb_launch(lr_simbatch_dd_kernel, lr_sb_dd{params, x_bins, m_birth, m_death}, n_reps, n_bins, steps_per_bin,
                        n_start, capacity, seed, counts, totals, workspace, workspace_bytes, stream_);
}
