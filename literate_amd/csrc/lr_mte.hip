// lr_mte.hip - the multi-trait extinction model (include/literate_hip_mte.h): MTEmodel.py's Metropolis-Hastings loop with
// Bayesian variable selection over several categorical traits, for chains on many problems (time slices of one data set)
// that share one table of trait-state combinations - all of them in one launch.
//
//   lr_mte_chain_kernel<CPL>   one wave per chain, four independent waves per workgroup: its initial state, or n_iters
//                              iterations from its state
//
// The likelihood is a function of three statistics per combination, so an iteration costs O(G T) whatever the number of
// lineages: combination g sits in lane g % 64, CPL = 1, 2, 4, 8 or 16 combinations to a lane, and the problem's n, E, B
// and the combination's codes (four bits a trait) stay in registers for the whole launch.  Category k of the concatenated
// traits sits in lane k % 64, two to a lane at most.  The wave's own slice of LDS carries what crosses lanes: exp(Y) (or
// Y^2) for the sums over a trait's states, q for the combinations' T gathers, sd for the prior.  No barrier: a wave never
// waits for another, and a wave's LDS accesses are served in program order.  Every sum is a fixed tree (a trait's states
// in order; a lane's combinations in order, then lr_wave_sum), no floating-point atomics: a chain's bits depend on its own
// arguments alone.
#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/literate_hip_mte.h"
#include "lr_chain.h"             // lr_bcast, LR_MULT_D
#include "lr_internal.h"          // lr_rows_due

#define LR_MTE_THREADS 256
#define LR_MTE_WAVES (LR_MTE_THREADS / LR_WAVE)
#define LR_MTE_HALF_LOG_2PI 0.91893853320467274178
#define LR_MTE_LGAMMA_1_5 (-0.12078223763524522235) /* log Gamma(1.5): the shape of the prior on 1 / sd^2 */
#define LR_MTE_LOG_0_1 (-2.30258509299404568402)    /* log of the rate 0.1 of the prior on beta_hp */
#define LR_MTE_INIT_BETA_BASE 1024u

static_assert(LR_MTE_MAX_CATS == 2 * LR_WAVE && LR_MTE_MAX_COMBOS == 16 * LR_WAVE && LR_MTE_ROW_W == 3 * LR_WAVE, "lane layout");
static_assert(LR_MTE_MAX_STATES <= 16 && LR_MTE_MAX_TRAITS <= 16, "a combination's codes are 16 fields of four bits");
static_assert(5 + 2 * LR_MTE_MAX_TRAITS + LR_MTE_MAX_CATS + 1 <= LR_MTE_ROW_W, "a row holds the largest model");
static_assert(LR_MTE_S_Y + LR_MTE_MAX_CATS == LR_MTE_STATE_W && LR_MTE_S_I + LR_MTE_MAX_TRAITS == LR_MTE_S_SD &&
              LR_MTE_S_SD + LR_MTE_MAX_TRAITS == LR_MTE_S_Y && LR_MTE_S_ACCEPTED + 3 <= LR_MTE_S_I, "state layout");
static_assert(64u * LR_MTE_MAX_TRAITS <= LR_MTE_INIT_BETA_BASE && 2 * LR_GAMMA_MAX_ATTEMPTS <= 64, "Gamma bases 64 apart share no attempt");

struct lr_mte_cfg {
    double log_pI, mult_l, th_y, th_m, th_i;
    long long rows_cap, slot0, chain0, bvs_from;
    int G, T, n_cats, n_chains, chains_per_problem, s_freq, i_init;
    uint32_t seed;
    unsigned char S[LR_MTE_MAX_TRAITS];
};

// a wave's slice of LDS
struct lr_mte_lds {
    double e[LR_MTE_MAX_CATS], q[LR_MTE_MAX_CATS], sd[LR_MTE_MAX_TRAITS];
};

// a lane's categories k = lane + 64 j (their trait, its first category and its number of states; `first`: state 0) and,
// in lane t < T, trait t's first category and number of states
struct lr_mte_cats {
    int t[2], off[2], S[2], myOff, myS;
    bool in[2], first[2];
};

// a lane's combinations g = lane + 64 i in registers, and the problem's totals
template <int CPL>
struct lr_mte_data {
    double n[CPL], E[CPL], B[CPL], N, Etot, Btot;
    unsigned long long codes[CPL];
};

struct lr_mte_chain {
    double Y[2], sd, m, beta, lik, prior, prop_y, prop_m, prop_i, acc_y, acc_m, acc_i;
    unsigned I;
};

// between a wave's writes to its LDS slice and other lanes' reads of them (and back): the accesses of one wave are served
// in program order, so this only keeps the compiler from moving them
__device__ __forceinline__ void lr_mte_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void lr_mte_cats_of(lr_mte_cats& K, const lr_mte_cfg& cfg, int lane) {
    K.myOff = 0, K.myS = 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) K.t[j] = 0, K.off[j] = 0, K.S[j] = 1, K.in[j] = false, K.first[j] = false;
    int off = 0;
    for (int t = 0; t < cfg.T; ++t) {
        const int S = cfg.S[t];
        if (lane == t) K.myOff = off, K.myS = S;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = lane + LR_WAVE * j;
            if (k >= off && k < off + S) K.t[j] = t, K.off[j] = off, K.S[j] = S, K.in[j] = true, K.first[j] = k == off;
        }
        off += S;
    }
}

template <int CPL>
__device__ __forceinline__ void lr_mte_load(lr_mte_data<CPL>& D, const uint8_t* __restrict__ code, const double* __restrict__ n,
                                            const double* __restrict__ E, const double* __restrict__ B, const lr_mte_cfg& cfg, int lane) {
    double sn = 0.0, se = 0.0, sb = 0.0;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int g = lane + LR_WAVE * i;
        const bool in = g < cfg.G;
        D.n[i] = in ? n[g] : 0.0, D.E[i] = in ? E[g] : 0.0, D.B[i] = in ? B[g] : 0.0;
        unsigned long long c = 0ull;
        if (in)
            for (int t = 0; t < cfg.T; ++t)
                c |= (unsigned long long)min((int)code[(size_t)g * cfg.T + t], (int)cfg.S[t] - 1) << (4 * t);
        D.codes[i] = c;
        sn += D.n[i], se += D.E[i], sb += D.B[i];
    }
    D.N = lr_wave_sum(sn), D.Etot = lr_wave_sum(se), D.Btot = lr_wave_sum(sb);
}

// v of the lane's categories -> the wave's e; readers sum their trait's range in ascending order
__device__ __forceinline__ void lr_mte_put(const double (&v)[2], const lr_mte_cats& K, lr_mte_lds& L, int lane) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (K.in[j]) L.e[lane + LR_WAVE * j] = v[j];
    lr_mte_order();
}
__device__ __forceinline__ double lr_mte_range_sum(const lr_mte_lds& L, int off, int S) {
    double a = 0.0;
    for (int x = off; x < off + S; ++x) a += L.e[x];
    return a;
}

// softmax(Y_t) of the lane's categories
__device__ __forceinline__ void lr_mte_softmax(const double (&Y)[2], const lr_mte_cats& K, lr_mte_lds& L, int lane, double (&sm)[2]) {
    double e[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) e[j] = K.in[j] ? exp(Y[j]) : 0.0;
    lr_mte_put(e, K, L, lane);
#pragma unroll
    for (int j = 0; j < 2; ++j) sm[j] = K.in[j] ? e[j] / lr_mte_range_sum(L, K.off[j], K.S[j]) : 0.0;
    lr_mte_order();
}

template <int CPL>
__device__ __forceinline__ double lr_mte_loglik(const double (&Y)[2], unsigned I, double m, const lr_mte_data<CPL>& D,
                                                const lr_mte_cats& K, lr_mte_lds& L, const lr_mte_cfg& cfg, int lane) {
    double sm[2];
    lr_mte_softmax(Y, K, L, lane, sm);
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (K.in[j]) L.q[lane + LR_WAVE * j] = ((I >> K.t[j]) & 1u) ? sm[j] : 1.0 / (double)K.S[j];
    lr_mte_order();
    double w[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) w[i] = 0.0;
    for (int t = 0; t < cfg.T; ++t) {
        const int o = lr_bcast_i(K.myOff, t);
#pragma unroll
        for (int i = 0; i < CPL; ++i) w[i] += L.q[o + (int)((D.codes[i] >> (4 * t)) & 15ull)];
    }
    lr_mte_order();
    double a_n = 0.0, a_b = 0.0, a_e = 0.0;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        a_n += D.n[i] * w[i], a_b += D.B[i] * w[i];
        a_e += D.E[i] != 0.0 ? D.E[i] * lr_log(w[i]) : 0.0;
    }
    a_n = lr_wave_sum(a_n), a_b = lr_wave_sum(a_b), a_e = lr_wave_sum(a_e);
    const double r = m / (a_n / D.N);
    const double lik = D.Etot * lr_log(r) + a_e - r * a_b;
    return lik != lik ? -INFINITY : lik;
}

// sd: lane t < T holds sd_t (the other lanes 1)
__device__ __forceinline__ double lr_mte_prior(const double (&Y)[2], unsigned I, double m, double sd, double beta, const lr_mte_cats& K,
                                               lr_mte_lds& L, const lr_mte_cfg& cfg, int lane) {
    if (lane < cfg.T) L.sd[lane] = sd;
    lr_mte_order();
    const double lx = lr_log(lane < cfg.T ? sd : beta);
    const double lbeta = lr_bcast(lx, LR_WAVE - 1);
    double p = 0.0;
    // Normal(Y; 0, sd_t): the -log sd_t of trait t's S_t states; Gamma(1 / sd_t^2; 1.5, rate beta): (1.5 - 1) log(1 / sd^2) = -log sd
    if (lane < cfg.T) p = -(double)K.myS * lx + (1.5 * lbeta - LR_MTE_LGAMMA_1_5 - lx - beta / (sd * sd));
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (K.in[j]) {
            const double z = Y[j] / L.sd[K.t[j]];
            p += -LR_MTE_HALF_LOG_2PI - 0.5 * z * z;
        }
    lr_mte_order();
    return lr_wave_sum(p) + (LR_MTE_LOG_0_1 - 0.1 * beta) - m + cfg.log_pI * (double)__popc(I);
}

// every sd_t = 1 / sqrt(Gamma(1.5 + S_t / 2) / (rate0 + sum_s Y_t[s]^2 / 2)) -> lane t < T
__device__ __forceinline__ double lr_mte_draw_sd(const double (&Y)[2], double rate0, const lr_mte_cats& K, lr_mte_lds& L,
                                                 const lr_mte_cfg& cfg, const lr_stream& rng, uint64_t it, uint32_t purpose, int lane) {
    const double y2[2] = {Y[0] * Y[0], Y[1] * Y[1]};
    lr_mte_put(y2, K, L, lane);
    double sd = 1.0;
    if (lane < cfg.T) {
        const double a = lr_mte_range_sum(L, K.myOff, K.myS);
        const double tau = lr_gamma(rng, it, purpose, 64u * (uint32_t)lane, 1.5 + 0.5 * (double)K.myS) / (rate0 + 0.5 * a);
        sd = 1.0 / sqrt(tau);
    }
    lr_mte_order();
    return sd;
}

// beta_hp = Gamma(1 + 1.5 T) / (0.1 + sum_t 1 / sd_t^2)
__device__ __forceinline__ double lr_mte_draw_beta(double sd, const lr_mte_cfg& cfg, const lr_stream& rng, uint64_t it, uint32_t purpose,
                                                   uint32_t base, int lane) {
    const double rate = 0.1 + lr_wave_sum(lane < cfg.T ? 1.0 / (sd * sd) : 0.0);
    return lr_gamma(rng, it, purpose, base, 1.0 + 1.5 * (double)cfg.T) / rate;
}

template <int CPL>
__device__ __forceinline__ void lr_mte_iterate(lr_mte_chain& S, const lr_mte_data<CPL>& D, const lr_mte_cats& K, lr_mte_lds& L,
                                               const lr_mte_cfg& cfg, const lr_stream& rng, long long it, int lane) {
    // the wave-uniform draws in one Philox call: lane 0 ACCEPT[0], lane 1 MOVE[0], lane 2 MOVE[1]
    const lr_u2 ud = lr_pair(rng, (uint64_t)it, lane == 0 ? LR_P_MTE_ACCEPT : LR_P_MTE_MOVE, lane == 2 ? 1u : 0u);
    const double log_u = lr_bcast(lr_log(lane == 0 ? ud.a : 1.0), 0);
    const double r = lr_bcast(ud.a, 1), coin = lr_bcast(ud.a, 2), um = lr_bcast(ud.b, 2);
    const int t = min((int)(lr_bcast(ud.b, 1) * (double)cfg.T), cfg.T - 1);
    double Y[2] = {S.Y[0], S.Y[1]}, m = S.m, hasting = 0.0;
    unsigned I = S.I;
    int kind;          // 0 Y, 1 m, 2 indicator, 3 Gibbs
    if (r < cfg.th_y) {
        kind = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t k = (uint32_t)(lane + LR_WAVE * j);
            if (K.in[j] && K.t[j] == t && !K.first[j] && lr_pair(rng, (uint64_t)it, LR_P_MTE_YMASK, k).a < 0.5)
                Y[j] += 0.5 * lr_normal(rng, (uint64_t)it, LR_P_MTE_YNORM, k);
        }
    } else if (r < cfg.th_m) {
        kind = 1;
        hasting = cfg.mult_l * (um - .5);
        m = S.m * exp(hasting);
    } else if (r < cfg.th_i && it >= cfg.bvs_from) {
        kind = 2;
        I ^= 1u << t;
    } else {
        kind = 3;
        if (coin > 0.5) S.beta = lr_mte_draw_beta(S.sd, cfg, rng, (uint64_t)it, LR_P_MTE_GIBBS_BETA, 0u, lane);
        else S.sd = lr_mte_draw_sd(S.Y, S.beta, K, L, cfg, rng, (uint64_t)it, LR_P_MTE_GIBBS_TAU, lane);
    }
    const double prior = lr_mte_prior(Y, I, m, S.sd, S.beta, K, L, cfg, lane);
    // (a Gibbs step leaves Y, I and m alone: the likelihood is the accepted one's)
    const double lik = kind == 3 ? S.lik : lr_mte_loglik<CPL>(Y, I, m, D, K, L, cfg, lane);
    const bool ok = kind == 3 || it == 0 || (lik - S.lik) + (prior - S.prior) + hasting >= log_u;          // MTE:358
    S.prop_y += kind == 0 ? 1.0 : 0.0, S.prop_m += kind == 1 ? 1.0 : 0.0, S.prop_i += kind == 2 ? 1.0 : 0.0;
    if (ok) {
        S.Y[0] = Y[0], S.Y[1] = Y[1], S.I = I, S.m = m, S.lik = lik, S.prior = prior;
        S.acc_y += kind == 0 ? 1.0 : 0.0, S.acc_m += kind == 1 ? 1.0 : 0.0, S.acc_i += kind == 2 ? 1.0 : 0.0;
    }
}

// mode 0: the initial state drawn; 1: the parameters taken from the state; 2: iterations
template <int CPL>
__global__ __launch_bounds__(LR_MTE_THREADS) void lr_mte_chain_kernel(
    const uint8_t* __restrict__ code, const double* __restrict__ n, const double* __restrict__ E, const double* __restrict__ B,
    lr_mte_cfg cfg, int mode, double* __restrict__ state, long long it0, long long n_iters, double* __restrict__ rows) {
    __shared__ lr_mte_lds lds[LR_MTE_WAVES];
    const int lane = threadIdx.x & (LR_WAVE - 1), wave = threadIdx.x / LR_WAVE;
    const int c = blockIdx.x * LR_MTE_WAVES + wave;
    if (c >= cfg.n_chains) return;          // the whole wave: no barrier anywhere below
    lr_mte_lds& L = lds[wave];
    const int prob = c / cfg.chains_per_problem;
    const lr_stream rng{cfg.seed, (uint32_t)(cfg.chain0 + c)};
    const size_t off = (size_t)prob * cfg.G;
    lr_mte_cats K;
    lr_mte_cats_of(K, cfg, lane);
    lr_mte_data<CPL> D;
    lr_mte_load<CPL>(D, code, n + off, E + off, B + off, cfg, lane);
    double* st = state + (size_t)c * LR_MTE_STATE_W;
    const int T = cfg.T, NC = cfg.n_cats;
    lr_mte_chain S;
    if (mode == 0) {
        S.m = D.Etot / D.Btot;          // get_mle_mu (MTE:64)
        S.I = cfg.i_init ? (1u << T) - 1u : 0u;
#pragma unroll
        for (int j = 0; j < 2; ++j)          // Y_t[0] = 0, the others Normal(0, 0.1) (MTE:231)
            S.Y[j] = K.in[j] && !K.first[j] ? 0.1 * lr_normal(rng, 0ull, LR_P_MTE_INIT_Y, (uint32_t)(lane + LR_WAVE * j)) : 0.0;
        S.sd = lr_mte_draw_sd(S.Y, 1.0, K, L, cfg, rng, 0ull, LR_P_MTE_INIT_HP, lane);          // MTE:233-235
        S.beta = lr_mte_draw_beta(S.sd, cfg, rng, 0ull, LR_P_MTE_INIT_HP, LR_MTE_INIT_BETA_BASE, lane);
    } else {
        S.m = st[LR_MTE_S_M], S.beta = st[LR_MTE_S_BETA];
        S.I = (unsigned)__ballot(lane < T && st[LR_MTE_S_I + (lane & (LR_MTE_MAX_TRAITS - 1))] != 0.0);
        S.sd = lane < T ? st[LR_MTE_S_SD + lane] : 1.0;
#pragma unroll
        for (int j = 0; j < 2; ++j) S.Y[j] = K.in[j] ? st[LR_MTE_S_Y + lane + LR_WAVE * j] : 0.0;
    }
    if (mode != 2) {
        S.lik = lr_mte_loglik<CPL>(S.Y, S.I, S.m, D, K, L, cfg, lane);
        S.prior = lr_mte_prior(S.Y, S.I, S.m, S.sd, S.beta, K, L, cfg, lane);
        S.prop_y = S.prop_m = S.prop_i = S.acc_y = S.acc_m = S.acc_i = 0.0;
    } else {
        S.lik = st[LR_MTE_S_LIK], S.prior = st[LR_MTE_S_PRIOR];
        S.prop_y = st[LR_MTE_S_PROPOSED], S.prop_m = st[LR_MTE_S_PROPOSED + 1], S.prop_i = st[LR_MTE_S_PROPOSED + 2];
        S.acc_y = st[LR_MTE_S_ACCEPTED], S.acc_m = st[LR_MTE_S_ACCEPTED + 1], S.acc_i = st[LR_MTE_S_ACCEPTED + 2];
        // iterations to go until the next one with it % s_freq == 0: one 64-bit modulo per launch, not one per iteration
        long long until_row = (cfg.s_freq - it0 % cfg.s_freq) % cfg.s_freq;
        long long slot = cfg.slot0;
        for (long long it = it0; it < it0 + n_iters; ++it) {
            lr_mte_iterate<CPL>(S, D, K, L, cfg, rng, it, lane);
            const bool sample = until_row == 0;
            until_row = sample ? cfg.s_freq - 1 : until_row - 1;
            if (sample) {
                // [it, posterior, likelihood, prior, m, I[T], softmax(Y) [NC], sd[T], beta_hp], the rest 0 (rare path)
                double* row = rows + ((size_t)slot * cfg.n_chains + c) * LR_MTE_ROW_W;
                slot += 1;
                double sm[2];
                lr_mte_softmax(S.Y, K, L, lane, sm);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (K.in[j]) L.q[lane + LR_WAVE * j] = sm[j];
                if (lane < T) L.sd[lane] = S.sd;
                lr_mte_order();
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) {
                    const int p = lane + LR_WAVE * jj;
                    double h = 0.0;
                    if (p == LR_MTE_R_IT) h = (double)it;
                    else if (p == LR_MTE_R_POST) h = S.lik + S.prior;
                    else if (p == LR_MTE_R_LIK) h = S.lik;
                    else if (p == LR_MTE_R_PRIOR) h = S.prior;
                    else if (p == LR_MTE_R_M) h = S.m;
                    else if (p < LR_MTE_R_I + T) h = (double)((S.I >> (p - LR_MTE_R_I)) & 1u);
                    else if (p < LR_MTE_R_I + T + NC) h = L.q[p - LR_MTE_R_I - T];
                    else if (p < LR_MTE_R_I + 2 * T + NC) h = L.sd[p - LR_MTE_R_I - T - NC];
                    else if (p == LR_MTE_R_I + 2 * T + NC) h = S.beta;
                    row[p] = h;
                }
                lr_mte_order();
            }
        }
    }
    // the state: what lies behind T or NC in a block is written as 0, so that a state is a function of the chain alone
    if (lane < LR_MTE_MAX_TRAITS) {
        double so = 0.0;
        if (lane == LR_MTE_S_M) so = S.m;
        if (lane == LR_MTE_S_BETA) so = S.beta;
        if (lane == LR_MTE_S_LIK) so = S.lik;
        if (lane == LR_MTE_S_PRIOR) so = S.prior;
        if (lane == LR_MTE_S_PROPOSED) so = S.prop_y;
        if (lane == LR_MTE_S_PROPOSED + 1) so = S.prop_m;
        if (lane == LR_MTE_S_PROPOSED + 2) so = S.prop_i;
        if (lane == LR_MTE_S_ACCEPTED) so = S.acc_y;
        if (lane == LR_MTE_S_ACCEPTED + 1) so = S.acc_m;
        if (lane == LR_MTE_S_ACCEPTED + 2) so = S.acc_i;
        st[lane] = so;
        st[LR_MTE_S_I + lane] = lane < T ? (double)((S.I >> lane) & 1u) : 0.0;
        st[LR_MTE_S_SD + lane] = lane < T ? S.sd : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) st[LR_MTE_S_Y + lane + LR_WAVE * j] = K.in[j] ? S.Y[j] : 0.0;
}

// ---- host -------------------------------------------------------------------------------------------------------------
// the checks of lr_mte_init (steps = false) and lr_mte_steps, in the header's order -> cfg
static int lr_mte_args(const lr_mte_problem* p, bool steps, int32_t given, int64_t it0, int64_t n_iters, int32_t s_freq,
                       const double* rows, int64_t rows_cap, int64_t slot0, lr_mte_cfg* cfg) {
    // (rows may be NULL where no row is due)
    int64_t need = 0;
    const bool counts_ok = !steps || lr_rows_due(it0, n_iters, s_freq, &need);
    if (!p) return LR_ERR_NULL;
    if (!p->code || !p->n_states || !p->n_states_host || !p->n || !p->E || !p->B || !p->state ||
        (steps && !rows && counts_ok && need > 0))
        return LR_ERR_NULL;
    if (p->G < 1 || p->T < 1 || p->P < 1 || p->chains_per_problem < 1 || p->G > LR_MTE_MAX_COMBOS || p->T > LR_MTE_MAX_TRAITS)
        return LR_ERR_SIZE;
    if ((int64_t)p->P * p->chains_per_problem > INT32_MAX) return LR_ERR_SIZE;
    int n_cats = 0;
    for (int t = 0; t < p->T; ++t) {
        if (p->n_states_host[t] < 1 || p->n_states_host[t] > LR_MTE_MAX_STATES) return LR_ERR_SIZE;
        n_cats += p->n_states_host[t];
    }
    if (n_cats > LR_MTE_MAX_CATS) return LR_ERR_SIZE;
    if (!steps && given != 0 && given != 1) return LR_ERR_SIZE;
    if ((p->bvs != 0 && p->bvs != 1) || (p->constant != 0 && p->constant != 1) || !(p->pI > 0.0 && p->pI < 1.0) || p->bvs_from < 0)
        return LR_ERR_MODEL;
    if (steps && (!counts_ok || slot0 < 0 || rows_cap < 0 || rows_cap - slot0 < need)) return LR_ERR_SIZE;
    cfg->log_pI = std::log(p->pI), cfg->mult_l = 2.0 * std::log(LR_MULT_D);
    // the selector's thresholds (MTE:287-300); with `constant` only m moves
    if (p->constant) cfg->th_y = 0.0, cfg->th_m = 1.0, cfg->th_i = 1.0;
    else if (p->bvs) cfg->th_y = 0.45, cfg->th_m = 0.46, cfg->th_i = 0.91;
    else cfg->th_y = 0.90, cfg->th_m = 0.95, cfg->th_i = 0.95;
    cfg->rows_cap = steps ? rows_cap : 0, cfg->slot0 = steps ? slot0 : 0, cfg->chain0 = p->chain0, cfg->bvs_from = p->bvs_from;
    cfg->G = p->G, cfg->T = p->T, cfg->n_cats = n_cats, cfg->n_chains = p->P * p->chains_per_problem;
    cfg->chains_per_problem = p->chains_per_problem, cfg->s_freq = steps ? s_freq : 1;
    cfg->i_init = !p->constant && !p->bvs, cfg->seed = (uint32_t)p->seed;
    for (int t = 0; t < LR_MTE_MAX_TRAITS; ++t) cfg->S[t] = t < p->T ? (unsigned char)p->n_states_host[t] : 1;
    return LR_OK;
}

template <int CPL>
static void lr_mte_launch_as(const lr_mte_problem* p, const lr_mte_cfg& cfg, int mode, int64_t it0, int64_t n_iters, double* rows) {
    const unsigned blocks = (unsigned)((cfg.n_chains + LR_MTE_WAVES - 1) / LR_MTE_WAVES);
    hipLaunchKernelGGL((lr_mte_chain_kernel<CPL>), dim3(blocks), dim3(LR_MTE_THREADS), 0, (hipStream_t)p->stream, p->code, p->n, p->E,
                       p->B, cfg, mode, p->state, (long long)it0, (long long)n_iters, rows);
}

static int lr_mte_launch(const lr_mte_problem* p, const lr_mte_cfg& cfg, int mode, int64_t it0, int64_t n_iters, double* rows) {
    const int cpl = (cfg.G + LR_WAVE - 1) / LR_WAVE;
    if (cpl <= 1) lr_mte_launch_as<1>(p, cfg, mode, it0, n_iters, rows);
    else if (cpl <= 2) lr_mte_launch_as<2>(p, cfg, mode, it0, n_iters, rows);
    else if (cpl <= 4) lr_mte_launch_as<4>(p, cfg, mode, it0, n_iters, rows);
    else if (cpl <= 8) lr_mte_launch_as<8>(p, cfg, mode, it0, n_iters, rows);
    else lr_mte_launch_as<16>(p, cfg, mode, it0, n_iters, rows);
    return (int)hipGetLastError();
}

extern "C" int lr_mte_init(const lr_mte_problem* p, int32_t given) {
    lr_mte_cfg cfg;
    const int rc = lr_mte_args(p, false, given, 0, 0, 1, nullptr, 0, 0, &cfg);
    if (rc != LR_OK) return rc;
    return lr_mte_launch(p, cfg, given ? 1 : 0, 0, 0, nullptr);
}

extern "C" int lr_mte_steps(const lr_mte_problem* p, int64_t it0, int64_t n_iters, int32_t s_freq, double* rows, int64_t rows_cap,
                            int64_t slot0) {
    lr_mte_cfg cfg;
    const int rc = lr_mte_args(p, true, 0, it0, n_iters, s_freq, rows, rows_cap, slot0, &cfg);
    if (rc != LR_OK) return rc;
    if (n_iters == 0) return LR_OK;
    return lr_mte_launch(p, cfg, 2, it0, n_iters, rows);
}
