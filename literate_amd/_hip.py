"""ctypes binding of libliterate_hip.so (include/literate_hip.h, include/literate_hip_age.h, include/literate_hip_ade.h,
include/literate_hip_adej.h, include/literate_hip_mlik.h, include/literate_hip_tmlik.h, include/literate_hip_rjbin.h, include/literate_hip_rjmc3.h,
include/literate_hip_parbin.h, include/literate_hip_score.h, include/literate_hip_abc.h, include/literate_hip_trait.h, include/literate_hip_mte.h,
include/literate_hip_mtrend.h).  Fails loudly:
no fallback."""
import ctypes as C
import os

from .build import LIB

c_i32, c_i64, c_f64, c_vp = C.c_int32, C.c_int64, C.c_double, C.c_void_p

LR_ERR_NULL, LR_ERR_SIZE, LR_ERR_MODEL, LR_ERR_WORKSPACE, LR_ERR_T0, LR_ERR_STATE, LR_ERR_ORDER = -1, -2, -3, -4, -5, -6, -7
ERRORS = {-1: "LR_ERR_NULL", -2: "LR_ERR_SIZE", -3: "LR_ERR_MODEL", -4: "LR_ERR_WORKSPACE", -5: "LR_ERR_T0",
          -6: "LR_ERR_STATE", -7: "LR_ERR_ORDER (lineages must be sorted by birth time for the persistent engines)"}

LR_KMAX, LR_ROW, LR_MAX_BINS = 32, 64, 4094
LR_ADE_MAX_BINS = 512      # lr_ade_classes, lr_ade_profile (include/literate_hip_ade.h)
LR_ADEJ_MAX_BINS, LR_ADEJ_MOVES, LR_ADEJ_STATE_W, LR_ADEJ_ROW_W = 128, 5, 96, 73      # include/literate_hip_adej.h
LR_MLIK_MAX_BINS, LR_MLIK_MAX_TEMPS, LR_MLIK_MOVES, LR_MLIK_STATE_W, LR_MLIK_ROW_W = 512, 128, 2, 16, 12      # include/literate_hip_mlik.h
LR_TMLIK_MAX_BINS, LR_TMLIK_MAX_TEMPS, LR_TMLIK_MAX_MODELS, LR_TMLIK_MOVES, LR_TMLIK_STATE_W, LR_TMLIK_ROW_W = 512, 128, 64, 2, 16, 12      # include/literate_hip_tmlik.h
LR_RJBIN_MAX_BINS, LR_RJBIN_STATE_W = 512, 448      # include/literate_hip_rjbin.h
# include/literate_hip_rjmc3.h (LR_P_SWAP: csrc/lr_device.h, beside LR_P_INIT)
LR_RJMC3_MAX_TEMPS, LR_RJMC3_S_POS, LR_RJMC3_LADDER_W, LR_RJMC3_WIDE_MAX_BINS, LR_P_SWAP = 8, 9, 4, 256, 11
LR_PARBIN_MAX_BINS, LR_PARBIN_STATE_W = 512, 16      # include/literate_hip_parbin.h
LR_SCORE_MAX_SAMPLES, LR_SCORE_COLS = 4096, 6      # include/literate_hip_score.h
# include/literate_hip_abc.h
LR_ABC_NPAR, LR_ABC_MAX_LIVING, LR_ABC_SEARCH_CAP, LR_ABC_LDS_BINS, LR_P_ABC = 6, 1 << 24, 200, 1024, 56
LR_ABC_FLAG_OVERFLOW, LR_ABC_FLAG_EXTINCT, LR_ABC_FLAG_REFUSED = 1, 2, 4
# include/literate_hip_trait.h
LR_TRAIT_F, LR_TRAIT_MAX_N, LR_TRAIT_CB, LR_TRAIT_TILE, LR_TRAIT_MAX_TILES = 38, 1 << 24, 8, 2048, 1024
LR_P_TRAIT_MOVE, LR_P_TRAIT_ACCEPT = 60, 61
LR_TRAIT_ROW_SCALARS, LR_TRAIT_ROW_WL, LR_TRAIT_ROW_WM, LR_TRAIT_STATE_W = 448, 512, 1024, 1536
# include/literate_hip_mte.h
LR_MTE_MAX_TRAITS, LR_MTE_MAX_STATES, LR_MTE_MAX_CATS, LR_MTE_MAX_COMBOS, LR_MTE_STATE_W, LR_MTE_ROW_W = 16, 16, 128, 1024, 176, 192
# include/literate_hip_mtrend.h
LR_MTREND_MAX_BINS, LR_MTREND_MAX_COVS, LR_MTREND_STATE_W, LR_MTREND_ROW_W, LR_MTREND_MOVES = 512, 16, 96, 72, 6
LR_WARN_KCAP = 2
LR_STATE_ROWS, LR_ISTATE_ROWS = 9, 5
LR_TRACE_HEAD = 13
LR_TRACE_W = LR_TRACE_HEAD + 2 * (2 * LR_KMAX - 1)
LR_TRAIT_ROW_W = LR_TRACE_W + 8
LR_SIMBATCH_GROUPS, LR_SIMBATCH_LDS_SLOTS = 512, 16384      # lr_simulate_bd_batch: most workgroups, list positions in LDS
LR_SHIFT_PRIOR_KCAP, LR_SHIFT_PRIOR_BLOCKS = 64, 768      # lr_shift_prior: most rates a replicate draws, most workgroups
LR_ESS_LDS_ROWS = 16384      # lr_ess_summary: longest kept series held in LDS (longer ones stream from the workspace)
# rows / scalar slots (include/literate_hip.h)
ROW_L, ROW_M, ROW_TL, ROW_TM, ROW_PL, ROW_PM, ROW_PTL, ROW_PTM, ROW_SCALARS = range(9)
(S_LIKA, S_PRIORA, S_PRIORPOIA, S_GRATE_L, S_GRATE_M, S_POI, S_HASTING, S_PRIOR_P, S_PRIORPOI_P, S_CONST_P,
 S_CONST_A, S_LIK_P, S_LOG_G0, S_LOG_G1, S_LOG_POI) = range(15)
IROW_EL, IROW_EM, IROW_PEL, IROW_PEM, IROW_SCALARS = range(5)
(I_KL, I_KM, I_PKL, I_PKM, I_GIBBS, I_INVALID, I_IT_LO, I_IT_HI, I_ACCEPTED, I_MOVE, I_NEXT_LO, I_NEXT_HI,
 I_SLOT) = range(13)


class McmcConfig(C.Structure):
    _fields_ = [("n_lineages", c_i64), ("n_bins", c_i32), ("n_chains", c_i32), ("model", c_i32),
                ("const_rates", c_i32), ("const_death_rate", c_i32), ("use_rate_HP", c_i32), ("s_freq", c_i32),
                ("n_trace_slots", c_i32), ("poisson_HP", c_f64), ("update_fraction", c_f64), ("t0", c_f64),
                ("start_time", c_f64), ("end_time", c_f64), ("seed", C.c_uint64), ("chain_offset", c_i64),
                ("unit_resolution", c_i32), ("engine_mode", c_i32), ("frac_birth", c_f64), ("frac_death", c_f64),
                ("sampler", c_i32), ("m_birth", c_i32), ("m_death", c_i32), ("team_request", c_i32),
                ("dd_present", c_f64), ("dd_init_death", c_f64)]


class McmcLayout(C.Structure):
    _fields_ = [("state_f64", c_i64), ("state_i32", c_i64), ("bin_consts", c_i64), ("lineage_idx", c_i64), ("args_blob", c_i64), ("tables", c_i64),
                ("partials", c_i64), ("trace", c_i64), ("total_bytes", c_i64), ("table_stride", c_i32),
                ("tiles", c_i32), ("chains_per_block", c_i32), ("trace_width", c_i32), ("n_parts", c_i32),
                ("pipelined", c_i32), ("persistent", c_i32), ("reserved1", c_i32), ("status", c_i64), ("xchg", c_i64),
                ("team_blocks", c_i32), ("table_mode", c_i32), ("lineage_frac", c_i64), ("pack_tmp", c_i64),
                ("spec_chains_per_team", c_i32), ("streaming", c_i32), ("packed_scan", c_i32), ("reserved3", c_i32)]


class TmlikProblem(C.Structure):
    """lr_tmlik_problem (include/literate_hip_tmlik.h): the descriptor both lr_tmlik_* entry points take; the stream rides in it"""
    _fields_ = [("n_spec", c_vp), ("n_exti", c_vp), ("DT", c_vp), ("trends", c_vp), ("wins", c_vp), ("state", c_vp),
                ("betas", c_vp), ("scales", c_vp), ("col", c_vp), ("flags", c_vp), ("key0", c_vp),
                ("n_bins", c_i32), ("n_cols", c_i32), ("n_models", c_i32), ("n_reps", c_i32), ("T", c_i32),
                ("seed", C.c_uint64), ("stream", c_vp)]


class RjbinProblem(C.Structure):
    """lr_rjbin_problem (include/literate_hip_rjbin.h): the descriptor both lr_rjbin_* entry points take; the stream rides in it"""
    _fields_ = [("sp", c_vp), ("ex", c_vp), ("br", c_vp), ("ex_dead", c_vp), ("br_dead", c_vp), ("start_time", c_vp),
                ("end_time", c_vp), ("state", c_vp), ("warn", c_vp),
                ("n_bins", c_i32), ("R", c_i32), ("chains_per_rep", c_i32), ("model", c_i32), ("const_rates", c_i32),
                ("const_death_rate", c_i32), ("use_rate_HP", c_i32), ("chain0", c_i64), ("poisson_HP", c_f64),
                ("update_fraction", c_f64), ("seed", C.c_uint64), ("stream", c_vp)]


class Rjmc3Problem(C.Structure):
    """lr_rjmc3_problem (include/literate_hip_rjmc3.h): lr_rjbin_problem's fields, then the ladder's; the stream rides in it"""
    _fields_ = RjbinProblem._fields_[:-1] + [("betas", c_vp), ("swaps", c_vp), ("T", c_i32), ("swap_every", c_i32), ("stream", c_vp)]


class ParbinProblem(C.Structure):
    """lr_parbin_problem (include/literate_hip_parbin.h): the descriptor both lr_parbin_* entry points take; the stream rides in it"""
    _fields_ = [("n_spec", c_vp), ("n_exti", c_vp), ("DT", c_vp), ("origin", c_vp), ("present", c_vp), ("trend", c_vp),
                ("state", c_vp), ("n_bins", c_i32), ("R", c_i32), ("chains_per_rep", c_i32), ("sampler", c_i32),
                ("m_birth", c_i32), ("m_death", c_i32), ("init_death", c_f64), ("chain0", c_i64), ("seed", C.c_uint64),
                ("stream", c_vp)]


class RttScoreProblem(C.Structure):
    """lr_rtt_score_problem (include/literate_hip_score.h): the descriptor lr_rtt_score takes; the stream rides in it"""
    _fields_ = [("trace", c_vp), ("truth", c_vp), ("rates", c_vp), ("shift_freq", c_vp), ("k_counts", c_vp), ("covered", c_vp),
                ("score", c_vp), ("n_samples", c_i32), ("n_chains", c_i32), ("chains_per_group", c_i32), ("reserved", c_i32),
                ("start_age", c_f64), ("end_age", c_f64), ("burnin", c_f64), ("stream", c_vp)]


class AbcProblem(C.Structure):
    """lr_abc_problem (include/literate_hip_abc.h): the descriptor lr_abc_simulate takes; the stream rides in it"""
    _fields_ = [("theta", c_vp), ("n_start", c_vp), ("sim_id", c_vp), ("obs", c_vp), ("weight", c_vp), ("dist", c_vp),
                ("flags", c_vp), ("counts", c_vp), ("k_end", c_vp), ("n_sims", c_i64), ("id0", c_i64), ("n_bins", c_i32),
                ("steps_per_bin", c_i32), ("max_living", c_i32), ("reserved", c_i32), ("seed", C.c_uint64), ("stream", c_vp)]


class AbcBinomialProblem(C.Structure):
    """lr_abc_binomial_problem (include/literate_hip_abc.h): the descriptor lr_abc_binomial takes; the stream rides in it"""
    _fields_ = [("n", c_vp), ("p", c_vp), ("u", c_vp), ("x", c_vp), ("used", c_vp), ("N", c_i64), ("n_u", c_i32),
                ("reserved", c_i32), ("stream", c_vp)]


class TraitWeightsProblem(C.Structure):
    """lr_trait_weights_problem (include/literate_hip_trait.h): the descriptor lr_trait_weights takes; the stream rides in it"""
    _fields_ = [("ts", c_vp), ("te", c_vp), ("x", c_vp), ("params", c_vp), ("W", c_vp), ("Slog_birth", c_vp), ("Slog_death", c_vp),
                ("workspace", c_vp), ("workspace_bytes", c_i64), ("n", c_i64), ("t0", c_f64), ("n_bins", c_i32), ("C", c_i32),
                ("stream", c_vp)]


class TraitProblem(C.Structure):
    """lr_trait_problem (include/literate_hip_trait.h): the descriptor both sampler entry points take; the stream rides in it"""
    _fields_ = [("ts", c_vp), ("te", c_vp), ("x", c_vp), ("sp", c_vp), ("ex", c_vp), ("state", c_vp), ("warn", c_vp),
                ("workspace", c_vp), ("workspace_bytes", c_i64), ("n", c_i64), ("chain0", c_i64), ("t0", c_f64),
                ("start_time", c_f64), ("end_time", c_f64), ("poisson_HP", c_f64), ("update_fraction", c_f64),
                ("win_x0", c_f64 * 2), ("win_kappa", c_f64 * 2), ("x0_lo", c_f64), ("x0_hi", c_f64),
                ("n_bins", c_i32), ("C", c_i32), ("const_rates", c_i32), ("const_death_rate", c_i32), ("use_rate_HP", c_i32),
                ("trait_every", c_i32), ("seed", C.c_uint64), ("stream", c_vp)]


class MteProblem(C.Structure):
    """lr_mte_problem (include/literate_hip_mte.h): the descriptor both lr_mte_* entry points take; the stream rides in it"""
    _fields_ = [("code", c_vp), ("n_states", c_vp), ("n_states_host", c_vp), ("n", c_vp), ("E", c_vp), ("B", c_vp), ("state", c_vp),
                ("G", c_i32), ("T", c_i32), ("P", c_i32), ("chains_per_problem", c_i32), ("bvs", c_i32), ("constant", c_i32),
                ("bvs_from", c_i64), ("pI", c_f64), ("chain0", c_i64), ("seed", C.c_uint64), ("stream", c_vp)]


class MtrendProblem(C.Structure):
    """lr_mtrend_problem (include/literate_hip_mtrend.h): the descriptor both lr_mtrend_* entry points take; the stream rides in it"""
    _fields_ = [("n_spec", c_vp), ("n_exti", c_vp), ("DT", c_vp), ("X", c_vp), ("sx_spec", c_vp), ("sx_exti", c_vp), ("state", c_vp),
                ("n_bins", c_i32), ("P", c_i32), ("C", c_i32), ("m_birth", c_i32), ("m_death", c_i32), ("no_death", c_i32),
                ("bvs", c_i32), ("reserved", c_i32), ("bvs_from", c_i64), ("pI", c_f64), ("slab_sd", c_f64), ("win", c_f64 * 2),
                ("chain0", c_i64), ("seed", C.c_uint64), ("stream", c_vp)]


# name -> (restype, argtypes); exactly the symbols include/literate_hip.h, literate_hip_age.h, literate_hip_ade.h and
# literate_hip_adej.h, literate_hip_mlik.h, literate_hip_tmlik.h, literate_hip_rjbin.h, literate_hip_rjmc3.h, literate_hip_parbin.h, literate_hip_score.h, literate_hip_abc.h, literate_hip_trait.h, literate_hip_mte.h, literate_hip_mtrend.h declare (+ the RNG debug hook)
SIGNATURES = {
    "lr_version": (c_i32, []),
    "lr_bin_events_workspace_bytes": (c_i64, [c_i64, c_i32]),
    "lr_bin_events": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "lr_bin_unit_events_workspace_bytes": (c_i64, [c_i64, c_i32]),
    "lr_bin_unit_events": (c_i32, [c_vp, c_vp, c_i64, c_f64, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "lr_expand_rates": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "lr_bd_loglik_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32, c_i32]),
    "lr_bd_loglik_plan": (c_i32, [c_i64, c_i32, c_i32, c_i32, C.POINTER(c_i32)]),
    "lr_bd_loglik_batch": (c_i32, [c_vp, c_vp, c_i64, c_f64, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_f64, c_vp,
                                   c_vp, c_i64, c_vp]),
    "lr_waic_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32, c_i32]),
    "lr_waic_plan": (c_i32, [c_i64, c_i32, c_i32, c_i32, C.POINTER(c_i32)]),
    "lr_waic_pointwise": (c_i32, [c_vp, c_vp, c_i64, c_f64, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_f64, c_vp, c_vp, c_vp,
                                  c_i64, c_vp]),
    "lr_loo_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32, c_i32]),
    "lr_loo_plan": (c_i32, [c_i64, c_i32, c_i32, c_i32, C.POINTER(c_i32)]),
    "lr_loo_pointwise": (c_i32, [c_vp, c_vp, c_i64, c_f64, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_f64, c_vp, c_vp, c_vp,
                                 c_i64, c_vp]),
    "lr_psis_rows_workspace_bytes": (c_i64, [c_i64, c_i32]),
    "lr_psis_rows": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "lr_rj_propose_score": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_f64, c_vp, c_vp, c_vp, c_vp,
                                    c_vp]),
    "lr_log_priors": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_f64, c_vp, c_vp, c_vp, c_vp]),
    "lr_dd_rates": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "lr_ddv2_rates": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "lr_binned_keiding": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "lr_simulate_bd": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_f64, c_f64, c_f64, c_f64, c_i64, c_i64, C.c_uint64, c_vp, c_vp,
                             c_vp, c_vp, c_vp, c_i64, c_vp]),
    "lr_simulate_bd_batch_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32, c_i64]),
    "lr_simulate_bd_batch": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_i64, C.c_uint64, c_vp, c_vp, c_vp, c_i64,
                                   c_vp]),
    "lr_simulate_dd_batch_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32, c_i64]),
    "lr_simulate_dd_batch": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_i64, C.c_uint64, c_vp, c_vp, c_vp,
                                   c_i64, c_vp]),
    "lr_trend_rates": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "lr_format_rows": (c_i64, [c_vp, c_vp, c_i64, C.c_uint64, c_i32, c_vp, c_i64]),
    "lr_rtt_summary_workspace_bytes": (c_i64, [c_i32, c_i32, c_f64, c_f64, c_f64, c_i32]),
    "lr_rtt_summary": (c_i32, [c_vp, c_i32, c_i32, c_f64, c_f64, c_f64, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "lr_shift_prior": (c_i32, [c_f64, c_f64, c_i64, c_i64, C.c_uint64, c_f64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "lr_ppc_age_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32]),
    "lr_ppc_age_plan": (c_i32, [c_i64, c_i32, c_i32, C.POINTER(c_i32)]),
    "lr_ppc_age": (c_i32, [c_vp, c_vp, c_i64, c_f64, c_i32, c_vp, c_i32, C.c_uint64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "lr_ade_classes": (c_i32, [c_vp, c_vp, c_i64, c_f64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "lr_ade_profile_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "lr_ade_profile": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "lr_adej_workspace_bytes": (c_i64, [c_i32]),
    "lr_adej_prepare": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i64, c_vp]),
    "lr_adej_loglik": (c_i32, [c_vp, c_i64, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    "lr_adej_init": (c_i32, [c_vp, c_i64, c_i32, c_f64, c_i32, c_i32, c_f64, c_f64, C.c_uint64, c_i32, c_i32, c_vp, c_vp]),
    "lr_adej_steps": (c_i32, [c_vp, c_i64, c_i32, c_f64, c_i32, c_i32, c_f64, c_f64, C.c_uint64, c_i32, c_i32, c_vp, c_i64, c_i64,
                              c_i32, c_vp, c_i64, c_vp]),
    "lr_mlik_init": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_f64, c_f64, c_i32, c_i32, c_f64, c_vp, c_vp, c_i32, C.c_uint64, c_i32, c_i32,
                             c_vp, c_vp]),
    "lr_mlik_steps": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_f64, c_f64, c_i32, c_i32, c_f64, c_vp, c_vp, c_i32, C.c_uint64, c_i32, c_i32,
                              c_vp, c_i64, c_i64, c_i32, c_vp, c_i64, c_vp]),
    "lr_mlik_estimate": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "lr_tmlik_init": (c_i32, [C.POINTER(TmlikProblem)]),
    "lr_tmlik_steps": (c_i32, [C.POINTER(TmlikProblem), c_i64, c_i64, c_i32, c_vp, c_i64, c_i64]),
    "lr_rjbin_init": (c_i32, [C.POINTER(RjbinProblem), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "lr_rjbin_steps": (c_i32, [C.POINTER(RjbinProblem), c_i64, c_i64, c_i32, c_vp, c_i64, c_i64]),
    "lr_rjmc3_init": (c_i32, [C.POINTER(Rjmc3Problem), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "lr_rjmc3_steps": (c_i32, [C.POINTER(Rjmc3Problem), c_i64, c_i64, c_i32, c_vp, c_vp, c_i64, c_i64]),
    "lr_parbin_init": (c_i32, [C.POINTER(ParbinProblem)]),
    "lr_parbin_steps": (c_i32, [C.POINTER(ParbinProblem), c_i64, c_i64, c_i32, c_vp, c_i64, c_i64]),
    "lr_rtt_score": (c_i32, [C.POINTER(RttScoreProblem)]),
    "lr_abc_simulate": (c_i32, [C.POINTER(AbcProblem)]),
    "lr_abc_binomial": (c_i32, [C.POINTER(AbcBinomialProblem)]),
    "lr_trait_weights_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32]),
    "lr_trait_weights_plan": (c_i32, [c_i64, c_i32, c_i32, C.POINTER(c_i32)]),
    "lr_trait_weights": (c_i32, [C.POINTER(TraitWeightsProblem)]),
    "lr_trait_workspace_bytes": (c_i64, [c_i64, c_i32, c_i32]),
    "lr_trait_init": (c_i32, [C.POINTER(TraitProblem), c_vp]),
    "lr_trait_steps": (c_i32, [C.POINTER(TraitProblem), c_i64, c_i64, c_i32, c_vp, c_i64, c_i64]),
    "lr_mte_init": (c_i32, [C.POINTER(MteProblem), c_i32]),
    "lr_mte_steps": (c_i32, [C.POINTER(MteProblem), c_i64, c_i64, c_i32, c_vp, c_i64, c_i64]),
    "lr_mtrend_init": (c_i32, [C.POINTER(MtrendProblem), c_i32]),
    "lr_mtrend_steps": (c_i32, [C.POINTER(MtrendProblem), c_i64, c_i64, c_i32, c_vp, c_i64, c_i64]),
    "lr_ess_summary_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32, c_vp, c_i32, c_f64, c_i32]),
    "lr_ess_summary": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_f64, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "lr_col_summary_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32, c_vp, c_i32, c_f64, c_i32, c_i32]),
    "lr_col_summary": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_f64, c_i32, c_vp, c_vp, c_i64, c_vp]),
    "lr_curve_summary_workspace_bytes": (c_i64, [c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_f64, c_i32, c_i32]),
    "lr_curve_summary": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32, c_f64, c_i32, c_vp,
                                 c_vp, c_i64, c_vp]),
    "lr_mcmc_query_layout": (c_i32, [C.POINTER(McmcConfig), C.POINTER(McmcLayout)]),
    "lr_mcmc_create": (c_i32, [C.POINTER(McmcConfig), c_vp, c_vp, c_vp, c_vp, c_i64, C.POINTER(c_vp)]),
    "lr_mcmc_init": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "lr_mcmc_steps": (c_i32, [c_vp, c_i64, c_vp]),
    "lr_mcmc_time_scan": (c_i32, [c_vp, c_i32, C.POINTER(C.c_float), c_vp]),
    "lr_mcmc_time_steps": (c_i32, [c_vp, c_i64, C.POINTER(C.c_float), c_vp]),
    "lr_mcmc_restore": (c_i32, [c_vp, c_vp]),
    "lr_mcmc_describe": (c_i32, [c_vp, C.c_char_p, c_i32]),
    "lr_mcmc_p4_config": (c_i32, [c_vp, C.POINTER(c_i32)]),
    "lr_mcmc_p4_resident": (c_i32, [c_vp, C.POINTER(c_i32)]),
    "lr_mcmc_p4_pipe": (c_i32, [c_vp, C.POINTER(c_i32)]),
    "lr_mcmc_p4_draws": (c_i32, [c_vp, C.POINTER(c_i32)]),
    "lr_mcmc_status": (c_i32, [c_vp, C.POINTER(c_i32), c_vp]),
    "lr_mcmc_warnings": (c_i32, [c_vp, C.POINTER(c_i32), c_vp]),
    "lr_mcmc_destroy": (c_i32, [c_vp]),
    "lr_debug_draws": (c_i32, [C.c_uint64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "lr_debug_stream2": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp]),
}

_lib = None


class HipLibraryError(RuntimeError):
    pass


def load():
    """dlopen the in-tree library (built by literate_amd.build / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise HipLibraryError("libliterate_hip.so not found at %s - run `python -m literate_amd.build` "
                              "(there is no CPU fallback)" % LIB)
    lib = C.CDLL(LIB)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc, what):
    if rc == 0:
        return
    if rc < 0:
        raise ValueError("%s: %s" % (what, ERRORS.get(rc, rc)))
    raise HipLibraryError("%s: hipError_t %d" % (what, rc))


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise HipLibraryError("no ROCm GPU visible: literate_amd has no CPU path")
    return torch


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else c_vp(t.data_ptr())


def stream_ptr(device=None):
    """torch's current HIP stream on `device` (None = the current device) as a void*."""
    import torch
    return c_vp(torch.cuda.current_stream(device).cuda_stream)


def launch(fn, device, *args):
    """Call an ABI entry point whose last argument is the stream: on `device`'s current torch stream, with `device`
    made current for the call (a launch on another device's stream is an error in HIP, and the library's own
    streams / events / graphs are created on the current device)."""
    import torch
    with torch.cuda.device(device):
        return fn(*args, stream_ptr(device))


def launch_problem(fn, device, problem, *args):
    """Call an entry point that takes a descriptor with the stream in it (lr_tmlik_*, lr_rjbin_*, lr_rjmc3_*, lr_parbin_*, lr_rtt_score, lr_abc_*, lr_trait_*, lr_mte_*, lr_mtrend_*): `device`'s current torch stream is put
    into problem.stream, `device` made current for the call."""
    import torch
    with torch.cuda.device(device):
        problem.stream = stream_ptr(device)
        return fn(C.byref(problem), *args)
