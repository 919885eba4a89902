"""frirl_amd -- MI355X-native FRIRL / FIVE hot path (package directory: fri-reinforcementlearning-c_amd/).

The product is the C-ABI shared library lib/libfrirl_hip.so (hand-written gfx950 HIP kernels,
declared in include/frirl_hip.h) plus the ANSI-C drop-in host library that exports the
reference's five_* / FIVE_* / frirl_* API on top of it.  This Python module is only plumbing for
tests and bench.py: a ctypes binding that hands raw device pointers of torch tensors to the C ABI.
There is no CPU fallback: a missing library raises, a missing GPU makes every call return
FRIRL_HIP_ENODEV (raised as FrirlHipError).
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
HIP_LIB_PATH = os.environ.get("FRIRL_HIP_LIB_OVERRIDE") or os.path.join(PKG_DIR, "lib", "libfrirl_hip.so")      # override: A/B of experimental builds (tools/)

NO_HIT = 0xFFFFFFFF
MAX_NANT = 16
MAX_ACTIONS = 32


class FrirlHipError(RuntimeError):
    pass


class Tables(C.Structure):
    """struct frirl_hip_tables (include/frirl_hip.h)."""
    _fields_ = [("nant", C.c_int32), ("U", C.c_int32), ("u", C.c_void_p), ("ve", C.c_void_p)]


class RuleBases(C.Structure):
    """struct frirl_hip_rulebases (include/frirl_hip.h)."""
    _fields_ = [("E", C.c_int32), ("maxR", C.c_int32), ("rb", C.c_void_p), ("nrules", C.c_void_p), ("uidx", C.c_void_p)]


MAX_GRID = 64
ENV_KINDS = {"mountaincar": 0, "cartpole": 1, "acrobot": 2}
ENV_EXTERNAL = 3          # FRIRL_HIP_ENV_EXTERNAL: the caller steps the environment (agent_begin / agent_observe)
UPD_INACTIVE, UPD_EXACT, UPD_SPREAD, UPD_INSERTED, UPD_SKIPPED, UPD_FULL = range(6)


class AgentDesc(C.Structure):
    """struct frirl_hip_agent (include/frirl_hip.h)."""
    _fields_ = [("alpha", C.c_double), ("gamma", C.c_double), ("qdiff_pos_boundary", C.c_double), ("qdiff_neg_boundary", C.c_double),
                ("weight_significant", C.c_double), ("skip_rules", C.c_int32), ("p", C.c_int32), ("A", C.c_int32), ("env_kind", C.c_int32),
                ("max_steps", C.c_int32), ("no_random", C.c_int32), ("grid_len", C.c_int32 * MAX_NANT), ("grid_div", C.c_double * MAX_NANT),
                ("values_def", C.c_double * MAX_NANT), ("grid_values", C.c_void_p), ("action_ve", C.c_void_p), ("epsilon", C.c_double),
                ("reward_good_above", C.c_double), ("qdiff_final_tolerance", C.c_double), ("seed", C.c_uint64), ("evaluate", C.c_int32), ("debug_flags", C.c_int32), ("env_id_base", C.c_uint64)]


HP_COLUMNS = ("alpha", "gamma", "qdiff_pos_boundary", "qdiff_neg_boundary", "weight_significant", "skip_rules")


class HparamRowsDesc(C.Structure):
    """struct frirl_hip_hparam_rows (include/frirl_hip.h)."""
    _fields_ = [(k, C.c_void_p) for k in HP_COLUMNS]


class ExploreRowsDesc(C.Structure):
    """struct frirl_hip_explore_rows (include/frirl_hip.h)."""
    _fields_ = [("epsilon", C.c_void_p), ("horizon", C.c_void_p), ("horizon_all", C.c_int32), ("reserved", C.c_int32)]


class TargetRowsDesc(C.Structure):
    """struct frirl_hip_target_rows (include/frirl_hip.h)."""
    _fields_ = [("target", C.c_void_p), ("target_all", C.c_int32), ("reserved", C.c_int32)]


TARGET_SARSA, TARGET_Q = 0, 1       # FRIRL_HIP_TARGET_*


class ExpectRowsDesc(C.Structure):
    """struct frirl_hip_expect_rows (include/frirl_hip.h)."""
    _fields_ = [("expected", C.c_void_p), ("expected_all", C.c_int32), ("reserved", C.c_uint32)]


class EnvsDesc(C.Structure):
    """struct frirl_hip_envs (include/frirl_hip.h)."""
    _fields_ = [("states", C.c_void_p), ("q_ant", C.c_void_p), ("fus", C.c_void_p), ("done", C.c_void_p), ("ep_steps", C.c_void_p),
                ("ep_reward", C.c_void_p), ("rant", C.c_void_p), ("status", C.c_void_p), ("start_states", C.c_void_p), ("episode", C.c_void_p),
                ("spread_ant", C.c_void_p), ("spread_R", C.c_void_p)]


class RolloutDesc(C.Structure):
    """struct frirl_hip_rollout (include/frirl_hip.h)."""
    _fields_ = [("start_states", C.c_void_p), ("exclude_mask", C.c_void_p), ("rule_slot", C.c_void_p), ("steps", C.c_void_p),
                ("reward", C.c_void_p), ("success", C.c_void_p), ("final_states", C.c_void_p)]


class RolloutBatchDesc(C.Structure):
    """struct frirl_hip_rollout_batch_rows (include/frirl_hip.h)."""
    _fields_ = [("n", C.c_int32), ("start_states", C.c_void_p), ("row_count", C.c_void_p), ("step_cap", C.c_void_p), ("active", C.c_void_p),
                ("steps", C.c_void_p), ("reward", C.c_void_p), ("success", C.c_void_p), ("final_states", C.c_void_p)]


class RolloutScore(C.Structure):
    """struct frirl_hip_rollout_score (include/frirl_hip.h)."""
    _fields_ = [("rows", C.c_int32), ("successes", C.c_int32), ("steps_sum", C.c_int64), ("reward_sum", C.c_double),
                ("reward_min", C.c_double), ("reward_max", C.c_double)]


class RolloutLogDesc(C.Structure):
    """struct frirl_hip_rollout_log (include/frirl_hip.h)."""
    _fields_ = [("n", C.c_int32), ("episodes", C.c_int32), ("T", C.c_int32), ("reserved", C.c_int32), ("start_states", C.c_void_p),
                ("row_count", C.c_void_p), ("active", C.c_void_p), ("obs", C.c_void_p), ("q_obs", C.c_void_p), ("action", C.c_void_p),
                ("reward", C.c_void_p), ("success", C.c_void_p), ("start", C.c_void_p), ("length", C.c_void_p), ("ep_steps", C.c_void_p),
                ("ep_reward", C.c_void_p), ("ep_success", C.c_void_p)]


class TeachResult(C.Structure):
    """struct frirl_hip_teach_result (include/frirl_hip.h)."""
    _fields_ = [("teacher", C.c_int32), ("episodes_recorded", C.c_int32), ("successes", C.c_int32), ("records", C.c_int32),
                ("students", C.c_int32), ("refused", C.c_int32), ("records_replayed", C.c_int64)]


class SelectResult(C.Structure):
    """struct frirl_hip_select_result (include/frirl_hip.h)."""
    _fields_ = [("best", C.c_int32), ("parents", C.c_int32), ("replaced", C.c_int32), ("reserved", C.c_int32), ("rules_copied", C.c_int64)]


CLONE_KEPT, CLONE_CLONED, CLONE_BAD_SRC, CLONE_CHAINED, CLONE_BAD_RULES = range(5)      # FRIRL_HIP_CLONE_*


class SelectInfo(C.Structure):
    """struct frirl_hip_select_info (include/frirl_hip.h)."""
    _fields_ = [("N", C.c_int32), ("status", C.c_int32), ("best", C.c_int32), ("bad_agent", C.c_int32)]


PLAN_OK, PLAN_NAN, PLAN_TOO_FEW = range(3)                                              # FRIRL_HIP_PLAN_*
# FRIRL_HIP_PERTURB_*: the bit of a column in PerturbSpec.columns; 0..4 take (down, up, lo, hi), 5..7 a flip probability
PERTURB_COLUMNS = ("alpha", "gamma", "weight_significant", "epsilon", "horizon", "skip_rules", "target", "expected")


class PerturbSpec(C.Structure):
    """struct frirl_hip_perturb_spec (include/frirl_hip.h)."""
    _fields_ = [("columns", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("down", C.c_double * 5), ("up", C.c_double * 5),
                ("lo", C.c_double * 5), ("hi", C.c_double * 5), ("flip", C.c_double * 3)]


class EvolveResult(C.Structure):
    """struct frirl_hip_evolve_result (include/frirl_hip.h)."""
    _fields_ = [("best", C.c_int32), ("parents", C.c_int32), ("replaced", C.c_int32), ("perturbed", C.c_int32), ("rules_copied", C.c_int64),
                ("generation", C.c_int32), ("plan_status", C.c_int32)]


class BatchDesc(C.Structure):
    """struct frirl_hip_batch_desc (include/frirl_hip.h)."""
    _fields_ = [("nant", C.c_int32), ("U", C.c_int32), ("E", C.c_int32), ("maxR", C.c_int32), ("u", C.c_void_p), ("ve", C.c_void_p),
                ("agent", AgentDesc), ("R0", C.c_int32), ("rant0", C.c_void_p), ("rconc0", C.c_void_p), ("start_states", C.c_void_p),
                ("device_select", C.c_int32), ("device", C.c_int32)]


class BatchStats(C.Structure):
    """struct frirl_hip_batch_stats_t (include/frirl_hip.h)."""
    _fields_ = [("reward_sum", C.c_double), ("steps_sum", C.c_double), ("rules_sum", C.c_double), ("reward_min", C.c_double),
                ("reward_max", C.c_double), ("agents", C.c_int64), ("converged", C.c_int64), ("episodes_max", C.c_int64),
                ("total_env_steps", C.c_int64), ("full_agents", C.c_int64)]


class SenderDesc(C.Structure):
    """struct frirl_hip_sender (include/frirl_hip.h)."""
    _fields_ = [("rant", C.c_void_p), ("rule_stride", C.c_int64), ("dim_stride", C.c_int64), ("rconc", C.c_void_p), ("S", C.c_int32),
                ("reserved", C.c_int32), ("S_dev", C.c_void_p)]


class ReduceResult(C.Structure):
    """struct frirl_hip_reduce_result (include/frirl_hip.h)."""
    _fields_ = [("rules_before", C.c_int32), ("rules_after", C.c_int32), ("rounds", C.c_int32), ("rollouts", C.c_int32),
                ("steps_incremental", C.c_int32), ("reserved", C.c_int32), ("reward", C.c_double)]


class ReduceStarts(C.Structure):
    """struct frirl_hip_reduce_starts (include/frirl_hip.h)."""
    _fields_ = [("n", C.c_int32), ("drop_bad_starts", C.c_int32), ("start_states", C.c_void_p), ("start_count", C.c_void_p)]


class ReduceStartResult(C.Structure):
    """struct frirl_hip_reduce_start_result (include/frirl_hip.h)."""
    _fields_ = [("used", C.c_int32), ("steps_incremental", C.c_int32), ("baseline_reward", C.c_double), ("reward", C.c_double)]


REDUCE_MAX_STARTS = 256


class MapPoints(C.Structure):
    """struct frirl_hip_map_points (include/frirl_hip.h)."""
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("points", C.c_void_p), ("point_count", C.c_void_p), ("active", C.c_void_p)]


class ReduceMapResult(C.Structure):
    """struct frirl_hip_reduce_map_result (include/frirl_hip.h)."""
    _fields_ = [("rules_before", C.c_int32), ("rules_after", C.c_int32), ("points", C.c_int32), ("tries", C.c_int32)]


class RuleUsageOut(C.Structure):
    """struct frirl_hip_rule_usage_out (include/frirl_hip.h)."""
    _fields_ = [("sum", C.c_void_p), ("peak", C.c_void_p), ("best", C.c_void_p)]


class ReduceOrdersResult(C.Structure):
    """struct frirl_hip_reduce_orders_result (include/frirl_hip.h)."""
    _fields_ = [("rules_before", C.c_int32), ("rules_after", C.c_int32), ("points", C.c_int32), ("chosen", C.c_int32), ("tries", C.c_int32),
                ("reserved", C.c_int32)]


REDUCE_MAX_ORDERS = 16


class LogPointsDesc(C.Structure):
    """struct frirl_hip_log_points_desc (include/frirl_hip.h)."""
    _fields_ = [("E", C.c_int32), ("n_logs", C.c_int32), ("T", C.c_int32), ("ns", C.c_int32), ("cap", C.c_int32), ("only_successful", C.c_int32),
                ("obs", C.c_void_p), ("q_obs", C.c_void_p), ("success", C.c_void_p), ("start", C.c_void_p), ("length", C.c_void_p),
                ("points", C.c_void_p), ("point_count", C.c_void_p), ("overflow", C.c_void_p)]


class RolloutPointsDesc(C.Structure):
    """struct frirl_hip_rollout_points_desc (include/frirl_hip.h)."""
    _fields_ = [("n", C.c_int32), ("cap", C.c_int32), ("only_successful", C.c_int32), ("reserved", C.c_int32), ("start_states", C.c_void_p),
                ("row_count", C.c_void_p), ("active", C.c_void_p), ("points", C.c_void_p), ("point_count", C.c_void_p), ("overflow", C.c_void_p),
                ("steps", C.c_void_p), ("reward", C.c_void_p), ("success", C.c_void_p)]


class ReduceMapTotals(C.Structure):
    """struct frirl_hip_reduce_map_totals (include/frirl_hip.h)."""
    _fields_ = [("agents_reduced", C.c_int32), ("agents_overflow", C.c_int32), ("agents_without_points", C.c_int32), ("reserved", C.c_int32),
                ("rules_before", C.c_int64), ("rules_after", C.c_int64), ("points", C.c_int64)]


POINTS_MAX_CAP = 512


class AgentIO(C.Structure):
    """struct frirl_hip_agent_io (include/frirl_hip.h)."""
    _fields_ = [("obs", C.c_void_p), ("q_obs", C.c_void_p), ("reward", C.c_void_p), ("success", C.c_void_p), ("reset", C.c_void_p),
                ("action_out", C.c_void_p), ("action_idx", C.c_void_p)]


class DemonstrationDesc(C.Structure):
    """struct frirl_hip_demonstration (include/frirl_hip.h)."""
    _fields_ = [("T", C.c_int32), ("agent_stride", C.c_int64), ("obs", C.c_void_p), ("q_obs", C.c_void_p), ("action", C.c_void_p),
                ("reward", C.c_void_p), ("success", C.c_void_p), ("start", C.c_void_p), ("length", C.c_void_p)]


class PolicyRowsDesc(C.Structure):
    """struct frirl_hip_policy_rows (include/frirl_hip.h)."""
    _fields_ = [("Q", C.c_int32), ("done", C.c_void_p), ("ep_steps", C.c_void_p), ("success", C.c_void_p), ("ep_reward", C.c_void_p),
                ("exclude_mask", C.c_void_p), ("rule_slot", C.c_void_p)]


class PolicyBatchRowsDesc(C.Structure):
    """struct frirl_hip_policy_batch_rows (include/frirl_hip.h)."""
    _fields_ = [("n", C.c_int32), ("done", C.c_void_p), ("ep_steps", C.c_void_p), ("success", C.c_void_p), ("ep_reward", C.c_void_p),
                ("row_count", C.c_void_p), ("step_cap", C.c_void_p), ("agents", C.c_void_p), ("nagents", C.c_int32),
                ("exclude_mask", C.c_void_p), ("rule_slot", C.c_void_p), ("rows_live", C.c_void_p)]


class ConvergenceDesc(C.Structure):
    """struct frirl_hip_convergence (include/frirl_hip.h)."""
    _fields_ = [("prev_nrules", C.c_void_p), ("prev_steps", C.c_void_p), ("prev_reward", C.c_void_p), ("prev_rconc", C.c_void_p),
                ("converged", C.c_void_p), ("episodes", C.c_void_p), ("epended", C.c_void_p)]


_lib = None
_DP = C.POINTER(C.c_double)
LEARN_CHUNK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32)      # frirl_hip_learn_chunk_fn

# The entry points that come in levels: base (level 0), base_rows, base_explore, base_target, base_expect take the first 0 .. 4 of the
# per-agent structs between the agent and the rest of their arguments.
_HEAD = [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc)]
_ROW_STRUCTS = [HparamRowsDesc, ExploreRowsDesc, TargetRowsDesc, ExpectRowsDesc]
_SUFFIX = ("", "_rows", "_explore", "_target", "_expect")
_LEARN_RUN_TAIL = [C.POINTER(EnvsDesc), C.POINTER(ConvergenceDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                   C.c_void_p]
_LEARN_TRAIN_TAIL = [C.POINTER(EnvsDesc), C.POINTER(ConvergenceDesc), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                     C.POINTER(C.c_int32), LEARN_CHUNK_FN, C.c_void_p, C.c_void_p]
_AGENT_TAIL = [C.POINTER(EnvsDesc), C.POINTER(AgentIO), C.c_void_p]                    # ..., stream
_TAUGHT_TAIL = [C.POINTER(EnvsDesc), C.POINTER(AgentIO), C.c_void_p, C.c_void_p]      # ..., teacher, stream


def _levels(base, tail, levels=range(5)):
    return {base + _SUFFIX[n]: (C.c_int, _HEAD + [C.POINTER(s) for s in _ROW_STRUCTS[:n]] + tail) for n in levels}


# name -> (restype, argtypes); every symbol include/frirl_hip.h declares
SIGNATURES = {
    "frirl_hip_version": (C.c_char_p, []),
    "frirl_hip_last_error": (C.c_char_p, []),
    "frirl_hip_device_count": (C.c_int, []),
    "frirl_hip_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "frirl_hip_set_option": (C.c_int, [C.c_char_p, C.c_int]),
    "frirl_hip_get_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "five_hip_rule_distance_uses_uidx": (C.c_int, [C.c_int32, C.c_int32]),
    "frirl_hip_step_uses_uidx": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "five_hip_rule_distance": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "five_hip_rule_distance_packed_words": (C.c_int, [C.c_int32, C.c_int32]),
    "frirl_hip_pack_indices": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_void_p, C.c_void_p]),
    "five_hip_rule_distance_packed": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "five_hip_rule_distance_packed_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "five_hip_rule_distance_packed_ws": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "five_hip_rule_distance_coded_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "frirl_hip_pack_codes": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "five_hip_rule_distance_coded_ws": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "five_hip_sqrt_unscaled_check": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "five_hip_rule_distance_sq_guard": (C.c_int, [C.POINTER(Tables), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "five_hip_vag_concl": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "five_hip_vag_concl_weight": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frirl_hip_get_best_action": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "five_hip_shepard_weight_check": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "frirl_hip_explore_check": (C.c_int, [C.POINTER(AgentDesc), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "five_hip_vag_concl_shared": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frirl_hip_get_best_action_shared": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_int,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "frirl_hip_rollout_shared": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_int32, C.POINTER(RolloutDesc), C.c_void_p]),
    "frirl_hip_rollout_batch_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_rollout_batch": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(RolloutBatchDesc), C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "frirl_hip_rollout_record": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(RolloutLogDesc), C.c_void_p]),
    "frirl_hip_reduce_shared": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_void_p, C.c_int, C.c_double, C.c_int,
                                          C.POINTER(C.c_int32), C.POINTER(ReduceResult), C.c_void_p]),
    "frirl_hip_reduce_batch_depth": (C.c_int, [C.c_int32, C.c_int32]),
    "frirl_hip_reduce_batch_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_reduce_batch": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_double, C.c_int, C.POINTER(C.c_int32), C.POINTER(ReduceResult), C.c_void_p, C.c_size_t, C.c_void_p]),
    "frirl_hip_reduce_walk_check": (C.c_int, [C.c_int, C.POINTER(C.c_int32), _DP, C.c_int, C.c_double, C.c_double, C.c_double,
                                              C.POINTER(C.c_uint32), _DP]),
    "frirl_hip_reduce_batch_starts_depth": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_reduce_batch_starts_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_reduce_batch_starts": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_void_p, C.POINTER(ReduceStarts),
                                                C.c_void_p, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int32), C.POINTER(ReduceResult),
                                                C.POINTER(ReduceStartResult), C.c_void_p, C.c_size_t, C.c_void_p]),
    "frirl_hip_reduce_walk_starts_check": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), _DP, C.POINTER(C.c_int32), _DP, C.c_double, C.c_double,
                                                     C.POINTER(C.c_uint32)]),
    "frirl_hip_reduce_walk_starts_rows_check": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _DP, C.POINTER(C.c_int32),
                                                          _DP, C.c_double, C.c_double, C.POINTER(C.c_uint32)]),
    "frirl_hip_policy_map_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_policy_map": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(MapPoints), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "frirl_hip_reduce_batch_map_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_reduce_batch_map": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_void_p, C.POINTER(MapPoints), C.c_int,
                                             C.POINTER(C.c_int32), C.POINTER(ReduceMapResult), C.c_void_p, C.c_size_t, C.c_void_p]),
    "frirl_hip_rule_usage_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_rule_usage": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(MapPoints), C.POINTER(RuleUsageOut),
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "frirl_hip_rule_order": (C.c_int, [C.POINTER(RuleBases), C.c_int32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frirl_hip_reduce_batch_map_orders_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_reduce_batch_map_orders": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_void_p, C.POINTER(MapPoints), C.c_int32,
                                                    C.c_void_p, C.POINTER(C.c_int32), C.POINTER(ReduceOrdersResult), C.POINTER(C.c_int32), C.c_void_p,
                                                    C.c_size_t, C.c_void_p]),
    "frirl_hip_log_points_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_log_points": (C.c_int, [C.POINTER(LogPointsDesc), C.c_void_p, C.c_size_t, C.c_void_p]),
    "frirl_hip_rollout_points_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_rollout_points": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(RolloutPointsDesc), C.c_void_p,
                                           C.c_size_t, C.c_void_p]),
    "frirl_hip_lanes_preferred": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_lanes_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_episode_run_lanes": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(EnvsDesc), C.c_int32,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
    "frirl_hip_rollout_resident_rules": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_learn_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "frirl_hip_learn_plan": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "frirl_hip_learn_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    **_levels("frirl_hip_learn_run", _LEARN_RUN_TAIL),
    "frirl_hip_learn_train_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    **_levels("frirl_hip_learn_train", _LEARN_TRAIN_TAIL),
    "five_hip_add_rule": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "frirl_hip_update_sarsa": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(EnvsDesc), C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frirl_hip_env_step": (C.c_int, [C.POINTER(AgentDesc), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "frirl_hip_episode_begin": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(EnvsDesc), C.c_void_p]),
    "frirl_hip_episode_step": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(EnvsDesc), C.c_void_p]),
    "frirl_hip_episode_steps": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(EnvsDesc), C.c_int32, C.c_void_p]),
    **_levels("frirl_hip_agent_begin", _AGENT_TAIL, [0]), "frirl_hip_agent_begin_taught": (C.c_int, _HEAD + _TAUGHT_TAIL),
    **_levels("frirl_hip_agent_begin", _TAUGHT_TAIL, [1, 2]),              # begin performs no update: no _begin_target
    **_levels("frirl_hip_agent_observe", _AGENT_TAIL, [0]), "frirl_hip_agent_observe_taught": (C.c_int, _HEAD + _TAUGHT_TAIL),
    **_levels("frirl_hip_agent_observe", _TAUGHT_TAIL, [1, 2, 3, 4]),
    "frirl_hip_learn_demonstration": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(EnvsDesc),
                                                C.POINTER(DemonstrationDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frirl_hip_policy_begin": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(PolicyRowsDesc), C.POINTER(AgentIO), C.c_void_p]),
    "frirl_hip_policy_observe": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(PolicyRowsDesc), C.POINTER(AgentIO),
                                           C.c_void_p]),
    "frirl_hip_reducer_create": (C.c_void_p, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_void_p, C.c_int, C.c_double, C.c_int,
                                              C.c_void_p]),
    "frirl_hip_reducer_next_round": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "frirl_hip_reducer_begin": (C.c_int, [C.c_void_p, C.POINTER(AgentIO)]),
    "frirl_hip_reducer_observe": (C.c_int, [C.c_void_p, C.POINTER(AgentIO), C.POINTER(C.c_int32)]),
    "frirl_hip_reducer_end_round": (C.c_int, [C.c_void_p]),
    "frirl_hip_reducer_result": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(ReduceResult)]),
    "frirl_hip_reducer_destroy": (None, [C.c_void_p]),
    "frirl_hip_policy_batch_begin": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(PolicyBatchRowsDesc),
                                               C.POINTER(AgentIO), C.c_void_p]),
    "frirl_hip_policy_batch_observe": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(PolicyBatchRowsDesc),
                                                 C.POINTER(AgentIO), C.c_void_p]),
    "frirl_hip_batch_reducer_create": (C.c_void_p, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_double, C.c_int, C.c_void_p]),
    "frirl_hip_batch_reducer_next_round": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "frirl_hip_batch_reducer_begin": (C.c_int, [C.c_void_p, C.POINTER(AgentIO)]),
    "frirl_hip_batch_reducer_observe": (C.c_int, [C.c_void_p, C.POINTER(AgentIO), C.POINTER(C.c_int32)]),
    "frirl_hip_batch_reducer_end_round": (C.c_int, [C.c_void_p]),
    "frirl_hip_batch_reducer_result": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(ReduceResult)]),
    "frirl_hip_batch_reducer_row_done": (C.c_void_p, [C.c_void_p]),
    "frirl_hip_batch_reducer_destroy": (None, [C.c_void_p]),
    "frirl_hip_batch_reducer_create_starts": (C.c_void_p, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_void_p, C.c_void_p,
                                                           C.POINTER(ReduceStarts), C.c_int, C.c_double, C.c_int, C.c_void_p]),
    "frirl_hip_batch_reducer_result_starts": (C.c_int, [C.c_void_p, C.POINTER(ReduceStartResult)]),
    "frirl_hip_batch_reducer_starts": (C.c_int, [C.c_void_p]),
    "frirl_hip_episode_run": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.POINTER(EnvsDesc), C.c_int32, C.c_int32, C.c_void_p]),
    "frirl_hip_convergence_init": (C.c_int, [C.POINTER(RuleBases), C.c_int, C.POINTER(ConvergenceDesc), C.c_void_p]),
    "frirl_hip_convergence_update": (C.c_int, [C.POINTER(RuleBases), C.c_int, C.POINTER(AgentDesc), C.POINTER(EnvsDesc), C.POINTER(ConvergenceDesc),
                                               C.c_void_p]),
    "frirl_hip_convergence_refresh": (C.c_int, [C.POINTER(RuleBases), C.c_int, C.POINTER(ConvergenceDesc), C.c_void_p]),
    "five_hip_bestact": (C.c_int, [C.POINTER(RuleBases), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # library-owned batch with host descriptors (C-level many-agent runner)
    "frirl_hip_batch_create": (C.c_void_p, [C.c_void_p]),
    "frirl_hip_batch_destroy": (None, [C.c_void_p]),
    "frirl_hip_batch_episode": (C.c_int, [C.c_void_p]),
    "frirl_hip_batch_train": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "frirl_hip_batch_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "frirl_hip_batch_agent_report": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _DP]),
    "frirl_hip_batch_set_hparams": (C.c_int, [C.c_void_p, C.POINTER(HparamRowsDesc)]),
    "frirl_hip_hparam_rows_check": (C.c_int, [C.POINTER(HparamRowsDesc), C.c_int32, C.POINTER(AgentDesc)]),
    "frirl_hip_batch_set_exploration": (C.c_int, [C.c_void_p, C.POINTER(ExploreRowsDesc)]),
    "frirl_hip_explore_rows_check": (C.c_int, [C.POINTER(ExploreRowsDesc), C.c_int32, C.POINTER(AgentDesc)]),
    "frirl_hip_explore_epsilon": (C.c_double, [C.c_double, C.c_int32, C.c_uint32]),
    "frirl_hip_batch_set_target": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "frirl_hip_batch_get_target": (C.c_int, [C.c_void_p, C.c_void_p]),
    "frirl_hip_target_rows_check": (C.c_int, [C.POINTER(TargetRowsDesc), C.c_int32]),
    "frirl_hip_batch_set_expected": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "frirl_hip_batch_get_expected": (C.c_int, [C.c_void_p, C.c_void_p]),
    "frirl_hip_expect_rows_check": (C.c_int, [C.POINTER(ExpectRowsDesc), C.c_int32]),
    "frirl_hip_batch_get_rulebase": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), _DP, _DP]),
    "frirl_hip_batch_save_rulebases": (C.c_int, [C.c_void_p, C.c_char_p]),
    "frirl_hip_batch_load_rulebases": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int32)]),
    "frirl_hip_batch_reduce": (C.c_int, [C.c_void_p, C.c_int32, C.c_int, C.c_double, C.c_int, C.POINTER(ReduceResult)]),
    "frirl_hip_batch_reduce_all": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.POINTER(ReduceResult), C.POINTER(C.c_int32)]),
    "frirl_hip_batch_reduce_all_starts": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int32, _DP, C.c_int, C.POINTER(ReduceResult),
                                                    C.POINTER(ReduceStartResult), C.POINTER(C.c_int32)]),
    "frirl_hip_batch_reduce_all_map": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, _DP, C.c_int, C.c_int32, C.POINTER(ReduceMapResult),
                                                 C.POINTER(ReduceMapTotals)]),
    "frirl_hip_batch_reduce_all_map_orders": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, _DP, C.c_int, C.c_int32, C.POINTER(ReduceOrdersResult),
                                                        C.POINTER(C.c_int32), C.POINTER(ReduceMapTotals)]),
    "frirl_hip_batch_evaluate": (C.c_int, [C.c_void_p, C.c_int32, _DP, C.POINTER(RolloutScore), C.POINTER(C.c_int32)]),
    "frirl_hip_batch_teach": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _DP, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(TeachResult)]),
    "frirl_hip_clone_agents": (C.c_int, [C.POINTER(RuleBases), C.c_int32, C.POINTER(EnvsDesc), C.POINTER(ConvergenceDesc), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "frirl_hip_select_plan": (C.c_int, [C.POINTER(RolloutScore), C.c_int32, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]),
    "frirl_hip_batch_clone": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32)]),
    "frirl_hip_batch_select": (C.c_int, [C.c_void_p, C.c_int32, _DP, C.c_int32, C.c_int32, C.c_int, C.POINTER(RolloutScore), C.POINTER(C.c_int32),
                                         C.POINTER(SelectResult)]),
    "frirl_hip_select_plan_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "frirl_hip_perturb_spec_check": (C.c_int, [C.POINTER(PerturbSpec)]),
    "frirl_hip_perturb_column_name": (C.c_char_p, [C.c_int32]),
    "frirl_hip_perturb_rows": (C.c_int, [C.POINTER(PerturbSpec), C.c_uint32, C.c_int32, C.c_void_p, C.POINTER(HparamRowsDesc), C.POINTER(ExploreRowsDesc),
                                         C.POINTER(TargetRowsDesc), C.POINTER(ExpectRowsDesc), C.c_void_p, C.c_void_p]),
    "frirl_hip_batch_evolve_step": (C.c_int, [C.c_void_p, C.c_int32, _DP, C.c_int32, C.c_int32, C.c_int, C.POINTER(PerturbSpec), C.POINTER(EvolveResult)]),
    "frirl_hip_batch_evolve": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _DP, C.c_int32, C.c_int32, C.c_int, C.POINTER(PerturbSpec),
                                         C.POINTER(EvolveResult)]),
    "frirl_hip_batch_evolve_best_score": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), _DP]),
    "frirl_hip_batch_get_hparams": (C.c_int, [C.c_void_p, C.POINTER(HparamRowsDesc)]),
    "frirl_hip_batch_get_exploration": (C.c_int, [C.c_void_p, C.POINTER(ExploreRowsDesc)]),
    "frirl_hip_batch_merge_round": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "frirl_hip_batch_train_merged": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "frirl_hip_merge_rb": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.POINTER(AgentDesc), C.c_void_p, C.POINTER(SenderDesc), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "frirl_hip_weights_from_spread": (C.c_int, [C.POINTER(Tables), C.POINTER(RuleBases), C.c_int, C.POINTER(EnvsDesc), C.c_void_p, C.c_void_p]),
    "frirl_hip_gen_def_states": (C.c_int, [_DP, C.c_int32, C.c_int32, C.c_int32, _DP, _DP]),
    # several GPUs from plain C (one batch + host thread per device, RCCL all-reduce of the report)
    "frirl_hip_shard": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "frirl_hip_multi_create": (C.c_void_p, [C.c_void_p, C.c_int64, C.c_int32]),
    "frirl_hip_multi_destroy": (None, [C.c_void_p]),
    "frirl_hip_multi_train": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "frirl_hip_multi_train_merged": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "frirl_hip_multi_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "frirl_hip_multi_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "frirl_hip_multi_get_rulebase": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), _DP, _DP]),
    # single rule base, host pointers (what the ANSI-C drop-in library calls)
    "five_hip_mirror_create": (C.c_void_p, [C.c_int32, C.c_int32, _DP, _DP, C.c_int32, C.c_int32]),
    "five_hip_mirror_destroy": (None, [C.c_void_p]),
    "five_hip_mirror_upload": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(_DP), _DP]),
    "five_hip_mirror_add_rule": (C.c_int, [C.c_void_p, _DP, C.c_double]),
    "five_hip_mirror_remove_rule": (C.c_int, [C.c_void_p, C.c_uint32]),
    "five_hip_mirror_set_rconc": (C.c_int, [C.c_void_p, _DP, C.c_int32]),
    "five_hip_mirror_get_rconc": (C.c_int, [C.c_void_p, _DP, C.c_int32]),
    "five_hip_mirror_numofrules": (C.c_int32, [C.c_void_p]),
    "five_hip_mirror_rule_distance": (C.c_int, [C.c_void_p, _DP, _DP, C.POINTER(C.c_uint32)]),
    "five_hip_mirror_vag_concl": (C.c_int, [C.c_void_p, _DP, _DP, C.POINTER(C.c_uint32)]),
    "five_hip_mirror_vag_concl_weight": (C.c_int, [C.c_void_p, _DP, _DP, C.POINTER(C.c_uint32)]),
    "five_hip_mirror_bestact": (C.c_int, [C.c_void_p, _DP, _DP]),
    "five_hip_mirror_get_best_action": (C.c_int, [C.c_void_p, _DP, _DP, C.c_int32, _DP, C.POINTER(C.c_uint32)]),
    "five_hip_mirror_greedy_step": (C.c_int, [C.c_void_p, C.POINTER(AgentDesc), _DP, C.c_double, _DP, _DP, _DP, C.c_int32, C.POINTER(C.c_uint32), _DP, _DP,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), _DP, _DP, _DP]),
    "five_hip_mirror_update_sarsa": (C.c_int, [C.c_void_p, C.POINTER(AgentDesc), _DP, C.c_double, _DP, C.POINTER(C.c_int32),
                                               C.POINTER(C.c_int32), _DP, _DP, _DP]),
}


def build(force=False, verbose=False):
    import importlib.util
    spec = importlib.util.spec_from_file_location("frirl_amd_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_all(force=force, verbose=verbose)


def lib():
    """The loaded C-ABI library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise FrirlHipError(f"{HIP_LIB_PATH} is missing: run `python __graft_entry__.py` (build()) first; "
                                "the FRIRL hot path has no CPU fallback")
        # One HIP runtime per process: torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Loaded
        # first, it satisfies this library's NEEDED entry, so kernels, streams and events all live in the
        # runtime torch uses.  (A plain C host links /opt/rocm's runtime and never sees torch.)
        import torch  # noqa: F401
        L = C.CDLL(HIP_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)      # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise FrirlHipError(f"{what}: rc={rc}: {lib().frirl_hip_last_error().decode()}")


def set_option(name, value):
    """frirl_hip_set_option: experiment / test switch (e.g. "no_uidx", "lanes_slices"); returns the previous value."""
    old = C.c_int()
    check(lib().frirl_hip_get_option(name.encode(), C.byref(old)), "frirl_hip_get_option")
    check(lib().frirl_hip_set_option(name.encode(), int(value)), "frirl_hip_set_option")
    return old.value


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _scratch(nbytes, device, stream):
    """A workspace for ONE asynchronous call that is dropped when the wrapper returns: allocated on the current stream and, where the
    call runs on another one, recorded on it, so that the caching allocator does not hand the block out again while the kernel uses it."""
    import torch
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=device)
    if stream is not None:
        ws.record_stream(stream)
    return ws


class Problem:
    """Device-resident tables + E rule bases (torch tensors own the HBM; the C ABI gets raw pointers)."""

    def __init__(self, u, ve, rb, nrules, uidx=None):
        """uidx: optional int16 tensor [E, nant, maxR] holding the 16-bit universe indices of the antecedents
        (frirl_hip_rulebases.uidx): the compressed mirror the scans stream instead of the f64 columns."""
        import torch
        assert u.is_cuda and ve.is_cuda and rb.is_cuda and nrules.is_cuda
        assert u.dtype == torch.float64 and ve.dtype == torch.float64 and rb.dtype == torch.float64 and nrules.dtype == torch.int32
        self.nant, self.U = u.shape
        self.E, cols, self.maxR = rb.shape
        assert cols == self.nant + 1 and ve.shape == u.shape and nrules.shape == (self.E,)
        self.u, self.ve, self.rb, self.nrules = u.contiguous(), ve.contiguous(), rb.contiguous(), nrules.contiguous()
        self.uidx = None
        if uidx is not None:
            assert uidx.is_cuda and uidx.dtype == torch.int16 and uidx.shape == (self.E, self.nant, self.maxR) and self.U <= 32767
            self.uidx = uidx.contiguous()
        self.tables = Tables(self.nant, self.U, self.u.data_ptr(), self.ve.data_ptr())
        self._bases = RuleBases(self.E, self.maxR, self.rb.data_ptr(), self.nrules.data_ptr(),
                                self.uidx.data_ptr() if self.uidx is not None else None)
        # packed copy of the index mirror (6-bit fields, five_hip_rule_distance_packed) for the shapes that form serves: derived
        # data, repacked before the next scan whenever uidx may have changed (see `bases` and _pidx_current)
        self.pidx = None
        self._pidx_key = None
        W = lib().five_hip_rule_distance_packed_words(self.nant, self.U) if self.uidx is not None else 0
        if W > 0:
            self.pidx = torch.empty((self.E, W, self.maxR), dtype=torch.int32, device=self.uidx.device)
            self._pack(None)
        # coded copy (3-byte lane-tiled codes, five_hip_rule_distance_coded_ws) beside pidx, where the rule bases' dictionaries allow
        # it: derived from uidx AND nrules, rebuilt with its dictionaries whenever either may have changed (_codes_current)
        self.codes = self._code_dict = self._code_rank = self._code_d = None
        self._codes_key = None
        if self.pidx is not None and self.nant <= 5:
            self._pack_codes(None)
        # workspaces of five_hip_rule_distance_packed_ws (per-call squared-difference tables), one per stream the scan is called on:
        # calls on different streams may run at the same time and must not share one
        self._rd_ws = {}
        self._ro_ws = {}          # workspaces of frirl_hip_rollout_batch, per stream as _rd_ws

    @property
    def bases(self):
        """The frirl_hip_rulebases handle for native calls.  Any of them may append, merge or compact rules (uidx changes
        under the packed mirror), so handing it out marks the mirror stale; the read-only scans below use the private one.
        Take it afresh for every native call: a handle kept across a rule_distance would escape the staleness mark."""
        self._pidx_key = None
        self._codes_key = None
        return self._bases

    def _pack(self, stream):
        check(lib().frirl_hip_pack_indices(C.byref(self.tables), C.byref(self._bases), _ptr(self.pidx), _stream(stream)),
              "frirl_hip_pack_indices")
        self._pidx_key = (self.uidx.data_ptr(), self.uidx._version)

    def _pidx_current(self, stream):
        """The packed mirror, repacked on `stream` first if uidx was handed to native code (bases) or edited in place since."""
        if self._pidx_key != (self.uidx.data_ptr(), self.uidx._version):
            self._pack(stream)
        return self.pidx

    def _pack_codes(self, stream):
        """Dictionaries of the coded copy from uidx and nrules (torch ops on `stream`'s device, one host read of their lengths) and the
        copy itself (frirl_hip_pack_codes); codes = None where the coded form does not apply."""
        import torch
        dev = self.uidx.device
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            nr = self.nrules.to(torch.int64)
            upto = (nr + (nr & 1)).clamp(max=self.maxR)                  # the odd last rule's partner column is scanned like a rule
            cols = torch.arange(self.maxR, device=dev)
            dimoff = (65 * torch.arange(self.nant, device=dev)).view(1, self.nant, 1)
            counts = torch.zeros((self.nant * 65,), dtype=torch.int64, device=dev)
            step = max(1, (1 << 26) // (self.nant * self.maxR))          # environments per pass: bounds the temporaries
            for e0 in range(0, self.E, step):
                v = self.uidx[e0:e0 + step].to(torch.int64) & 63
                live = (cols.view(1, -1) < upto[e0:e0 + step].view(-1, 1)).unsqueeze(1)
                v = torch.where(live, v, torch.full_like(v, 64)) + dimoff
                counts += torch.bincount(v.flatten(), minlength=self.nant * 65)
            present = counts.view(self.nant, 65)[:, :64] > 0
            rank = (present.cumsum(1) - 1).clamp(min=0).to(torch.uint8).contiguous()
            idx = torch.arange(64, device=dev).expand(self.nant, 64)
            dct = torch.where(present, idx, torch.full_like(idx, 255)).sort(1).values.to(torch.uint8).contiguous()
            d = present.sum(1).clamp(min=1).to(torch.int32).cpu().tolist()        # the one host read
        darr = (C.c_int32 * self.nant)(*d)
        n = lib().five_hip_rule_distance_coded_bytes(self.nant, self.U, self.E, self.maxR, darr)
        if n:
            if self.codes is None or self.codes.numel() != n:
                self.codes = torch.empty((n,), dtype=torch.uint8, device=dev)
            self._code_dict, self._code_rank, self._code_d = dct, rank, darr
            check(lib().frirl_hip_pack_codes(C.byref(self.tables), C.byref(self._bases), _ptr(rank), darr, _ptr(self.codes), _stream(stream)),
                  "frirl_hip_pack_codes")
        else:
            self.codes = self._code_dict = self._code_rank = self._code_d = None
        self._codes_key = (self.uidx.data_ptr(), self.uidx._version, self.nrules.data_ptr(), self.nrules._version)

    def _codes_current(self, stream):
        """The coded copy (or None), rebuilt on `stream` first if uidx or nrules were handed to native code (bases) or edited in place since."""
        if self.nant <= 5 and self._codes_key != (self.uidx.data_ptr(), self.uidx._version, self.nrules.data_ptr(), self.nrules._version):
            self._pack_codes(stream)
        return self.codes

    def _rd_workspace(self, stream):
        """The packed scan's workspace for `stream` (uint8 tensor, allocated on first use), or None for a shape without one."""
        import torch
        key = _stream(stream).value
        if key not in self._rd_ws:
            n = lib().five_hip_rule_distance_packed_workspace_bytes(self.nant, self.U, self.E)
            self._rd_ws[key] = torch.empty((n,), dtype=torch.uint8, device=self.pidx.device) if n else None
        return self._rd_ws[key]

    def rule_distance(self, x, ruledists=None, hit=None, materialise=True, stream=None):
        """five_hip_rule_distance (five_hip_rule_distance_packed_ws while the packed mirror exists): returns (ruledists [E,maxR]
        or None, hit [E] int32 with -1 = none)."""
        import torch
        assert x.is_cuda and x.dtype == torch.float64 and x.shape == (self.E, self.nant) and x.is_contiguous()
        if materialise and ruledists is None:
            ruledists = torch.empty((self.E, self.maxR), dtype=torch.float64, device=x.device)
        if hit is None:
            hit = torch.empty((self.E,), dtype=torch.int32, device=x.device)
        if self.pidx is not None and self._codes_current(stream) is not None:
            ws = self._rd_workspace(stream)
            rc = lib().five_hip_rule_distance_coded_ws(C.byref(self.tables), C.byref(self._bases), _ptr(self.codes), _ptr(self._code_dict), self._code_d,
                                                       _ptr(self._pidx_current(stream)), _ptr(x), _ptr(ruledists) if materialise else None,
                                                       _ptr(hit), _ptr(ws), ws.numel() if ws is not None else 0, _stream(stream))
            check(rc, "five_hip_rule_distance_coded_ws")
        elif self.pidx is not None:
            ws = self._rd_workspace(stream)
            rc = lib().five_hip_rule_distance_packed_ws(C.byref(self.tables), C.byref(self._bases), _ptr(self._pidx_current(stream)), _ptr(x),
                                                        _ptr(ruledists) if materialise else None, _ptr(hit), _ptr(ws),
                                                        ws.numel() if ws is not None else 0, _stream(stream))
            check(rc, "five_hip_rule_distance_packed_ws")
        else:
            rc = lib().five_hip_rule_distance(C.byref(self.tables), C.byref(self._bases), _ptr(x),
                                              _ptr(ruledists) if materialise else None, _ptr(hit), _stream(stream))
            check(rc, "five_hip_rule_distance")
        return (ruledists if materialise else None), hit

    def vag_concl(self, x, p=0, stream=None):
        """five_hip_vag_concl: (conc [E] float64, hit [E] int32 with -1 = interpolated)."""
        import torch
        assert x.is_cuda and x.dtype == torch.float64 and x.shape == (self.E, self.nant) and x.is_contiguous()
        conc = torch.empty((self.E,), dtype=torch.float64, device=x.device)
        hit = torch.empty((self.E,), dtype=torch.int32, device=x.device)
        check(lib().five_hip_vag_concl(C.byref(self.tables), C.byref(self._bases), p, _ptr(x), _ptr(conc), _ptr(hit), _stream(stream)),
              "five_hip_vag_concl")
        return conc, hit

    def vag_concl_weight(self, x, p=0, weights=None, stream=None):
        """five_hip_vag_concl_weight: (weights [E,maxR], hit [E]); rows of exact-hit environments are untouched."""
        import torch
        assert x.is_cuda and x.dtype == torch.float64 and x.shape == (self.E, self.nant) and x.is_contiguous()
        if weights is None:
            weights = torch.full((self.E, self.maxR), float("nan"), dtype=torch.float64, device=x.device)
        hit = torch.empty((self.E,), dtype=torch.int32, device=x.device)
        check(lib().five_hip_vag_concl_weight(C.byref(self.tables), C.byref(self._bases), p, _ptr(x), _ptr(weights), _ptr(hit),
                                              _stream(stream)), "five_hip_vag_concl_weight")
        return weights, hit

    def get_best_action(self, states, action_ve, p=0, stream=None):
        """frirl_hip_get_best_action: (actconc [E,A], best [E] int32)."""
        import torch
        assert states.is_cuda and states.dtype == torch.float64 and states.shape == (self.E, self.nant - 1) and states.is_contiguous()
        A = action_ve.numel()
        actconc = torch.empty((self.E, A), dtype=torch.float64, device=states.device)
        best = torch.empty((self.E,), dtype=torch.int32, device=states.device)
        check(lib().frirl_hip_get_best_action(C.byref(self.tables), C.byref(self._bases), p, _ptr(states), _ptr(action_ve), A,
                                              _ptr(actconc), _ptr(best), _stream(stream)), "frirl_hip_get_best_action")
        return actconc, best

    def vag_concl_shared(self, x, p=0, stream=None):
        """five_hip_vag_concl_shared: Q observations against this ONE rule base (E == 1)."""
        import torch
        assert self.E == 1 and x.is_cuda and x.dtype == torch.float64 and x.shape[1] == self.nant and x.is_contiguous()
        Q = x.shape[0]
        conc = torch.empty((Q,), dtype=torch.float64, device=x.device)
        hit = torch.empty((Q,), dtype=torch.int32, device=x.device)
        check(lib().five_hip_vag_concl_shared(C.byref(self.tables), C.byref(self._bases), p, Q, _ptr(x), _ptr(conc), _ptr(hit), _stream(stream)),
              "five_hip_vag_concl_shared")
        return conc, hit

    def get_best_action_shared(self, states, action_ve, p=0, stream=None):
        """frirl_hip_get_best_action_shared: Q states against this ONE rule base (E == 1)."""
        import torch
        assert self.E == 1 and states.is_cuda and states.dtype == torch.float64 and states.shape[1] == self.nant - 1 and states.is_contiguous()
        Q, A = states.shape[0], action_ve.numel()
        actconc = torch.empty((Q, A), dtype=torch.float64, device=states.device)
        best = torch.empty((Q,), dtype=torch.int32, device=states.device)
        check(lib().frirl_hip_get_best_action_shared(C.byref(self.tables), C.byref(self._bases), p, Q, _ptr(states), _ptr(action_ve), A, _ptr(actconc),
                                                     _ptr(best), _stream(stream)), "frirl_hip_get_best_action_shared")
        return actconc, best

    def rollout_shared(self, agent, Q, start_states=None, exclude_mask=None, rule_slot=None, stream=None):
        """frirl_hip_rollout_shared: Q greedy roll-outs (frirl_test_run's episode) on this ONE rule base (E == 1).
        Returns (steps[Q] i32, reward[Q] f64, success[Q] i32, final_states[Q][nant-1])."""
        import torch
        dev_ = self.rb.device
        assert self.E == 1
        ro = RolloutDesc()
        steps = torch.empty((Q,), dtype=torch.int32, device=dev_)
        reward = torch.empty((Q,), dtype=torch.float64, device=dev_)
        success = torch.empty((Q,), dtype=torch.int32, device=dev_)
        final = torch.empty((Q, self.nant - 1), dtype=torch.float64, device=dev_)
        if start_states is not None:
            assert start_states.shape == (Q, self.nant - 1) and start_states.dtype == torch.float64 and start_states.is_contiguous()
            ro.start_states = _ptr(start_states)
        if exclude_mask is not None:
            assert exclude_mask.shape == (Q,) and exclude_mask.dtype == torch.int32 and rule_slot.dtype == torch.uint8 and rule_slot.numel() == self.maxR
            ro.exclude_mask, ro.rule_slot = _ptr(exclude_mask), _ptr(rule_slot)
        ro.steps, ro.reward, ro.success, ro.final_states = _ptr(steps), _ptr(reward), _ptr(success), _ptr(final)
        check(lib().frirl_hip_rollout_shared(C.byref(self.tables), C.byref(self.bases), C.byref(agent.desc), Q, C.byref(ro), _stream(stream)),
              "frirl_hip_rollout_shared")
        return steps, reward, success, final

    def _ro_workspace(self, n, A, stream):
        """The batched roll-out's workspace for `stream` (uint8 tensor, grown when a call needs more)."""
        import torch
        key = _stream(stream).value
        need = lib().frirl_hip_rollout_batch_workspace_bytes(self.nant, self.E, self.maxR, n, A)
        ws = self._ro_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ro_ws[key] = torch.empty((max(need, 16),), dtype=torch.uint8, device=self.rb.device)
        return ws, need

    def rollout_batch(self, agent, n, start_states=None, row_count=None, step_cap=None, active=None, scores=False, stream=None, out=None):
        """frirl_hip_rollout_batch: n greedy roll-outs (frirl_test_run's episode) on EVERY rule base of this problem, row q = e * n + j on
        the rule base of agent e.  start_states [E * n, nant-1] f64 (None = agent.values_def); row_count / step_cap [E] int32; active [E]
        uint8 / bool.  Returns (steps [E*n] i32, reward [E*n] f64, success [E*n] i32, final_states [E*n, nant-1][, scores [E, 40] uint8:
        struct frirl_hip_rollout_score per agent, see rollout_scores]).  out: the caller's (steps, reward, success, final_states) to write
        into.  Does not synchronise."""
        import torch
        dev_ = self.rb.device
        Q = self.E * n
        if out is None:
            out = (torch.empty((Q,), dtype=torch.int32, device=dev_), torch.empty((Q,), dtype=torch.float64, device=dev_),
                   torch.empty((Q,), dtype=torch.int32, device=dev_), torch.empty((Q, self.nant - 1), dtype=torch.float64, device=dev_))
        steps, reward, success, final = out
        ro = RolloutBatchDesc()
        ro.n = n
        if start_states is not None:
            assert start_states.shape == (Q, self.nant - 1) and start_states.dtype == torch.float64 and start_states.is_contiguous()
            ro.start_states = _ptr(start_states)
        for x in (row_count, step_cap):
            assert x is None or (x.shape == (self.E,) and x.dtype == torch.int32 and x.is_contiguous())
        assert active is None or (active.shape == (self.E,) and active.dtype in (torch.uint8, torch.bool) and active.is_contiguous())
        ro.row_count, ro.step_cap, ro.active = _ptr(row_count), _ptr(step_cap), _ptr(active)
        ro.steps, ro.reward, ro.success, ro.final_states = _ptr(steps), _ptr(reward), _ptr(success), _ptr(final)
        sc = torch.empty((self.E, C.sizeof(RolloutScore)), dtype=torch.uint8, device=dev_) if scores else None
        ws, need = self._ro_workspace(n, agent.desc.A, stream)
        check(lib().frirl_hip_rollout_batch(C.byref(self.tables), C.byref(self._bases), C.byref(agent.desc), C.byref(ro), _ptr(sc), _ptr(ws), need,
                                            _stream(stream)), "frirl_hip_rollout_batch")
        return (steps, reward, success, final, sc) if scores else (steps, reward, success, final)

    def rollout_record(self, agent, n, episodes, T, start_states=None, row_count=None, active=None, stream=None, out=None):
        """frirl_hip_rollout_record: n logs of `episodes` greedy (or epsilon-greedy) episodes on EVERY rule base of this problem, every
        step written as a record; log q = e * n + j on the rule base of agent e.  start_states [E * n, episodes, nant-1] f64 (None =
        agent.values_def); row_count [E] int32; active [E] uint8 / bool.  Returns a RolloutLog (out: the caller's, to write into);
        its .demonstration() feeds learn_demonstration from the same memory.  Does not synchronise."""
        import torch
        Q, ns = self.E * n, self.nant - 1
        log = out if out is not None else RolloutLog.empty(Q, episodes, T, ns, self.rb.device)
        assert (log.Q, log.K, log.T, log.ns) == (Q, episodes, T, ns)
        lg = RolloutLogDesc()
        lg.n, lg.episodes, lg.T = n, episodes, T
        if start_states is not None:
            assert start_states.shape == (Q, episodes, ns) and start_states.dtype == torch.float64 and start_states.is_contiguous()
            lg.start_states = _ptr(start_states)
        assert row_count is None or (row_count.shape == (self.E,) and row_count.dtype == torch.int32 and row_count.is_contiguous())
        assert active is None or (active.shape == (self.E,) and active.dtype in (torch.uint8, torch.bool) and active.is_contiguous())
        lg.row_count, lg.active = _ptr(row_count), _ptr(active)
        for name in RolloutLog.FIELDS:
            setattr(lg, name, _ptr(getattr(log, name)))
        log.n = n
        check(lib().frirl_hip_rollout_record(C.byref(self.tables), C.byref(self._bases), C.byref(agent.desc), C.byref(lg), _stream(stream)),
              "frirl_hip_rollout_record")
        return log

    def rollout_points(self, agent, n, cap=POINTS_MAX_CAP, only_successful=False, start_states=None, row_count=None, active=None, stream=None,
                       out=None, rows_out=None):
        """frirl_hip_rollout_points: n roll-outs (one episode each) on EVERY rule base of this problem, row q = e * n + j on the rule base
        of agent e, keeping per agent the de-duplicated set of the points the policy was asked at -- the sets rollout_record(episodes=1,
        T=max_steps + 1) followed by RolloutLog.points gives, without the logs.  start_states [E * n, nant-1] f64 (None =
        agent.values_def); row_count [E] int32; active [E] uint8 / bool.  Returns (points [E, cap, ns] f64, point_count [E] int32,
        overflow [E] int32, steps [E*n] i32, reward [E*n] f64, success [E*n] i32); the order of a list is unspecified.  out: the caller's
        (points, point_count, overflow) to write into, else points comes zeroed; rows_out: the caller's (steps, reward, success).  Does
        not synchronise."""
        import torch
        dev_ = self.rb.device
        Q, ns = self.E * n, self.nant - 1
        if out is None:
            out = (torch.zeros((self.E, cap, ns), dtype=torch.float64, device=dev_), torch.empty((self.E,), dtype=torch.int32, device=dev_),
                   torch.empty((self.E,), dtype=torch.int32, device=dev_))
        if rows_out is None:
            rows_out = (torch.empty((Q,), dtype=torch.int32, device=dev_), torch.empty((Q,), dtype=torch.float64, device=dev_),
                        torch.empty((Q,), dtype=torch.int32, device=dev_))
        points, count, overflow = out
        steps, reward, success = rows_out
        assert points.shape == (self.E, cap, ns) and points.dtype == torch.float64 and points.is_contiguous()
        for x in (count, overflow):
            assert x.shape == (self.E,) and x.dtype == torch.int32 and x.is_contiguous()
        rp = RolloutPointsDesc()
        rp.n, rp.cap, rp.only_successful = n, cap, 1 if only_successful else 0
        if start_states is not None:
            assert start_states.shape == (Q, ns) and start_states.dtype == torch.float64 and start_states.is_contiguous()
            rp.start_states = _ptr(start_states)
        assert row_count is None or (row_count.shape == (self.E,) and row_count.dtype == torch.int32 and row_count.is_contiguous())
        assert active is None or (active.shape == (self.E,) and active.dtype in (torch.uint8, torch.bool) and active.is_contiguous())
        rp.row_count, rp.active = _ptr(row_count), _ptr(active)
        rp.points, rp.point_count, rp.overflow = _ptr(points), _ptr(count), _ptr(overflow)
        rp.steps, rp.reward, rp.success = _ptr(steps), _ptr(reward), _ptr(success)
        nbytes = lib().frirl_hip_rollout_points_workspace_bytes(self.nant, self.E, self.maxR, n, cap, agent.desc.A)
        ws = _scratch(nbytes, dev_, stream)
        check(lib().frirl_hip_rollout_points(C.byref(self.tables), C.byref(self._bases), C.byref(agent.desc), C.byref(rp), _ptr(ws), nbytes,
                                             _stream(stream)), "frirl_hip_rollout_points")
        return points, count, overflow, steps, reward, success

    def reduce_shared(self, agent, strategy, reward_tolerance=0.0, depth=0, rant=None, stream=None):
        """frirl_hip_reduce_shared: the reference's rule-base reduction as speculative batched try-remove; compacts this
        ONE rule base in place.  Returns (kept original indices, ReduceResult)."""
        import numpy as np
        assert self.E == 1
        R0 = int(self.nrules[0].item())
        kept = np.zeros(R0, dtype=np.int32)
        res = ReduceResult()
        check(lib().frirl_hip_reduce_shared(C.byref(self.tables), C.byref(self.bases), C.byref(agent.desc), _ptr(rant) if rant is not None else None,
                                            strategy, reward_tolerance, depth, kept.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(res), _stream(stream)),
              "frirl_hip_reduce_shared")
        return kept[: res.rules_after], res

    def reduce_batch(self, agent, strategy, reward_tolerance=0.0, depth=0, rant=None, start_states=None, active=None, stream=None):
        """frirl_hip_reduce_batch: the rule-base reduction of EVERY rule base of this problem in one run of rounds, agent e replaying
        from start_states[e] ([E, nant-1] f64, None = agent.values_def); active: [E] uint8 / bool, None = all; rant: [E, nant, maxR]
        compacted alongside.  Compacts the rule bases in place.  Returns (list of kept original indices, list of ReduceResult)."""
        import numpy as np
        import torch
        dev_ = self.rb.device
        if start_states is not None:
            assert start_states.shape == (self.E, self.nant - 1) and start_states.dtype == torch.float64 and start_states.is_contiguous()
        if active is not None:
            assert active.shape == (self.E,) and active.dtype in (torch.uint8, torch.bool) and active.is_contiguous()
        if rant is not None:
            assert rant.shape == (self.E, self.nant, self.maxR) and rant.dtype == torch.float64 and rant.is_contiguous()
        nbytes = lib().frirl_hip_reduce_batch_workspace_bytes(self.nant, self.E, self.maxR, depth)
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev_)
        kept = np.zeros((self.E, self.maxR), dtype=np.int32)
        res = (ReduceResult * self.E)()
        check(lib().frirl_hip_reduce_batch(C.byref(self.tables), C.byref(self.bases), C.byref(agent.desc), _ptr(rant), _ptr(start_states), _ptr(active),
                                           strategy, reward_tolerance, depth, kept.ctypes.data_as(C.POINTER(C.c_int32)), res, _ptr(ws), nbytes,
                                           _stream(stream)), "frirl_hip_reduce_batch")
        return [kept[e, : res[e].rules_after].copy() for e in range(self.E)], list(res)

    def reduce_batch_starts(self, agent, strategy, reward_tolerance, depth, start_states, start_count=None, drop_bad_starts=False, rant=None,
                            active=None, stream=None):
        """frirl_hip_reduce_batch_starts: reduce_batch with every removal validated against the start states start_states[e, :start_count[e]]
        ([E, n, nant-1] f64; start_count [E] int32, None = n): a removal is accepted iff the replay from EVERY used start accepts it.
        drop_bad_starts: starts whose baseline episode is not good are left out instead of blocking every removal.  Compacts the rule
        bases in place.  Returns (list of kept original indices, list of ReduceResult, per-start ReduceStartResult [E][n])."""
        import numpy as np
        import torch
        dev_ = self.rb.device
        assert start_states.dim() == 3 and start_states.shape[0] == self.E and start_states.shape[2] == self.nant - 1
        assert start_states.dtype == torch.float64 and start_states.is_contiguous()
        n = int(start_states.shape[1])
        if start_count is not None:
            assert start_count.shape == (self.E,) and start_count.dtype == torch.int32 and start_count.is_contiguous()
        if active is not None:
            assert active.shape == (self.E,) and active.dtype in (torch.uint8, torch.bool) and active.is_contiguous()
        if rant is not None:
            assert rant.shape == (self.E, self.nant, self.maxR) and rant.dtype == torch.float64 and rant.is_contiguous()
        st = ReduceStarts(n, 1 if drop_bad_starts else 0, _ptr(start_states), _ptr(start_count))
        nbytes = lib().frirl_hip_reduce_batch_starts_workspace_bytes(self.nant, self.E, self.maxR, depth, n)
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev_)
        kept = np.zeros((self.E, self.maxR), dtype=np.int32)
        res = (ReduceResult * self.E)()
        per = (ReduceStartResult * (self.E * n))()
        check(lib().frirl_hip_reduce_batch_starts(C.byref(self.tables), C.byref(self.bases), C.byref(agent.desc), _ptr(rant), C.byref(st), _ptr(active),
                                                  strategy, reward_tolerance, depth, kept.ctypes.data_as(C.POINTER(C.c_int32)), res, per, _ptr(ws),
                                                  nbytes, _stream(stream)), "frirl_hip_reduce_batch_starts")
        return ([kept[e, : res[e].rules_after].copy() for e in range(self.E)], list(res),
                [[per[e * n + k] for k in range(n)] for e in range(self.E)])

    def _map_points(self, points, point_count, active):
        import torch
        assert points.is_cuda and points.dtype == torch.float64 and points.dim() == 3 and points.is_contiguous()
        assert points.shape[0] == self.E and points.shape[2] == self.nant - 1 and points.shape[1] >= 1
        assert point_count is None or (point_count.shape == (self.E,) and point_count.dtype == torch.int32 and point_count.is_contiguous())
        assert active is None or (active.shape == (self.E,) and active.dtype in (torch.uint8, torch.bool) and active.is_contiguous())
        return MapPoints(int(points.shape[1]), 0, _ptr(points), _ptr(point_count), _ptr(active))

    def policy_map(self, agent, points, point_count=None, active=None, actconc=True, stream=None, out=None):
        """frirl_hip_policy_map: the greedy action of EVERY rule base of this problem at its own points, points [E, n, nant-1] f64 used as
        given; point_count [E] int32 (None = n); active [E] uint8 / bool.  Returns (best [E, n] int32, actconc [E, n, A] f64 or None):
        best is -1 and actconc untouched for a point that does not exist, an inactive agent or nrules outside 1..maxR.  out: the caller's
        (best, actconc) to write into.  Does not synchronise."""
        import torch
        mp = self._map_points(points, point_count, active)
        n, A = mp.n, agent.desc.A
        if out is None:
            out = (torch.empty((self.E, n), dtype=torch.int32, device=points.device),
                   torch.empty((self.E, n, A), dtype=torch.float64, device=points.device) if actconc else None)
        best, conc = out
        assert best.shape == (self.E, n) and best.dtype == torch.int32 and best.is_contiguous()
        assert conc is None or (conc.shape == (self.E, n, A) and conc.dtype == torch.float64 and conc.is_contiguous())
        nbytes = lib().frirl_hip_policy_map_workspace_bytes(self.nant, self.E, n)
        ws = _scratch(nbytes, points.device, stream)
        check(lib().frirl_hip_policy_map(C.byref(self.tables), C.byref(self._bases), C.byref(agent.desc), C.byref(mp), _ptr(best), _ptr(conc), _ptr(ws),
                                         nbytes, _stream(stream)), "frirl_hip_policy_map")
        return best, conc

    def reduce_batch_map(self, agent, points, point_count=None, active=None, strategy=1, rant=None, stream=None):
        """frirl_hip_reduce_batch_map: try-remove of EVERY rule base of this problem, a removal kept iff the greedy action stays the same at
        every one of the agent's points (points / point_count / active as policy_map); rant: [E, nant, maxR] compacted alongside.
        Compacts the rule bases in place.  Returns (list of ReduceMapResult, list of kept original indices)."""
        import numpy as np
        import torch
        mp = self._map_points(points, point_count, active)
        if rant is not None:
            assert rant.shape == (self.E, self.nant, self.maxR) and rant.dtype == torch.float64 and rant.is_contiguous()
        nbytes = lib().frirl_hip_reduce_batch_map_workspace_bytes(self.nant, self.E, self.maxR, mp.n)
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=points.device)
        kept = np.zeros((self.E, self.maxR), dtype=np.int32)
        res = (ReduceMapResult * self.E)()
        check(lib().frirl_hip_reduce_batch_map(C.byref(self.tables), C.byref(self.bases), C.byref(agent.desc), _ptr(rant), C.byref(mp), strategy,
                                               kept.ctypes.data_as(C.POINTER(C.c_int32)), res, _ptr(ws), nbytes, _stream(stream)),
              "frirl_hip_reduce_batch_map")
        return list(res), [kept[e, : res[e].rules_after].copy() for e in range(self.E)]

    def rule_usage(self, agent, points, point_count=None, active=None, peak=False, stream=None):
        """frirl_hip_rule_usage: how much the greedy policy of EVERY rule base leans on each of its rules at its points (points /
        point_count / active as policy_map): per point the normalised Shepard weights of the rules in the greedy action's conclusion
        (one-hot on an exact hit), summed over the points.  Returns (sum [E, maxR] f64, peak [E, maxR] f64 or None, best [E, n] int32);
        the sum / peak rows of an inactive agent or one with nrules outside 1..maxR are zeros here (the call leaves them untouched).
        Does not synchronise."""
        import torch
        mp = self._map_points(points, point_count, active)
        total = torch.zeros((self.E, self.maxR), dtype=torch.float64, device=points.device)
        top = torch.zeros((self.E, self.maxR), dtype=torch.float64, device=points.device) if peak else None
        best = torch.empty((self.E, mp.n), dtype=torch.int32, device=points.device)
        out = RuleUsageOut(total.data_ptr(), top.data_ptr() if peak else None, best.data_ptr())
        nbytes = lib().frirl_hip_rule_usage_workspace_bytes(self.nant, self.E, mp.n)
        ws = _scratch(nbytes, points.device, stream)
        check(lib().frirl_hip_rule_usage(C.byref(self.tables), C.byref(self._bases), C.byref(agent.desc), C.byref(mp), C.byref(out), _ptr(ws), nbytes,
                                         _stream(stream)), "frirl_hip_rule_usage")
        return total, top, best

    def rule_order(self, keys=None, descending=False, active=None, stream=None, out=None):
        """frirl_hip_rule_order: every rule base's rules in the stable order of keys [E, maxR] f64 (None: |Q|, i.e. the candidate order of
        strategy 1, or 2 with descending); NaN keys last.  Returns order [E, maxR] int32: the first nrules[e] entries of row e (the rest,
        and the rows of skipped agents, are -1 here; the call leaves them untouched).  Does not synchronise."""
        import torch
        if keys is not None:
            assert keys.is_cuda and keys.shape == (self.E, self.maxR) and keys.dtype == torch.float64 and keys.is_contiguous()
        assert active is None or (active.shape == (self.E,) and active.dtype in (torch.uint8, torch.bool) and active.is_contiguous())
        if out is None:
            out = torch.full((self.E, self.maxR), -1, dtype=torch.int32, device=self.rb.device)
        assert out.shape == (self.E, self.maxR) and out.dtype == torch.int32 and out.is_contiguous()
        check(lib().frirl_hip_rule_order(C.byref(self._bases), self.nant, _ptr(keys), 1 if descending else 0, _ptr(active), _ptr(out), _stream(stream)),
              "frirl_hip_rule_order")
        return out

    def reduce_batch_map_orders(self, agent, points, orders, point_count=None, active=None, rant=None, stream=None):
        """frirl_hip_reduce_batch_map_orders: reduce_batch_map with the caller's candidate orders, orders [E, K, maxR] int32 (K in 1..16,
        e.g. torch.stack of rule_order results along dim 1): every order is tried on its own and the one that leaves the fewest rules is
        applied (ties: the lowest k).  Compacts the rule bases in place.  Returns (list of ReduceOrdersResult, list of kept original
        indices, after_per_order [E, K] numpy int32)."""
        import numpy as np
        import torch
        mp = self._map_points(points, point_count, active)
        assert orders.is_cuda and orders.dim() == 3 and orders.shape[0] == self.E and orders.shape[2] == self.maxR
        assert orders.dtype == torch.int32 and orders.is_contiguous()
        K = int(orders.shape[1])
        if rant is not None:
            assert rant.shape == (self.E, self.nant, self.maxR) and rant.dtype == torch.float64 and rant.is_contiguous()
        nbytes = lib().frirl_hip_reduce_batch_map_orders_workspace_bytes(self.nant, self.E, self.maxR, mp.n, K)
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=points.device)
        kept = np.zeros((self.E, self.maxR), dtype=np.int32)
        after = np.zeros((self.E, max(K, 1)), dtype=np.int32)
        res = (ReduceOrdersResult * self.E)()
        check(lib().frirl_hip_reduce_batch_map_orders(C.byref(self.tables), C.byref(self.bases), C.byref(agent.desc), _ptr(rant), C.byref(mp), K, _ptr(orders),
                                                      kept.ctypes.data_as(C.POINTER(C.c_int32)), res, after.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(ws),
                                                      nbytes, _stream(stream)), "frirl_hip_reduce_batch_map_orders")
        return list(res), [kept[e, : res[e].rules_after].copy() for e in range(self.E)], after

    def policy_begin(self, agent, rows, obs, reset=None, stream=None):
        """frirl_hip_policy_begin: rows (PolicyRows) selected by `reset` ([Q] uint8 / bool, None = all) start a greedy episode on this ONE
        rule base from the caller's observations obs [Q, nant-1].  Returns (action values [Q], action indices [Q]); rows that were not
        restarted are not written.  Does not synchronise."""
        io, action, action_idx = _agent_io(self, obs, reset=reset, E=rows.Q)
        check(lib().frirl_hip_policy_begin(C.byref(self.tables), C.byref(self._bases), C.byref(agent.desc), C.byref(rows.desc), C.byref(io),
                                           _stream(stream)), "frirl_hip_policy_begin")
        return action, action_idx

    def policy_observe(self, agent, rows, obs, reward, success, q_obs=None, stream=None):
        """frirl_hip_policy_observe: one greedy step of every row that is not done, from what the caller's environment returned for the
        last action (as agent_observe).  Returns (action values, action indices); rows that were done are not written."""
        io, action, action_idx = _agent_io(self, obs, q_obs, reward, success, E=rows.Q)
        check(lib().frirl_hip_policy_observe(C.byref(self.tables), C.byref(self._bases), C.byref(agent.desc), C.byref(rows.desc), C.byref(io),
                                             _stream(stream)), "frirl_hip_policy_observe")
        return action, action_idx

    def policy_batch_begin(self, agent, rows, obs, reset=None, out=None, stream=None):
        """frirl_hip_policy_batch_begin: rows (PolicyBatchRows; row q on the rule base of agent q // rows.n) selected by `reset` start a
        greedy episode from the caller's observations obs [E * n, nant-1].  Returns (action values, action indices); rows that were not
        restarted are not written (out: the caller's (action, action_idx) tensors to write into).  Does not synchronise."""
        io, action, action_idx = _agent_io(self, obs, reset=reset, E=rows.Q, out=out)
        check(lib().frirl_hip_policy_batch_begin(C.byref(self.tables), C.byref(self._bases), C.byref(agent.desc), C.byref(rows.desc), C.byref(io),
                                                 _stream(stream)), "frirl_hip_policy_batch_begin")
        return action, action_idx

    def policy_batch_observe(self, agent, rows, obs, reward, success, q_obs=None, out=None, stream=None):
        """frirl_hip_policy_batch_observe: one greedy step of every row that is not done (as policy_observe, every agent on its own rule
        base).  Returns (action values, action indices); rows that were done are not written."""
        io, action, action_idx = _agent_io(self, obs, q_obs, reward, success, E=rows.Q, out=out)
        check(lib().frirl_hip_policy_batch_observe(C.byref(self.tables), C.byref(self._bases), C.byref(agent.desc), C.byref(rows.desc), C.byref(io),
                                                   _stream(stream)), "frirl_hip_policy_batch_observe")
        return action, action_idx

    def merge_rb(self, agent, sndr_rant, sndr_rconc, weights, rant_store=None, active=None, stream=None):
        """frirl_hip_merge_rb: every (active) rule base of this batch takes over the sender rules sndr_rant [S][nant] (AoS),
        sndr_rconc [S]; weights [E][maxR] persists between calls (zeros at first).  Returns full [E] int32."""
        import torch
        S = sndr_rconc.numel()
        assert sndr_rant.shape == (S, self.nant) and sndr_rant.is_contiguous() and weights.shape == (self.E, self.maxR)
        snd = SenderDesc(sndr_rant.data_ptr(), self.nant, 1, sndr_rconc.data_ptr(), S, 0, None)
        full = torch.zeros((self.E,), dtype=torch.int32, device=self.rb.device)
        check(lib().frirl_hip_merge_rb(C.byref(self.tables), C.byref(self.bases), C.byref(agent.desc), _ptr(rant_store), C.byref(snd), _ptr(weights),
                                       _ptr(active), _ptr(full), _stream(stream)), "frirl_hip_merge_rb")
        return full

    def clone_agents(self, envs, src, conv=None, weights=None, stream=None):
        """frirl_hip_clone_agents: agent e becomes a copy of the learner state of agent src[e] (int32 [E] on the device) -- rule base,
        index mirror, and with envs (Envs or None) / conv (Convergence or None) / weights ([E, maxR] or None) the raw antecedents,
        sticky flag, spread state, merge weights and a cleared convergence state.  Returns the status tensor [E] int32 (CLONE_*).
        Does not synchronise.  The packed index mirror and the codes are marked stale, as for every call that may rewrite uidx."""
        import torch
        assert src.is_cuda and src.dtype == torch.int32 and src.shape == (self.E,) and src.is_contiguous()
        assert weights is None or (weights.shape == (self.E, self.maxR) and weights.dtype == torch.float64 and weights.is_contiguous())
        status = torch.empty((self.E,), dtype=torch.int32, device=self.rb.device)
        check(lib().frirl_hip_clone_agents(C.byref(self.bases), self.nant, None if envs is None else C.byref(envs.desc),
                                           None if conv is None else C.byref(conv.desc), _ptr(weights), _ptr(src), _ptr(status), _stream(stream)),
              "frirl_hip_clone_agents")
        return status

    def select_plan_device(self, scores, parents, replace, eligible=None, stream=None):
        """select_plan_device (below) for the E agents of this problem: (src, rank, info) as device tensors."""
        assert scores.shape[0] == self.E, (tuple(scores.shape), self.E)
        return select_plan_device(scores, parents, replace, eligible=eligible, stream=stream)

    def perturb_rows(self, spec, generation, status, rows=None, explore=None, target=None, expect=None, stream=None):
        """perturb_rows (below) for the E agents of this problem: the rows are rewritten in place; returns the count tensor."""
        assert status.shape == (self.E,), (tuple(status.shape), self.E)
        return perturb_rows(spec, generation, status, rows=rows, explore=explore, target=target, expect=expect, stream=stream)

    def add_rule(self, rant, rconc, active=None, rant_store=None, stream=None):
        """five_hip_add_rule: appends rant[e] -> rconc[e]; returns added [E] int32."""
        import torch
        added = torch.empty((self.E,), dtype=torch.int32, device=rant.device)
        check(lib().five_hip_add_rule(C.byref(self.tables), C.byref(self.bases), _ptr(rant), _ptr(rconc), _ptr(active), _ptr(rant_store),
                                      _ptr(added), _stream(stream)), "five_hip_add_rule")
        return added


class Agent:
    """Host-side frirl_hip_agent: hyper-parameters + grids (device copies of the small tables are owned here)."""

    def __init__(self, device, nant, grids, grid_div, values_def, action_ve, alpha, gamma, qdiff_pos, qdiff_neg, weight_thr=0.05,
                 skip_rules=1, p=0, env_kind=0, max_steps=1000, epsilon=0.0, no_random=1, seed=0, reward_good_above=0.0,
                 qdiff_final_tolerance=250.0, env_id_base=0, evaluate=0, debug_flags=0):
        import numpy as np
        import torch
        assert len(grids) == nant and all(1 <= len(g) <= MAX_GRID for g in grids)
        gv = np.zeros((nant, MAX_GRID))
        for k, g in enumerate(grids):
            gv[k, : len(g)] = g
        self.grid_values = torch.from_numpy(gv).to(device)
        self.action_ve = torch.as_tensor(np.asarray(action_ve, dtype=np.float64)).to(device)
        self.A = len(grids[-1])
        assert self.action_ve.numel() == self.A
        d = AgentDesc()
        d.alpha, d.gamma, d.qdiff_pos_boundary, d.qdiff_neg_boundary = alpha, gamma, qdiff_pos, qdiff_neg
        d.weight_significant, d.skip_rules, d.p, d.A, d.env_kind, d.max_steps = weight_thr, skip_rules, p, self.A, env_kind, max_steps
        for k in range(nant):
            d.grid_len[k] = len(grids[k])
            d.grid_div[k] = grid_div[k] if k < len(grid_div) else 0.0
            d.values_def[k] = values_def[k] if k < len(values_def) else 0.0
        d.grid_values, d.action_ve = self.grid_values.data_ptr(), self.action_ve.data_ptr()
        d.no_random, d.epsilon, d.seed, d.env_id_base, d.evaluate = no_random, epsilon, seed, env_id_base, evaluate
        d.debug_flags = debug_flags
        d.reward_good_above, d.qdiff_final_tolerance = reward_good_above, qdiff_final_tolerance
        self.desc, self.nant = d, nant


class Envs:
    """Device-resident per-environment episode state (struct frirl_hip_envs)."""

    def __init__(self, problem, device, keep_rant=True, rant_init=None, start_states=None):
        import torch
        E, nant, maxR = problem.E, problem.nant, problem.maxR
        self.start_states = start_states
        self.episode = torch.zeros((E,), dtype=torch.int32, device=device)
        self.states = torch.zeros((E, nant - 1), dtype=torch.float64, device=device)
        self.q_ant = torch.zeros((E, nant), dtype=torch.float64, device=device)
        self.fus = torch.zeros((E,), dtype=torch.int32, device=device)
        self.done = torch.zeros((E,), dtype=torch.int32, device=device)
        self.ep_steps = torch.zeros((E,), dtype=torch.int32, device=device)
        self.ep_reward = torch.zeros((E,), dtype=torch.float64, device=device)
        self.status = torch.zeros((E,), dtype=torch.int32, device=device)
        self.rant = None
        if keep_rant:
            self.rant = torch.zeros((E, nant, maxR), dtype=torch.float64, device=device) if rant_init is None else rant_init
        self.spread_ant = torch.zeros((E, nant), dtype=torch.float64, device=device)     # what determines FIVERB.weights after learning
        self.spread_R = torch.zeros((E,), dtype=torch.int32, device=device)
        self.desc = EnvsDesc(self.states.data_ptr(), self.q_ant.data_ptr(), self.fus.data_ptr(), self.done.data_ptr(), self.ep_steps.data_ptr(),
                             self.ep_reward.data_ptr(), self.rant.data_ptr() if self.rant is not None else None, self.status.data_ptr(),
                             self.start_states.data_ptr() if self.start_states is not None else None, self.episode.data_ptr(),
                             self.spread_ant.data_ptr(), self.spread_R.data_ptr())


class HparamRows:
    """Per-agent learning hyper-parameters (struct frirl_hip_hparam_rows): one value per agent of a batch of E for each column given
    -- alpha, gamma, qdiff_pos_boundary, qdiff_neg_boundary, weight_significant (float64) and skip_rules (int32, 0 / 1) -- as anything
    torch.as_tensor takes, of length E; a column left None keeps the Agent's value for every agent.  Owns the device tensors and the
    struct.  Taken by agent_begin / agent_observe / train_persistent / train as rows=."""

    def __init__(self, E, device, alpha=None, gamma=None, qdiff_pos_boundary=None, qdiff_neg_boundary=None, weight_significant=None,
                 skip_rules=None):
        import torch
        self.E, self.desc = E, HparamRowsDesc()
        given = dict(alpha=alpha, gamma=gamma, qdiff_pos_boundary=qdiff_pos_boundary, qdiff_neg_boundary=qdiff_neg_boundary,
                     weight_significant=weight_significant, skip_rules=skip_rules)
        for k in HP_COLUMNS:
            t = None
            if given[k] is not None:
                t = torch.as_tensor(given[k], dtype=torch.int32 if k == "skip_rules" else torch.float64).to(device).contiguous()
                assert t.shape == (E,), (k, tuple(t.shape), E)
                setattr(self.desc, k, t.data_ptr())
            setattr(self, k, t)


def _rows(rows, E):
    if rows is None:
        return None
    assert rows.E == E, (rows.E, E)
    return None if rows.desc is None else C.byref(rows.desc)


def _level_entry(base, E, rows=None, explore=None, target=None, teacher=None, expect=None):
    """The entry point of the family `base` (SIGNATURES: _levels) for the per-agent structs given: the last one given picks base_rows,
    base_explore, base_target or base_expect, which take the structs before it as well (None = NULL); with none of them `base` itself or, with a
    teacher, base_taught.  Returns (the function, its name for check(), the struct arguments that follow the agent, the teacher
    argument that precedes the stream in the agent calls: nothing for `base` itself, which has none)."""
    level = 4 if expect is not None else 3 if target is not None else 2 if explore is not None else 1 if rows is not None else 0
    name = base + (_SUFFIX[level] if level or teacher is None else "_taught")
    structs = [_rows(r, E) for r in (rows, explore, target, expect)[:level]]
    taught = [] if name == base else [None if teacher is None else _teacher(teacher, E)]
    return getattr(lib(), name), name, structs, taught


class ExploreRows:
    """Per-agent exploration (struct frirl_hip_explore_rows): agent e of a batch of E picks at epsilon[e], falling linearly to zero
    over horizon[e] episodes (0 = constant; explore_epsilon gives the rate of an episode).  epsilon (float64) and horizon (int32) are
    anything torch.as_tensor takes, of length E; epsilon None keeps the Agent's epsilon, horizon None gives every agent horizon_all.
    Owns the device tensors and the struct.  Taken by agent_begin / agent_observe / train_persistent / train as explore=."""

    def __init__(self, E, device, epsilon=None, horizon=None, horizon_all=0):
        import torch
        self.E, self.desc = E, ExploreRowsDesc()
        self.desc.horizon_all = int(horizon_all)
        for k, v, dt in (("epsilon", epsilon, torch.float64), ("horizon", horizon, torch.int32)):
            t = None
            if v is not None:
                t = torch.as_tensor(v, dtype=dt).to(device).contiguous()
                assert t.shape == (E,), (k, tuple(t.shape), E)
                setattr(self.desc, k, t.data_ptr())
            setattr(self, k, t)

    @classmethod
    def null(cls, E):
        """The NULL struct pointer: explore=ExploreRows.null(E) goes through the _explore entry point with no rows at all."""
        self = cls.__new__(cls)
        self.E, self.desc, self.epsilon, self.horizon = E, None, None, None
        return self


class TargetRows:
    """Per-agent TD target (struct frirl_hip_target_rows): agent e of a batch of E learns towards Q(s', a') of the action it takes
    (TARGET_SARSA, 0) or towards Q(s', g) of the greedy action its pick started from (TARGET_Q, 1).  target (uint8) is anything
    torch.as_tensor takes, of length E; None gives every agent target_all.  Owns the device tensor and the struct.  Taken by
    agent_observe / train_persistent / train as target=."""

    def __init__(self, E, device, target=None, target_all=TARGET_SARSA):
        import torch
        self.E, self.desc, self.target = E, TargetRowsDesc(), None
        self.desc.target_all = int(target_all)
        if target is not None:
            self.target = torch.as_tensor(target, dtype=torch.uint8).to(device).contiguous()
            assert self.target.shape == (E,), (tuple(self.target.shape), E)
            self.desc.target = self.target.data_ptr()

    @classmethod
    def null(cls, E):
        """The NULL struct pointer: target=TargetRows.null(E) goes through the _target entry point, which calls the _explore one."""
        self = cls.__new__(cls)
        self.E, self.desc, self.target = E, None, None
        return self


class ExpectRows:
    """Per-agent expected SARSA (struct frirl_hip_expect_rows): an agent e of a batch of E whose flag is 1 learns towards the expectation
    of Q(s', .) under its own epsilon-greedy pick; its TD target is then not consulted.  expected (uint8 0 / 1) is anything
    torch.as_tensor takes, of length E; None gives every agent expected_all.  Owns the device tensor and the struct.  Taken by
    agent_observe / train_persistent / train as expect=."""

    def __init__(self, E, device, expected=None, expected_all=0):
        import torch
        self.E, self.desc, self.expected = E, ExpectRowsDesc(), None
        self.desc.expected_all = int(expected_all)
        if expected is not None:
            self.expected = torch.as_tensor(expected, dtype=torch.uint8).to(device).contiguous()
            assert self.expected.shape == (E,), (tuple(self.expected.shape), E)
            self.desc.expected = self.expected.data_ptr()

    @classmethod
    def null(cls, E):
        """The NULL struct pointer: expect=ExpectRows.null(E) goes through the _expect entry point, which calls the _target one."""
        self = cls.__new__(cls)
        self.E, self.desc, self.expected = E, None, None
        return self


def explore_epsilon(eps, horizon, episode):
    """frirl_hip_explore_epsilon: the exploration rate of an agent with row values (eps, horizon) in the episode whose stream key is
    `episode` (the first learning episode is 1) -- the host build of the function the kernels call."""
    return float(lib().frirl_hip_explore_epsilon(float(eps), int(horizon), int(episode)))


def rollout_scores(sc):
    """The [E, 40] uint8 tensor Problem.rollout_batch(scores=True) returns as a host array of RolloutScore (synchronises)."""
    raw = sc.cpu().numpy().tobytes()
    return (RolloutScore * sc.shape[0]).from_buffer_copy(raw)


def update_sarsa(problem, agent, envs, q_ant, reward, cur_q_ant, active=None, stream=None):
    check(lib().frirl_hip_update_sarsa(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), C.byref(envs.desc), _ptr(q_ant),
                                       _ptr(reward), _ptr(cur_q_ant), _ptr(active), _stream(stream)), "frirl_hip_update_sarsa")


def env_step(agent, action, states, stream=None):
    import torch
    E, ns = states.shape
    new_states, q_states = torch.empty_like(states), torch.empty_like(states)
    reward = torch.empty((E,), dtype=torch.float64, device=states.device)
    success = torch.empty((E,), dtype=torch.int32, device=states.device)
    check(lib().frirl_hip_env_step(C.byref(agent.desc), E, ns, _ptr(action), _ptr(states), _ptr(new_states), _ptr(reward), _ptr(success),
                                   _ptr(q_states), _stream(stream)), "frirl_hip_env_step")
    return new_states, reward, success, q_states


def explore_check(agent, env, episode, step, greedy, stream=None):
    """frirl_hip_explore_check: the exploration stream and pick of `agent` (A, epsilon, no_random, seed, env_id_base) at the key
    tuples env / episode / step [n] (int64 tensors holding uint32 values) with greedy actions greedy [n] int32.
    Returns (picked action [n] int32, units [n, 2] float64: draw 0 and draw 1)."""
    import torch
    n = env.numel()
    as_u32 = [k.to(torch.int64).bitwise_and(0xFFFFFFFF).to(torch.uint32).contiguous() for k in (env, episode, step)]
    greedy = greedy.to(torch.int32).contiguous()
    action = torch.empty((n,), dtype=torch.int32, device=greedy.device)
    units = torch.empty((n, 2), dtype=torch.float64, device=greedy.device)
    check(lib().frirl_hip_explore_check(C.byref(agent.desc), n, _ptr(as_u32[0]), _ptr(as_u32[1]), _ptr(as_u32[2]), _ptr(greedy), _ptr(action),
                                        _ptr(units), _stream(stream)), "frirl_hip_explore_check")
    return action, units


def episode_begin(problem, agent, envs, stream=None):
    check(lib().frirl_hip_episode_begin(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), C.byref(envs.desc),
                                        _stream(stream)), "frirl_hip_episode_begin")


def episode_step(problem, agent, envs, stream=None):
    check(lib().frirl_hip_episode_step(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), C.byref(envs.desc),
                                       _stream(stream)), "frirl_hip_episode_step")


def _agent_io(problem, obs, q_obs=None, reward=None, success=None, reset=None, E=None, out=None):
    import torch
    E, ns = (problem.E if E is None else E), problem.nant - 1
    assert obs.is_cuda and obs.dtype == torch.float64 and obs.shape == (E, ns) and obs.is_contiguous()
    io = AgentIO()
    io.obs = obs.data_ptr()
    if q_obs is not None:
        assert q_obs.dtype == torch.float64 and q_obs.shape == (E, ns) and q_obs.is_contiguous()
        io.q_obs = q_obs.data_ptr()
    if reward is not None:
        assert reward.dtype == torch.float64 and reward.shape == (E,) and reward.is_contiguous()
        assert success.dtype == torch.int32 and success.shape == (E,) and success.is_contiguous()
        io.reward, io.success = reward.data_ptr(), success.data_ptr()
    if reset is not None:
        assert reset.dtype in (torch.uint8, torch.bool) and reset.shape == (E,) and reset.is_contiguous()
        io.reset = reset.data_ptr()
    if out is not None:         # the caller's buffers: rows the call skips keep what they hold
        action, action_idx = out
    else:
        action = torch.empty((E,), dtype=torch.float64, device=obs.device)
        action_idx = torch.empty((E,), dtype=torch.int32, device=obs.device)
    io.action_out, io.action_idx = action.data_ptr(), action_idx.data_ptr()
    return io, action, action_idx


def _teacher(teacher, E):
    import torch
    assert teacher.is_cuda and teacher.dtype == torch.int32 and teacher.shape == (E,) and teacher.is_contiguous()
    return _ptr(teacher)


def agent_begin(problem, agent, envs, obs, reset=None, stream=None, teacher=None, rows=None, explore=None):
    """frirl_hip_agent_begin: start an episode from the caller's observations obs [E, nant-1] (float64, on the device) for the rows
    selected by `reset` ([E] uint8 / bool, None = all).  Returns (action values [E] float64, action indices [E] int32): the first
    action of every restarted row (the other rows' entries are not written).  teacher [E] int32 (frirl_hip_agent_begin_taught): a row
    whose entry is an action index 0..A-1 takes that action, any other value leaves the row its own pick.  rows: an HparamRows
    (frirl_hip_agent_begin_rows; the begin call reads no learning hyper-parameter).  explore: an ExploreRows
    (frirl_hip_agent_begin_explore): row e picks at its own rate for the episode it starts.  Does not synchronise."""
    io, action, action_idx = _agent_io(problem, obs, reset=reset)
    fn, name, structs, taught = _level_entry("frirl_hip_agent_begin", problem.E, rows, explore, teacher=teacher)
    check(fn(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), *structs, C.byref(envs.desc), C.byref(io), *taught, _stream(stream)), name)
    return action, action_idx


def agent_observe(problem, agent, envs, obs, reward, success, q_obs=None, stream=None, teacher=None, rows=None, explore=None, target=None, expect=None):
    """frirl_hip_agent_observe: one SARSA step of every row that is not done, from what the caller's environment returned for the
    last action -- obs [E, nant-1] float64, reward [E] float64, success [E] int32 (1 ends the episode), q_obs [E, nant-1] its
    quantised form or None (the generic grid rule on the device).  Returns (action values, action indices) of the next action;
    rows that were done are not written.  teacher [E] int32 (frirl_hip_agent_observe_taught): a row whose entry is an action index
    takes it as its next action and learns towards Q(s', a_teacher).  rows: an HparamRows (frirl_hip_agent_observe_rows): row e
    learns under its own values of the columns given.  explore: an ExploreRows (frirl_hip_agent_observe_explore): row e picks at
    its own rate in its current episode.  target: a TargetRows (frirl_hip_agent_observe_target): row e learns towards Q(s', a') or
    Q(s', g); a taught row under TARGET_Q takes the teacher's action and learns towards Q(s', g).  expect: an ExpectRows
    (frirl_hip_agent_observe_expect): a flagged row learns towards the expectation of Q(s', .) under its own pick, whatever action it
    takes.  Does not synchronise."""
    io, action, action_idx = _agent_io(problem, obs, q_obs, reward, success)
    fn, name, structs, taught = _level_entry("frirl_hip_agent_observe", problem.E, rows, explore, target, teacher, expect)
    check(fn(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), *structs, C.byref(envs.desc), C.byref(io), *taught, _stream(stream)), name)
    return action, action_idx


class Demonstration:
    """Recorded logs for learn_demonstration (struct frirl_hip_demonstration): obs [L, T, nant-1] float64, action [L, T] int32,
    reward [L, T] float64, success [L, T] int32, optional q_obs (as obs), start [L, T] uint8 / bool and length [E] int32, all on the
    device and contiguous.  L = E gives every agent its own log, L = 1 makes every agent replay the one log (agent_stride = 0)."""

    def __init__(self, obs, action, reward, success, q_obs=None, start=None, length=None):
        import torch
        L, T, ns = obs.shape
        assert obs.is_cuda and obs.dtype == torch.float64 and obs.is_contiguous() and T >= 1
        assert action.dtype == torch.int32 and action.shape == (L, T) and action.is_contiguous()
        assert reward.dtype == torch.float64 and reward.shape == (L, T) and reward.is_contiguous()
        assert success.dtype == torch.int32 and success.shape == (L, T) and success.is_contiguous()
        assert q_obs is None or (q_obs.dtype == torch.float64 and q_obs.shape == obs.shape and q_obs.is_contiguous())
        assert start is None or (start.dtype in (torch.uint8, torch.bool) and start.shape == (L, T) and start.is_contiguous())
        assert length is None or (length.dtype == torch.int32 and length.dim() == 1 and length.is_contiguous())
        self.obs, self.action, self.reward, self.success, self.q_obs, self.start, self.length = obs, action, reward, success, q_obs, start, length
        self.L, self.T, self.ns = L, T, ns
        self.desc = DemonstrationDesc(T, T if L > 1 else 0, obs.data_ptr(), q_obs.data_ptr() if q_obs is not None else None, action.data_ptr(),
                                      reward.data_ptr(), success.data_ptr(), start.data_ptr() if start is not None else None,
                                      length.data_ptr() if length is not None else None)


class RolloutLog:
    """The logs Problem.rollout_record writes (struct frirl_hip_rollout_log): obs / q_obs [Q, T, nant-1] float64, action / success
    [Q, T] int32, reward [Q, T] float64, start [Q, T] uint8, length [Q] int32 and per episode ep_steps / ep_success [Q, K] int32,
    ep_reward [Q, K] float64; Q = E * n logs of K episodes and capacity T."""
    FIELDS = ("obs", "q_obs", "action", "reward", "success", "start", "length", "ep_steps", "ep_reward", "ep_success")

    def __init__(self, obs, q_obs, action, reward, success, start, length, ep_steps, ep_reward, ep_success):
        import torch
        Q, T, ns = obs.shape
        K = ep_steps.shape[1]
        for x, shape, dt in ((obs, (Q, T, ns), torch.float64), (q_obs, (Q, T, ns), torch.float64), (action, (Q, T), torch.int32),
                             (reward, (Q, T), torch.float64), (success, (Q, T), torch.int32), (start, (Q, T), torch.uint8),
                             (length, (Q,), torch.int32), (ep_steps, (Q, K), torch.int32), (ep_reward, (Q, K), torch.float64),
                             (ep_success, (Q, K), torch.int32)):
            assert x.is_cuda and x.shape == shape and x.dtype == dt and x.is_contiguous()
        self.obs, self.q_obs, self.action, self.reward, self.success, self.start, self.length = obs, q_obs, action, reward, success, start, length
        self.ep_steps, self.ep_reward, self.ep_success = ep_steps, ep_reward, ep_success
        self.Q, self.K, self.T, self.ns, self.n = Q, K, T, ns, None

    @classmethod
    def empty(cls, Q, K, T, ns, device):
        import torch
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        return cls(mk((Q, T, ns), torch.float64), mk((Q, T, ns), torch.float64), mk((Q, T), torch.int32), mk((Q, T), torch.float64),
                   mk((Q, T), torch.int32), mk((Q, T), torch.uint8), mk((Q,), torch.int32), mk((Q, K), torch.int32), mk((Q, K), torch.float64),
                   mk((Q, K), torch.int32))

    def points(self, cap, only_successful=False, stream=None):
        """log_points over these logs (needs the n of the rollout_record call that wrote them): (points [E, cap, ns], point_count [E],
        overflow [E]), ready for Problem.policy_map / reduce_batch_map."""
        assert self.n is not None and self.Q % self.n == 0
        return log_points(self.obs, self.q_obs, self.success, self.start, self.length, self.Q // self.n, cap, only_successful, stream)

    def demonstration(self, log=None, E=None):
        """A Demonstration over the same memory, no copy.  log=None: one log per agent (needs n == 1).  log=q: that one log for E
        students, its length expanded to [E] (a device op; nothing is read back)."""
        if log is None:
            assert self.n == 1, "one log per agent needs n == 1"
            return Demonstration(self.obs, self.action, self.reward, self.success, q_obs=self.q_obs, start=self.start, length=self.length)
        assert E is not None and E >= 1 and 0 <= log < self.Q
        s = slice(log, log + 1)
        return Demonstration(self.obs[s], self.action[s], self.reward[s], self.success[s], q_obs=self.q_obs[s], start=self.start[s],
                             length=self.length[s].repeat(E))


def log_points(obs, q_obs, success, start, length, E, cap, only_successful=False, stream=None):
    """frirl_hip_log_points: per agent the de-duplicated points of its logs (obs / q_obs [E * n_logs, T, ns] f64, success [E * n_logs, T]
    int32, start [E * n_logs, T] uint8, length [E * n_logs] int32; logs e * n_logs + j belong to agent e): a start record's obs, every
    other record's q_obs, first occurrence first.  Returns (points [E, cap, ns] f64 -- rows at and beyond point_count[e] are zero --,
    point_count [E] int32, overflow [E] int32).  Does not synchronise."""
    import torch
    Q, T, ns = obs.shape
    assert Q % E == 0 and Q >= E >= 1
    for x, shape, dt in ((obs, (Q, T, ns), torch.float64), (q_obs, (Q, T, ns), torch.float64), (success, (Q, T), torch.int32),
                         (start, (Q, T), torch.uint8), (length, (Q,), torch.int32)):
        assert x.is_cuda and x.shape == shape and x.dtype == dt and x.is_contiguous()
    dev_ = obs.device
    points = torch.zeros((E, cap, ns), dtype=torch.float64, device=dev_)
    count = torch.empty((E,), dtype=torch.int32, device=dev_)
    overflow = torch.empty((E,), dtype=torch.int32, device=dev_)
    lp = LogPointsDesc(E, Q // E, T, ns, cap, 1 if only_successful else 0, _ptr(obs), _ptr(q_obs), _ptr(success), _ptr(start), _ptr(length),
                       _ptr(points), _ptr(count), _ptr(overflow))
    nbytes = lib().frirl_hip_log_points_workspace_bytes(E, Q // E, T)
    ws = _scratch(nbytes, dev_, stream)
    check(lib().frirl_hip_log_points(C.byref(lp), _ptr(ws), nbytes, _stream(stream)), "frirl_hip_log_points")
    return points, count, overflow


def grid_points(desc, device=None):
    """The Cartesian product of the state grids of a problem description (demo_describe / describe): [cells, nant-1] float64, the
    last state varying fastest (torch.cartesian_prod order).  With Problem.policy_map before and after a reduction, "how many
    cells of the grid changed their greedy action" is (best_before != best_after).sum()."""
    import torch
    axes = [torch.as_tensor(list(g), dtype=torch.float64, device=device) for g in desc["grids"][:-1]]
    return torch.cartesian_prod(*axes).reshape(-1, len(axes)).contiguous()


def demo_batch_object(env, E, maxR, start_states=None, seed=0, env_id_base=0):
    """frirl_hip_batch_create for a demo: E agents from the reference's initial rule base (the 2^nant corner rules, Q = 0), agent e
    starting its episodes at start_states[e] (host [E, nant-1], None = values_def); seed and env_id_base key the exploration stream
    (the batch is greedy, no_random = 1, until frirl_hip_batch_set_exploration gives it rows).  Returns the handle for the frirl_hip_batch_*
    calls of lib(); release it with lib().frirl_hip_batch_destroy."""
    import numpy as np
    d = demo_describe(env)
    nant = d["nant"]
    grid = np.zeros((nant, MAX_GRID))
    for k, g in enumerate(d["grids"]):
        grid[k, : len(g)] = g
    ncorner = 2 ** nant
    rant0 = np.zeros((ncorner, nant))
    for k in range(nant):
        div = ncorner >> (k + 1)
        rant0[:, k] = [d["grids"][k].min() if ((j // div) % 2) == 0 else d["grids"][k].max() for j in range(ncorner)]
    rconc0 = np.zeros(ncorner)
    u, ve, ave = np.ascontiguousarray(d["u"]), np.ascontiguousarray(d["ve"]), np.ascontiguousarray(d["action_ve"])
    st = None if start_states is None else np.ascontiguousarray(start_states, dtype=np.float64)
    assert st is None or st.shape == (E, nant - 1)
    desc = BatchDesc()
    desc.nant, desc.U, desc.E, desc.maxR, desc.u, desc.ve = nant, d["U"], E, maxR, u.ctypes.data, ve.ctypes.data
    desc.R0, desc.rant0, desc.rconc0 = ncorner, rant0.ctypes.data, rconc0.ctypes.data
    desc.start_states = None if st is None else st.ctypes.data
    ag = desc.agent
    ag.alpha, ag.gamma, ag.qdiff_pos_boundary, ag.qdiff_neg_boundary = d["alpha"], d["gamma"], d["qdiff_pos"], d["qdiff_neg"]
    ag.weight_significant, ag.skip_rules, ag.A, ag.env_kind, ag.max_steps, ag.no_random = d["weight_thr"], d["skip_rules"], d["A"], d["kind"], d["max_steps"], 1
    ag.reward_good_above, ag.qdiff_final_tolerance = d["reward_good_above"], d["qdiff_final_tolerance"]
    ag.seed, ag.env_id_base = seed, env_id_base
    for k in range(nant):
        ag.grid_len[k], ag.grid_div[k], ag.values_def[k] = len(d["grids"][k]), d["grid_div"][k], d["values_def"][k]
    ag.grid_values, ag.action_ve = grid.ctypes.data, ave.ctypes.data
    b = lib().frirl_hip_batch_create(C.byref(desc))          # copies every host array before it returns
    if not b:
        raise FrirlHipError("frirl_hip_batch_create: " + lib().frirl_hip_last_error().decode())
    return b


def batch_set_hparams(batch, **columns):
    """frirl_hip_batch_set_hparams on a library-owned batch: per-agent hyper-parameters for frirl_hip_batch_train, one host array of
    length E per keyword (HP_COLUMNS: alpha, gamma, qdiff_pos_boundary, qdiff_neg_boundary, weight_significant, skip_rules); a column
    left out keeps the batch's value.  No keyword at all clears every row.  The library validates and copies before it returns."""
    import numpy as np
    unknown = set(columns) - set(HP_COLUMNS)
    if unknown:
        raise TypeError(f"batch_set_hparams: unknown column(s) {sorted(unknown)}; the columns are {HP_COLUMNS}")
    desc, keep = HparamRowsDesc(), []
    for k, v in columns.items():
        if v is None:
            continue
        a = np.ascontiguousarray(v, dtype=np.int32 if k == "skip_rules" else np.float64)
        keep.append(a)
        setattr(desc, k, a.ctypes.data)
    check(lib().frirl_hip_batch_set_hparams(batch, C.byref(desc) if keep else None), "frirl_hip_batch_set_hparams")


def batch_set_exploration(batch, epsilon=None, horizon=None, horizon_all=0, clear=False):
    """frirl_hip_batch_set_exploration on a library-owned batch: per-agent exploration for frirl_hip_batch_train, host arrays of
    length E -- epsilon (None: the batch's epsilon for every agent) and horizon in episodes (None: horizon_all for every agent).
    clear=True (or no argument at all) clears the rows.  The library validates and copies before it returns."""
    import numpy as np
    if clear or (epsilon is None and horizon is None and horizon_all == 0):
        check(lib().frirl_hip_batch_set_exploration(batch, None), "frirl_hip_batch_set_exploration")
        return
    desc = ExploreRowsDesc()
    desc.horizon_all = int(horizon_all)
    eps = None if epsilon is None else np.ascontiguousarray(epsilon, dtype=np.float64)
    hor = None if horizon is None else np.ascontiguousarray(horizon, dtype=np.int32)
    if eps is not None:
        desc.epsilon = eps.ctypes.data
    if hor is not None:
        desc.horizon = hor.ctypes.data
    check(lib().frirl_hip_batch_set_exploration(batch, C.byref(desc)), "frirl_hip_batch_set_exploration")


def batch_set_target(batch, target=None, target_all=TARGET_SARSA):
    """frirl_hip_batch_set_target on a library-owned batch: the TD target of every agent for frirl_hip_batch_train -- a host array of
    length E of TARGET_SARSA / TARGET_Q, or None: target_all for every agent.  (None, TARGET_SARSA) clears the target.  The library
    validates and copies before it returns."""
    import numpy as np
    col = None if target is None else np.ascontiguousarray(target, dtype=np.uint8)
    assert col is None or col.shape == (_batch_agents(batch),)
    check(lib().frirl_hip_batch_set_target(batch, None if col is None else col.ctypes.data, int(target_all)), "frirl_hip_batch_set_target")


def batch_get_target(batch):
    """frirl_hip_batch_get_target: uint8 [E], the TD target every agent trains under (TARGET_SARSA while none is set)."""
    import numpy as np
    out = np.zeros(_batch_agents(batch), dtype=np.uint8)
    check(lib().frirl_hip_batch_get_target(batch, out.ctypes.data), "frirl_hip_batch_get_target")
    return out


def batch_set_expected(batch, expected=None, expected_all=0):
    """frirl_hip_batch_set_expected on a library-owned batch: the expected-SARSA flag of every agent for frirl_hip_batch_train -- a host
    array of length E of 0 / 1, or None: expected_all for every agent.  (None, 0) clears the flags.  The library validates and copies
    before it returns."""
    import numpy as np
    col = None if expected is None else np.ascontiguousarray(expected, dtype=np.uint8)
    assert col is None or col.shape == (_batch_agents(batch),)
    check(lib().frirl_hip_batch_set_expected(batch, None if col is None else col.ctypes.data, int(expected_all)), "frirl_hip_batch_set_expected")


def batch_get_expected(batch):
    """frirl_hip_batch_get_expected: uint8 [E], the expected-SARSA flag every agent trains under (0 while none is set)."""
    import numpy as np
    out = np.zeros(_batch_agents(batch), dtype=np.uint8)
    check(lib().frirl_hip_batch_get_expected(batch, out.ctypes.data), "frirl_hip_batch_get_expected")
    return out


def batch_agent_report(batch):
    """frirl_hip_batch_agent_report on a library-owned batch: dict of host arrays [E] -- converged, episodes, rules (int32), ep_steps
    (int32) and ep_reward (float64) of the last finished episode: per agent what frirl_hip_batch_stats sums (E is its `agents`)."""
    import numpy as np
    st = BatchStats()
    check(lib().frirl_hip_batch_stats(batch, C.byref(st)), "frirl_hip_batch_stats")
    E = int(st.agents)
    out = {k: np.zeros(E, dtype=np.int32) for k in ("converged", "episodes", "rules", "ep_steps")}
    out["ep_reward"] = np.zeros(E)
    i32 = C.POINTER(C.c_int32)
    check(lib().frirl_hip_batch_agent_report(batch, out["converged"].ctypes.data_as(i32), out["episodes"].ctypes.data_as(i32), out["rules"].ctypes.data_as(i32),
                                             out["ep_steps"].ctypes.data_as(i32), out["ep_reward"].ctypes.data_as(_DP)), "frirl_hip_batch_agent_report")
    return out


def batch_teach(batch, teacher, episodes, start_states=None, passes=1, students=None):
    """frirl_hip_batch_teach on a library-owned batch (the handle frirl_hip_batch_create returned): agent `teacher` records `episodes`
    greedy episodes, every student (students: [E] array of 0 / 1, None = everybody but the teacher) replays the log `passes` times.
    start_states: host [episodes, nant-1] float64 or None.  Returns the TeachResult."""
    import numpy as np
    st = None if start_states is None else np.ascontiguousarray(start_states, dtype=np.float64)
    mask = None if students is None else np.ascontiguousarray(students, dtype=np.uint8)
    res = TeachResult()
    check(lib().frirl_hip_batch_teach(batch, teacher, episodes, None if st is None else st.ctypes.data_as(_DP), passes,
                                      None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(res)), "frirl_hip_batch_teach")
    return res


def _batch_agents(batch):
    st = BatchStats()
    check(lib().frirl_hip_batch_stats(batch, C.byref(st)), "frirl_hip_batch_stats")
    return int(st.agents)


def select_plan(scores, parents, replace, eligible=None):
    """frirl_hip_select_plan (host only): scores is a sequence of RolloutScore, or of (successes, reward_sum) pairs; eligible a
    sequence of 0 / 1 or None = all.  Returns (src [E], rank [N]) as numpy int32: rank orders the eligible agents best first, and the
    `replace` worst of them get the best `parents` as sources in turn."""
    import numpy as np
    E = len(scores)
    sc = (RolloutScore * max(E, 1))()
    for e, s in enumerate(scores):
        if isinstance(s, RolloutScore):
            sc[e] = s
        else:
            sc[e].successes, sc[e].reward_sum = int(s[0]), float(s[1])
    el = None if eligible is None else np.ascontiguousarray(eligible, dtype=np.uint8)
    assert el is None or el.shape == (E,)
    src, rank = np.zeros(max(E, 1), dtype=np.int32), np.zeros(max(E, 1), dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    check(lib().frirl_hip_select_plan(sc, E, None if el is None else el.ctypes.data_as(C.POINTER(C.c_uint8)), parents, replace, src.ctypes.data_as(i32),
                                      rank.ctypes.data_as(i32)), "frirl_hip_select_plan")
    return src[:E], rank[: E if el is None else int((el != 0).sum())]


def batch_clone(batch, src, inherit_rows=False):
    """frirl_hip_batch_clone on a library-owned batch: agent e becomes a copy of agent src[e] (host sequence [E]); with inherit_rows
    the clones also take their sources' hyper-parameter, exploration and target rows.  Returns the number of agents cloned."""
    import numpy as np
    s = np.ascontiguousarray(src, dtype=np.int32)
    assert s.shape == (_batch_agents(batch),)
    cloned = C.c_int32(0)
    check(lib().frirl_hip_batch_clone(batch, s.ctypes.data_as(C.POINTER(C.c_int32)), 1 if inherit_rows else 0, C.byref(cloned)), "frirl_hip_batch_clone")
    return cloned.value


def batch_select(batch, n, parents, replace, start_states=None, inherit_rows=False):
    """frirl_hip_batch_select on a library-owned batch: evaluate every agent from n start states (host [E, n, nant-1] or None = its own),
    replace the `replace` worst by copies of the `parents` best.  Returns (list of RolloutScore, src numpy int32 [E], SelectResult)."""
    import numpy as np
    E = _batch_agents(batch)
    st = None if start_states is None else np.ascontiguousarray(start_states, dtype=np.float64)
    assert st is None or (st.ndim == 3 and st.shape[:2] == (E, n))
    scores, src, res = (RolloutScore * E)(), np.zeros(E, dtype=np.int32), SelectResult()
    check(lib().frirl_hip_batch_select(batch, n, None if st is None else st.ctypes.data_as(_DP), parents, replace, 1 if inherit_rows else 0, scores,
                                       src.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(res)), "frirl_hip_batch_select")
    return list(scores), src, res


def select_plan_device(scores, parents, replace, eligible=None, stream=None):
    """frirl_hip_select_plan_device: scores is the [E, 40] uint8 device tensor of Problem.rollout_batch(scores=True), eligible a device
    tensor [E] uint8 / bool or None = all.  Returns (src [E] int32, rank [E] int32 padded with -1, info [4] int32: N, status (PLAN_*),
    best, bad_agent) on the device.  Does not synchronise."""
    import torch
    assert scores.is_cuda and scores.dtype == torch.uint8 and scores.dim() == 2 and scores.shape[1] == C.sizeof(RolloutScore) and scores.is_contiguous()
    E = scores.shape[0]
    if eligible is not None:
        eligible = eligible.view(torch.uint8) if eligible.dtype == torch.bool else eligible
        assert eligible.is_cuda and eligible.dtype == torch.uint8 and eligible.shape == (E,) and eligible.is_contiguous()
    src = torch.empty((max(E, 1),), dtype=torch.int32, device=scores.device)
    rank, info = torch.empty_like(src), torch.empty((4,), dtype=torch.int32, device=scores.device)
    check(lib().frirl_hip_select_plan_device(_ptr(scores), E, _ptr(eligible), parents, replace, _ptr(src), _ptr(rank), _ptr(info), _stream(stream)),
          "frirl_hip_select_plan_device")
    return src, rank, info


def perturb_spec(seed=0, **columns):
    """A PerturbSpec from keywords named as PERTURB_COLUMNS: alpha / gamma / weight_significant / epsilon / horizon take
    (down, up, lo, hi), skip_rules / target / expected a flip probability.  Only the columns given are enabled."""
    unknown = set(columns) - set(PERTURB_COLUMNS)
    if unknown:
        raise TypeError(f"perturb_spec: unknown column(s) {sorted(unknown)}; the columns are {PERTURB_COLUMNS}")
    spec = PerturbSpec()
    spec.seed = int(seed)
    for name, v in columns.items():
        c = PERTURB_COLUMNS.index(name)
        spec.columns |= 1 << c
        if c < 5:
            spec.down[c], spec.up[c], spec.lo[c], spec.hi[c] = (float(x) for x in v)
        else:
            spec.flip[c - 5] = float(v)
    return spec


def perturb_rows(spec, generation, status, rows=None, explore=None, target=None, expect=None, stream=None):
    """frirl_hip_perturb_rows: the agents whose status ([E] int32 on the device, as Problem.clone_agents returns it) is CLONE_CLONED get
    the enabled columns of rows (HparamRows), explore (ExploreRows), target (TargetRows) and expect (ExpectRows) stepped or flipped in
    place under the draws of (spec.seed, agent, generation, column).  Returns the [1] int32 device tensor counting the agents touched.
    Does not synchronise."""
    import torch
    assert status.is_cuda and status.dtype == torch.int32 and status.dim() == 1 and status.is_contiguous()
    E = status.shape[0]
    count = torch.empty((1,), dtype=torch.int32, device=status.device)
    check(lib().frirl_hip_perturb_rows(C.byref(spec), int(generation), E, _ptr(status), _rows(rows, E), _rows(explore, E), _rows(target, E), _rows(expect, E),
                                       _ptr(count), _stream(stream)), "frirl_hip_perturb_rows")
    return count


def batch_evolve_step(batch, n, parents, replace, start_states=None, inherit_rows=False, spec=None):
    """frirl_hip_batch_evolve_step on a library-owned batch: evaluate, rank, plan, clone, inherit and (with a PerturbSpec) perturb on the
    batch's stream, one read-back.  start_states: host [E, n, nant-1] or None = every agent's own.  Returns the EvolveResult."""
    import numpy as np
    st = None if start_states is None else np.ascontiguousarray(start_states, dtype=np.float64)
    assert st is None or (st.ndim == 3 and st.shape[:2] == (_batch_agents(batch), n))
    res = EvolveResult()
    check(lib().frirl_hip_batch_evolve_step(batch, n, None if st is None else st.ctypes.data_as(_DP), parents, replace, 1 if inherit_rows else 0,
                                            None if spec is None else C.byref(spec), C.byref(res)), "frirl_hip_batch_evolve_step")
    return res


def batch_evolve(batch, generations, episodes_per_generation, n, parents, replace, start_states=None, inherit_rows=False, spec=None):
    """frirl_hip_batch_evolve: `generations` times frirl_hip_batch_train for episodes_per_generation more episodes, then
    batch_evolve_step.  Returns the list of EvolveResult, one per generation."""
    import numpy as np
    st = None if start_states is None else np.ascontiguousarray(start_states, dtype=np.float64)
    assert st is None or (st.ndim == 3 and st.shape[:2] == (_batch_agents(batch), n))
    res = (EvolveResult * max(generations, 1))()
    check(lib().frirl_hip_batch_evolve(batch, generations, episodes_per_generation, n, None if st is None else st.ctypes.data_as(_DP), parents, replace,
                                       1 if inherit_rows else 0, None if spec is None else C.byref(spec), res), "frirl_hip_batch_evolve")
    return list(res)[:generations]


def batch_get_hparams(batch):
    """frirl_hip_batch_get_hparams: dict of host arrays [E], one per column of HP_COLUMNS -- the row each agent trains under (the
    batch's own value where the column is not set)."""
    import numpy as np
    E = _batch_agents(batch)
    out = {k: np.zeros(E, dtype=np.int32 if k == "skip_rules" else np.float64) for k in HP_COLUMNS}
    desc = HparamRowsDesc()
    for k in HP_COLUMNS:
        setattr(desc, k, out[k].ctypes.data)
    check(lib().frirl_hip_batch_get_hparams(batch, C.byref(desc)), "frirl_hip_batch_get_hparams")
    return out


def batch_get_exploration(batch):
    """frirl_hip_batch_get_exploration: dict(epsilon float64 [E], horizon int32 [E]) -- the exploration row of every agent (the batch's
    epsilon / the rows' horizon_all where the column is not set)."""
    import numpy as np
    E = _batch_agents(batch)
    out = dict(epsilon=np.zeros(E), horizon=np.zeros(E, dtype=np.int32))
    desc = ExploreRowsDesc()
    desc.epsilon, desc.horizon = out["epsilon"].ctypes.data, out["horizon"].ctypes.data
    check(lib().frirl_hip_batch_get_exploration(batch, C.byref(desc)), "frirl_hip_batch_get_exploration")
    return out


def batch_reduce_all_map(batch, strategy, n, start_states=None, only_successful=True, cap=0):
    """frirl_hip_batch_reduce_all_map on a library-owned batch (the handle frirl_hip_batch_create returned): every agent's rule base
    reduced with the removals validated on the policy map at the points its greedy policy visits from n start states (start_states:
    host [E, n, nant-1] float64; None: n must be 1, every agent's own start).  cap: points per agent at most, 0 = 512; an agent with
    more is left untouched.  Returns (list of ReduceMapResult, ReduceMapTotals)."""
    import numpy as np
    st = None if start_states is None else np.ascontiguousarray(start_states, dtype=np.float64)
    stats = BatchStats()
    check(lib().frirl_hip_batch_stats(batch, C.byref(stats)), "frirl_hip_batch_stats")
    E = int(stats.agents)
    assert st is None or (st.ndim == 3 and st.shape[:2] == (E, n))
    res = (ReduceMapResult * E)()
    tot = ReduceMapTotals()
    check(lib().frirl_hip_batch_reduce_all_map(batch, strategy, n, None if st is None else st.ctypes.data_as(_DP), 1 if only_successful else 0, cap, res,
                                               C.byref(tot)), "frirl_hip_batch_reduce_all_map")
    return list(res), tot


def batch_reduce_all_map_orders(batch, order_set, n, start_states=None, only_successful=True, cap=0):
    """frirl_hip_batch_reduce_all_map_orders on a library-owned batch: batch_reduce_all_map with the reduction run over several candidate
    orders per agent, the smallest result kept.  order_set: bits 1 = |Q| ascending, 2 = |Q| descending, 4 = least-used first, 8 =
    most-used first (usage: Problem.rule_usage's sum at the agents' points).  Returns (list of ReduceOrdersResult, after_per_order
    [E, popcount(order_set)] numpy int32, ReduceMapTotals)."""
    import numpy as np
    st = None if start_states is None else np.ascontiguousarray(start_states, dtype=np.float64)
    stats = BatchStats()
    check(lib().frirl_hip_batch_stats(batch, C.byref(stats)), "frirl_hip_batch_stats")
    E = int(stats.agents)
    assert st is None or (st.ndim == 3 and st.shape[:2] == (E, n))
    res = (ReduceOrdersResult * E)()
    after = np.zeros((E, max(bin(order_set & 15).count("1"), 1)), dtype=np.int32)
    tot = ReduceMapTotals()
    check(lib().frirl_hip_batch_reduce_all_map_orders(batch, order_set, n, None if st is None else st.ctypes.data_as(_DP), 1 if only_successful else 0, cap,
                                                      res, after.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(tot)),
          "frirl_hip_batch_reduce_all_map_orders")
    return list(res), after, tot


def learn_demonstration(problem, agent, envs, demo, passes=1, stream=None):
    """frirl_hip_learn_demonstration: every agent replays its recorded log `demo` (Demonstration) `passes` times in one launch, as the
    chain of agent_begin / agent_observe calls with teacher = the logged action would.  Returns (replayed [E] int32: records
    consumed, refused [E] uint8: an append was refused at a full rule base).  Does not synchronise."""
    import torch
    assert demo.ns == problem.nant - 1 and demo.L in (1, problem.E) and (demo.length is None or demo.length.shape == (problem.E,))
    replayed = torch.empty((problem.E,), dtype=torch.int32, device=demo.obs.device)
    refused = torch.empty((problem.E,), dtype=torch.uint8, device=demo.obs.device)
    check(lib().frirl_hip_learn_demonstration(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), C.byref(envs.desc),
                                              C.byref(demo.desc), passes, _ptr(replayed), _ptr(refused), _stream(stream)),
          "frirl_hip_learn_demonstration")
    return replayed, refused


class PolicyRows:
    """Device-resident per-row episode state of a caller-stepped roll-out on one shared rule base (struct frirl_hip_policy_rows)."""

    def __init__(self, Q, device, exclude_mask=None, rule_slot=None):
        import torch
        self.Q = Q
        self.done = torch.zeros((Q,), dtype=torch.int32, device=device)
        self.ep_steps = torch.zeros((Q,), dtype=torch.int32, device=device)
        self.success = torch.zeros((Q,), dtype=torch.int32, device=device)
        self.ep_reward = torch.zeros((Q,), dtype=torch.float64, device=device)
        self.exclude_mask, self.rule_slot = exclude_mask, rule_slot
        if exclude_mask is not None:
            assert exclude_mask.shape == (Q,) and exclude_mask.dtype == torch.int32 and rule_slot.dtype == torch.uint8
        self.desc = PolicyRowsDesc(Q, self.done.data_ptr(), self.ep_steps.data_ptr(), self.success.data_ptr(), self.ep_reward.data_ptr(),
                                   _ptr(exclude_mask), _ptr(rule_slot))


class PolicyBatchRows:
    """Device-resident per-row episode state of caller-stepped roll-outs on EVERY agent's own rule base (struct
    frirl_hip_policy_batch_rows): E * n rows, row q belongs to agent q // n.  row_count / step_cap / agents: int32 tensors or None;
    exclude_mask [E * n] int32 with rule_slot [E, maxR] uint8; rows_live: [1] int32 the calls add the rows still running to."""

    def __init__(self, E, n, device, row_count=None, step_cap=None, agents=None, exclude_mask=None, rule_slot=None, rows_live=None):
        import torch
        self.E, self.n, self.Q = E, n, E * n
        Q = self.Q
        self.done = torch.zeros((Q,), dtype=torch.int32, device=device)
        self.ep_steps = torch.zeros((Q,), dtype=torch.int32, device=device)
        self.success = torch.zeros((Q,), dtype=torch.int32, device=device)
        self.ep_reward = torch.zeros((Q,), dtype=torch.float64, device=device)
        for x, shape in ((row_count, (E,)), (step_cap, (E,)), (rows_live, (1,)), (exclude_mask, (Q,))):
            assert x is None or (x.dtype == torch.int32 and x.shape == shape and x.is_contiguous())
        assert agents is None or (agents.dtype == torch.int32 and agents.dim() == 1 and agents.is_contiguous())
        if exclude_mask is not None:
            assert rule_slot.dtype == torch.uint8 and rule_slot.is_contiguous() and rule_slot.shape[0] == E
        self.row_count, self.step_cap, self.agents, self.rows_live = row_count, step_cap, agents, rows_live
        self.exclude_mask, self.rule_slot = exclude_mask, rule_slot
        self.desc = PolicyBatchRowsDesc(n, self.done.data_ptr(), self.ep_steps.data_ptr(), self.success.data_ptr(), self.ep_reward.data_ptr(),
                                        _ptr(row_count), _ptr(step_cap), _ptr(agents), 0 if agents is None else agents.numel(),
                                        _ptr(exclude_mask), _ptr(rule_slot), _ptr(rows_live))


class _ReducerBase:
    """What Reducer and BatchReducer share: the calls of a round on the handle self.h, named frirl_hip_<_name>_<call>."""
    _name = None

    def _call(self, call, *args):
        fn = f"frirl_hip_{self._name}_{call}"
        check(getattr(lib(), fn)(self.h, *args), fn)

    def __init_subclass__(cls):
        cls._observe_fn = f"frirl_hip_{cls._name}_observe"       # the per-step call: no name is built per step

    def _begin_out(self, obs):
        """The action tensors begin hands to the library, or None: fresh ones."""
        return None

    def begin(self, obs):
        io, action, action_idx = _agent_io(self.problem, obs, E=self.Q, out=self._begin_out(obs))
        self._call("begin", C.byref(io))
        self._out = (action, action_idx)
        return action, action_idx

    def observe(self, obs, reward, success, q_obs=None, count_live=True):
        """Returns (action values, action indices, rows still live or None when count_live is False: no synchronisation).  The
        action tensors are those begin returned, updated in place: rows whose replay has ended keep their last action."""
        io, action, action_idx = _agent_io(self.problem, obs, q_obs, reward, success, E=self.Q, out=getattr(self, "_out", None))
        live = C.c_int32()
        check(getattr(lib(), self._observe_fn)(self.h, C.byref(io), C.byref(live) if count_live else None), self._observe_fn)
        return action, action_idx, (live.value if count_live else None)

    def end_round(self):
        self._call("end_round")

    def close(self):
        if self.h:
            getattr(lib(), f"frirl_hip_{self._name}_destroy")(self.h)
            self.h = None

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            self.close()


class BatchReducer(_ReducerBase):
    """frirl_hip_batch_reducer: the rule-base reduction of EVERY rule base of `problem` with the caller's environment, round by round.
    starts = n (1..REDUCE_MAX_STARTS): every removal is validated against n start states per agent (frirl_hip_batch_reducer_create_starts;
    start_count [E] int32 or None = n, drop_bad_starts as Problem.reduce_batch_starts).  The rows of a round are then
    row (e * nodes + node) * n + k = tree node `node` of agent e from its start k (round 0: row e * n + k)."""
    _name = "batch_reducer"

    def __init__(self, problem, agent, strategy, reward_tolerance=0.0, depth=0, rant=None, active=None, stream=None, starts=None, start_count=None,
                 drop_bad_starts=False):
        import torch
        if rant is not None:
            assert rant.shape == (problem.E, problem.nant, problem.maxR) and rant.dtype == torch.float64 and rant.is_contiguous()
        if active is not None:
            assert active.shape == (problem.E,) and active.dtype in (torch.uint8, torch.bool) and active.is_contiguous()
        self.problem, self._keep = problem, (rant, active, agent, start_count)
        args = (C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), _ptr(rant), _ptr(active))
        if starts is None:
            assert start_count is None and not drop_bad_starts, "start_count and drop_bad_starts go with starts"
            fn = "frirl_hip_batch_reducer_create"
            self.h = lib().frirl_hip_batch_reducer_create(*args, strategy, reward_tolerance, depth, _stream(stream))
        else:
            if start_count is not None:
                assert start_count.shape == (problem.E,) and start_count.dtype == torch.int32 and start_count.is_contiguous()
            fn = "frirl_hip_batch_reducer_create_starts"
            st = ReduceStarts(int(starts), 1 if drop_bad_starts else 0, None, _ptr(start_count))
            self.h = lib().frirl_hip_batch_reducer_create_starts(*args, C.byref(st), strategy, reward_tolerance, depth, _stream(stream))
        if not self.h:
            raise FrirlHipError(f"{fn}: {lib().frirl_hip_last_error().decode()}")
        self.starts = lib().frirl_hip_batch_reducer_starts(self.h)
        self.Q = self.rows_per_agent = self.agents_live = 0

    def next_round(self):
        """Rows of the next round: E rows in round 0 (the baseline replays), then E * (2^depth - 1); 0 = finished.  Row q belongs to
        agent q // rows_per_agent."""
        q, n, live = C.c_int32(), C.c_int32(), C.c_int32()
        self._call("next_round", C.byref(q), C.byref(n), C.byref(live))
        self.Q, self.rows_per_agent, self.agents_live = q.value, n.value, live.value
        return q.value

    def _begin_out(self, obs):                  # rows that are never stepped hold action 0.0
        import torch
        return (torch.zeros((self.Q,), dtype=torch.float64, device=obs.device), torch.zeros((self.Q,), dtype=torch.int32, device=obs.device))

    def row_done(self):
        """[Q] int32 view of the reducer's own `done` array: 1 = the caller need not step this row."""
        import torch
        if self.Q == 0:
            return torch.zeros((0,), dtype=torch.int32, device=self.problem.rb.device)
        iface = {"shape": (self.Q,), "typestr": "<i4", "data": (lib().frirl_hip_batch_reducer_row_done(self.h), False), "version": 2}
        holder = type("_DevArray", (), {"__cuda_array_interface__": iface})()
        return torch.as_tensor(holder, device=self.problem.rb.device)

    def result(self):
        """(list of kept original indices, list of ReduceResult) so far; between rounds only."""
        import numpy as np
        E = self.problem.E
        kept = np.zeros((E, self.problem.maxR), dtype=np.int32)
        res = (ReduceResult * E)()
        self._call("result", kept.ctypes.data_as(C.POINTER(C.c_int32)), res)
        return [kept[e, : res[e].rules_after].copy() for e in range(E)], list(res)

    def result_starts(self):
        """Per-start ReduceStartResult [E][n] so far (n = 1 for a reducer made without starts); between rounds only."""
        E, n = self.problem.E, self.starts
        per = (ReduceStartResult * (E * n))()
        self._call("result_starts", per)
        return [[per[e * n + k] for k in range(n)] for e in range(E)]


class Reducer(_ReducerBase):
    """frirl_hip_reducer: the rule-base reduction of ONE rule base (problem.E == 1) with the caller's environment, round by round."""
    _name = "reducer"

    def __init__(self, problem, agent, strategy, reward_tolerance=0.0, depth=0, rant=None, stream=None):
        assert problem.E == 1
        self.problem, self.R0 = problem, int(problem.nrules[0].item())
        self.h = lib().frirl_hip_reducer_create(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), _ptr(rant), strategy,
                                                reward_tolerance, depth, _stream(stream))
        if not self.h:
            raise FrirlHipError(f"frirl_hip_reducer_create: {lib().frirl_hip_last_error().decode()}")
        self.Q = 0

    def next_round(self):
        """Rows to replay from the start state in the next round (round 0: the baseline replay, 1 row); 0 = finished."""
        q = C.c_int32()
        self._call("next_round", C.byref(q))
        self.Q = q.value
        return q.value

    def result(self):
        """(kept original indices, ReduceResult) so far."""
        import numpy as np
        kept = np.zeros(self.R0, dtype=np.int32)
        res = ReduceResult()
        self._call("result", kept.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(res))
        return kept[: res.rules_after], res


def _reduce_rounds(red, reset_fn, step_fn, result=None):
    """The round loop of reduce_external / reduce_external_batch on an open reducer; reset_fn(red) -> obs of the round's rows."""
    import torch
    try:
        while red.next_round() > 0:
            states = reset_fn(red).contiguous()
            action, _ = red.begin(states)
            live = red.Q
            while live > 0:
                out = step_fn(states, action)
                obs, reward, success = out[0].contiguous(), out[1].contiguous(), out[2].to(torch.int32).contiguous()
                nxt, _, live = red.observe(obs, reward, success, q_obs=out[3].contiguous() if len(out) > 3 else None)
                states, action = obs, nxt          # rows that are done keep their last action; what they return is no longer read
            red.end_round()
        return red.result() if result is None else result(red)
    finally:
        red.close()


def reduce_external(problem, agent, reset_fn, step_fn, strategy, reward_tolerance=0.0, depth=0, rant=None):
    """The reduction's round loop with the caller's environment: reset_fn(Q) -> obs [Q, nant-1] (Q environments at the start state),
    step_fn(states, action) -> obs, reward, success or obs, reward, success, q_obs (q_obs: the environment's own quantiser).
    Returns (kept original indices, ReduceResult); compacts problem's rule base in place."""
    return _reduce_rounds(Reducer(problem, agent, strategy, reward_tolerance, depth, rant), lambda red: reset_fn(red.Q), step_fn)


def reduce_external_batch(problem, agent, reset_fn, step_fn, strategy, reward_tolerance=0.0, depth=0, rant=None, active=None):
    """The batched reduction's round loop with the caller's environment, every rule base of `problem` at once:
    reset_fn(Q, rows_per_agent) -> obs [Q, nant-1] with agent q // rows_per_agent's start state in row q; step_fn as for
    reduce_external.  Returns (list of kept original indices, list of ReduceResult), as Problem.reduce_batch; compacts in place."""
    return _reduce_rounds(BatchReducer(problem, agent, strategy, reward_tolerance, depth, rant, active),
                          lambda red: reset_fn(red.Q, red.rows_per_agent), step_fn)


def reduce_external_batch_starts(problem, agent, reset_fn, step_fn, strategy, n, reward_tolerance=0.0, depth=0, rant=None, active=None,
                                 start_count=None, drop_bad_starts=False):
    """reduce_external_batch with every removal validated against n start states per agent (BatchReducer(starts=n)):
    reset_fn(Q, rows_per_agent, n) -> obs [Q, nant-1] with start q % n of agent q // rows_per_agent in row q; step_fn as for
    reduce_external.  Returns (kept, results, per_start) as Problem.reduce_batch_starts; compacts in place."""
    red = BatchReducer(problem, agent, strategy, reward_tolerance, depth, rant, active, starts=n, start_count=start_count, drop_bad_starts=drop_bad_starts)
    return _reduce_rounds(red, lambda r: reset_fn(r.Q, r.rows_per_agent, n), step_fn, result=lambda r: r.result() + (r.result_starts(),))


def dist():
    """The multi-GPU helper module (fri-reinforcementlearning-c_amd/dist.py)."""
    import importlib.util
    import sys
    if "frirl_amd_dist" in sys.modules:
        return sys.modules["frirl_amd_dist"]
    spec = importlib.util.spec_from_file_location("frirl_amd_dist", os.path.join(PKG_DIR, "dist.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["frirl_amd_dist"] = mod
    spec.loader.exec_module(mod)
    return mod


DROPIN_LIB_PATH = os.path.join(PKG_DIR, "lib", "libfrirl_dropin.so")
_dropin = None


def dropin():
    """ctypes handle of the ANSI-C drop-in library (the reference's five_* / FIVE_* / frirl_* API)."""
    global _dropin
    if _dropin is None:
        lib()                                   # loads torch's HIP runtime + libfrirl_hip.so first
        if not os.path.exists(DROPIN_LIB_PATH):
            raise FrirlHipError(f"{DROPIN_LIB_PATH} is missing: run build() first")
        D = C.CDLL(DROPIN_LIB_PATH)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        D.frirl_demo_describe.restype = C.c_int
        D.frirl_demo_describe.argtypes = [C.c_char_p, ip, ip, ip, dp, dp, dp, ip, dp, dp, dp, dp, ip]
        D.frirl_describe_tables.restype = C.c_int
        D.frirl_describe_tables.argtypes = [C.c_int, C.c_int, ip, dp, dp, dp, dp, dp, dp]
        D.frirl_gen_fixres_arr.restype = None
        D.frirl_gen_fixres_arr.argtypes = [dp, C.c_int, C.c_double]
        _dropin = D
    return _dropin


def episode_steps(problem, agent, envs, nsteps, stream=None):
    check(lib().frirl_hip_episode_steps(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), C.byref(envs.desc), nsteps,
                                        _stream(stream)), "frirl_hip_episode_steps")


def episode_run(problem, agent, envs, nsteps, lds_rules, stream=None):
    """frirl_hip_episode_run: up to nsteps steps per environment in ONE launch, rule bases resident in LDS."""
    check(lib().frirl_hip_episode_run(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), C.byref(envs.desc), nsteps, lds_rules,
                                      _stream(stream)), "frirl_hip_episode_run")


def episode_run_lanes(problem, agent, envs, nsteps, workspace=None, stream=None):
    """frirl_hip_episode_run_lanes: lane-group episodes for many agents with small rule bases; `workspace` is a
    float64 CUDA tensor of >= lanes_workspace_elems(problem, agent) elements (allocated and cached on the problem if None)."""
    import torch
    need = lib().frirl_hip_lanes_workspace_bytes(problem.nant, problem.E, problem.maxR, agent.A)
    if workspace is None:
        workspace = getattr(problem, "_lanes_ws", None)
        if workspace is None or workspace.numel() * 8 < need:
            workspace = torch.empty((need // 8,), dtype=torch.float64, device=problem.rb.device)
            problem._lanes_ws = workspace
    check(lib().frirl_hip_episode_run_lanes(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), C.byref(envs.desc), nsteps,
                                            _ptr(workspace), workspace.numel() * 8, _stream(stream)), "frirl_hip_episode_run_lanes")


def can_run_persistent(problem, agent):
    return agent.A <= 8 and 2 * 8 * problem.nant * problem.U <= 16 * 1024


class Convergence:
    """Device-resident construct-loop bookkeeping (struct frirl_hip_convergence)."""

    def __init__(self, problem, device):
        import torch
        E, maxR = problem.E, problem.maxR
        self.prev_nrules = torch.zeros((E,), dtype=torch.int32, device=device)
        self.prev_steps = torch.zeros((E,), dtype=torch.int32, device=device)
        self.prev_reward = torch.zeros((E,), dtype=torch.float64, device=device)
        self.prev_rconc = torch.zeros((E, maxR), dtype=torch.float64, device=device)
        self.converged = torch.zeros((E,), dtype=torch.int32, device=device)
        self.episodes = torch.zeros((E,), dtype=torch.int32, device=device)
        self.full = torch.zeros((E,), dtype=torch.bool, device=device)     # agents whose rule base refused an append (capacity)
        self.epended = torch.zeros((E,), dtype=torch.int32, device=device)  # the cheap "same as the previous episode" test held (frirl_desc.epended)
        self.desc = ConvergenceDesc(self.prev_nrules.data_ptr(), self.prev_steps.data_ptr(), self.prev_reward.data_ptr(),
                                    self.prev_rconc.data_ptr(), self.converged.data_ptr(), self.episodes.data_ptr(), self.epended.data_ptr())
        check(lib().frirl_hip_convergence_init(C.byref(problem.bases), problem.nant, C.byref(self.desc), _stream()), "frirl_hip_convergence_init")

    @property
    def full_envs(self):
        """Number of agents that hit FRIRL_HIP_UPD_FULL at least once: their TD updates were dropped from then on."""
        return int(self.full.sum().item())

    def update(self, problem, agent, envs, stream=None):
        self.full |= (envs.status == UPD_FULL) | (problem.nrules >= problem.maxR)     # an append was (or will be) refused
        check(lib().frirl_hip_convergence_update(C.byref(problem.bases), problem.nant, C.byref(agent.desc), C.byref(envs.desc), C.byref(self.desc),
                                                 _stream(stream)), "frirl_hip_convergence_update")


def train(problem, agent, envs, max_episodes=1000, check_every=50, on_episode=None, persistent=True, persistent_max_rules=256, lanes=None, rows=None, explore=None, target=None):
    """Batched construct run: frirl_sequential_run's loop (reference frirl_sequential_run.c:55-165) for E agents
    at once.  Episodes run until every environment's rule base is "considered complete" or max_episodes-1 episodes
    have run (:51,59).  Converged environments are masked out of later episodes.  Returns the Convergence object.
    rows (an HparamRows): only the persistent learner takes per-agent hyper-parameters, so the run goes through train_persistent
    (on_episode is not called) or raises FrirlHipError where it does not cover the shape.  explore (an ExploreRows), target (a TargetRows): likewise."""
    import torch
    if rows is not None or explore is not None or target is not None:
        if not learn_supported(problem, agent):
            raise FrirlHipError("frirl_amd.train: rows= / explore= / target= need the persistent learner (learn_supported), which does not cover this shape; "
                                "the per-episode kernels take no per-agent hyper-parameters, exploration or TD target")
        return train_persistent(problem, agent, envs, max_episodes=max_episodes, rows=rows, explore=explore, target=target).conv
    conv = Convergence(problem, problem.rb.device)
    max_steps = agent.desc.max_steps
    if lanes is None:           # lane-group kernel where it is the faster form (many agents / small rule bases)
        lanes = bool(lib().frirl_hip_lanes_preferred(problem.nant, problem.E, agent.A))
    for ep in range(1, max_episodes):
        episode_begin(problem, agent, envs)
        envs.done.copy_(torch.maximum(envs.done, conv.converged))       # converged agents sit this episode out
        steps = 0
        if lanes:
            # many agents, small rule bases: lane-group kernel, the whole episode in one launch (no reductions / barriers)
            episode_run_lanes(problem, agent, envs, max_steps)
            steps = max_steps
        elif persistent and can_run_persistent(problem, agent):
            # small rule bases: the whole episode in one launch out of LDS; an environment whose rule base outgrows
            # the LDS slab comes back not-done (status FULL) and finishes through the step kernel below
            # (measured: it pays only while the LDS slab is small enough for >= ~12 waves per CU, i.e. the 256-rule slab;
            #  larger slabs cut the number of resident environments more than they cut the per-step latency)
            need = int(problem.nrules.max().item()) + 128
            if need <= persistent_max_rules:
                episode_run(problem, agent, envs, max_steps, 256 if need <= 256 else (512 if need <= 512 else 1024))
                if bool((envs.done != 0).all()):
                    steps = max_steps
        while steps < max_steps:
            n = min(check_every, max_steps - steps)
            episode_steps(problem, agent, envs, n)
            steps += n
            if bool((envs.done != 0).all()):
                break
        conv.update(problem, agent, envs)
        if on_episode is not None:
            on_episode(ep, conv)
        if bool((conv.converged != 0).all()):
            break
    if conv.full_envs:
        import warnings
        warnings.warn(f"frirl_amd.train: {conv.full_envs} of {problem.E} rule bases reached their capacity of {problem.maxR} rules: "
                      "appends were refused (FRIRL_HIP_UPD_FULL) and those TD updates dropped", RuntimeWarning)
    return conv


def learn_supported(problem, agent):
    """True when frirl_hip_learn_run (the persistent construct loop) covers this shape."""
    return problem.uidx is not None and bool(lib().frirl_hip_learn_supported(problem.nant, problem.U, agent.A, agent.desc.p, agent.desc.env_kind))


class LearnRun:
    """Result of train_persistent: the Convergence object plus per-agent totals (device tensors)."""

    def __init__(self, conv, steps_total, work, launches):
        self.conv, self.steps_total, self.work, self.launches = conv, steps_total, work, launches


def train_persistent(problem, agent, envs, max_episodes=1000, budget=4096, on_chunk=None, stream=None, rows=None, explore=None, target=None, expect=None):
    """The construct loop of frirl_sequential_run for E agents through frirl_hip_learn_train: every agent runs its episodes
    back to back on the device; after each launch (the work of `budget` steps of a mean agent) the agents that are still
    learning are compacted and launched again until none is left -- the launch plan, the queue and the compaction are the
    library's (csrc/learn.hip), the host reads two counters per launch.  on_chunk(launch index, live agent ids, conv) is
    called after every launch (the place for the per-chunk reward statistics).  rows: an HparamRows (frirl_hip_learn_train_rows):
    agent e learns under its own values of the columns given.  explore: an ExploreRows (frirl_hip_learn_train_explore): agent e
    picks at its own epsilon, annealed over its own horizon.  target: a TargetRows (frirl_hip_learn_train_target): agent e learns
    towards Q(s', a') or Q(s', g).  expect: an ExpectRows (frirl_hip_learn_train_expect): a flagged agent learns towards the expectation
    of Q(s', .) under its own pick.  Returns a LearnRun."""
    import torch
    dev_ = problem.rb.device
    conv = Convergence(problem, dev_)
    envs.done.fill_(1)                                   # fresh agents: every one starts its first episode
    steps_total = torch.zeros((problem.E,), dtype=torch.int64, device=dev_)
    work = torch.zeros((problem.E, 2), dtype=torch.int64, device=dev_)
    need = lib().frirl_hip_learn_train_workspace_bytes(problem.nant, problem.E, problem.maxR, agent.A)
    ws = getattr(problem, "_learn_ws", None)
    if ws is None or ws.numel() * 8 < need:
        ws = torch.empty(((need + 7) // 8,), dtype=torch.float64, device=dev_)
        problem._learn_ws = ws
    problem._learn_progress = (steps_total, work)        # for on_chunk callbacks that report per-launch progress
    ws32 = ws.view(torch.int32)
    failure = []

    def chunk(_user, launch, live_ptr, n):               # `live` is a slice of the workspace
        try:
            off = (live_ptr - ws.data_ptr()) // 4
            on_chunk(launch, ws32[off:off + n], conv)
        except BaseException as exc:                     # an exception must not unwind through the C frame
            failure.append(exc)
    cb = LEARN_CHUNK_FN(chunk) if on_chunk is not None else C.cast(None, LEARN_CHUNK_FN)
    launches = C.c_int32(0)
    refused = conv.full.view(torch.uint8)
    fn, name, structs, _ = _level_entry("frirl_hip_learn_train", problem.E, rows, explore, target, expect=expect)
    check(fn(C.byref(problem.tables), C.byref(problem.bases), C.byref(agent.desc), *structs, C.byref(envs.desc), C.byref(conv.desc), budget, max_episodes,
             _ptr(work), _ptr(steps_total), _ptr(refused), _ptr(ws), ws.numel() * 8, C.byref(launches), cb, None, _stream(stream)), name)
    if failure:
        raise failure[0]
    if conv.full_envs:
        import warnings
        warnings.warn(f"frirl_amd.train_persistent: {conv.full_envs} of {problem.E} rule bases reached their capacity of {problem.maxR} rules: "
                      "appends were refused (FRIRL_HIP_UPD_FULL) and those TD updates dropped", RuntimeWarning)
    return LearnRun(conv, steps_total, work, launches.value)


def demo_describe(env):
    """Tables, grids and hyper-parameters of a demo, built by the drop-in library's own host functions
    (frirl_init_ve etc.); no GPU needed."""
    import numpy as np
    D = dropin()
    ns, U, A, ms = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    if D.frirl_demo_describe(env.encode(), C.byref(ns), C.byref(U), C.byref(A), None, None, None, None, None, None, None, None, C.byref(ms)) != 0:
        raise ValueError(f"unknown demo environment {env!r}")
    nant = ns.value + 1
    u, ve = np.zeros((nant, U.value)), np.zeros((nant, U.value))
    grid = np.zeros((nant, MAX_GRID))
    grid_len = np.zeros(nant, dtype=np.int32)
    grid_div, values_def = np.zeros(nant), np.zeros(nant)
    action_ve, hp = np.zeros(A.value), np.zeros(8)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = D.frirl_demo_describe(env.encode(), C.byref(ns), C.byref(U), C.byref(A), u.ctypes.data_as(dp), ve.ctypes.data_as(dp),
                               grid.ctypes.data_as(dp), grid_len.ctypes.data_as(ip), grid_div.ctypes.data_as(dp),
                               values_def.ctypes.data_as(dp), action_ve.ctypes.data_as(dp), hp.ctypes.data_as(dp), C.byref(ms))
    assert rc == 0
    return dict(env=env, kind=ENV_KINDS[env], nstates=ns.value, nant=nant, U=U.value, A=A.value, u=u, ve=ve,
                grids=[grid[k, : grid_len[k]].copy() for k in range(nant)], grid_div=grid_div, values_def=values_def, action_ve=action_ve,
                alpha=hp[0], gamma=hp[1], qdiff_pos=hp[2], qdiff_neg=hp[3], weight_thr=hp[4], skip_rules=int(hp[5]),
                reward_good_above=hp[6], qdiff_final_tolerance=hp[7], max_steps=ms.value)


def demo_batch(env, E, R, maxR, device, seed=0, max_steps=None, compressed=True, keep_rant=True):
    """E environments of a demo on `device`, each with a private synthetic rule base of R rules: the 2^nant
    corner rules first (reference frirl_init_rb.c:99-126, Q = 0), then rules on the universe grid (uniform
    indices; action column on the A action values) with Q ~ U(-1500, 1500).
    Returns (Problem, Agent, Envs)."""
    import numpy as np
    import torch
    d = demo_describe(env)
    nant, U, A = d["nant"], d["U"], d["A"]
    assert maxR >= R and maxR % 2 == 0 and R >= 2 ** nant
    g = torch.Generator(device=device).manual_seed(0x5EED0000 + seed)
    u_d, ve_d = torch.from_numpy(d["u"]).to(device), torch.from_numpy(d["ve"]).to(device)
    rb = torch.zeros((E, nant + 1, maxR), dtype=torch.float64, device=device)
    rant = torch.zeros((E, nant, maxR), dtype=torch.float64, device=device) if keep_rant else None     # raw antecedents (rule-base dumps only)
    uidx = torch.zeros((E, nant, maxR), dtype=torch.int16, device=device) if compressed else None
    ncorner = 2 ** nant
    # action universe index of every action value (nearest universe point, as FIVE_add_rule snaps it)
    ua = d["u"][nant - 1]
    a_idx = torch.tensor([int(np.argmin(np.abs(ua - v))) for v in d["grids"][nant - 1]], device=device)
    for k in range(nant):
        idx = torch.randint(0, U, (E, R), generator=g, device=device)
        if k == nant - 1:
            idx = a_idx[torch.randint(0, A, (E, R), generator=g, device=device)]
        gk = d["grids"][k]
        lo_i, hi_i = int(np.argmin(np.abs(d["u"][k] - gk.min()))), int(np.argmin(np.abs(d["u"][k] - gk.max())))
        divider = ncorner >> (k + 1)
        corner = torch.tensor([lo_i if ((j // divider) % 2) == 0 else hi_i for j in range(ncorner)], device=device)
        idx[:, :ncorner] = corner[None]
        rb[:, k, :R] = ve_d[k][idx]
        if keep_rant:
            rant[:, k, :R] = u_d[k][idx]
        if compressed:
            uidx[:, k, :R] = idx.to(torch.int16)
        del idx
    rb[:, nant, ncorner:R] = torch.rand((E, R - ncorner), generator=g, device=device, dtype=torch.float64) * 3000.0 - 1500.0
    nrules = torch.full((E,), R, dtype=torch.int32, device=device)
    prob = Problem(u_d, ve_d, rb, nrules, uidx)
    agent = demo_agent(d, device, max_steps)
    envs = Envs(prob, device, keep_rant=keep_rant, rant_init=rant)
    return prob, agent, envs


def demo_agent(d, device, max_steps=None, p=0, **kw):
    return Agent(device, d["nant"], d["grids"], d["grid_div"], d["values_def"], d["action_ve"], d["alpha"], d["gamma"], d["qdiff_pos"],
                 d["qdiff_neg"], d["weight_thr"], d["skip_rules"], p, d["kind"], max_steps or d["max_steps"],
                 reward_good_above=d["reward_good_above"], qdiff_final_tolerance=d["qdiff_final_tolerance"], **kw)


def describe(states, actions, U, alpha, gamma, qdiff_pos, qdiff_neg, weight_thr=0.05, skip_rules=1, reward_good_above=0.0,
             qdiff_final_tolerance=250.0, max_steps=1000, name="external"):
    """Tables, grids and hyper-parameters of the caller's own environment, in the form demo_describe returns (kind = ENV_EXTERNAL),
    built by the drop-in library's frirl_describe_tables (the reference's frirl_init_ve etc.); no GPU needed.
      states:  one dict per state dimension (struct frirl_dimension_desc): "values" (its grid of possible rule places) or "n" (that
               many values at step "div" around 0, frirl_gen_fixres_arr), "div" (values_div: the generic quantiser's step),
               "steep" (values_steep, default 1.0), "default" (values_def, default 0.0), "universe_div" (step of its universe)
      actions: dict with "values" (the action values) or "n" + "div", and "universe_div"
      U:       points per universe (universe_len, the same for every dimension)"""
    import numpy as np
    D = dropin()
    dims = list(states) + [dict(actions, steep=0.0, default=0.0)]
    nant = len(dims)
    assert 2 <= nant <= MAX_NANT - 1
    grid = np.zeros((nant, MAX_GRID))
    grid_len = np.zeros(nant, dtype=np.int32)
    grid_div, values_def, steep, udiv = np.zeros(nant), np.zeros(nant), np.zeros(nant), np.zeros(nant)
    for k, d in enumerate(dims):
        if d.get("values") is not None:
            v = np.asarray(d["values"], dtype=np.float64)
        else:
            v = np.zeros(int(d["n"]))
            D.frirl_gen_fixres_arr(v.ctypes.data_as(C.POINTER(C.c_double)), len(v), float(d["div"]))
        assert 1 <= len(v) <= MAX_GRID
        grid[k, : len(v)] = v
        grid_len[k] = len(v)
        grid_div[k], values_def[k] = float(d.get("div", 0.0)), float(d.get("default", 0.0))
        steep[k], udiv[k] = float(d.get("steep", 1.0)), float(d["universe_div"])
    A = int(grid_len[-1])
    u, ve, action_ve = np.zeros((nant, U)), np.zeros((nant, U)), np.zeros(A)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    if D.frirl_describe_tables(nant - 1, U, grid_len.ctypes.data_as(ip), grid.ctypes.data_as(dp), steep.ctypes.data_as(dp), udiv.ctypes.data_as(dp),
                               u.ctypes.data_as(dp), ve.ctypes.data_as(dp), action_ve.ctypes.data_as(dp)) != 0:
        raise ValueError("frirl_describe_tables refused the description (nant 2..15, U >= 2, 1..64 grid values, 1..32 actions, universe_div > 0)")
    return dict(env=name, kind=ENV_EXTERNAL, nstates=nant - 1, nant=nant, U=U, A=A, u=u, ve=ve,
                grids=[grid[k, : grid_len[k]].copy() for k in range(nant)], grid_div=grid_div, values_def=values_def, action_ve=action_ve,
                alpha=float(alpha), gamma=float(gamma), qdiff_pos=float(qdiff_pos), qdiff_neg=float(qdiff_neg), weight_thr=float(weight_thr),
                skip_rules=int(skip_rules), reward_good_above=float(reward_good_above), qdiff_final_tolerance=float(qdiff_final_tolerance),
                max_steps=int(max_steps))


def fresh_batch(desc, E, maxR, device, start_states=None, **agent_kw):
    """E agents of the environment `desc` (describe / demo_describe) starting from the reference's initial rule base: the 2^nant
    corner rules with Q = 0 (frirl_init_rb.c:99-126), grid min/max as antecedents.  Returns (Problem, Agent, Envs)."""
    import numpy as np
    import torch
    d = desc
    nant = d["nant"]
    ncorner = 2 ** nant
    assert maxR % 2 == 0 and maxR >= ncorner
    u_d, ve_d = torch.from_numpy(d["u"]).to(device), torch.from_numpy(d["ve"]).to(device)
    rant0 = np.zeros((nant, ncorner))
    for k in range(nant):
        gk = d["grids"][k]
        divider = ncorner >> (k + 1)
        rant0[k] = [gk.min() if ((j // divider) % 2) == 0 else gk.max() for j in range(ncorner)]
    prob = Problem(u_d, ve_d, torch.zeros((E, nant + 1, maxR), dtype=torch.float64, device=device),
                   torch.zeros((E,), dtype=torch.int32, device=device), torch.zeros((E, nant, maxR), dtype=torch.int16, device=device))
    agent = demo_agent(d, device, **agent_kw)
    envs = Envs(prob, device, start_states=start_states)
    for j in range(ncorner):        # FIVE_add_rule per corner, exactly as FIVEInit does for the initial rules
        ra = torch.from_numpy(np.ascontiguousarray(rant0[:, j])).to(device).expand(E, nant).contiguous()
        prob.add_rule(ra, torch.zeros((E,), dtype=torch.float64, device=device), rant_store=envs.rant)
    return prob, agent, envs


def demo_fresh_batch(env, E, maxR, device, start_states=None, **agent_kw):
    """E agents of a demo starting from the reference's initial rule base (fresh_batch).  Returns (Problem, Agent, Envs)."""
    return fresh_batch(demo_describe(env), E, maxR, device, start_states=start_states, **agent_kw)
