"""ctypes binding of libcattleherd.so (C ABI in include/cattleherd.h).

The product path has no CPU fallback: if the HIP library is missing or no device is visible,
``lib()`` / ``HerdBatch`` raise.
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CH_LIB_PATH") or os.path.join(_PKG, "libcattleherd.so")  # override: A/B diagnostics

CH_OK, CH_ERR_INVALID, CH_ERR_DEVICE, CH_ERR_NOMEM, CH_ERR_UNSUPPORTED = 0, -1, -2, -3, -4
CH_MODE_CTDE, CH_MODE_MARL = 0, 1
CH_PREC_F64, CH_PREC_F32 = 0, 1
CH_STEP_AUTORESET, CH_STEP_RANDOM_ACTIONS = 0x1, 0x2
METRIC_NAMES = ("steps", "episodes", "return_sum", "length_sum", "terminated", "truncated", "nan_rewards",
                "effectiveness_sum")
ABI_VERSION = 6
# Physics enum (utils/enums.py:13-21, include/cattleherd.h CH_PHYS_*)
PHYSICS = {"pyb": 0, "dyn": 1, "pyb_gnd": 2, "pyb_drag": 3, "pyb_dw": 4, "pyb_gnd_drag_dw": 5, "dyn_rk4": 6}

# every symbol include/cattleherd.h declares
EXPORTS = ("ch_default_config", "ch_create", "ch_destroy", "ch_last_error", "ch_shape", "ch_reset", "ch_reset_with",
           "ch_step", "ch_step_n",
           "ch_state_size", "ch_get_state", "ch_set_state", "ch_metrics", "ch_metrics_device", "ch_sync",
           "ch_get_eval", "ch_builtin_spawn_table", "ch_rollout_store", "ch_rollout_post", "ch_rollout_gae", "ch_rollout_collect",
           "ch_spawn_table", "ch_mlp_forward", "ch_mlp_forward_masked", "ch_policy_forward", "ch_mlp_packed_size",
           "ch_mlp_pack", "ch_outputs_to_host", "ch_marl_rollout_collect", "ch_ppo_param_count", "ch_ppo_scratch_size",
           "ch_ppo_grad", "ch_ppo_adam", "ch_ppo_train", "ch_marl_ppo_param_count", "ch_marl_ppo_scratch_size",
           "ch_marl_ppo_grad", "ch_marl_ppo_adam", "ch_marl_ppo_train", "ch_eval_begin", "ch_eval_record",
           "ch_evaluate_policy", "ch_marl_eval_begin", "ch_marl_eval_mark", "ch_marl_eval_record",
           "ch_marl_evaluate_policy", "ch_eval_log_begin", "ch_eval_log_mark", "ch_eval_log_record", "ch_eval_log_run",
           "ch_ep_ring_begin", "ch_ep_ring_record", "ch_rollout_collect_log", "ch_ppo_train_log",
           "ch_explained_variance_scratch", "ch_explained_variance", "ch_marl_ep_ring_begin", "ch_marl_ep_ring_record",
           "ch_marl_rollout_collect_log", "ch_marl_ppo_train_log", "ch_ppo_train_opt", "ch_norm_scratch_size",
           "ch_norm_begin", "ch_norm_obs_update", "ch_norm_obs_apply", "ch_norm_reward", "ch_rollout_collect_norm",
           "ch_ppo_pop_create", "ch_ppo_pop_destroy", "ch_ppo_train_pop", "ch_rollout_pop_create",
           "ch_rollout_pop_destroy", "ch_rollout_collect_pop", "ch_ep_ring_pop_begin", "ch_ep_ring_pop_record",
           "ch_rollout_collect_pop_log", "ch_ep_ring_pop_summary", "ch_explained_variance_pop_scratch",
           "ch_explained_variance_pop")
# the on-device evaluations' symbols: an older library (an A/B baseline loaded through CH_LIB_PATH) lacks them
_EVAL_EXPORTS = ("ch_eval_begin", "ch_eval_record", "ch_evaluate_policy", "ch_marl_eval_begin", "ch_marl_eval_mark",
                 "ch_marl_eval_record", "ch_marl_evaluate_policy", "ch_eval_log_begin", "ch_eval_log_mark",
                 "ch_eval_log_record", "ch_eval_log_run")
# the SB3 training log's symbols (cattleherd/train_log.py): an older library lacks them too
_TRAIN_LOG_EXPORTS = ("ch_ep_ring_begin", "ch_ep_ring_record", "ch_rollout_collect_log", "ch_ppo_train_log",
                      "ch_explained_variance_scratch", "ch_explained_variance")
# the RLlib training log's (cattleherd/train_log.py, the MARL half): likewise
_MARL_TRAIN_LOG_EXPORTS = ("ch_marl_ep_ring_begin", "ch_marl_ep_ring_record", "ch_marl_rollout_collect_log",
                           "ch_marl_ppo_train_log")
# ch_marl_ppo_train_log's columns: ch_marl_ppo_train's five, then vf_loss_unclipped, total_loss, vf_explained_var
CH_MARL_PPO_LOG_STATS = 8
CH_PPO_LOG_STATS = 6   # ch_ppo_train_log's columns: policy loss, value loss, mean entropy, grad norm, approx_kl, clip_fraction
# target_kl / clip_range_vf (cattleherd/ppo.py): likewise
_PPO_OPT_EXPORTS = ("ch_ppo_train_opt",)
CH_PPO_OPT_STATS = 7   # ch_ppo_train_opt's columns: ch_ppo_train_log's six, then the step's state (1 applied, 0 tripped, -1 not run)
# the device-side VecNormalize's (cattleherd/vec_normalize.py): likewise
_NORM_EXPORTS = ("ch_norm_scratch_size", "ch_norm_begin", "ch_norm_obs_update", "ch_norm_obs_apply", "ch_norm_reward",
                 "ch_rollout_collect_norm")
# the population update's (cattleherd/ppo_pop.py): likewise
_PPO_POP_EXPORTS = ("ch_ppo_pop_create", "ch_ppo_pop_destroy", "ch_ppo_train_pop")
# the population collection's (cattleherd/rollout_pop.py): likewise
_ROLLOUT_POP_EXPORTS = ("ch_rollout_pop_create", "ch_rollout_pop_destroy", "ch_rollout_collect_pop")
# the population's training log (cattleherd/train_log.py PopulationEpisodeRing, explained_variance_pop): likewise
_TRAIN_LOG_POP_EXPORTS = ("ch_ep_ring_pop_begin", "ch_ep_ring_pop_record", "ch_rollout_collect_pop_log",
                          "ch_ep_ring_pop_summary", "ch_explained_variance_pop_scratch", "ch_explained_variance_pop")
CH_EP_RING_POP_SUMMARY = 4   # ch_ep_ring_pop_summary's columns: count, mean return, mean length, total
CH_ACT_NONE, CH_ACT_TANH, CH_ACT_RELU = 0, 1, 2


class ChConfig(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("mode", ctypes.c_int32), ("num_drones", ctypes.c_int32),
                ("num_cattle", ctypes.c_int32), ("min_drones", ctypes.c_int32), ("max_drones", ctypes.c_int32),
                ("curriculum_level", ctypes.c_int32), ("ctrl_freq", ctypes.c_int32), ("pyb_freq", ctypes.c_int32),
                ("compat", ctypes.c_int32), ("precision", ctypes.c_int32), ("torque_world", ctypes.c_int32),
                ("gyro", ctypes.c_int32), ("marl_wrapper", ctypes.c_int32), ("damping", ctypes.c_double), ("seed", ctypes.c_uint64),
                ("env_id_offset", ctypes.c_int64), ("spawn_table", ctypes.POINTER(ctypes.c_double)),
                ("spawn_scenarios", ctypes.c_int32), ("spawn_cows", ctypes.c_int32), ("physics", ctypes.c_int32),
                ("eval_metrics", ctypes.c_int32), ("link_lag", ctypes.c_int32)]


class ChStepIO(ctypes.Structure):
    _fields_ = [("actions", ctypes.c_void_p), ("actions_out", ctypes.c_void_p), ("obs", ctypes.c_void_p),
                ("reward", ctypes.c_void_p), ("terminated", ctypes.c_void_p), ("truncated", ctypes.c_void_p),
                ("terminal_obs", ctypes.c_void_p), ("agent_active", ctypes.c_void_p),
                ("reset_happened", ctypes.c_void_p), ("flags", ctypes.c_uint32), ("_pad", ctypes.c_uint32),
                ("episode_stats", ctypes.c_void_p)]


class ChHostOut(ctypes.Structure):
    _fields_ = [("obs", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("terminated", ctypes.c_void_p),
                ("truncated", ctypes.c_void_p), ("reset_happened", ctypes.c_void_p), ("agent_active", ctypes.c_void_p),
                ("ended_count", ctypes.c_int64), ("ended_env", ctypes.c_void_p), ("ended_obs", ctypes.c_void_p),
                ("ended_stats", ctypes.c_void_p)]


class ChMlp(ctypes.Structure):
    _fields_ = [("n_layers", ctypes.c_int32), ("dims", ctypes.c_int32 * 5), ("weight", ctypes.c_void_p * 4),
                ("bias", ctypes.c_void_p * 4), ("hidden_act", ctypes.c_int32), ("clip", ctypes.c_int32),
                ("lo", ctypes.c_float), ("hi", ctypes.c_float), ("packed", ctypes.c_void_p),
                ("split_out", ctypes.c_int32 * 4), ("split_in", ctypes.c_int32 * 4)]


# the native PPO updates' structs (ch_ppo_* for SB3's CTDE policy, ch_marl_ppo_* for RLlib's shared DTDE policy)
class ChPpoNet(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("act_dim", ctypes.c_int32), ("n_pi", ctypes.c_int32),
                ("n_vf", ctypes.c_int32), ("pi", ctypes.c_int32 * 2), ("vf", ctypes.c_int32 * 2),
                ("pi_weight", ctypes.c_void_p * 3), ("pi_bias", ctypes.c_void_p * 3),
                ("vf_weight", ctypes.c_void_p * 3), ("vf_bias", ctypes.c_void_p * 3), ("log_std", ctypes.c_void_p)]


class ChPpoHparams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("learning_rate", "beta1", "beta2", "eps", "clip_range", "ent_coef",
                                               "vf_coef", "max_grad_norm")] + \
        [("normalize_advantage", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class ChPpoData(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("obs", "actions", "old_log_prob", "advantages", "returns")] + \
        [("rows", ctypes.c_int64)]


class ChPpoOpts(ctypes.Structure):
    _fields_ = [("target_kl", ctypes.c_double), ("clip_range_vf", ctypes.c_double), ("old_values", ctypes.c_void_p),
                ("stop_dev", ctypes.c_void_p)]


class ChPpoMember(ctypes.Structure):
    """One member of ch_ppo_train_pop's population: what ch_ppo_train_opt takes, by value."""
    _fields_ = [("net", ChPpoNet), ("hp", ChPpoHparams), ("data", ChPpoData), ("opts", ChPpoOpts)] + \
        [(k, ctypes.c_void_p) for k in ("idx", "m", "v", "step_dev", "stats", "scratch")]


class ChMarlPpoNet(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("act_dim", ctypes.c_int32), ("n_actor", ctypes.c_int32),
                ("n_critic", ctypes.c_int32), ("actor", ctypes.c_int32 * 2), ("critic", ctypes.c_int32 * 2),
                ("actor_weight", ctypes.c_void_p * 3), ("actor_bias", ctypes.c_void_p * 3),
                ("critic_weight", ctypes.c_void_p * 3), ("critic_bias", ctypes.c_void_p * 3)]


class ChMarlPpoHparams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("learning_rate", "beta1", "beta2", "eps", "clip_param", "vf_clip_param",
                                               "vf_loss_coeff", "entropy_coeff", "log_std_clip", "grad_clip")] + \
        [("kl_coeff_dev", ctypes.c_void_p)]


class ChMarlPpoData(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("obs", "actions", "old_log_prob", "old_dist_inputs", "advantages",
                                               "value_targets")] + [("rows", ctypes.c_int64)]


# the on-device evaluate_policy's structs (ch_eval_*; cattleherd/eval_policy.py)
class ChEvalTable(ctypes.Structure):
    _fields_ = [("capacity", ctypes.c_int32), ("_pad", ctypes.c_int32)] + \
        [(k, ctypes.c_void_p) for k in ("quota", "count", "ep_return", "ep_length", "ep_flags", "ep_end_step",
                                        "remaining")]


class ChEvalIO(ctypes.Structure):
    _fields_ = [("step", ctypes.POINTER(ChStepIO)), ("mean", ctypes.c_void_p), ("env_actions", ctypes.c_void_p)]


# the DTDE driver's on-device evaluation (ch_marl_eval_*; cattleherd/marl_eval.py)
class ChMarlEvalTable(ctypes.Structure):
    _fields_ = [("capacity", ctypes.c_int32), ("_pad", ctypes.c_int32)] + \
        [(k, ctypes.c_void_p) for k in ("quota", "count", "ep_return", "agent_return", "ep_length", "agent_length",
                                        "ep_end_step", "remaining", "acc_return", "acc_length", "acc_steps", "live")]


class ChMarlEvalIO(ctypes.Structure):
    _fields_ = [("step", ctypes.POINTER(ChStepIO)), ("policy_out", ctypes.c_void_p), ("env_actions", ctypes.c_void_p)]


# the device-side evaluator log (ch_eval_log_*; cattleherd/eval_log.py)
class ChEvalLog(ctypes.Structure):
    _fields_ = [("n_sel", ctypes.c_int32), ("capacity", ctypes.c_int32)] + \
        [(k, ctypes.c_void_p) for k in ("sel_env", "rows", "dropped", "time", "effectiveness", "num_drones", "episode",
                                        "flags", "drone_xy", "drone_vxy", "drone_dist", "cattle_xy", "cattle_vxy",
                                        "start_cattle_vxy", "start_counter")]


class ChEvalLogIO(ctypes.Structure):
    _fields_ = [("step", ctypes.POINTER(ChStepIO)), ("mean", ctypes.c_void_p), ("env_actions", ctypes.c_void_p),
                ("done_mask", ctypes.c_void_p)]


# the SB3 training log's episode ring (ch_ep_ring_*; cattleherd/train_log.py)
class ChEpRing(ctypes.Structure):
    _fields_ = [("window", ctypes.c_int32), ("_pad", ctypes.c_int32)] + \
        [(k, ctypes.c_void_p) for k in ("ep_return", "ep_length", "ep_env", "total")]


# a population's episode rings (ch_ep_ring_pop_*; cattleherd/train_log.py)
class ChEpRingPop(ctypes.Structure):
    _fields_ = [("window", ctypes.c_int32), ("n_members", ctypes.c_int32)] + \
        [(k, ctypes.c_void_p) for k in ("ep_return", "ep_length", "ep_env", "total")]


# the RLlib training log's episode ring (ch_marl_ep_ring_*; cattleherd/train_log.py)
MARL_RING_ARRAYS = ("ep_return", "agent_return", "ep_length", "agent_length", "ep_env", "total", "acc_return",
                    "acc_length", "acc_steps", "env_steps", "agent_steps")


class ChMarlEpRing(ctypes.Structure):
    _fields_ = [("window", ctypes.c_int32), ("_pad", ctypes.c_int32)] + [(k, ctypes.c_void_p) for k in MARL_RING_ARRAYS]


# the device-side VecNormalize (ch_norm_*; cattleherd/vec_normalize.py)
class ChNorm(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("dim", "training", "norm_obs", "norm_reward")] + \
        [(k, ctypes.c_double) for k in ("clip_obs", "clip_reward", "epsilon", "gamma")] + [("n_envs", ctypes.c_int64)] + \
        [(k, ctypes.c_void_p) for k in ("mean", "var", "count", "ret_stats", "ret", "scratch")] + \
        [("scratch_doubles", ctypes.c_int64)] + [(k, ctypes.c_void_p) for k in ("obs_n", "terminal_obs_n", "reward_n")]


class ChError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libcattleherd error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libcattleherd.so; raises if it is missing (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    P = ctypes.POINTER
    L.ch_default_config.argtypes = [P(ChConfig), i32, i32, i32]
    L.ch_create.argtypes = [P(ChConfig), i64, i32, P(vp)]
    L.ch_destroy.argtypes = [vp]
    L.ch_last_error.argtypes = [vp]
    L.ch_last_error.restype = ctypes.c_char_p
    L.ch_shape.argtypes = [vp, P(i64), P(i32), P(i32), P(i32)]
    L.ch_reset.argtypes = [vp, vp, vp, vp]
    L.ch_reset_with.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ch_step.argtypes = [vp, P(ChStepIO), vp]
    if hasattr(L, "ch_step_n"):   # (an older library, e.g. an A/B baseline loaded through CH_LIB_PATH, lacks it)
        L.ch_step_n.argtypes = [vp, P(ChStepIO), i32, vp]
        L.ch__multi_steps.argtypes = [vp]
        L.ch__multi_steps.restype = i64
    L.ch_state_size.argtypes = [vp, P(i64), P(i64)]
    L.ch_get_state.argtypes = [vp, vp, vp, vp]
    L.ch_set_state.argtypes = [vp, vp, vp, vp]
    L.ch_metrics.argtypes = [vp, vp, i32, vp]
    L.ch_metrics_device.argtypes = [vp, vp, i32, vp]
    L.ch_sync.argtypes = [vp, vp]
    L.ch_get_eval.argtypes = [vp, vp, vp]
    L.ch_builtin_spawn_table.argtypes = [vp, P(i32), P(i32)]
    L.ch_spawn_table.argtypes = [i32, vp, P(i32), P(i32)]
    L.ch_mlp_forward.argtypes = [P(ChMlp), vp, i64, vp, vp]
    L.ch_mlp_forward_masked.argtypes = [P(ChMlp), vp, i64, vp, vp, vp]
    L.ch_policy_forward.argtypes = [vp, P(ChMlp), vp, vp, vp]
    L.ch_mlp_packed_size.argtypes = [P(ChMlp)]
    L.ch_mlp_pack.argtypes = [P(ChMlp), vp, vp]
    L.ch_outputs_to_host.argtypes = [vp, P(ChStepIO), P(ChHostOut), vp]
    if hasattr(L, "ch__mlp_last_launch"):   # internal (tests / diagnostics): see mlp_last_launch below
        L.ch__mlp_last_launch.argtypes = [P(i32 * 4)]
        L.ch__mlp_launch_counts.argtypes = [P(i64 * len(MLP_KERNELS))]
        L.ch__mlp_last_launch.restype = L.ch__mlp_launch_counts.restype = ctypes.c_int
    if hasattr(L, "ch__mlp_plan"):   # internal: the host-only planner and its kernel table, see mlp_plan below
        L.ch__mlp_kernel.argtypes = [i32, P(i32 * 8)]
        L.ch__mlp_kernel.restype = ctypes.c_char_p
        L.ch__mlp_plan.argtypes = [P(P(ChMlp)), P(i64), P(i32), i32, i32, i32, i32, i32, i32, P(i32 * 12)]
        L.ch__mlp_plan.restype = ctypes.c_int
    if hasattr(L, "ch__ppo_plan"):   # internal: the PPO update's host-only step plan and kernel table, see ppo_plan below
        L.ch__ppo_plan.argtypes = [i32, i32, i32, i32, i32, P(i32 * 6)]
        L.ch__ppo_kernel.argtypes = [i32]
        L.ch__ppo_kernel.restype = ctypes.c_char_p
        L.ch__ppo_last_step.argtypes = [P(i32 * 5)]
        L.ch__ppo_plan.restype = L.ch__ppo_last_step.restype = ctypes.c_int
    if hasattr(L, "ch__step_plan"):   # internal: the env step's host-only planner and kernel table, see step_plan below
        L.ch__step_plan.argtypes = [i32, i32, i32, i32, i32, i64, i32, i64, i32, i32, i32, P(i64 * 13)]
        L.ch__step_plan_of.argtypes = [vp, P(i64 * 13)]
        L.ch__step_kernel.argtypes = [i32, P(i32 * 11)]
        L.ch__step_rule.argtypes = [i32]
        L.ch__step_kernel.restype = L.ch__step_rule.restype = ctypes.c_char_p
        L.ch__step_plan.restype = L.ch__step_plan_of.restype = ctypes.c_int
    for pre, (N, H, D) in (("ch_ppo_", (P(ChPpoNet), P(ChPpoHparams), P(ChPpoData))),
                           ("ch_marl_ppo_", (P(ChMarlPpoNet), P(ChMarlPpoHparams), P(ChMarlPpoData)))):
        getattr(L, pre + "param_count").argtypes = [N]
        getattr(L, pre + "scratch_size").argtypes = [N, i64]
        getattr(L, pre + "grad").argtypes = [N, H, D, vp, i64, vp, vp, vp, vp]
        getattr(L, pre + "adam").argtypes = [N, H, vp, vp, vp, vp, vp, vp]
        getattr(L, pre + "train").argtypes = [N, H, D, vp, i64, i64, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "ch_evaluate_policy"):
        L.ch_eval_begin.argtypes = [vp, P(ChEvalTable), i32, vp]
        L.ch_eval_record.argtypes = [vp, P(ChEvalTable), P(ChStepIO), i64, vp]
        L.ch_evaluate_policy.argtypes = [vp, P(ChMlp), P(ChEvalTable), P(ChEvalIO), i64, i32, i64, P(i64), P(i64), vp]
    if hasattr(L, "ch_marl_evaluate_policy"):
        L.ch_marl_eval_begin.argtypes = [vp, P(ChMarlEvalTable), i32, vp]
        L.ch_marl_eval_mark.argtypes = [vp, P(ChMarlEvalTable), vp]
        L.ch_marl_eval_record.argtypes = [vp, P(ChMarlEvalTable), P(ChStepIO), i64, vp]
        L.ch_marl_evaluate_policy.argtypes = [vp, P(ChMlp), P(ChMarlEvalTable), P(ChMarlEvalIO), i64, i32, i64, P(i64),
                                              P(i64), vp]
    if hasattr(L, "ch_eval_log_run"):
        L.ch_eval_log_begin.argtypes = [vp, P(ChEvalLog), vp]
        L.ch_eval_log_mark.argtypes = [vp, P(ChEvalLog), vp]
        L.ch_eval_log_record.argtypes = [vp, P(ChEvalLog), P(ChStepIO), vp]
        L.ch_eval_log_run.argtypes = [vp, P(ChMlp), P(ChEvalLog), P(ChEvalLogIO), i64, vp]
    if hasattr(L, "ch_ep_ring_record"):
        L.ch_ep_ring_begin.argtypes = [vp, P(ChEpRing), vp]
        L.ch_ep_ring_record.argtypes = [vp, P(ChEpRing), P(ChStepIO), vp]
        L.ch_ppo_train_log.argtypes = L.ch_ppo_train.argtypes
        L.ch_explained_variance_scratch.argtypes = [i64]
        L.ch_explained_variance.argtypes = [vp, vp, i64, vp, vp, vp]
    if hasattr(L, "ch_ep_ring_pop_record"):
        L.ch_ep_ring_pop_begin.argtypes = [vp, P(ChEpRingPop), vp]
        L.ch_ep_ring_pop_record.argtypes = [vp, P(ChEpRingPop), P(ChStepIO), vp]
        L.ch_ep_ring_pop_summary.argtypes = [P(ChEpRingPop), vp, vp]
        L.ch_explained_variance_pop_scratch.argtypes = [i64, i32]
        L.ch_explained_variance_pop.argtypes = [vp, vp, i32, i64, vp, vp, vp]
    if hasattr(L, "ch_marl_ep_ring_record"):
        L.ch_marl_ep_ring_begin.argtypes = [vp, P(ChMarlEpRing), vp]
        L.ch_marl_ep_ring_record.argtypes = [vp, P(ChMarlEpRing), vp, P(ChStepIO), vp]
        L.ch_marl_ppo_train_log.argtypes = L.ch_marl_ppo_train.argtypes
    if hasattr(L, "ch_ppo_train_opt"):
        L.ch_ppo_train_opt.argtypes = [P(ChPpoNet), P(ChPpoHparams), P(ChPpoData), P(ChPpoOpts), vp, i64, i64, vp, vp, vp,
                                       vp, vp, vp]
    if hasattr(L, "ch_ppo_train_pop"):
        L.ch_ppo_pop_create.argtypes = [i32, i32, P(vp)]
        L.ch_ppo_pop_destroy.argtypes = [vp]
        L.ch_ppo_train_pop.argtypes = [vp, P(ChPpoMember), i32, i64, i64, vp]
        L.ch__ppo_pop_plan.argtypes = [i32, P(i32 * 3)]
        L.ch__ppo_pop_plan.restype = ctypes.c_int
        L.ch__ppo_pop_kernel.argtypes = [i32]
        L.ch__ppo_pop_kernel.restype = ctypes.c_char_p
    if hasattr(L, "ch_norm_begin"):
        N = P(ChNorm)
        L.ch_norm_scratch_size.argtypes = [i64, i32]
        L.ch_norm_begin.argtypes = [N, vp]
        L.ch_norm_obs_update.argtypes = [N, vp, i64, vp]
        L.ch_norm_obs_apply.argtypes = [N, vp, i64, vp, vp, vp]
        L.ch_norm_reward.argtypes = [N, vp, vp, vp, i64, vp, vp]
    optional = ("ch_step_n",) + _EVAL_EXPORTS + _TRAIN_LOG_EXPORTS + _MARL_TRAIN_LOG_EXPORTS + _PPO_OPT_EXPORTS + \
        _NORM_EXPORTS + _PPO_POP_EXPORTS + _ROLLOUT_POP_EXPORTS + _TRAIN_LOG_POP_EXPORTS
    for name in EXPORTS:
        if name not in ("ch_last_error",) and (name not in optional or hasattr(L, name)):
            getattr(L, name).restype = ctypes.c_int
    L.ch_mlp_packed_size.restype = ctypes.c_int64
    L.ch_ppo_param_count.restype = L.ch_ppo_scratch_size.restype = ctypes.c_int64
    L.ch_marl_ppo_param_count.restype = L.ch_marl_ppo_scratch_size.restype = ctypes.c_int64
    if hasattr(L, "ch_explained_variance_scratch"):
        L.ch_explained_variance_scratch.restype = ctypes.c_int64
    if hasattr(L, "ch_norm_scratch_size"):
        L.ch_norm_scratch_size.restype = ctypes.c_int64
    if hasattr(L, "ch_explained_variance_pop_scratch"):
        L.ch_explained_variance_pop_scratch.restype = ctypes.c_int64
    _lib = L
    return L


def check(rc, handle=None):
    if rc != CH_OK:
        msg = lib().ch_last_error(handle)
        raise ChError(rc, msg.decode() if msg else "")
    return rc


# Internal (tests / diagnostics): ch__mlp_last_launch's kernel numbers, as k_mlp2<NW, TW, SHARE, RT> / k_mlp<NW, TWMAX, DEPTH>
MLP_KERNELS = ("none", "k_mlp2<8,1>", "k_mlp2<8,2>", "k_mlp2<4,2>", "k_mlp2<8,1,true>", "k_mlp2<8,1,false,2>",
               "k_mlp2<4,4,false,2>", "k_mlp2<4,4,false,4>", "k_mlp<8,1,2>", "k_mlp<8,2,2>", "k_mlp<4,4,1>")


def mlp_last_launch():
    """Internal (tests / diagnostics): (kernel name, row tiles per workgroup, grid, dynamic LDS bytes) of the policy
    forward launched last in this process (ch__mlp_last_launch; kept on the host, no device work)."""
    out = (ctypes.c_int32 * 4)()
    check(lib().ch__mlp_last_launch(ctypes.byref(out)))
    return MLP_KERNELS[out[0]], int(out[1]), int(out[2]), int(out[3])


def mlp_launch_counts():
    """Internal (tests / diagnostics): {kernel name: launches since the library was loaded} (ch__mlp_launch_counts)."""
    out = (ctypes.c_int64 * len(MLP_KERNELS))()
    check(lib().ch__mlp_launch_counts(ctypes.byref(out)))
    return {k: int(v) for k, v in zip(MLP_KERNELS, out)}


MLP_KERNEL_COLUMNS = ("family", "nw", "tw", "share", "rt", "packed_only", "max_pair0", "raw_ragged")


def mlp_kernel_table():
    """Internal (tests / diagnostics): the library's forward-kernel table (csrc/ch_mlp_plan.h kMlpTable), one dict per
    row in ch__mlp_last_launch's numbering: its name and MLP_KERNEL_COLUMNS (family: 2 k_mlp2, 1 k_mlp, 0 none)."""
    rows = []
    while True:
        out = (ctypes.c_int32 * 8)()
        name = lib().ch__mlp_kernel(len(rows), ctypes.byref(out))
        if name is None:
            return rows
        rows.append(dict(zip(MLP_KERNEL_COLUMNS, (int(v) for v in out)), name=name.decode()))


def mlp_plan(nets, rows, cus, kcap=None, v1=False, nw4=False, wide4=False, rt=0):
    """Internal (tests / diagnostics): what a forward of up to three ``nets`` (ChMlp; only dims, n_layers, packed and
    non-NULL weights matter) over ``rows`` rows each would launch on a device of ``cus`` compute units under the given
    switches (CH_MLP_V1, CH_MLP2_NW4, CH_MLP_WIDE4, CH_MLP_RT) -- planned on the host, no device needed.  ``kcap``:
    live input widths (0: dims[0]).  Returns a dict: v2, rt, lda, ldh, lds, and kernel names and grids per live segment."""
    n = len(nets)
    ptrs = (ctypes.POINTER(ChMlp) * n)(*[ctypes.pointer(m) for m in nets])
    out = (ctypes.c_int32 * 12)()
    check(lib().ch__mlp_plan(ptrs, (ctypes.c_int64 * n)(*rows), (ctypes.c_int32 * n)(*(kcap or [0] * n)), n, cus,
                             int(v1), int(nw4), int(wide4), rt, ctypes.byref(out)))
    v = [int(x) for x in out]
    live = v[5]
    return {"v2": bool(v[0]), "rt": v[1], "lda": v[2], "ldh": v[3], "lds": v[4],
            "kernel": [MLP_KERNELS[k] for k in v[6:6 + live]], "grid": v[9:9 + live]}


def ppo_kernel_table():
    """Internal (tests / diagnostics): the names of the native PPO update's kernel table (csrc/ch_ppo.hip kPpoTable),
    one per instantiation, row 0 "none"."""
    rows = []
    while True:
        name = lib().ch__ppo_kernel(len(rows))
        if name is None:
            return rows
        rows.append(name.decode())


def ppo_plan(flavour, log=False, gate=False, vclip=False, opts=None):
    """Internal (tests / diagnostics): what one minibatch step launches (csrc/ch_ppo.h ppo_plan; host only) for the
    base ``flavour`` (0 SB3, 1 RLlib), ``*_train_log``'s statistics, and ``ch_ppo_train_opt`` with its KL gate armed
    and / or its value clip on (``opts``: the call is ``ch_ppo_train_opt``; default: ``gate or vclip``).  Returns a
    dict: the fb, dw and adam kernels' names, the update bits, the statistics row's width and whether the kernels take
    the option structs.  Raises ``ChError`` for a combination that does not exist."""
    out = (ctypes.c_int32 * 6)()
    check(lib().ch__ppo_plan(flavour, int(log), int(gate or vclip if opts is None else opts), int(gate), int(vclip),
                             ctypes.byref(out)))
    names = ppo_kernel_table()
    return {"fb": names[out[0]], "dw": names[out[1]], "adam": names[out[2]], "update": int(out[3]),
            "n_stats": int(out[4]), "opts": bool(out[5])}


def ppo_pop_kernel_table():
    """Internal (tests / diagnostics): the names of the population update's kernel table (csrc/ch_ppo.hip
    kPpoPopTable), one per instantiation."""
    rows = []
    while True:
        name = lib().ch__ppo_pop_kernel(len(rows))
        if name is None:
            return rows
        rows.append(name.decode())


def ppo_pop_plan(vclip=False):
    """Internal (tests / diagnostics): the kernels of one population step (csrc/ch_ppo.h ppo_pop_plan; host only) with
    the value clip on or off, as a dict of the fb, dw and adam kernels' names."""
    out = (ctypes.c_int32 * 3)()
    check(lib().ch__ppo_pop_plan(int(vclip), ctypes.byref(out)))
    names = ppo_pop_kernel_table()
    return {"fb": names[out[0]], "dw": names[out[1]], "adam": names[out[2]]}


def ppo_last_step():
    """Internal (tests / diagnostics): the kernels of the PPO minibatch step launched last in this process, as
    (fb, dw, adam names, the Adam launch's update bits, its grid) -- ch__ppo_last_step; kept on the host."""
    out = (ctypes.c_int32 * 5)()
    check(lib().ch__ppo_last_step(ctypes.byref(out)))
    names = ppo_kernel_table()
    return names[out[0]], names[out[1]], names[out[2]], int(out[3]), int(out[4])


# Internal (tests / diagnostics): the step kernels' table (csrc/ch_step_plan.h kStepTable), one name per instantiation
# of k_step2<R, MODE, GT, NT, MT, PHYS, PW, TOBS>, k_step2_multi<R, MODE, GT, NT, MT, PHYS, PW, WPE> and
# k_step2_actor<R, MODE, GT, NT, MT, TOBS> (trailing default arguments left out); a plan's rows index it
_STEP2 = ("1,0,0,0,true", "0,16,4,16,true", "0,0,0,0,true", "1,16,4,32,false,true", "1,0,0,0,false,true",
          "0,0,0,0,false,true", "1,0,0,0", "0,8,4,16", "0,16,4,16,false,false,true", "0,16,4,16", "0,16,2,8", "0,4,2,8",
          "0,0,0,0")
STEP_KERNELS = tuple(f"k_step2<{r},{a}>" for r in ("double", "float") for a in _STEP2) + (
    "k_step2_multi<double,1,16,4,32,false,true>", "k_step2_multi<double,0,16,4,16>", "k_step2_multi<double,0,8,4,16>",
    "k_step2_multi<double,0,16,2,8>", "k_step2_multi<double,0,4,2,8>", "k_step2_multi<float,0,16,4,16,false,false,4>",
    "k_step2_multi<float,0,16,4,16>", "k_step2_actor<double,0,16,4,16,false>", "k_step2_actor<double,0,16,4,16,true>")
STEP_KERNEL_COLUMNS = ("family", "precision", "mode", "gt", "nt", "mt", "phys", "pw", "tobs_wpe", "max_block", "pipelined")
# the planner's geometry rules in the order it applies them (ch__step_rule); bit r of a plan's "rules": rule r fired
STEP_RULES = ("generic", "4x16", "2x8", "per_wave", "sep", "v1_fallback")
STEP_PLAN_COLUMNS = ("kernel", "G", "block", "lds", "pw", "sep", "step_row", "step_row_tobs", "multi_row", "multi_block",
                     "multi_lds", "fused_actor", "rules")


def step_kernel_table():
    """Internal (tests / diagnostics): the library's step-kernel table, one dict per row: its name and
    STEP_KERNEL_COLUMNS (family: 0 k_step2, 1 k_step2_multi, 2 k_step2_actor; tobs_wpe: TOBS, for k_step2_multi WPE)."""
    rows = []
    while True:
        out = (ctypes.c_int32 * 11)()
        name = lib().ch__step_kernel(len(rows), ctypes.byref(out))
        if name is None:
            return rows
        rows.append(dict(zip(STEP_KERNEL_COLUMNS, (int(v) for v in out)), name=name.decode()))


def step_rules():
    """Internal (tests / diagnostics): the names of the planner's geometry rules, in order (ch__step_rule)."""
    names = []
    while (name := lib().ch__step_rule(len(names))) is not None:
        names.append(name.decode())
    return tuple(names)


def _step_plan_dict(out):
    d = dict(zip(STEP_PLAN_COLUMNS, (int(v) for v in out)))
    d["rules"] = tuple(n for r, n in enumerate(STEP_RULES) if d["rules"] >> r & 1)
    return d


def step_plan(mode, num_drones, num_cattle, precision, physics, n_envs, cus, lds_budget, kernel=0, geometry=(0, 0)):
    """Internal (tests / diagnostics): what ch_create plans for a handle of this shape on a device of ``cus`` compute
    units with ``lds_budget`` bytes of LDS per workgroup (csrc/ch_step_plan.cpp step_plan; host only, no device needed);
    ``kernel`` / ``geometry``: as after ch__set_kernel / ch__set_geometry.  Returns a dict of STEP_PLAN_COLUMNS (rows
    index STEP_KERNELS, -1: none; rules: the names of the geometry rules that fired).  Raises ``ChError`` with the code
    the setter would return when the planner refuses the overrides."""
    out = (ctypes.c_int64 * 13)()
    rc = lib().ch__step_plan(mode, num_drones, num_cattle, precision, physics, n_envs, cus, lds_budget, kernel,
                             geometry[0], geometry[1], ctypes.byref(out))
    if rc != CH_OK:
        raise ChError(rc, "ch__step_plan")
    return _step_plan_dict(out)


def step_plan_of(handle):
    """Internal (tests): the plan a handle holds (ch__step_plan_of), as step_plan returns it."""
    out = (ctypes.c_int64 * 13)()
    check(lib().ch__step_plan_of(handle, ctypes.byref(out)), handle)
    return _step_plan_dict(out)


def default_config(mode, num_drones, num_cattle):
    c = ChConfig()
    check(lib().ch_default_config(ctypes.byref(c), mode, num_drones, num_cattle))
    return c


def code_object_hash(path=None):
    """sha256 (hex, first 16 digits) of the device code in libcattleherd.so: the ``.hip_fatbin`` ELF section
    that holds the gfx950 code objects.  Host-side code and build paths do not enter it, so a rebuild of the same
    kernel sources with the same compiler and flags gives the same hash.  bench.py accepts a committed counter
    record (profiles/counters/) only for the code object it was measured on."""
    import hashlib
    import struct
    with open(path or LIB_PATH, "rb") as fh:
        data = fh.read()
    if data[:4] != b"\x7fELF" or data[4] != 2:
        raise ValueError("not an ELF64 file")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    sec = [struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize) for i in range(shnum)]
    stro = sec[shstrndx][4]
    for name, _typ, _flags, _addr, off, size in sec:
        end = data.index(b"\0", stro + name)
        if data[stro + name:end] == b".hip_fatbin":
            return hashlib.sha256(data[off:off + size]).hexdigest()[:16]
    raise ValueError("no .hip_fatbin section")


def spawn_table(cows):
    """The spawn table ch_create uses by default (numpy float64 [100, max(cows,16), 2])."""
    import numpy as np
    s, c = ctypes.c_int32(), ctypes.c_int32()
    check(lib().ch_spawn_table(cows, None, ctypes.byref(s), ctypes.byref(c)))
    out = np.zeros((s.value, c.value, 2), np.float64)
    check(lib().ch_spawn_table(cows, out.ctypes.data, None, None))
    return out
