"""ctypes binding of libusim.so -- exactly the symbols declared in include/usim.h.

The product path has no CPU fallback: if the shared library is missing or cannot be loaded the import of the
simulator raises, and every entry point that needs a GPU returns a negative usim_status that is raised as
RuntimeError(usim_strerror)."""
import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "lib" / "libusim.so"

OBS_DIM = 19
MAXC = 8
NSCALAR = 40
POLICY_PACKED = 2 * 128 * 256      # USIM_POLICY_PACKED
POLICY_SCRATCH = 1280              # USIM_POLICY_SCRATCH
POLICY_MAX_MEMBERS = 65535         # USIM_POLICY_MAX_MEMBERS: members of a policy population (a grid axis)
POLICY_FUSED_ROW = 48             # doubles per row of usim_policy_fused.work_dev (one row of partial sums per 32 environments)
PPO_STATS = 8                      # USIM_PPO_STATS
PPO_WORKGROUPS = 128               # USIM_PPO_WORKGROUPS: gradient workgroups per network (tiles of 32 minibatch rows at this stride)
PPO_GATE_WORDS = 4                 # USIM_PPO_GATE_WORDS: stop flag, gradient calls evaluated, optimizer steps applied, 0
PPO_HYPER_WORDS = 8                # USIM_PPO_HYPER_WORDS: a member's row of usim_ppo_batch_multi.hyper_dev (lr, clip_range, ent_coef, vf_coef, max_grad_norm, clip_range_vf, target_kl, 0)
BC_NLL, BC_MSE = 0, 1             # USIM_BC_NLL, USIM_BC_MSE: the policy term of usim_bc_grad
RESET_PARAMS = 13
LOG_WIDTH = 53
WARM_WORDS = 8 + 16 * 4            # USIM_WARM_WORDS
FULL_BODY_WORDS = 13 + 4 * 270 + 8 + 64      # USIM_FULL_BODY_WORDS: the free body (13), then the warm start of the full torso's contact solve
PACK_HEAD_WORDS = 21               # USIM_PACK_HEAD_WORDS: obs[19], rew, done
PACK_EPISODE_WORDS = 23            # USIM_PACK_EPISODE_WORDS: env index, ep_length, ep_return, status, terminal_observation[19]
MONITOR_HEADER_WORDS = 16          # USIM_MONITOR_HEADER_WORDS: episodes, length_sum, return_sum, truncated, launches (64 bits each), six zero words
MONITOR_ROW_WORDS = 4              # USIM_MONITOR_ROW_WORDS: ep_return bits, ep_length, environment index, launch number
MONITOR_MAX_WINDOW = 1 << 20       # USIM_MONITOR_MAX_WINDOW
PLAN_REFIT_MAX_K = 4096            # USIM_PLAN_REFIT_MAX_K: candidates per group usim_plan_refit ranks
METRICS = 13                       # USIM_METRICS: the metrics of error_metrics.METRICS, in that order
METRICS_HEADER_WORDS = 64          # USIM_METRICS_HEADER_WORDS: episodes, launches, length_sum, nonfinite (64 bits each), total[13], total_sq[13] (float64), four zero words
METRICS_ROW_WORDS = 32             # USIM_METRICS_ROW_WORDS: 13 float64 metrics, environment index, episode length, launch number, three zero words


def monitor_words(window):
    """usim_monitor_words(window): 32-bit words of the block usim_monitor_step keeps for a ring of `window` episodes"""
    w = int(window)
    if not 1 <= w <= MONITOR_MAX_WINDOW:
        raise ValueError(f"window must be 1 .. {MONITOR_MAX_WINDOW}, got {window!r}")
    return MONITOR_HEADER_WORDS + MONITOR_ROW_WORDS * w


def metrics_words(n, window):
    """usim_metrics_words(n, window): 32-bit words of the block usim_metrics_step keeps for n environments and a ring of `window` episodes"""
    n_, w = int(n), int(window)
    if n_ < 1:
        raise ValueError(f"n must be at least 1, got {n!r}")
    if not 1 <= w <= MONITOR_MAX_WINDOW:
        raise ValueError(f"window must be 1 .. {MONITOR_MAX_WINDOW}, got {window!r}")
    words = METRICS_HEADER_WORDS + METRICS_ROW_WORDS * w + 2 * METRICS * n_
    if words > 2 ** 31 - 1:
        raise ValueError(f"a metrics block for {n_} environments and a window of {w} is beyond 2^31 - 1 words")
    return words


def record_words(m, episodes, horizon):
    """usim_record_words(m, episodes, horizon): 32-bit words of the block usim_record_step keeps for `episodes` episodes of m environments"""
    m_, e, h = int(m), int(episodes), int(horizon)
    if m_ < 1 or e < 1 or h < 1:
        raise ValueError(f"m, episodes and horizon must be at least 1, got {m!r}, {episodes!r}, {horizon!r}")
    words = (m_ + m_ * e + 3) // 4 * 4 + m_ * e * h * LOG_WIDTH
    if words > 2 ** 31 - 1:
        raise ValueError(f"a record block of {m_} x {e} episodes of {h} rows is beyond 2^31 - 1 words")
    return words


def pack_words(n):
    """USIM_PACK_WORDS(n): 32-bit words of the block usim_pack_step fills for n environments"""
    return 4 + int(n) * (PACK_HEAD_WORDS + PACK_EPISODE_WORDS)


def policy_fused_rows(n):
    """USIM_POLICY_FUSED_ROWS(n)"""
    return (int(n) + 31) // 32


def policy_fused_work(n):
    """USIM_POLICY_FUSED_WORK(n): doubles of usim_policy_fused.work_dev -- the rows, then two 32-bit arrival flags per row and a status word"""
    return policy_fused_rows(n) * (POLICY_FUSED_ROW + 1) + 2


MODE = {"tracking": 0, "fixed": 1, "variable_z": 2, "wrench": 3}
TORSO = {"none": 0, "rigid": 0, "top": 1, "soft": 1, "full": 2}
ROBOT = {"Panda": 0, "UR5e": 1}             # ultrasound.py:137

# usim_save_envs / usim_load_envs: 32-bit words of a snapshot row (USIM_SNAPSHOT_WORDS_*)
SNAPSHOT_WORDS_RIGID = 40          # the scalar state words
SNAPSHOT_WORDS_TOP = 240           # + the 200 lattice words of the top-face torso
SNAPSHOT_WORDS_TOP_WARM = 312      # + WARM_WORDS, the solver's kept contact list (warm_start = 1)
SNAPSHOT_WORDS_FULL = 1752         # scalar words + the 1712 lattice / body / solver words of the full torso


def snapshot_words(torso, warm=False):
    """usim_snapshot_words of a handle with this torso (a key of TORSO, or its number) and warm_start setting; the warm start adds words to the top-face row only"""
    t = TORSO[torso] if isinstance(torso, str) else int(torso)
    if t not in (0, 1, 2):
        raise ValueError(f"torso must be one of {sorted(TORSO)} or 0 .. 2, got {torso!r}")
    if t == 1:
        return SNAPSHOT_WORDS_TOP_WARM if warm else SNAPSHOT_WORDS_TOP
    return SNAPSHOT_WORDS_FULL if t == 2 else SNAPSHOT_WORDS_RIGID


class UsimConfig(C.Structure):
    """struct usim_config (include/usim.h)"""
    _fields_ = [(n, C.c_int32) for n in (
        "struct_size", "mode", "torso", "horizon", "early_termination", "deterministic_trajectory", "torso_solref_randomization",
        "initial_probe_pos_randomization", "friction_randomization", "torso_drop", "pgs_iters", "ik_iters", "env_offset",
        "lanes_per_env", "torso_shape", "waves_per_simd", "robot")] + \
        [("seed", C.c_uint64)] + [(n, C.c_double) for n in (
            "control_dt", "kp_fixed", "damping_ratio", "kp_min", "kp_max", "out_max_pos", "out_max_ori", "stiffness", "damping",
            "elem_friction", "probe_friction", "probe_radius", "probe_halflen", "probe_radius2", "probe_height")] + \
        [("substeps", C.c_int32), ("probe_geoms", C.c_int32), ("probe_friction2", C.c_double), ("probe_halfwidth", C.c_double), ("probe_tip", C.c_double), ("pair_model", C.c_int32), ("warm_start", C.c_int32), ("armature_scale", C.c_double), ("joint_frictionloss", C.c_double)]


class UsimStepIO(C.Structure):
    """struct usim_step_io (include/usim.h); all members are device pointers"""
    _fields_ = [(n, C.c_void_p) for n in (
        "act_dev", "obs_dev", "rew_dev", "done_dev", "term_obs_dev", "contacts_dev", "ep_return_dev", "ep_length_dev",
        "act_out_dev", "status_dev", "log_dev")]


class UsimPolicyNet(C.Structure):
    """struct usim_policy_net (include/usim.h): device pointers to the MlpPolicy parameters"""
    _fields_ = [(n, C.c_void_p) for n in ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "act_w", "act_b", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "val_w", "val_b", "log_std", "w2_packed")]


class UsimNormStats(C.Structure):
    """struct usim_norm_stats (include/usim.h): device pointers to the VecNormalize statistics + its four constants"""
    _fields_ = [(n, C.c_void_p) for n in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "returns", "scratch")] + \
               [(n, C.c_double) for n in ("clip_obs", "clip_reward", "gamma", "epsilon")]


class UsimPolicyOut(C.Structure):
    """struct usim_policy_out (include/usim.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("act_env_dev", "nobs_dev", "act_dev", "value_dev", "logp_dev", "episode_start_dev")]


class UsimPolicyFused(C.Structure):
    """struct usim_policy_fused (include/usim.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("work_dev", "rew_prev_dev", "done_prev_dev", "nrew_prev_dev", "raw_sum_dev")] + \
               [(n, C.c_int32) for n in ("update_obs", "have_prev", "norm_reward", "reserved_")]


class UsimPpoBatch(C.Structure):
    """struct usim_ppo_batch (include/usim.h): device pointers to the flattened rollout-buffer slices + the minibatch's index list and loss constants"""
    _fields_ = [(n, C.c_void_p) for n in ("obs_dev", "act_dev", "old_logp_dev", "adv_dev", "ret_dev", "index_dev")] + \
               [(n, C.c_int32) for n in ("rows", "batch", "act_dim", "normalize_advantage")] + \
               [(n, C.c_float) for n in ("clip_range", "ent_coef", "vf_coef", "reserved_")] + \
               [(n, C.c_void_p) for n in ("old_value_dev", "gate_dev")] + [(n, C.c_float) for n in ("clip_range_vf", "target_kl")]


class UsimPpoBatchMulti(C.Structure):
    """struct usim_ppo_batch_multi (include/usim.h): usim_ppo_batch for K members -- the data over K x rows rows, the index lists [K][index_stride], the
    hyper-parameter table [K][PPO_HYPER_WORDS] and the gates [K][PPO_GATE_WORDS]"""
    _fields_ = [(n, C.c_void_p) for n in ("obs_dev", "act_dev", "old_logp_dev", "adv_dev", "ret_dev", "old_value_dev", "index_dev", "hyper_dev", "gate_dev")] + \
               [(n, C.c_int32) for n in ("index_stride", "rows", "batch", "act_dim", "normalize_advantage", "value_clip")]


class UsimBcBatch(C.Structure):
    """struct usim_bc_batch (include/usim.h): device pointers to normalised observations, expert actions and optional value targets + the minibatch's index list"""
    _fields_ = [(n, C.c_void_p) for n in ("obs_dev", "act_dev", "value_dev", "index_dev")] + \
               [(n, C.c_int32) for n in ("rows", "batch", "act_dim", "loss")] + [("ent_coef", C.c_float), ("vf_coef", C.c_float), ("reserved_", C.c_float * 2)]


# every exported symbol of include/usim.h: name -> (restype, argtypes)
SYMBOLS = {
    "usim_policy_step_fused": (C.c_int, [C.POINTER(UsimPolicyNet), C.POINTER(UsimNormStats), C.POINTER(UsimPolicyFused), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.POINTER(UsimPolicyOut), C.c_void_p]),
    "usim_policy_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_policy_step": (C.c_int, [C.POINTER(UsimPolicyNet), C.POINTER(UsimNormStats), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(UsimPolicyOut), C.c_void_p]),
    "usim_policy_reward": (C.c_int, [C.POINTER(UsimNormStats), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_policy_bootstrap": (C.c_int, [C.POINTER(UsimPolicyNet), C.POINTER(UsimNormStats), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_policy_gae": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "usim_policy_pack_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "usim_policy_step_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(UsimNormStats), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(UsimPolicyOut), C.c_void_p]),
    "usim_policy_reward_multi": (C.c_int, [C.POINTER(UsimNormStats), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "usim_pack_step": (C.c_int, [C.POINTER(UsimStepIO), C.c_int, C.c_void_p, C.c_void_p]),
    "usim_score_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_monitor_words": (C.c_int, [C.c_int]),
    "usim_monitor_step": (C.c_int, [C.POINTER(UsimStepIO), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_explained_variance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "usim_metrics_words": (C.c_int, [C.c_int, C.c_int]),
    "usim_metrics_step": (C.c_int, [C.POINTER(UsimStepIO), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_record_words": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "usim_record_step": (C.c_int, [C.POINTER(UsimStepIO), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "usim_plan_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_plan_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_score_block_tail": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_plan_sample_elem": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64,
                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_plan_refit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_plan_tail": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_float, C.c_void_p, C.c_void_p]),
    "usim_ppo_params": (C.c_int, [C.c_int]),
    "usim_ppo_work_floats": (C.c_int64, [C.c_int]),
    "usim_ppo_grad": (C.c_int, [C.POINTER(UsimPolicyNet), C.POINTER(UsimPpoBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_bc_grad": (C.c_int, [C.POINTER(UsimPolicyNet), C.POINTER(UsimBcBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_ppo_adam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                C.c_void_p, C.c_void_p]),
    "usim_ppo_adam_gated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_ppo_work_floats_multi": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "usim_ppo_grad_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(UsimPpoBatchMulti), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_ppo_adam_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_default_config":(C.c_int, [C.POINTER(UsimConfig)]),
    "usim_create": (C.c_int, [C.POINTER(UsimConfig), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "usim_destroy": (None, [C.c_void_p]),
    "usim_set_mapping": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "usim_set_steps_per_launch": (C.c_int, [C.c_void_p, C.c_int]),
    "usim_get_steps_per_launch": (C.c_int, [C.c_void_p]),
    "usim_refill_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "usim_refill_bank": (C.c_int, [C.c_void_p, C.c_void_p]),
    "usim_num_envs": (C.c_int, [C.c_void_p]),
    "usim_action_dim": (C.c_int, [C.c_void_p]),
    "usim_num_elements": (C.c_int, [C.c_void_p]),
    "usim_has_warm_start": (C.c_int, [C.c_void_p]),
    "usim_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_reset_explicit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_step": (C.c_int, [C.c_void_p, C.POINTER(UsimStepIO), C.c_int, C.c_void_p]),
    "usim_random_actions": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "usim_rollout_random": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(UsimStepIO), C.c_int, C.c_void_p]),
    "usim_rollout_actions": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(UsimStepIO), C.c_int, C.c_void_p]),
    "usim_time_steps": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(UsimStepIO), C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "usim_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "usim_get_body_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "usim_set_body_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "usim_get_warm_start": (C.c_int, [C.c_void_p, C.c_void_p]),
    "usim_set_warm_start": (C.c_int, [C.c_void_p, C.c_void_p]),
    "usim_snapshot_words": (C.c_int, [C.c_void_p]),
    "usim_save_envs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "usim_load_envs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "usim_profile_step": (C.c_int, [C.c_void_p, C.POINTER(UsimStepIO), C.c_int64, C.POINTER(C.c_uint64), C.c_int]),
    "usim_strerror": (C.c_char_p, [C.c_int]),
    "usim_last_hip_error": (C.c_char_p, [C.c_void_p]),
    "usim_version": (C.c_char_p, []),
}

_lib = None


def load():
    """dlopen libusim.so and bind every symbol; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get("USIM_LIB", LIB_PATH))
    if not path.exists():
        raise RuntimeError(f"libusim.so not found at {path}: build it with `python __graft_entry__.py build` "
                           f"(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(str(path))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(lib, rc, handle=None):
    if rc == 0:
        return
    msg = lib.usim_strerror(rc).decode()
    if handle:
        detail = lib.usim_last_hip_error(handle).decode()
        if detail:
            msg += f" [{detail}]"
    raise RuntimeError(f"usim error {rc}: {msg}")
