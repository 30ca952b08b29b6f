"""ctypes binding of libpbg_amd.so (include/pbg.h).

The library is the product: there is no CPU fallback.  If it is missing or fails to
load, every entry point raises -- build it with ``python __graft_entry__.py`` (or
``make -C pybullet-gym_amd``)."""
from __future__ import annotations

import ctypes
import os

from . import robots

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpbg_amd.so")

ROBOT_IDS = {s.env_id: s.robot_id for s in robots.BY_ID}


class PbgError(RuntimeError):
    pass


class Info(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "robot_id", "n_envs", "action_dim", "obs_dim", "n_dof", "n_joints", "n_links", "n_feet", "state_words",
        "aux_words", "substeps", "max_episode_steps", "reset_dofs", "floating", "lanes_per_env", "block", "lds_bytes",
        "vgprs", "scratch_bytes", "lds_rows", "record_version")]


class StepIO(ctypes.Structure):
    _fields_ = [("act", ctypes.c_void_p), ("obs", ctypes.c_void_p), ("rew", ctypes.c_void_p),
                ("done", ctypes.c_void_p), ("rew64", ctypes.c_void_p), ("trunc", ctypes.c_void_p),
                ("term_obs", ctypes.c_void_p), ("ncontact", ctypes.c_void_p), ("autoreset", ctypes.c_int),
                ("rew_terms", ctypes.c_void_p), ("csig", ctypes.c_void_p)]


class DebugOpts(ctypes.Structure):
    """pbg_debug_opts_t: test / diagnostic launch options (-1 = default)."""
    _fields_ = [("kernel", ctypes.c_int), ("lds_rows", ctypes.c_int), ("gang_dist", ctypes.c_int),
                ("gang_lanes", ctypes.c_int)]


class CreateOpts(ctypes.Structure):
    """pbg_create_opts_t (pbg_create_v2): versioned by struct_size; precision 64 (default) or 32."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("precision", ctypes.c_int), ("kernel", ctypes.c_int),
                ("lds_rows", ctypes.c_int), ("gang_dist", ctypes.c_int), ("gang_lanes", ctypes.c_int)]

    def __init__(self, precision=64, kernel=-1, lds_rows=-1, gang_dist=-1, gang_lanes=-1):
        super().__init__(ctypes.sizeof(CreateOpts), precision, kernel, lds_rows, gang_dist, gang_lanes)


class SimParams(ctypes.Structure):
    """pbg_sim_params_t: the scene of a handle (scene_bases.py:8-18,58-73)."""
    _fields_ = [("gravity", ctypes.c_double), ("timestep", ctypes.c_double), ("frame_skip", ctypes.c_int),
                ("solver_iterations", ctypes.c_int), ("contact_erp", ctypes.c_double),
                ("joint_limit_erp", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class RolloutIO(ctypes.Structure):
    """pbg_rollout_io_t (pbg_rollout): versioned by struct_size; device pointers of caller-owned buffers.  The
    struct's first version, which ends with done_traj: the library keeps accepting it."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_steps", ctypes.c_int), ("autoreset", ctypes.c_int),
                ("reserved", ctypes.c_int), ("obs", ctypes.c_void_p), ("act", ctypes.c_void_p),
                ("rew", ctypes.c_void_p), ("rew64", ctypes.c_void_p), ("done", ctypes.c_void_p),
                ("cur_return", ctypes.c_void_p), ("cur_length", ctypes.c_void_p), ("done_return", ctypes.c_void_p),
                ("done_length", ctypes.c_void_p), ("done_episodes", ctypes.c_void_p), ("obs_traj", ctypes.c_void_p),
                ("act_traj", ctypes.c_void_p), ("rew_traj", ctypes.c_void_p), ("done_traj", ctypes.c_void_p)]

    def __init__(self, **kw):
        super().__init__(struct_size=ctypes.sizeof(type(self)), **kw)


class RolloutIO2(RolloutIO):
    """pbg_rollout_io_t version 2: the appended truncation records, both or neither (autoreset only)."""
    _fields_ = [("trunc_traj", ctypes.c_void_p), ("term_obs_traj", ctypes.c_void_p)]


PPO_GRAD_FMA, PPO_GRAD_MFMA = 0, 1  # PBG_PPO_GRAD_FMA, PBG_PPO_GRAD_MFMA


class PPOGradOpts(ctypes.Structure):
    """pbg_ppo_grad_opts_t (pbg_ppo_grad_create_ex): versioned by struct_size."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("path", ctypes.c_int)]

    def __init__(self, **kw):
        super().__init__(struct_size=ctypes.sizeof(PPOGradOpts), **kw)


class PPOGradIO(ctypes.Structure):
    """pbg_ppo_grad_io_t (pbg_ppo_grad_run, pbg_ppo_grad_host): versioned by struct_size.  The struct's first version,
    which ends with v_out: the library keeps accepting it."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("batch_rows", ctypes.c_int), ("mb_rows", ctypes.c_int),
                ("reserved", ctypes.c_int), ("theta_actor", ctypes.c_void_p), ("theta_critic", ctypes.c_void_p),
                ("log_std", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("inv_std", ctypes.c_void_p),
                ("clip", ctypes.c_float), ("clip_eps", ctypes.c_float), ("vf_coef", ctypes.c_float),
                ("ent_coef", ctypes.c_float), ("obs", ctypes.c_void_p), ("act", ctypes.c_void_p),
                ("logp_old", ctypes.c_void_p), ("adv", ctypes.c_void_p), ("ret", ctypes.c_void_p),
                ("idx", ctypes.c_void_p), ("adv_norm", ctypes.c_void_p), ("grad_actor", ctypes.c_void_p),
                ("grad_critic", ctypes.c_void_p), ("grad_log_std", ctypes.c_void_p), ("stats", ctypes.c_void_p),
                ("logp_out", ctypes.c_void_p), ("v_out", ctypes.c_void_p)]

    def __init__(self, **kw):
        super().__init__(struct_size=ctypes.sizeof(type(self)), **kw)


class PPOGradIO2(PPOGradIO):
    """pbg_ppo_grad_io_t with the appended value clipping (value_old float32 [B], vf_clip) and KL gate (int32 [2])."""
    _fields_ = [("value_old", ctypes.c_void_p), ("gate", ctypes.c_void_p), ("vf_clip", ctypes.c_float),
                ("reserved2", ctypes.c_int)]


PPO_OPT_MAX_BLOCKS = 8  # PBG_PPO_OPT_MAX_BLOCKS


class PPOOptIO(ctypes.Structure):
    """pbg_ppo_opt_io_t (pbg_ppo_opt_step, pbg_ppo_opt_host): versioned by struct_size; m, v, t, bpow: the host
    twin's state.  The struct's first version, which ends with bpow: the library keeps accepting it."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_int),
                ("param", ctypes.c_void_p * PPO_OPT_MAX_BLOCKS), ("grad", ctypes.c_void_p * PPO_OPT_MAX_BLOCKS),
                ("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("max_grad_norm", ctypes.c_double), ("info", ctypes.c_void_p),
                ("m", ctypes.c_void_p * PPO_OPT_MAX_BLOCKS), ("v", ctypes.c_void_p * PPO_OPT_MAX_BLOCKS),
                ("t", ctypes.c_void_p), ("bpow", ctypes.c_void_p)]

    def __init__(self, **kw):
        arrays = {k: kw.pop(k) for k in ("param", "grad", "m", "v") if k in kw}
        super().__init__(struct_size=ctypes.sizeof(type(self)), **kw)
        for k, ptrs in arrays.items():
            for b, p in enumerate(ptrs):
                getattr(self, k)[b] = p


class PPOOptIO2(PPOOptIO):
    """pbg_ppo_opt_io_t with the appended lr_ptr: a float64 [1] the step reads in place of lr (None: lr)."""
    _fields_ = [("lr_ptr", ctypes.c_void_p)]


class PPOOptIO3(PPOOptIO2):
    """pbg_ppo_opt_io_t with the appended KL gate: an int32 [2] whose first word, when not 0, makes the step a no-op.
    The reserved word takes the struct to 352 bytes: 344 is a size the second version's contract refuses."""
    _fields_ = [("gate", ctypes.c_void_p), ("reserved2", ctypes.c_uint64)]


POLICY_MAX_DIM = 256  # PBG_POLICY_MAX_DIM: obs_dim, h1, h2
POLICY_MAX_ACT = 64   # PBG_POLICY_MAX_ACT

_lib = None


def lib():
    """Load libpbg_amd.so, failing loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PbgError(f"{LIB_PATH} not found: the HIP extension is not built "
                       "(run `python __graft_entry__.py` or `make -C pybullet-gym_amd`)")
    L = ctypes.CDLL(LIB_PATH)
    P, I, H = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    L.pbg_create.argtypes = [ctypes.c_char_p, I, I, ctypes.c_uint64, I, ctypes.POINTER(H)]
    L.pbg_create.restype = I
    L.pbg_create_debug.argtypes = [ctypes.c_char_p, I, I, ctypes.c_uint64, I, ctypes.POINTER(DebugOpts),
                                   ctypes.POINTER(H)]
    L.pbg_create_ex.argtypes = [ctypes.c_char_p, I, I, ctypes.c_uint64, I, ctypes.POINTER(SimParams),
                                ctypes.POINTER(DebugOpts), ctypes.POINTER(H)]
    L.pbg_create_v2.argtypes = [ctypes.c_char_p, I, I, ctypes.c_uint64, I, ctypes.POINTER(SimParams),
                                ctypes.POINTER(CreateOpts), ctypes.POINTER(H)]
    L.pbg_precision.argtypes = [H]
    L.pbg_default_sim_params.argtypes = [ctypes.c_char_p, ctypes.POINTER(SimParams)]
    L.pbg_get_sim_params.argtypes = [H, ctypes.POINTER(SimParams)]
    L.pbg_sample_actions.argtypes = [I, I, I, ctypes.c_uint64, ctypes.c_uint32, I, P, P]
    L.pbg_destroy.argtypes = [H]
    L.pbg_destroy.restype = None
    L.pbg_info.argtypes = [H, ctypes.POINTER(Info)]
    L.pbg_reset.argtypes = [H, P, P, P, P]
    L.pbg_step.argtypes = [H, P, P, P, P, P]
    L.pbg_step_ex.argtypes = [H, ctypes.POINTER(StepIO), P]
    L.pbg_get_state.argtypes = [H, P, P, P]
    L.pbg_set_state.argtypes = [H, P, P, P]
    L.pbg_pack_record_sizes.argtypes = [ctypes.c_char_p, ctypes.POINTER(I), ctypes.POINTER(I)]
    L.pbg_pack.argtypes = [ctypes.c_char_p, I, P, P, P]
    if hasattr(L, "pbg_debug_poison"):  # diagnostic entry (tools/vgpr_poison_probe.py also loads older builds)
        L.pbg_debug_poison.argtypes = [H, ctypes.c_uint32, P]
        L.pbg_debug_poison.restype = I
    L.pbg_last_error.restype = ctypes.c_char_p
    if hasattr(L, "pbg_policy_create"):  # the tools also load diagnostic and older builds without the policy
        FP = ctypes.POINTER(ctypes.c_float)
        L.pbg_policy_create.argtypes = [I, I, I, I, I, FP, FP, FP, FP, FP, FP, ctypes.POINTER(H)]
        L.pbg_policy_destroy.argtypes = [H]
        L.pbg_policy_destroy.restype = None
        L.pbg_policy_act.argtypes = [H, I, P, P, P]
        L.pbg_policy_act_host.argtypes = [H, I, P, P]
        L.pbg_rollout.argtypes = [H, H, ctypes.POINTER(RolloutIO), P]
        for f in ("pbg_policy_create", "pbg_policy_act", "pbg_policy_act_host", "pbg_rollout"):
            getattr(L, f).restype = I
    if hasattr(L, "pbg_population_create"):  # policy populations / evolution strategies
        U64, U32, F = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float
        L.pbg_population_create.argtypes = [I, I, I, I, I, I, I, ctypes.POINTER(H)]
        L.pbg_population_destroy.argtypes = [H]
        L.pbg_population_destroy.restype = None
        L.pbg_population_noise.argtypes = [H, U64, U32, P, P]
        L.pbg_population_noise_host.argtypes = [I, I, I, I, U64, U32, I, I, P]
        L.pbg_population_perturb.argtypes = [H, P, F, U64, U32, P]
        L.pbg_population_set_member.argtypes = [H, I, P, P]
        L.pbg_population_get_member.argtypes = [H, I, P, P]
        L.pbg_population_act.argtypes = [H, I, P, P, P]
        L.pbg_rollout_population.argtypes = [H, H, ctypes.POINTER(RolloutIO), P]
        L.pbg_population_fitness.argtypes = [H, I, P, P, P, P]
        L.pbg_population_grad.argtypes = [H, P, U64, U32, P, P]
        for f in POPULATION_EXPORTED:
            if f != "pbg_population_destroy":
                getattr(L, f).restype = I
    if hasattr(L, "pbg_obs_stats_create"):  # running observation normalisation
        F = ctypes.c_float
        L.pbg_obs_stats_create.argtypes = [I, I, I, ctypes.POINTER(H)]
        L.pbg_obs_stats_destroy.argtypes = [H]
        L.pbg_obs_stats_destroy.restype = None
        L.pbg_obs_stats_update.argtypes = [H, I, I, P, P, P]
        L.pbg_obs_stats_finalize.argtypes = [H, P, P, P]
        L.pbg_obs_stats_get_totals.argtypes = [H, P, P]
        L.pbg_obs_stats_set_totals.argtypes = [H, P, P]
        L.pbg_policy_set_obs_norm.argtypes = [H, P, P, F]
        L.pbg_population_set_obs_norm.argtypes = [H, P, P, F, P]
        L.pbg_policy_attach_obs_stats.argtypes = [H, H]
        L.pbg_population_attach_obs_stats.argtypes = [H, H]
        for f in OBS_NORM_EXPORTED:
            if f != "pbg_obs_stats_destroy":
                getattr(L, f).restype = I
    if hasattr(L, "pbg_action_noise_create"):  # stochastic actions and advantage estimation
        U64, U32, D = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double
        L.pbg_action_noise_create.argtypes = [I, I, U64, ctypes.POINTER(H)]
        L.pbg_action_noise_destroy.argtypes = [H]
        L.pbg_action_noise_destroy.restype = None
        L.pbg_action_noise_set_std.argtypes = [H, P, P]
        L.pbg_action_noise_set_counter.argtypes = [H, U32, P]
        L.pbg_action_noise_get_counter.argtypes = [H, P, P]
        L.pbg_action_noise_set_eps2_traj.argtypes = [H, P]
        L.pbg_action_noise_fill.argtypes = [H, I, I, U32, P, P]
        L.pbg_action_noise_host.argtypes = [I, U64, I, I, U32, P]
        L.pbg_policy_attach_action_noise.argtypes = [H, H]
        L.pbg_population_attach_action_noise.argtypes = [H, H]
        L.pbg_gae.argtypes = [I, I, P, P, P, D, D, P, P, P]
        L.pbg_gae_host.argtypes = [I, I, P, P, P, D, D, P, P]
        for f in ACTION_NOISE_EXPORTED:
            if f != "pbg_action_noise_destroy":
                getattr(L, f).restype = I
    if hasattr(L, "pbg_ppo_grad_create"):  # the PPO update's backward pass
        L.pbg_ppo_grad_create.argtypes = [I, I, I, I, I, I, ctypes.POINTER(H)]
        L.pbg_ppo_grad_destroy.argtypes = [H]
        L.pbg_ppo_grad_destroy.restype = None
        L.pbg_ppo_grad_run.argtypes = [H, ctypes.POINTER(PPOGradIO), P]
        L.pbg_ppo_grad_host.argtypes = [I, I, I, I, ctypes.POINTER(PPOGradIO)]
        for f in PPO_GRAD_EXPORTED:
            if f != "pbg_ppo_grad_destroy":
                getattr(L, f).restype = I
    if hasattr(L, "pbg_ppo_grad_create_ex"):  # its matrix-core path
        L.pbg_ppo_grad_create_ex.argtypes = [I, I, I, I, I, I, ctypes.POINTER(PPOGradOpts), ctypes.POINTER(H)]
        L.pbg_ppo_grad_create_ex.restype = I
    if hasattr(L, "pbg_ppo_opt_create"):  # the advantage normaliser and the clip + Adam step
        I64P = ctypes.POINTER(ctypes.c_int64)
        L.pbg_adv_norm.argtypes = [I, I, P, P, P, P]
        L.pbg_adv_norm_host.argtypes = [I, I, P, P, P]
        L.pbg_ppo_opt_create.argtypes = [I, I, I64P, ctypes.POINTER(H)]
        L.pbg_ppo_opt_destroy.argtypes = [H]
        L.pbg_ppo_opt_destroy.restype = None
        L.pbg_ppo_opt_step.argtypes = [H, P, P]
        L.pbg_ppo_opt_reset.argtypes = [H, P]
        L.pbg_ppo_opt_get_state.argtypes = [H, P, P, P, P]
        L.pbg_ppo_opt_host.argtypes = [I, I64P, P]
        for f in PPO_OPT_EXPORTED:
            if f != "pbg_ppo_opt_destroy":
                getattr(L, f).restype = I
    if hasattr(L, "pbg_perm_create"):  # counter-based permutations and the on-device learning rate
        U64, U32, D = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double
        L.pbg_perm_create.argtypes = [I, U64, ctypes.POINTER(H)]
        L.pbg_perm_destroy.argtypes = [H]
        L.pbg_perm_destroy.restype = None
        L.pbg_perm_fill.argtypes = [H, I, I, P, P]
        L.pbg_perm_set_counter.argtypes = [H, U32, P]
        L.pbg_perm_get_counter.argtypes = [H, P, P]
        L.pbg_perm_host.argtypes = [U64, U32, I, I, P]
        L.pbg_ppo_lr_linear.argtypes = [P, U32, D, P, P]
        L.pbg_ppo_lr_linear_host.argtypes = [P, U32, D, P]
        for f in PERM_EXPORTED:
            if f != "pbg_perm_destroy":
                getattr(L, f).restype = I
    if hasattr(L, "pbg_ppo_grad_run_part"):  # the gradient as parts and the statistics' slots
        L.pbg_ppo_grad_geometry.argtypes = [H, I, ctypes.POINTER(I), ctypes.POINTER(ctypes.c_int64)]
        L.pbg_ppo_grad_run_part.argtypes = [H, ctypes.POINTER(PPOGradIO), I, I, P, P, P]
        L.pbg_ppo_grad_reduce.argtypes = [H, ctypes.POINTER(PPOGradIO), I, P, P, P]
        L.pbg_obs_stats_get_slots.argtypes = [H, I, I, P, P, P]
        L.pbg_obs_stats_set_slots.argtypes = [H, I, I, P, P, P]
        for f in PPO_PARTS_EXPORTED:
            getattr(L, f).restype = I
    if hasattr(L, "pbg_population_act_where"):  # truncation bootstrapping: the masked actor launch and its GAE
        D = ctypes.c_double
        L.pbg_population_act_where.argtypes = [H, I, I, P, P, P, P]
        L.pbg_gae_trunc.argtypes = [I, I, P, P, P, P, P, D, D, P, P, P]
        L.pbg_gae_trunc_host.argtypes = [I, I, P, P, P, P, P, D, D, P, P]
        for f in TRUNC_EXPORTED:
            getattr(L, f).restype = I
    if hasattr(L, "pbg_ppo_gate"):  # value clipping and the KL gate
        L.pbg_ppo_gate_reset.argtypes = [P, P]
        L.pbg_ppo_gate.argtypes = [P, ctypes.c_double, P, P]
        L.pbg_ppo_gate_host.argtypes = [P, ctypes.c_double, P]
        for f in PPO_GATE_EXPORTED:
            getattr(L, f).restype = I
    if hasattr(L, "pbg_ret_stats_create"):  # reward scaling by a running std of the discounted return
        D, F = ctypes.c_double, ctypes.c_float
        L.pbg_ret_stats_create.argtypes = [I, I, I, D, ctypes.POINTER(H)]
        L.pbg_ret_stats_destroy.argtypes = [H]
        L.pbg_ret_stats_destroy.restype = None
        L.pbg_ret_stats_walk.argtypes = [H, I, I, I, P, P, P]
        L.pbg_ret_stats_finalize.argtypes = [H, I, D, P]
        L.pbg_ret_stats_apply.argtypes = [H, I, F, P, P, P]
        L.pbg_ret_stats_reset.argtypes = [H, P]
        L.pbg_ret_stats_get_slots.argtypes = [H, I, I, P, P, P]
        L.pbg_ret_stats_set_slots.argtypes = [H, I, I, P, P, P]
        L.pbg_ret_stats_get_totals.argtypes = [H, P, P, P]
        L.pbg_ret_stats_set_totals.argtypes = [H, P, P, P]
        for f in ("carry", "scale"):
            getattr(L, f"pbg_ret_stats_get_{f}").argtypes = [H, P, P]
            getattr(L, f"pbg_ret_stats_set_{f}").argtypes = [H, P, P]
        for f in RET_STATS_EXPORTED:
            if f != "pbg_ret_stats_destroy":
                getattr(L, f).restype = I
    for f in ("pbg_info", "pbg_reset", "pbg_step", "pbg_step_ex", "pbg_get_state", "pbg_set_state",
              "pbg_pack_record_sizes", "pbg_pack", "pbg_create_debug", "pbg_sample_actions", "pbg_create_ex",
              "pbg_default_sim_params", "pbg_get_sim_params", "pbg_create_v2", "pbg_precision"):
        getattr(L, f).restype = I
    _lib = L
    return L


POLICY_EXPORTED = ("pbg_policy_create", "pbg_policy_destroy", "pbg_policy_act", "pbg_policy_act_host", "pbg_rollout")
POPULATION_EXPORTED = ("pbg_population_create", "pbg_population_destroy", "pbg_population_noise",
                       "pbg_population_noise_host", "pbg_population_perturb", "pbg_population_set_member",
                       "pbg_population_get_member", "pbg_population_act", "pbg_rollout_population",
                       "pbg_population_fitness", "pbg_population_grad")
OBS_NORM_EXPORTED = ("pbg_obs_stats_create", "pbg_obs_stats_destroy", "pbg_obs_stats_update", "pbg_obs_stats_finalize",
                     "pbg_obs_stats_get_totals", "pbg_obs_stats_set_totals", "pbg_policy_set_obs_norm",
                     "pbg_population_set_obs_norm", "pbg_policy_attach_obs_stats", "pbg_population_attach_obs_stats")
ACTION_NOISE_EXPORTED = ("pbg_action_noise_create", "pbg_action_noise_destroy", "pbg_action_noise_set_std",
                         "pbg_action_noise_set_counter", "pbg_action_noise_get_counter", "pbg_action_noise_set_eps2_traj",
                         "pbg_action_noise_fill", "pbg_action_noise_host", "pbg_policy_attach_action_noise",
                         "pbg_population_attach_action_noise", "pbg_gae", "pbg_gae_host")
PPO_GRAD_EXPORTED = ("pbg_ppo_grad_create", "pbg_ppo_grad_destroy", "pbg_ppo_grad_run", "pbg_ppo_grad_host")
PPO_GRAD_EX_EXPORTED = ("pbg_ppo_grad_create_ex",)
PPO_OPT_EXPORTED = ("pbg_adv_norm", "pbg_adv_norm_host", "pbg_ppo_opt_create", "pbg_ppo_opt_destroy", "pbg_ppo_opt_step",
                    "pbg_ppo_opt_reset", "pbg_ppo_opt_get_state", "pbg_ppo_opt_host")
PERM_EXPORTED = ("pbg_perm_create", "pbg_perm_destroy", "pbg_perm_fill", "pbg_perm_set_counter", "pbg_perm_get_counter",
                 "pbg_perm_host", "pbg_ppo_lr_linear", "pbg_ppo_lr_linear_host")
PPO_PARTS_EXPORTED = ("pbg_ppo_grad_geometry", "pbg_ppo_grad_run_part", "pbg_ppo_grad_reduce", "pbg_obs_stats_get_slots",
                      "pbg_obs_stats_set_slots")
TRUNC_EXPORTED = ("pbg_population_act_where", "pbg_gae_trunc", "pbg_gae_trunc_host")
RET_STATS_EXPORTED = ("pbg_ret_stats_create", "pbg_ret_stats_destroy", "pbg_ret_stats_walk", "pbg_ret_stats_finalize",
                      "pbg_ret_stats_apply", "pbg_ret_stats_reset", "pbg_ret_stats_get_slots", "pbg_ret_stats_set_slots",
                      "pbg_ret_stats_get_totals", "pbg_ret_stats_set_totals", "pbg_ret_stats_get_carry",
                      "pbg_ret_stats_set_carry", "pbg_ret_stats_get_scale", "pbg_ret_stats_set_scale")
PPO_GATE_EXPORTED = ("pbg_ppo_gate_reset", "pbg_ppo_gate", "pbg_ppo_gate_host")
EXPORTED =("pbg_create", "pbg_create_debug", "pbg_create_ex", "pbg_create_v2", "pbg_precision",
            "pbg_default_sim_params", "pbg_get_sim_params",
            "pbg_destroy", "pbg_info", "pbg_reset", "pbg_step", "pbg_step_ex",
            "pbg_get_state", "pbg_set_state", "pbg_pack_record_sizes", "pbg_pack", "pbg_sample_actions",
            "pbg_debug_poison", "pbg_last_error") + POLICY_EXPORTED + POPULATION_EXPORTED + OBS_NORM_EXPORTED + \
    ACTION_NOISE_EXPORTED + PPO_GRAD_EXPORTED + PPO_OPT_EXPORTED + PERM_EXPORTED + PPO_GRAD_EX_EXPORTED + PPO_PARTS_EXPORTED + \
    TRUNC_EXPORTED + RET_STATS_EXPORTED + PPO_GATE_EXPORTED


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().pbg_last_error().decode(errors="replace")
        raise PbgError(f"{what} failed ({rc}): {msg}")


def default_sim_params(env_id: str) -> SimParams:
    """The scene parameters the reference builds env_id with (host-only call, no GPU needed)."""
    p = SimParams()
    check(lib().pbg_default_sim_params(env_id_bytes(env_id), ctypes.byref(p)), "pbg_default_sim_params")
    return p


def sim_params(env_id: str, overrides: dict = None) -> SimParams:
    """default_sim_params(env_id) with the fields in `overrides` replaced (unknown keys raise)."""
    p = default_sim_params(env_id)
    names = {n for n, _ in SimParams._fields_}
    for k, v in (overrides or {}).items():
        if k not in names:
            raise PbgError(f"unknown sim parameter {k!r}; known: {sorted(names)}")
        setattr(p, k, v)
    return p


def env_id_bytes(env_id: str) -> bytes:
    if env_id not in ROBOT_IDS:
        raise PbgError(f"unknown env id {env_id!r}; known: {sorted(ROBOT_IDS)}")
    return env_id.encode()
