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

# Every entry point of include/pbg.h, once: group -> {name: (restype, argtypes)}.  "core" is what every build has;
# any other group is bound when the loaded library has its first name (the tools also load diagnostic and older
# builds), and GROUP_EXPORTED is its names.  A new unit is one group here.
_P = _H = ctypes.c_void_p
_I, _U32, _U64, _F, _D, _S = (ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float, ctypes.c_double,
                              ctypes.c_char_p)
_HP, _IP, _I64P, _FP = (ctypes.POINTER(t) for t in (_H, _I, ctypes.c_int64, ctypes.c_float))
_SIM, _DBG, _RIO, _GIO = (ctypes.POINTER(t) for t in (SimParams, DebugOpts, RolloutIO, PPOGradIO))
SIGNATURES = {
    "core": {
        "pbg_create": (_I, [_S, _I, _I, _U64, _I, _HP]),
        "pbg_create_debug": (_I, [_S, _I, _I, _U64, _I, _DBG, _HP]),
        "pbg_create_ex": (_I, [_S, _I, _I, _U64, _I, _SIM, _DBG, _HP]),
        "pbg_create_v2": (_I, [_S, _I, _I, _U64, _I, _SIM, ctypes.POINTER(CreateOpts), _HP]),
        "pbg_precision": (_I, [_H]),
        "pbg_default_sim_params": (_I, [_S, _SIM]),
        "pbg_get_sim_params": (_I, [_H, _SIM]),
        "pbg_destroy": (None, [_H]),
        "pbg_info": (_I, [_H, ctypes.POINTER(Info)]),
        "pbg_reset": (_I, [_H, _P, _P, _P, _P]),
        "pbg_step": (_I, [_H, _P, _P, _P, _P, _P]),
        "pbg_step_ex": (_I, [_H, ctypes.POINTER(StepIO), _P]),
        "pbg_get_state": (_I, [_H, _P, _P, _P]),
        "pbg_set_state": (_I, [_H, _P, _P, _P]),
        "pbg_pack_record_sizes": (_I, [_S, _IP, _IP]),
        "pbg_pack": (_I, [_S, _I, _P, _P, _P]),
        "pbg_sample_actions": (_I, [_I, _I, _I, _U64, _U32, _I, _P, _P]),
        "pbg_last_error": (_S, []),
    },
    "debug_poison": {  # diagnostic entry (tools/vgpr_poison_probe.py also loads older builds)
        "pbg_debug_poison": (_I, [_H, _U32, _P]),
    },
    "policy": {
        "pbg_policy_create": (_I, [_I, _I, _I, _I, _I, _FP, _FP, _FP, _FP, _FP, _FP, _HP]),
        "pbg_policy_destroy": (None, [_H]),
        "pbg_policy_act": (_I, [_H, _I, _P, _P, _P]),
        "pbg_policy_act_host": (_I, [_H, _I, _P, _P]),
        "pbg_rollout": (_I, [_H, _H, _RIO, _P]),
    },
    "population": {  # policy populations / evolution strategies
        "pbg_population_create": (_I, [_I, _I, _I, _I, _I, _I, _I, _HP]),
        "pbg_population_destroy": (None, [_H]),
        "pbg_population_noise": (_I, [_H, _U64, _U32, _P, _P]),
        "pbg_population_noise_host": (_I, [_I, _I, _I, _I, _U64, _U32, _I, _I, _P]),
        "pbg_population_perturb": (_I, [_H, _P, _F, _U64, _U32, _P]),
        "pbg_population_set_member": (_I, [_H, _I, _P, _P]),
        "pbg_population_get_member": (_I, [_H, _I, _P, _P]),
        "pbg_population_act": (_I, [_H, _I, _P, _P, _P]),
        "pbg_rollout_population": (_I, [_H, _H, _RIO, _P]),
        "pbg_population_fitness": (_I, [_H, _I, _P, _P, _P, _P]),
        "pbg_population_grad": (_I, [_H, _P, _U64, _U32, _P, _P]),
    },
    "obs_norm": {  # running observation normalisation
        "pbg_obs_stats_create": (_I, [_I, _I, _I, _HP]),
        "pbg_obs_stats_destroy": (None, [_H]),
        "pbg_obs_stats_update": (_I, [_H, _I, _I, _P, _P, _P]),
        "pbg_obs_stats_finalize": (_I, [_H, _P, _P, _P]),
        "pbg_obs_stats_get_totals": (_I, [_H, _P, _P]),
        "pbg_obs_stats_set_totals": (_I, [_H, _P, _P]),
        "pbg_policy_set_obs_norm": (_I, [_H, _P, _P, _F]),
        "pbg_population_set_obs_norm": (_I, [_H, _P, _P, _F, _P]),
        "pbg_policy_attach_obs_stats": (_I, [_H, _H]),
        "pbg_population_attach_obs_stats": (_I, [_H, _H]),
    },
    "action_noise": {  # stochastic actions and advantage estimation
        "pbg_action_noise_create": (_I, [_I, _I, _U64, _HP]),
        "pbg_action_noise_destroy": (None, [_H]),
        "pbg_action_noise_set_std": (_I, [_H, _P, _P]),
        "pbg_action_noise_set_counter": (_I, [_H, _U32, _P]),
        "pbg_action_noise_get_counter": (_I, [_H, _P, _P]),
        "pbg_action_noise_set_eps2_traj": (_I, [_H, _P]),
        "pbg_action_noise_fill": (_I, [_H, _I, _I, _U32, _P, _P]),
        "pbg_action_noise_host": (_I, [_I, _U64, _I, _I, _U32, _P]),
        "pbg_policy_attach_action_noise": (_I, [_H, _H]),
        "pbg_population_attach_action_noise": (_I, [_H, _H]),
        "pbg_gae": (_I, [_I, _I, _P, _P, _P, _D, _D, _P, _P, _P]),
        "pbg_gae_host": (_I, [_I, _I, _P, _P, _P, _D, _D, _P, _P]),
    },
    "ppo_grad": {  # the PPO update's backward pass
        "pbg_ppo_grad_create": (_I, [_I, _I, _I, _I, _I, _I, _HP]),
        "pbg_ppo_grad_destroy": (None, [_H]),
        "pbg_ppo_grad_run": (_I, [_H, _GIO, _P]),
        "pbg_ppo_grad_host": (_I, [_I, _I, _I, _I, _GIO]),
    },
    "ppo_opt": {  # the advantage normaliser and the clip + Adam step
        "pbg_adv_norm": (_I, [_I, _I, _P, _P, _P, _P]),
        "pbg_adv_norm_host": (_I, [_I, _I, _P, _P, _P]),
        "pbg_ppo_opt_create": (_I, [_I, _I, _I64P, _HP]),
        "pbg_ppo_opt_destroy": (None, [_H]),
        "pbg_ppo_opt_step": (_I, [_H, _P, _P]),
        "pbg_ppo_opt_reset": (_I, [_H, _P]),
        "pbg_ppo_opt_get_state": (_I, [_H, _P, _P, _P, _P]),
        "pbg_ppo_opt_host": (_I, [_I, _I64P, _P]),
    },
    "perm": {  # counter-based permutations and the on-device learning rate
        "pbg_perm_create": (_I, [_I, _U64, _HP]),
        "pbg_perm_destroy": (None, [_H]),
        "pbg_perm_fill": (_I, [_H, _I, _I, _P, _P]),
        "pbg_perm_set_counter": (_I, [_H, _U32, _P]),
        "pbg_perm_get_counter": (_I, [_H, _P, _P]),
        "pbg_perm_host": (_I, [_U64, _U32, _I, _I, _P]),
        "pbg_ppo_lr_linear": (_I, [_P, _U32, _D, _P, _P]),
        "pbg_ppo_lr_linear_host": (_I, [_P, _U32, _D, _P]),
    },
    "ppo_grad_ex": {  # the gradient's matrix-core path
        "pbg_ppo_grad_create_ex": (_I, [_I, _I, _I, _I, _I, _I, ctypes.POINTER(PPOGradOpts), _HP]),
    },
    "ppo_parts": {  # the gradient as parts and the statistics' slots
        "pbg_ppo_grad_geometry": (_I, [_H, _I, _IP, _I64P]),
        "pbg_ppo_grad_run_part": (_I, [_H, _GIO, _I, _I, _P, _P, _P]),
        "pbg_ppo_grad_reduce": (_I, [_H, _GIO, _I, _P, _P, _P]),
        "pbg_obs_stats_get_slots": (_I, [_H, _I, _I, _P, _P, _P]),
        "pbg_obs_stats_set_slots": (_I, [_H, _I, _I, _P, _P, _P]),
    },
    "trunc": {  # truncation bootstrapping: the masked actor launch and its GAE
        "pbg_population_act_where": (_I, [_H, _I, _I, _P, _P, _P, _P]),
        "pbg_gae_trunc": (_I, [_I, _I, _P, _P, _P, _P, _P, _D, _D, _P, _P, _P]),
        "pbg_gae_trunc_host": (_I, [_I, _I, _P, _P, _P, _P, _P, _D, _D, _P, _P]),
    },
    "ret_stats": {  # reward scaling by a running std of the discounted return
        "pbg_ret_stats_create": (_I, [_I, _I, _I, _D, _HP]),
        "pbg_ret_stats_destroy": (None, [_H]),
        "pbg_ret_stats_walk": (_I, [_H, _I, _I, _I, _P, _P, _P]),
        "pbg_ret_stats_finalize": (_I, [_H, _I, _D, _P]),
        "pbg_ret_stats_apply": (_I, [_H, _I, _F, _P, _P, _P]),
        "pbg_ret_stats_reset": (_I, [_H, _P]),
        "pbg_ret_stats_get_slots": (_I, [_H, _I, _I, _P, _P, _P]),
        "pbg_ret_stats_set_slots": (_I, [_H, _I, _I, _P, _P, _P]),
        "pbg_ret_stats_get_totals": (_I, [_H, _P, _P, _P]),
        "pbg_ret_stats_set_totals": (_I, [_H, _P, _P, _P]),
        "pbg_ret_stats_get_carry": (_I, [_H, _P, _P]),
        "pbg_ret_stats_set_carry": (_I, [_H, _P, _P]),
        "pbg_ret_stats_get_scale": (_I, [_H, _P, _P]),
        "pbg_ret_stats_set_scale": (_I, [_H, _P, _P]),
    },
    "ppo_gate": {  # value clipping and the KL gate
        "pbg_ppo_gate_reset": (_I, [_P, _P]),
        "pbg_ppo_gate": (_I, [_P, _D, _P, _P]),
        "pbg_ppo_gate_host": (_I, [_P, _D, _P]),
    },
}
EXPORTED = tuple(n for sigs in SIGNATURES.values() for n in sigs)
# POLICY_EXPORTED, POPULATION_EXPORTED, OBS_NORM_EXPORTED, ACTION_NOISE_EXPORTED, PPO_GRAD_EXPORTED, PPO_OPT_EXPORTED,
# PERM_EXPORTED, PPO_GRAD_EX_EXPORTED, PPO_PARTS_EXPORTED, TRUNC_EXPORTED, RET_STATS_EXPORTED, PPO_GATE_EXPORTED
globals().update({f"{g.upper()}_EXPORTED": tuple(sigs) for g, sigs in SIGNATURES.items()
                  if g not in ("core", "debug_poison")})

_lib = None


def lib():
    """Load libpbg_amd.so, failing loudly if it is absent, and give every entry point its signature."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PbgError(f"{LIB_PATH} not found: the HIP extension is not built "
                       "(run `python __graft_entry__.py` or `make -C pybullet-gym_amd`)")
    L = ctypes.CDLL(LIB_PATH)
    for group, sigs in SIGNATURES.items():
        if group != "core" and not hasattr(L, next(iter(sigs))):
            continue
        for name, (restype, argtypes) in sigs.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


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
