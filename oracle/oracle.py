"""ctypes binding of the CPU oracle (libpbg_oracle.so).  TEST INFRASTRUCTURE ONLY.

Importable from tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg; the
product package (pybullet-gym_amd/) never imports this module.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # the repository root: the package's import shim
import pybulletgym_amd  # noqa: E402,F401
from pybulletgym_amd import robots  # noqa: E402  (the robot registry; torch-free)

LIB_PATH = os.path.join(HERE, "libpbg_oracle.so")
ROBOT_IDS = {s.key: s.robot_id for s in robots.BY_ID}
ENV_KEYS = {s.env_id: s.key for s in robots.BY_ID}

_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        os.environ.setdefault("OMP_STACKSIZE", "16M")  # Atlas-sized per-env frames on worker threads
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.c_void_p
        L.pbg_oracle_info.argtypes = [ctypes.c_int, P]
        L.pbg_oracle_reset.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P]
        L.pbg_oracle_reset_mask.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, P]
        L.pbg_oracle_step.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, P, P, P, ctypes.c_int, P, P]
        L.pbg_oracle_step_ex.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, P, P, P, ctypes.c_int, P, P,
                                         ctypes.c_int, P]
        L.pbg_oracle_count_flops.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P]
        L.pbg_oracle_set_physics.argtypes = [P, ctypes.c_int]
        L.pbg_oracle_set_sim_params.argtypes = [P]
        L.pbg_oracle_pack.argtypes = [ctypes.c_int, P, P]
        L.pbg_oracle_pack_flag.argtypes = [ctypes.c_int, P, P, P, P]
        L.pbg_oracle_pack_harder.argtypes = [ctypes.c_int, P, P, P, P, P, P]
        L.pbg_oracle_set_rng.argtypes = [ctypes.c_uint64, ctypes.c_int]
        L.pbg_oracle_set_mca_seed.argtypes = [ctypes.c_uint64]
        L.pbg_oracle_set_mca_seed.restype = None
        L.pbg_oracle_dynamics.argtypes = [ctypes.c_int, P, P, P]
        L.pbg_oracle_link_com.argtypes = [ctypes.c_int, P, P]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def robot_id(name: str) -> int:
    return ROBOT_IDS[ENV_KEYS.get(name, name)]


class Info:
    FIELDS = ("NL", "NJ", "NDOF", "NA", "NO", "NR", "NF", "NP", "NS", "NPAIR", "OBS", "SD", "AD",
              "floating", "kind", "substeps")

    def __init__(self, rid):
        out = np.zeros(16, dtype=np.int32)
        assert lib().pbg_oracle_info(rid, _p(out)) == 0
        for k, v in zip(self.FIELDS, out):
            setattr(self, k, int(v))


class OracleEnvs:
    """Batch of n envs stepped by the CPU oracle (float64 physics)."""

    def __init__(self, name: str, n: int, nthreads: int = 1, seed: int = 0, env_offset: int = 0, precision: int = 64):
        """seed / env_offset key the Philox draws of HumanoidFlagrun's flag (as the kernels').
        precision 32: the physics in IEEE float32 (the conditioning probe of the parity tests);
        33: float32 Monte Carlo arithmetic (oracle/mca.h; set_mca_seed picks the stream)."""
        self.precision = precision
        lib().pbg_oracle_set_rng(seed, env_offset)
        self.rid = robot_id(name)
        self.info = Info(self.rid)
        self.n = n
        self.nthreads = nthreads
        self.state = np.zeros((n, self.info.SD), dtype=np.float64)
        self.aux = np.zeros((n, self.info.AD), dtype=np.float64)
        self.csig = np.zeros(n, dtype=np.uint32)      # last step's contact-set signatures
        self.asig = np.zeros(n, dtype=np.uint32)      # last step's solver active-set signatures
        self.terms = np.zeros((n, 5), dtype=np.float64)  # last step's reward terms

    def reset(self, qinit: np.ndarray, mask: np.ndarray = None, obs: np.ndarray = None) -> np.ndarray:
        """Reset all envs (or those with mask != 0, writing their rows of `obs`)."""
        qinit = np.ascontiguousarray(qinit, dtype=np.float64).reshape(self.n, self.info.NR)
        if obs is None:
            obs = np.zeros((self.n, self.info.OBS), dtype=np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        assert lib().pbg_oracle_reset_mask(self.rid, self.n, _p(self.state), _p(self.aux), _p(qinit), _p(obs),
                                           _p(m)) == 0
        return obs

    def step(self, act: np.ndarray):
        act = np.ascontiguousarray(act, dtype=np.float32).reshape(self.n, self.info.NA)
        obs = np.zeros((self.n, self.info.OBS), dtype=np.float32)
        rew = np.zeros(self.n, dtype=np.float64)
        done = np.zeros(self.n, dtype=np.uint8)
        nc = np.zeros(self.n, dtype=np.int32)
        assert lib().pbg_oracle_step_ex(self.rid, self.n, _p(self.state), _p(self.aux), _p(act), _p(obs),
                                        _p(rew), _p(done), _p(nc), self.nthreads, _p(self.csig), _p(self.terms),
                                        self.precision, _p(self.asig)) == 0
        return obs, rew, done.astype(bool), nc


SIM_PARAM_FIELDS = ("gravity", "timestep", "frame_skip", "solver_iterations", "contact_erp", "joint_limit_erp")


def set_sim_params(params: dict = None):
    """The scene of the product's pbg_create_ex (include/pbg.h pbg_sim_params_t) for every
    following oracle call: ``params`` maps all six SIM_PARAM_FIELDS; None restores the
    reference's scene."""
    if params is None:
        lib().pbg_oracle_set_sim_params(None)
        return
    v = np.array([float(params[k]) for k in SIM_PARAM_FIELDS], np.float64)
    lib().pbg_oracle_set_sim_params(v.ctypes.data_as(ctypes.c_void_p))


def set_mca_seed(seed: int):
    """Stream of the float32 Monte Carlo arithmetic (precision 33): env e of the next step
    calls draws from the stream keyed by (seed, e)."""
    lib().pbg_oracle_set_mca_seed(seed)


def dynamics(name: str, state: np.ndarray):
    rid = robot_id(name)
    info = Info(rid)
    M = np.zeros((info.NDOF, info.NDOF))
    C = np.zeros(info.NDOF)
    lib().pbg_oracle_dynamics(rid, _p(np.ascontiguousarray(state, dtype=np.float64)), _p(M), _p(C))
    return M, C


def link_com(name: str, state: np.ndarray):
    rid = robot_id(name)
    info = Info(rid)
    out = np.zeros((info.NL + 1, 3))
    lib().pbg_oracle_link_com(rid, _p(np.ascontiguousarray(state, dtype=np.float64)), _p(out))
    return out


class _PackIn(ctypes.Structure):
    _fields_ = [("part_xyz", ctypes.c_void_p), ("n_parts", ctypes.c_int),
                ("body_quat", ctypes.c_void_p), ("body_pos", ctypes.c_void_p),
                ("body_vel", ctypes.c_void_p), ("jq", ctypes.c_void_p), ("jqd", ctypes.c_void_p),
                ("feet_prev", ctypes.c_void_p), ("feet_new", ctypes.c_void_p), ("act", ctypes.c_void_p),
                ("potential_old", ctypes.c_double), ("initial_z", ctypes.c_double),
                ("target_x", ctypes.c_double), ("target_y", ctypes.c_double),
                ("body_avel", ctypes.c_void_p), ("head_z", ctypes.c_double)]


class _PackOut(ctypes.Structure):
    _fields_ = [("obs", ctypes.c_void_p), ("reward", ctypes.c_double), ("done", ctypes.c_uint8),
                ("potential", ctypes.c_double), ("initial_z", ctypes.c_double),
                ("feet_out", ctypes.c_void_p), ("rewards", ctypes.c_double * 5), ("dist", ctypes.c_double),
                ("pitch", ctypes.c_double), ("at_limit", ctypes.c_int), ("body_xyz", ctypes.c_double * 3)]


def pack(name, part_xyz, body_quat, body_pos, body_vel, jq, jqd, feet_prev, feet_new, act,
         potential_old, initial_z, flag=None, body_avel=None, harder=None, head_z=0.0):
    """Run the oracle's pack on explicit inputs (golden-vector tests).  flag (HumanoidFlagrun):
    [target x, y, flag_timeout, next draw x, y]; the result then carries flag_out.  harder
    (HumanoidFlagrunHarder, with flag): [frame, on_ground, crawl_start, crawl_ignored, launch
    draws 5]; the result then carries harder_out (pbg_oracle_pack_harder)."""
    rid = robot_id(name)
    info = Info(rid)
    arrs = dict(part_xyz=np.ascontiguousarray(part_xyz, dtype=np.float64),
                body_quat=np.ascontiguousarray(body_quat, dtype=np.float64),
                body_pos=np.ascontiguousarray(body_pos, dtype=np.float64),
                body_vel=np.ascontiguousarray(body_vel, dtype=np.float64),
                jq=np.ascontiguousarray(jq, dtype=np.float64), jqd=np.ascontiguousarray(jqd, dtype=np.float64),
                feet_prev=np.ascontiguousarray(feet_prev, dtype=np.float32))
    fn = None if feet_new is None else np.ascontiguousarray(feet_new, dtype=np.uint8)
    ac = None if act is None else np.ascontiguousarray(act, dtype=np.float32)
    pin = _PackIn(_p(arrs["part_xyz"]), len(arrs["part_xyz"]), _p(arrs["body_quat"]), _p(arrs["body_pos"]),
                  _p(arrs["body_vel"]), _p(arrs["jq"]), _p(arrs["jqd"]), _p(arrs["feet_prev"]), _p(fn),
                  _p(ac), float(potential_old), float(initial_z), 1e3, 0.0, None, float(head_z))
    if body_avel is not None:
        arrs["body_avel"] = np.ascontiguousarray(body_avel, dtype=np.float64)
        pin.body_avel = _p(arrs["body_avel"])
    obs = np.zeros(info.OBS, dtype=np.float32)
    feet_out = np.zeros(max(1, info.NF), dtype=np.float32)
    pout = _PackOut()
    pout.obs = _p(obs)
    pout.feet_out = _p(feet_out)
    flag_out = np.zeros(3)
    harder_out = np.zeros(11)
    if flag is None:
        assert lib().pbg_oracle_pack(rid, ctypes.byref(pin), ctypes.byref(pout)) == 0
    elif harder is not None:
        fin = np.ascontiguousarray(flag, dtype=np.float64)
        hin = np.ascontiguousarray(harder, dtype=np.float64)
        assert lib().pbg_oracle_pack_harder(rid, ctypes.byref(pin), ctypes.byref(pout), _p(fin), _p(flag_out),
                                            _p(hin), _p(harder_out)) == 0
    else:
        fin = np.ascontiguousarray(flag, dtype=np.float64)
        assert lib().pbg_oracle_pack_flag(rid, ctypes.byref(pin), ctypes.byref(pout), _p(fin), _p(flag_out)) == 0
    return dict(obs=obs, reward=pout.reward, done=bool(pout.done), potential=pout.potential,
                initial_z=pout.initial_z, feet=feet_out[:info.NF].copy(), rewards=list(pout.rewards),
                flag_out=flag_out, harder_out=harder_out)
