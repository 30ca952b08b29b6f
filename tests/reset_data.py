"""Shared builders of the reset tests (tests/test_reset_host.py, tests/test_autoreset_gpu.py): the case
tables, the aux record's layout, the pre-state of the in-launch auto-reset comparison and the float64
oracle's reset as its reference.  numpy and the CPU oracle only: nothing here needs a GPU.

The pre-state (part A): n = 40 envs, env_offset 1000, a fixed seed.  After reset and five warm-up steps
of the Philox actions the state records (phys, aux) are rewritten by ``build_pre``:

  * the episode counter becomes 1 + e % 4 for every env;
  * T = {e % 3 == 1}: ``elapsed`` becomes max_episode_steps - 1, so the next step truncates, and the first
    foot's contact flag is set, so every reset there has a flag to clear (the step reads the previous flags
    of a HalfCheetah's other feet only, for its alive test);
  * D = {e % 3 == 2}: the physical state (and the potential / initial_z / floor / feet words, which a
    HalfCheetah's alive test reads) is replaced by one from which the next step terminates:
      - pendulum family: the first hinge 1.2 rad off upright, at rest (|theta| > 0.2; the double
        pendulum's tip at 2 * 0.6 * cos(1.2) + 0.3 = 0.73 <= 1);
      - Ant: on its back (base quaternion (1, 0, 0, 0)) with the torso centre lowered to LOW_Z, under the
        alive height 0.26, at rest: the legs point away from the floor, and the contact on the torso sphere
        (radius 0.25) lifts its centre to 0.24 at the most.  Random actions almost never topple an Ant, so
        the oracle reaches no such state by itself;
      - AntMuJoCo, HumanoidMuJoCo: their alive test reads state[0] + initial_z with state[0] the torso's
        absolute height (mujoco gym_locomotion_envs.py), which no state above the floor fails; the D envs
        carry an initial_z of LOW_INITIAL_Z in their aux record instead, so the step terminates and the
        reset has to write initial_z again;
      - every other id: a state the float64 oracle reaches under random actions one step before it
        reports done (``oracle_terminal_states``, a fixed seed, found on the CPU), with the frame and crawl
        words of HumanoidFlagrunHarder, whose on-ground counter is set to 169, one frame short of its end;
  * N = {e % 3 == 0}: the survivors, untouched.

InvertedPendulumSwingup and the MuJoCo HalfCheetah have no termination rule: their D envs are left as they
are and survive, and only truncation resets anything there."""
import json
import os

import numpy as np

import oracle
import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import rng

N, OFF, SEED, WARMUP = 40, 1000, 0x2B5E7, 5
ACT_SEED = 0x5EED
MIN_TERMINATED = 4
LOW_Z = 0.2
LOW_INITIAL_Z = -2.0
HINGE = 1.2
HARDER_GROUND_FRAMES = 170  # csrc/sim_params.h PBG_HARDER_GROUND_FRAMES
MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pybullet-gym_amd", "models")

ENVS = ["InvertedPendulumPyBulletEnv-v0", "HopperPyBulletEnv-v0", "HalfCheetahPyBulletEnv-v0",
        "AntPyBulletEnv-v0", "HumanoidPyBulletEnv-v0", "Walker2DPyBulletEnv-v0",
        "InvertedPendulumSwingupPyBulletEnv-v0", "InvertedDoublePendulumPyBulletEnv-v0",
        "HumanoidFlagrunPyBulletEnv-v0", "HopperMuJoCoEnv-v0", "Walker2DMuJoCoEnv-v0",
        "HalfCheetahMuJoCoEnv-v0", "AntMuJoCoEnv-v0", "HumanoidMuJoCoEnv-v0", "InvertedDoublePendulumMuJoCoEnv-v0",
        "HumanoidFlagrunHarderPyBulletEnv-v0", "AtlasPyBulletEnv-v0"]
# ids without a termination rule (gym_pendulum_envs.py:26-39 swingup; mujoco gym_locomotion_envs.py HalfCheetah)
TRUNCATION_ONLY = ("InvertedPendulumSwingupPyBulletEnv-v0", "HalfCheetahMuJoCoEnv-v0")
MUJOCO_3D = ("AntMuJoCoEnv-v0", "HumanoidMuJoCoEnv-v0")

# part A: (env id, precision, launch options).  Default plan: lane for the pendulum family, quad for Ant and
# AntMuJoCo (float64: its own translation unit), gang for the rest.  Then the lane reset of walker kinds 0, 2, 3,
# flagrun and harder (kernel=0), the gang reset on a quad robot (kernel=2), both gang widths and both dynamics.
VARIANTS = [(e, p, {"kernel": 0}) for e in ("HopperPyBulletEnv-v0", "HopperMuJoCoEnv-v0", "AntMuJoCoEnv-v0",
                                             "HumanoidFlagrunPyBulletEnv-v0", "HumanoidFlagrunHarderPyBulletEnv-v0")
            for p in (32, 64)]
VARIANTS += [("AntPyBulletEnv-v0", p, {"kernel": 2}) for p in (32, 64)]
VARIANTS += [("HumanoidPyBulletEnv-v0", 32, {"gang_lanes": 16}), ("HumanoidPyBulletEnv-v0", 32, {"gang_lanes": 32}),
             ("HopperPyBulletEnv-v0", 32, {"gang_dist": 0}), ("HopperPyBulletEnv-v0", 32, {"gang_dist": 1})]
CASES_A = [(e, p, {}) for e in ENVS for p in (32, 64)] + VARIANTS


def case_id(c):
    e, p, o = c
    return "-".join([e.replace("PyBulletEnv-v0", "").replace("Env-v0", ""), f"f{p}"] + [f"{k}{v}" for k, v in o.items()])


# the bounds the suite already holds a reset to (tests/test_gpu.py test_reset_matches_oracle,
# tests/test_f64.py test_f64_reset_matches_oracle)
BOUNDS = {32: dict(state=dict(atol=1e-7, rtol=1e-7), aux=dict(atol=2e-6, rtol=0.0), obs_atol=1e-5),
          64: dict(state=dict(atol=1e-13, rtol=1e-13), aux=dict(atol=1e-13, rtol=1e-13), obs_rel=1.01 * 2.0 ** -23)}

_TABLES = {}


def table(env_id):
    """The model table of env_id (reset_dof, reset_offset, max_episode_steps, ...)."""
    if env_id not in _TABLES:
        with open(os.path.join(MODELS, f"{oracle.ENV_KEYS[env_id]}.json")) as f:
            _TABLES[env_id] = json.load(f)
    return _TABLES[env_id]


class Layout:
    """Word indices of the aux record (csrc/sim_params.h PBG_AUX_RECORD_WORDS) and of q / qd in the state."""

    def __init__(self, env_id):
        t = table(env_id)
        self.NJ, self.NF, self.NR = t["NJ"], t["NF"], t["NR"]
        self.flagrun, self.harder = bool(t.get("flagrun", 0)), bool(t.get("harder", 0))
        self.AD = 4 + self.NF + (4 if self.flagrun else 0) + (5 if self.harder else 0) + 1
        self.SD = 13 + 2 * self.NJ + (13 if self.harder else 0)
        self.pot, self.z0, self.elapsed, self.floor = 0, 1, 2, 3
        self.feet = list(range(4, 4 + self.NF))
        f = 4 + self.NF
        self.flag_target = [f, f + 1] if self.flagrun else []
        self.flag_timeout = [f + 2] if self.flagrun else []
        self.flag_count = [f + 3] if self.flagrun else []
        self.frame = [f + 4] if self.harder else []
        self.onground = [f + 5] if self.harder else []
        self.crawl = [f + 6, f + 7] if self.harder else []  # crawl_start (NaN = None), crawl_ignored
        self.launches = [f + 8] if self.harder else []
        self.episode = self.AD - 1
        # everything a reset leaves as a small integer or a flag, against the continuous words
        self.continuous = [self.pot, self.z0] + self.flag_target + self.crawl
        self.discrete = [i for i in range(self.AD) if i not in self.continuous]
        # what a reset carries over from the aux record it starts from
        self.carried = self.flag_count + self.launches
        self.q = np.arange(13, 13 + self.NJ)
        self.qd = np.arange(13 + self.NJ, 13 + 2 * self.NJ)
        self.reset_q = 13 + np.asarray(t["reset_dof"], dtype=np.int64)
        self.reset_offset = np.asarray(t["reset_offset"], dtype=np.float64)
        self.max_steps = int(t["max_episode_steps"])


def sets(n=N):
    e = np.arange(n)
    return e % 3 == 0, e % 3 == 1, e % 3 == 2  # N (survivors), T (truncated), D (terminated)


def host_actions(env_id, n, steps, step0=0, env_offset=OFF):
    """The Philox action batches ``sample_actions(..., seed=ACT_SEED, env_offset=env_offset)`` draws on the device."""
    na = table(env_id)["NA"]
    return rng.sample_actions(na, np.arange(env_offset, env_offset + n), np.arange(step0, step0 + steps), seed=ACT_SEED)


def expected_reset_q(env_id, precision, gids, episodes, seed=SEED):
    """The reset dofs after a reset, in the handle's scalar type: offset + noise, one rounding each."""
    L = Layout(env_id)
    noise = rng.reset_noise(seed, gids, episodes, L.NR)
    if precision == 32:
        return (L.reset_offset.astype(np.float32)[None, :] + noise).astype(np.float32)
    return L.reset_offset[None, :] + noise.astype(np.float64)


_TERMINAL = {}


def oracle_terminal_states(env_id, count, n=48, max_steps=150, seed=77):
    """(phys, aux) records, ``count`` of each, that the float64 oracle holds one step before it reports done:
    n envs from the reset draw of episode 0 under Philox actions (seed ACT_SEED, global ids from 0), each env's
    first termination, in the order the oracle meets them (by step, then by env).  Deterministic.
    HumanoidFlagrunHarder may crawl: it ends only once its on-ground counter reaches 170 frames, far past any
    short rollout, so there the event taken is the step that first counts a frame on the ground (z < 0.8), and
    ``build_pre`` sets the counter one short of its limit."""
    key = (env_id, count)
    if key in _TERMINAL:
        return _TERMINAL[key]
    o = oracle.OracleEnvs(env_id, n, nthreads=min(16, os.cpu_count() or 1), seed=seed)
    o.reset(rng.reset_noise(seed, np.arange(n), 0, o.info.NR).astype(np.float64))
    seen = np.zeros(n, bool)
    phys, aux = [], []
    L = Layout(env_id)
    for t in range(max_steps):
        s0, a0 = o.state.copy(), o.aux.copy()
        act = rng.sample_actions(o.info.NA, np.arange(n), [t], seed=ACT_SEED)[0]
        _, _, done, _ = o.step(act)
        if L.harder:
            done = done | (o.aux[:, L.onground[0]] > 0)
        new = done & ~seen
        phys.extend(s0[new])
        aux.extend(a0[new])
        seen |= done
        if len(phys) >= count:
            break
        if seen.any():  # an env that ended goes on from a fresh reset (its later terminations are not taken)
            o.reset(rng.reset_noise(seed, np.arange(n), 1, o.info.NR).astype(np.float64), mask=done.astype(np.uint8))
    assert len(phys) >= count, (env_id, len(phys), count)
    _TERMINAL[key] = (np.array(phys[:count]), np.array(aux[:count]))
    return _TERMINAL[key]


def build_pre(env_id, phys, aux):
    """The part-A pre-state from the records after the warm-up (numpy [n, SD], [n, AD]); returns new
    arrays (pre_phys, pre_aux) and aux_c, the control run's aux (nobody's elapsed raised)."""
    L = Layout(env_id)
    n = len(phys)
    assert phys.shape == (n, L.SD) and aux.shape == (n, L.AD)
    e = np.arange(n)
    _, T, D = sets(n)
    phys, aux = phys.copy(), aux.copy()
    aux[:, L.episode] = 1 + e % 4
    t = table(env_id)
    if env_id in TRUNCATION_ONLY:
        pass
    elif t["kind"] == 1:  # pendulum family: the first hinge beyond its done angle, at rest
        d = np.flatnonzero(D)
        phys[np.ix_(d, L.qd)] = 0.0
        phys[d, L.reset_q[0]] = HINGE + 0.01 * (d % 7)
    elif env_id == "AntPyBulletEnv-v0":  # on its back, the torso centre under the alive height, at rest
        d = np.flatnonzero(D)
        phys[d, 2] = LOW_Z
        phys[d, 3:7] = [1.0, 0.0, 0.0, 0.0]
        phys[d, 7:13] = 0.0
        phys[np.ix_(d, L.qd)] = 0.0
    elif env_id in MUJOCO_3D:  # an initial_z that puts state[0] + initial_z under the alive height
        d = np.flatnonzero(D)
        aux[d, L.z0] = LOW_INITIAL_Z - 0.01 * (d % 7)
    else:
        d = np.flatnonzero(D)
        sp, sa = oracle_terminal_states(env_id, len(d))
        phys[d] = sp
        for w in [L.pot, L.z0, L.floor] + L.feet + L.frame + L.crawl:
            aux[d, w] = sa[:, w]
        if L.harder:
            aux[d, L.onground[0]] = HARDER_GROUND_FRAMES - 1
    if L.feet:  # five steps in, an Ant or a Humanoid is still falling towards the floor
        aux[T, L.feet[0]] = 1.0
    aux_c = aux.copy()
    aux[T, L.elapsed] = L.max_steps - 1
    return phys, aux, aux_c


def oracle_warmup(env_id, n=N):
    """What the device does before part A's rewrite, on the float64 oracle: reset (episode 0 noise) and
    WARMUP steps of the Philox actions.  Returns the oracle."""
    o = oracle.OracleEnvs(env_id, n, nthreads=min(16, os.cpu_count() or 1), seed=SEED, env_offset=OFF)
    o.reset(rng.reset_noise(SEED, np.arange(OFF, OFF + n), 0, o.info.NR).astype(np.float64))
    acts = host_actions(env_id, n, WARMUP)
    for t in range(WARMUP):
        o.step(acts[t])
    return o


def oracle_reset_reference(env_id, phys, aux, mask, q=None, seed=SEED, env_offset=OFF):
    """Reference 2: the float64 oracle resets the masked envs of (phys, aux) with the Philox noise of each
    env's own episode counter (or the rows of q).  Returns (state, aux, obs); unmasked obs rows are NaN."""
    L = Layout(env_id)
    n = len(phys)
    o = oracle.OracleEnvs(env_id, n, seed=seed, env_offset=env_offset)
    o.state[:] = phys
    o.aux[:] = aux
    if q is None:
        q = rng.reset_noise(seed, np.arange(env_offset, env_offset + n), aux[:, L.episode].astype(np.uint32), L.NR)
    obs = np.full((n, o.info.OBS), np.nan, dtype=np.float32)
    o.reset(np.asarray(q, dtype=np.float64), mask=np.asarray(mask, dtype=np.uint8), obs=obs)
    return o.state, o.aux, obs


def bits(a):
    """The array's words as unsigned integers, for bitwise comparisons (NaN payloads and -0.0 included)."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
