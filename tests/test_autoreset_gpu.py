"""The resets the suite compared with nothing: the reset every step kernel does inside its launch (lane
``reset_env``, gang ``reset_env_epi<R, 4>``, quad ``team_reset``; both precisions), ``pbg_reset`` with a
mask, and the lane kernel's 32- and 64-lane workgroups.  Run on an MI355X:  python -m pytest tests -m gpu

A. In-launch auto-reset.  From the pre-state of tests/reset_data.py (40 envs at env_offset 1000: a third
   truncates, a third terminates, a third survives; episode counters 1 + e % 4) one step with auto-reset is
   compared, every env of it, with
     * a control run C of the same step without auto-reset (flags, survivors' bits, terminal observation,
       rewards);
     * the host Philox draw of each env's own (global id, episode), bit for bit;
     * reference 1, the standalone ``reset(mask)`` of the same precision from the same records: physical
       record and discrete bookkeeping equal, the continuous words and the observation within the bounds below;
     * reference 2, the float64 oracle's masked reset, within the bounds the suite already holds a reset to
       (reset_data.BOUNDS: test_reset_matches_oracle, test_f64_reset_matches_oracle).
   The envs that reset are T and every env C reports done: the D envs that terminate, and any other env that
   happens to (Hopper and the MuJoCo Hopper fall within six random steps); everything else is a survivor.
   The step itself may re-draw Flagrun's flag or launch Harder's cube before the reset: the two counters a
   reset carries over (flag draws, cube launches) are taken from C's record after the step.
B. ``reset(mask=...)``: all ones equal to None, unmasked rows untouched, bool like uint8, with ``init_q``
   against the oracle, and the host Philox draw of episodes 0 and 1 for every id and both precisions.
C. The lane kernel at ``info.block`` 32 and 64 (24 and 40 envs per CU, plus 7): three 64-env windows of the
   big batch bitwise equal to the same envs run alone at width 16, and teacher forcing against the oracle.
"""
import numpy as np
import pytest
import torch

import oracle
import pybulletgym_amd  # noqa: F401
from pybulletgym_amd.vec_env import VecEnv, sample_actions

import reset_data as rd
from reset_data import bits
from test_f64 import _teacher_forced64
from test_gpu import _rel, _report, _teacher_forced

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.detach().cpu().numpy().copy()


def _scalar(a, precision):
    """State words in the handle's scalar type (the float64 records hold float32 values exactly)."""
    return a.astype(np.float32) if precision == 32 else a


def _state(env):
    phys, aux = env.get_state()
    return _np(phys), _np(aux)


def _set(env, phys, aux):
    env.set_state(torch.from_numpy(phys), torch.from_numpy(aux))


def _within_reset_bounds(precision, what, got, want, ctx):
    """got against want under the bound the suite states for a reset; returns the largest difference."""
    b = rd.BOUNDS[precision]
    if what == "obs":
        if precision == 32:
            np.testing.assert_allclose(got, want, atol=b["obs_atol"], rtol=0, err_msg=str(ctx))
        else:
            assert _rel(got, want).max() <= b["obs_rel"], (ctx, float(_rel(got, want).max()))
    else:
        np.testing.assert_allclose(got, want, err_msg=str(ctx), **b[what])
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float(np.nanmax(d)) if d.size else 0.0


# ------------------------------------------------------------------ A. the reset inside the step's launch
def _step_outputs(env, act):
    res = env.step(act, want_reward64=True)
    out = dict(obs=_np(res.obs), rew=_np(res.reward), rew64=_np(env.reward64), done=_np(res.done).astype(bool),
               trunc=_np(res.truncated).astype(bool), term_obs=_np(res.terminal_obs))
    out["phys"], out["aux"] = _state(env)
    return out


@pytest.mark.parametrize("case", rd.CASES_A, ids=rd.case_id)
def test_in_launch_autoreset_matches_control_philox_standalone_reset_and_oracle(case):
    env_id, precision, opts = case
    L = rd.Layout(env_id)
    n = rd.N
    kw = dict(seed=rd.SEED, env_offset=rd.OFF, precision=precision, **opts)
    env = VecEnv(env_id, n, autoreset=True, **kw)
    assert env.precision == precision and (env.info.state_words, env.info.aux_words) == (L.SD, L.AD)
    assert env.info.max_episode_steps == L.max_steps and env.info.reset_dofs == L.NR
    acts = sample_actions(env.info.action_dim, n, rd.WARMUP + 1, seed=rd.ACT_SEED, env_offset=rd.OFF)
    env.reset()
    for t in range(rd.WARMUP):
        env.step(acts[t])
    pre_phys, pre_aux, aux_c = rd.build_pre(env_id, *_state(env))
    _set(env, pre_phys, pre_aux)
    pre_phys, back = _state(env)  # the records as the handle holds them: its scalar type for the state and initial_z
    keep = [i for i in range(L.AD) if i != L.z0]
    np.testing.assert_array_equal(bits(back[:, keep]), bits(pre_aux[:, keep]))
    np.testing.assert_array_equal(back[:, L.z0], _scalar(pre_aux[:, L.z0], precision).astype(np.float64))
    pre_aux[:, L.z0] = aux_c[:, L.z0] = back[:, L.z0]
    Nn, T, D = rd.sets(n)
    pre_epi = pre_aux[:, L.episode].astype(np.uint32)
    gids = np.arange(rd.OFF, rd.OFF + n)

    got = _step_outputs(env, acts[rd.WARMUP])
    ctl_env = VecEnv(env_id, n, autoreset=False, **kw)
    _set(ctl_env, pre_phys, aux_c)
    ctl = _step_outputs(ctl_env, acts[rd.WARMUP])
    assert (ctl_env.info.lanes_per_env, ctl_env.info.block) == (env.info.lanes_per_env, env.info.block)

    # 1. flags: C's elapsed is 6, so whatever it reports done has terminated
    assert not ctl["trunc"].any()
    term = ctl["done"]
    reset = T | term
    np.testing.assert_array_equal(got["done"], reset)
    np.testing.assert_array_equal(got["trunc"], T & ~term)
    orc = oracle.OracleEnvs(env_id, n, seed=rd.SEED, env_offset=rd.OFF)
    orc.state[:], orc.aux[:] = pre_phys, aux_c
    _, _, done_o, _ = orc.step(_np(acts[rd.WARMUP]))
    counted = int((D & term & done_o).sum())
    if env_id in rd.TRUNCATION_ONLY:
        assert not term.any()
    else:
        assert counted >= rd.MIN_TERMINATED, counted
    assert (~reset).any() and (T & ~term).any()  # neither comparison below is empty
    r = np.flatnonzero(reset)

    # 2. discrete bookkeeping of every env that reset
    ga = got["aux"]
    assert (ga[r, L.elapsed] == 0).all() and (ga[r, L.floor] == 1).all()
    assert (ga[np.ix_(r, L.feet + L.frame + L.onground)] == 0).all()
    assert not L.feet or (pre_aux[np.ix_(np.flatnonzero(T), L.feet)] != 0).any(axis=1).all()  # there was a flag to clear
    np.testing.assert_array_equal(ga[r, L.episode], pre_epi[r].astype(np.float64) + 1)
    if L.harder:
        assert np.isnan(ga[r, L.crawl[0]]).all()

    # 3. the Philox draw of (seed, global id, the env's own episode index), in the handle's scalar type
    want_q = rd.expected_reset_q(env_id, precision, gids[r], pre_epi[r])
    np.testing.assert_array_equal(bits(_scalar(got["phys"][r][:, L.reset_q], precision)), bits(want_q))

    # the aux record the reset starts from: pre, with the draw counters the step itself may have advanced
    aux_ref = pre_aux.copy()
    aux_ref[:, L.carried] = ctl["aux"][:, L.carried]

    # 4. reference 1: the standalone reset of the same records
    alone = VecEnv(env_id, n, autoreset=False, **kw)
    _set(alone, pre_phys, aux_ref)
    alone.obs.fill_(float("nan"))
    mask = torch.from_numpy(reset.astype(np.uint8))
    obs1 = _np(alone.reset(mask=mask))
    phys1, aux1 = _state(alone)
    np.testing.assert_array_equal(bits(got["phys"][r]), bits(phys1[r]))
    np.testing.assert_array_equal(ga[np.ix_(r, L.discrete)], aux1[np.ix_(r, L.discrete)])
    ctx = rd.case_id(case)
    _within_reset_bounds(precision, "aux", ga[np.ix_(r, L.continuous)], aux1[np.ix_(r, L.continuous)], (ctx, "aux vs standalone"))
    _within_reset_bounds(precision, "obs", got["obs"][r], obs1[r].astype(np.float64), (ctx, "obs vs standalone"))
    not_bitwise = int((bits(ga[r]) != bits(aux1[r])).sum() + (bits(got["obs"][r]) != bits(obs1[r])).sum())

    # 5. reference 2: the float64 oracle's masked reset
    s2, a2, o2 = rd.oracle_reset_reference(env_id, pre_phys, aux_ref, reset)
    d_state = _within_reset_bounds(precision, "state", got["phys"][r], s2[r], (ctx, "state vs oracle"))
    d_aux = _within_reset_bounds(precision, "aux", ga[r], a2[r], (ctx, "aux vs oracle"))
    d_obs = _within_reset_bounds(precision, "obs", got["obs"][r], o2[r].astype(np.float64), (ctx, "obs vs oracle"))

    # 6. survivors: a reset in a neighbouring lane, quad or gang changes nothing
    s = np.flatnonzero(~reset)
    for k in ("phys", "aux", "obs", "rew", "rew64", "done"):
        np.testing.assert_array_equal(bits(got[k][s]), bits(ctl[k][s]), err_msg=f"{ctx}: survivors' {k}")

    # 7. what the step reports of the env that ended
    np.testing.assert_array_equal(bits(got["term_obs"][r]), bits(ctl["obs"][r]))
    np.testing.assert_array_equal(bits(got["rew"][r]), bits(ctl["rew"][r]))
    np.testing.assert_array_equal(bits(got["rew64"][r]), bits(ctl["rew64"][r]))

    b = rd.BOUNDS[precision]
    _report(dict(test=f"autoreset[{ctx}]", lanes_per_env=int(env.info.lanes_per_env), block=int(env.info.block),
                 reset_truncated=int((T & ~term).sum()), reset_terminated=int(term.sum()),
                 terminated_in_D_with_oracle=counted, survivors=int(len(s)),
                 oracle_state_max_abs=d_state, oracle_state_bound=b["state"],
                 oracle_aux_max_abs=d_aux, oracle_aux_bound=b["aux"],
                 oracle_obs_max_abs=d_obs, oracle_obs_bound=b.get("obs_atol", b.get("obs_rel")),
                 standalone_words_not_bitwise=not_bitwise,
                 standalone_words_compared=int(len(r) * (L.AD + env.info.obs_dim))))
    for e in (env, ctl_env, alone):
        e.close()


# ------------------------------------------------------------------ B. pbg_reset with a mask
MASKED = ["AntPyBulletEnv-v0", "HumanoidFlagrunHarderPyBulletEnv-v0", "InvertedPendulumSwingupPyBulletEnv-v0",
          "HopperMuJoCoEnv-v0"]
N_B = 97  # reset_kernel's blocks are 64 lanes: one full, one partial
SENTINEL = -12345.5


def _reset_from(env, phys0, aux0, **kw):
    _set(env, phys0, aux0)
    env.obs.fill_(SENTINEL)
    obs = _np(env.reset(**kw))
    return (obs,) + _state(env)


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("env_id", MASKED)
def test_masked_reset(env_id, precision):
    L = rd.Layout(env_id)
    n = N_B
    env = VecEnv(env_id, n, seed=rd.SEED, env_offset=rd.OFF, autoreset=False, precision=precision)
    acts = sample_actions(env.info.action_dim, n, rd.WARMUP, seed=rd.ACT_SEED, env_offset=rd.OFF)
    env.reset()
    for t in range(rd.WARMUP):
        env.step(acts[t])
    phys0, aux0 = _state(env)
    assert (aux0[:, L.elapsed] == rd.WARMUP).all() and (aux0[:, L.episode] == 1).all()
    e = np.arange(n)
    m = (e * 7) % 5 < 2
    m[[0, 63, 64, 96]] = [True, False, True, True]  # both sides of the block edge, the last env
    assert 0 < m.sum() < n

    # all ones == None
    full = _reset_from(env, phys0, aux0)
    ones = _reset_from(env, phys0, aux0, mask=torch.ones(n, dtype=torch.uint8))
    for a, b in zip(full, ones):
        np.testing.assert_array_equal(bits(a), bits(b))
    assert (full[2][:, L.elapsed] == 0).all() and (full[2][:, L.episode] == 2).all()

    # a mixed mask: unmasked rows untouched, masked rows as the full reset's
    obs, phys, aux = _reset_from(env, phys0, aux0, mask=torch.from_numpy(m.astype(np.uint8)))
    np.testing.assert_array_equal(bits(phys[~m]), bits(phys0[~m]))
    np.testing.assert_array_equal(bits(aux[~m]), bits(aux0[~m]))
    assert (obs[~m] == np.float32(SENTINEL)).all()
    np.testing.assert_array_equal(bits(phys[m]), bits(full[1][m]))
    np.testing.assert_array_equal(bits(aux[m]), bits(full[2][m]))
    np.testing.assert_array_equal(bits(obs[m]), bits(full[0][m]))
    np.testing.assert_array_equal(aux[:, L.episode], np.where(m, 2.0, 1.0))
    want_q = rd.expected_reset_q(env_id, precision, rd.OFF + e[m], 1)
    np.testing.assert_array_equal(bits(_scalar(phys[m][:, L.reset_q], precision)), bits(want_q))

    # a bool mask behaves like the uint8 one
    for a, b in zip(_reset_from(env, phys0, aux0, mask=torch.from_numpy(m)), (obs, phys, aux)):
        np.testing.assert_array_equal(bits(a), bits(b))

    # mask and init_q: masked env e takes row e of init_q; against the oracle's masked reset
    q = np.random.default_rng(5).uniform(-0.1, 0.1, (n, L.NR)).astype(np.float32)
    obs_q, phys_q, aux_q = _reset_from(env, phys0, aux0, mask=torch.from_numpy(m), init_q=torch.from_numpy(q))
    np.testing.assert_array_equal(bits(phys_q[~m]), bits(phys0[~m]))
    np.testing.assert_array_equal(bits(aux_q[~m]), bits(aux0[~m]))
    assert (obs_q[~m] == np.float32(SENTINEL)).all()
    if precision == 32:
        want = L.reset_offset.astype(np.float32)[None, :] + q[m]
    else:
        want = L.reset_offset[None, :] + q[m].astype(np.float64)
    np.testing.assert_array_equal(bits(_scalar(phys_q[m][:, L.reset_q], precision)), bits(want))
    s2, a2, o2 = rd.oracle_reset_reference(env_id, phys0, aux0, m, q=q)
    ctx = (env_id, precision, "masked init_q")
    _within_reset_bounds(precision, "state", phys_q[m], s2[m], ctx)
    _within_reset_bounds(precision, "aux", aux_q[m], a2[m], ctx)
    _within_reset_bounds(precision, "obs", obs_q[m], o2[m].astype(np.float64), ctx)
    env.close()


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("env_id", rd.ENVS)
def test_standalone_reset_matches_host_philox(env_id, precision):
    """test_gpu.test_rng_reset_matches_host_philox for every id and both precisions, at episode indices 0 and 1."""
    L = rd.Layout(env_id)
    n = N_B
    env = VecEnv(env_id, n, seed=rd.SEED, env_offset=rd.OFF, autoreset=False, precision=precision)
    gids = np.arange(rd.OFF, rd.OFF + n)
    for episode in (0, 1):
        env.reset()
        phys, aux = _state(env)
        want = rd.expected_reset_q(env_id, precision, gids, episode)
        np.testing.assert_array_equal(bits(_scalar(phys[:, L.reset_q], precision)), bits(want), err_msg=f"episode {episode}")
        assert (aux[:, L.episode] == episode + 1).all()
        rest = np.setdiff1d(np.concatenate([L.q, L.qd]), L.reset_q)
        assert (phys[:, rest] == 0).all()
    env.close()


# ------------------------------------------------------------------ C. lane workgroups of 32 and 64 lanes
LANE_CASES = [("InvertedPendulumPyBulletEnv-v0", 32, {}), ("InvertedPendulumPyBulletEnv-v0", 64, {}),
              ("InvertedDoublePendulumPyBulletEnv-v0", 32, {}), ("InvertedDoublePendulumPyBulletEnv-v0", 64, {}),
              ("HopperPyBulletEnv-v0", 32, {"kernel": 0}), ("HopperPyBulletEnv-v0", 64, {"kernel": 0}),
              ("HalfCheetahMuJoCoEnv-v0", 32, {"kernel": 0})]
LANE_STEPS, WINDOW = 30, 64


def _wide_n(width):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {32: 24, 64: 40}[width] * cus + 7


def _lane_run(env_id, precision, opts, n, off, acts, block, keep):
    """30 auto-reset steps; returns per step (obs, reward, done) of the env ranges in keep, and their final state."""
    env = VecEnv(env_id, n, seed=rd.SEED, env_offset=off, autoreset=True, precision=precision, **opts)
    assert env.info.lanes_per_env == 1 and env.info.block == block, (env.info.lanes_per_env, env.info.block, block)
    env.reset()
    trace = [[] for _ in keep]
    for t in range(LANE_STEPS):
        res = env.step(acts[t])
        for k, (a, b) in enumerate(keep):
            trace[k].append((_np(res.obs[a:b]), _np(res.reward[a:b]), _np(res.done[a:b])))
    phys, aux = _state(env)
    env.close()
    return trace, [(phys[a:b], aux[a:b]) for a, b in keep]


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("case", LANE_CASES, ids=rd.case_id)
def test_lane_kernel_wide_workgroups_bitwise_equal_width_16(case, width):
    env_id, precision, opts = case
    n = _wide_n(width)
    mid = n // 2 - (n // 2) % 64 + 37  # 37 past a 64-lane block's first env: aligned to no workgroup width
    assert (n - WINDOW) % 16 != 0 and WINDOW < mid < n - 2 * WINDOW
    windows = [(0, WINDOW), (mid, mid + WINDOW), (n - WINDOW, n)]
    na = rd.table(env_id)["NA"]
    acts = sample_actions(na, n, LANE_STEPS, seed=rd.ACT_SEED)
    big, big_state = _lane_run(env_id, precision, opts, n, 0, acts, width, windows)
    ended = 0
    for k, (a, b) in enumerate(windows):
        small, small_state = _lane_run(env_id, precision, opts, WINDOW, a, acts[:, a:b].contiguous(), 16, [(0, WINDOW)])
        for t in range(LANE_STEPS):
            for x, y, name in zip(big[k][t], small[0][t], ("obs", "reward", "done")):
                np.testing.assert_array_equal(bits(x), bits(y), err_msg=f"{name}, envs {a}..{b}, step {t}")
            ended += int(big[k][t][2].sum())
        np.testing.assert_array_equal(bits(big_state[k][0]), bits(small_state[0][0]), err_msg=f"state, envs {a}..{b}")
        np.testing.assert_array_equal(bits(big_state[k][1]), bits(small_state[0][1]), err_msg=f"aux, envs {a}..{b}")
    _report(dict(test=f"lane_width[{rd.case_id(case)},{width}]", n=n, block=width, window_starts=[w[0] for w in windows],
                 episodes_ended_in_windows=ended))


def test_lane_kernel_width_64_teacher_forced_against_oracle():
    n = _wide_n(64)
    for env_id, precision, opts in (("InvertedDoublePendulumPyBulletEnv-v0", 32, {}), ("HopperPyBulletEnv-v0", 64, {"kernel": 0})):
        env = VecEnv(env_id, n, precision=precision, **opts)
        assert env.info.lanes_per_env == 1 and env.info.block == 64, (env.info.lanes_per_env, env.info.block)
        env.close()
    _teacher_forced("InvertedDoublePendulumPyBulletEnv-v0", n, 20, sample=128)
    _teacher_forced64("HopperPyBulletEnv-v0", n, 20, sample=128, kernel=0)
