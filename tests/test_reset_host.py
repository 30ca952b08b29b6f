"""The references of the reset tests, checked on the CPU before they judge a kernel (tests/test_autoreset_gpu.py):
the float64 oracle's masked reset, the host Philox reset noise, and the pre-state recipe of the in-launch
auto-reset comparison (tests/reset_data.py).  Runs anywhere."""
import numpy as np
import pytest

import oracle
import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import rng

import reset_data as rd

MASKED = ["AntPyBulletEnv-v0", "HumanoidFlagrunHarderPyBulletEnv-v0", "InvertedPendulumSwingupPyBulletEnv-v0",
          "HopperMuJoCoEnv-v0", "HumanoidFlagrunPyBulletEnv-v0", "InvertedDoublePendulumPyBulletEnv-v0"]


def _oracle_at(env_id, state, aux):
    """A fresh oracle holding (state, aux).  The oracle's Philox key is process-wide (pbg_oracle_set_rng),
    set by the constructor: build the oracle that draws right before it draws."""
    o = oracle.OracleEnvs(env_id, len(state), seed=rd.SEED, env_offset=rd.OFF)
    o.state[:] = state
    o.aux[:] = aux
    return o


def test_layout_matches_oracle_record_sizes():
    for env_id in rd.ENVS:
        L, info = rd.Layout(env_id), oracle.Info(oracle.robot_id(env_id))
        assert (L.SD, L.AD, L.NR, L.NF, L.NJ) == (info.SD, info.AD, info.NR, info.NF, info.NJ), env_id
        assert sorted(L.continuous + L.discrete) == list(range(L.AD))


@pytest.mark.parametrize("env_id", MASKED)
def test_oracle_masked_reset_touches_masked_rows_only(env_id):
    """Unmasked rows of state, aux and obs keep their bits; masked rows equal an unmasked reset's in
    everything that does not depend on the aux record the reset starts from; the episode word and
    Flagrun's draw counter advance by one where masked and nowhere else."""
    n = 23
    L = rd.Layout(env_id)
    w = rd.oracle_warmup(env_id, n)
    s0, a0 = w.state.copy(), w.aux.copy()
    a0[:, L.episode] = 1 + np.arange(n) % 4
    mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    m = mask.astype(bool)
    q = rng.reset_noise(rd.SEED, np.arange(rd.OFF, rd.OFF + n), a0[:, L.episode].astype(np.uint32), L.NR).astype(np.float64)

    o = _oracle_at(env_id, s0, a0)
    obs = np.full((n, o.info.OBS), np.float32(7.5))
    o.reset(q, mask=mask, obs=obs)
    np.testing.assert_array_equal(rd.bits(o.state[~m]), rd.bits(s0[~m]))
    np.testing.assert_array_equal(rd.bits(o.aux[~m]), rd.bits(a0[~m]))
    assert (obs[~m] == np.float32(7.5)).all() and not (obs[m] == np.float32(7.5)).all(axis=1).any()
    np.testing.assert_array_equal(o.aux[m, L.episode], a0[m, L.episode] + 1)
    for c in L.flag_count:
        adv = o.aux[:, c] - a0[:, c]
        assert (adv[~m] == 0).all() and (adv[m] >= 1).all()  # the reset's draw (and a re-draw within 1 m of the flag)
    assert (o.aux[m, L.elapsed] == 0).all() and (o.aux[m, L.floor] == 1).all()
    for f in L.feet + L.frame + L.onground:
        assert (o.aux[m, f] == 0).all()

    full = _oracle_at(env_id, s0, a0)
    obs_f = full.reset(q)
    np.testing.assert_array_equal(rd.bits(o.state[m]), rd.bits(full.state[m]))
    np.testing.assert_array_equal(rd.bits(obs[m]), rd.bits(obs_f[m]))
    np.testing.assert_array_equal(rd.bits(o.aux[m]), rd.bits(full.aux[m]))
    # and the reset dofs are offset + noise, everything else of the joint state zero
    np.testing.assert_array_equal(o.state[m][:, L.reset_q], L.reset_offset[None, :] + q[m])
    rest = np.setdiff1d(np.concatenate([L.q, L.qd]), L.reset_q)
    assert (o.state[m][:, rest] == 0).all()


def test_oracle_reset_ignores_the_state_it_overwrites():
    """Masked rows do not depend on the physical state, potential, initial_z, elapsed or feet words before."""
    env_id, n = "HumanoidFlagrunHarderPyBulletEnv-v0", 12
    L = rd.Layout(env_id)
    w = rd.oracle_warmup(env_id, n)
    q = rng.reset_noise(rd.SEED, np.arange(rd.OFF, rd.OFF + n), 0, L.NR).astype(np.float64)
    a = _oracle_at(env_id, w.state, w.aux)
    obs_a = a.reset(q)
    s2, x2 = np.random.default_rng(1).normal(size=w.state.shape), w.aux.copy()
    for c in [L.pot, L.z0, L.elapsed] + L.feet + L.flag_target + L.flag_timeout + L.frame + L.onground + L.crawl:
        x2[:, c] = 3.0
    b = _oracle_at(env_id, s2, x2)
    obs_b = b.reset(q)
    np.testing.assert_array_equal(rd.bits(a.state), rd.bits(b.state))
    np.testing.assert_array_equal(rd.bits(a.aux), rd.bits(b.aux))
    np.testing.assert_array_equal(rd.bits(obs_a), rd.bits(obs_b))


def test_reset_noise_depends_on_seed_global_id_and_episode_alone():
    gid = np.array([1000, 1001, 5, 1000, 77], dtype=np.int64)
    epi = np.array([1, 2, 3, 1, 0], dtype=np.uint32)
    a = rng.reset_noise(rd.SEED, gid, epi, 17)
    np.testing.assert_array_equal(a[0], a[3])  # same (id, episode): same row, wherever it stands
    for i in range(len(gid)):  # a row alone, or inside another batch, or as a prefix of a wider draw
        np.testing.assert_array_equal(rng.reset_noise(rd.SEED, gid[i:i + 1], epi[i:i + 1], 17)[0], a[i])
        np.testing.assert_array_equal(rng.reset_noise(rd.SEED, gid[i:i + 1], int(epi[i]), 30)[0, :17], a[i])
    rows = {a[i].tobytes() for i in (0, 1, 2, 4)}
    assert len(rows) == 4
    assert not np.array_equal(rng.reset_noise(rd.SEED + 1, gid, epi, 17), a)
    assert not np.array_equal(rng.reset_noise(rd.SEED, gid, epi + 1, 17), a)  # a wrong episode index shows
    assert not np.array_equal(rng.reset_noise(rd.SEED, gid + 1, epi, 17), a)
    assert a.min() >= -0.1 and a.max() < 0.1


def test_expected_reset_q_rounds_once_per_scalar_type():
    env_id = "InvertedPendulumSwingupPyBulletEnv-v0"
    gid, epi = np.arange(rd.OFF, rd.OFF + 8), np.arange(8) % 4
    noise = rng.reset_noise(rd.SEED, gid, epi, 1)
    q32, q64 = rd.expected_reset_q(env_id, 32, gid, epi), rd.expected_reset_q(env_id, 64, gid, epi)
    assert q32.dtype == np.float32 and q64.dtype == np.float64
    np.testing.assert_array_equal(q32, np.float32(3.1415) + noise)
    np.testing.assert_array_equal(q64, 3.1415 + noise.astype(np.float64))
    assert not np.array_equal(q32.astype(np.float64), q64)


@pytest.mark.parametrize("env_id", rd.ENVS)
def test_pre_state_recipe_terminates_on_the_oracle(env_id):
    """The part-A pre-state on the float64 oracle alone: the step after it terminates at least MIN_TERMINATED
    of the D envs of every id that has a termination rule, none where there is none, and the T envs reach
    the time limit without terminating more often than their neighbours."""
    L = rd.Layout(env_id)
    w = rd.oracle_warmup(env_id)
    phys, aux, aux_c = rd.build_pre(env_id, w.state, w.aux)
    Nn, T, D = rd.sets()
    e = np.arange(rd.N)
    np.testing.assert_array_equal(aux[:, L.episode], 1 + e % 4)
    assert (aux[T, L.elapsed] == L.max_steps - 1).all() and (aux_c[:, L.elapsed] == rd.WARMUP).all()
    np.testing.assert_array_equal(rd.bits(phys[~D]), rd.bits(w.state[~D]))
    o = _oracle_at(env_id, phys, aux_c)
    _, _, done, _ = o.step(rd.host_actions(env_id, rd.N, 1, step0=rd.WARMUP)[0])
    assert np.isfinite(o.state).all()
    if env_id in rd.TRUNCATION_ONLY:
        assert not done.any()
    else:
        assert int(done[D].sum()) >= rd.MIN_TERMINATED, (env_id, int(done[D].sum()))
    # deterministic: the recipe gives the same records again
    phys2, aux2, _ = rd.build_pre(env_id, w.state, w.aux)
    np.testing.assert_array_equal(rd.bits(phys), rd.bits(phys2))
    np.testing.assert_array_equal(rd.bits(aux), rd.bits(aux2))


def test_case_table_reaches_every_reset_path():
    ids = [rd.case_id(c) for c in rd.CASES_A]
    assert len(set(ids)) == len(ids) == 2 * len(rd.ENVS) + 16
    assert {e for e, _, _ in rd.CASES_A} == set(rd.ENVS)
    for e in rd.ENVS:
        assert {p for x, p, o in rd.CASES_A if x == e and not o} == {32, 64}
