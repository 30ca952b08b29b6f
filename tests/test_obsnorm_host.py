"""Observation normalisation on the host (include/pbg.h "Running observation normalisation"; no GPU): the
host policy with a normaliser against numpy, NaN and inf rows, off = never set, the npz round trip and the
argument errors of the create / set entry points that need no device.

The transform is  v = (x - mean) * inv_std;  v < -clip ? -clip : (v > clip ? clip : v)  with one float32
rounding per operation: numpy's float32 subtraction and multiplication are those two roundings, so the
expectations below are exact and compared with array_equal.  The device actors are compared bit for bit
against this host path in test_obsnorm_gpu.py."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.policy import MLPPolicy, NPZ_KEYS

import policy_data as pd

DIMS = ((5, 16, 8, 1), (28, 128, 64, 8), (256, 256, 256, 64))


def make_norm(obs_dim, seed=0):
    """A seeded normaliser: means of order one, inv_std spanning 0.1 .. 10 (the variance floor's bound)."""
    rng = np.random.default_rng([11, seed, obs_dim])
    mean = rng.standard_normal(obs_dim).astype(np.float32)
    inv_std = (10.0 ** rng.uniform(-1.0, 1.0, obs_dim)).astype(np.float32)
    return mean, inv_std


def chain(obs, mean, inv_std, c):
    """The transform with the comparison chain spelled out (what the library computes, NaN and inf included)."""
    with np.errstate(invalid="ignore"):
        v = (obs - mean) * inv_std
        assert v.dtype == np.float32
        return np.where(v < -c, np.float32(-c), np.where(v > c, np.float32(c), v)).astype(np.float32)


@pytest.mark.parametrize("dims", DIMS, ids=str)
def test_host_normaliser_equals_numpy(dims):
    ws = pd.synthetic_weights(dims)
    obs = (3.0 * pd.seeded_obs(dims[0], 200, seed=4)).astype(np.float32)  # up to +-15: both clamps are taken
    mean, inv_std = make_norm(dims[0])
    plain = MLPPolicy(*ws)
    for c in (5.0, 0.75):
        pi = MLPPolicy(*ws, obs_norm=(mean, inv_std, c))
        xn = np.clip((obs - mean) * inv_std, np.float32(-c), np.float32(c))
        assert xn.dtype == np.float32 and (xn == c).any() and (xn == -c).any() and (np.abs(xn) < c).any()
        assert np.array_equal(xn, chain(obs, mean, inv_std, c))
        want = plain.act(xn)
        got = pi.act(obs)
        assert got.dtype == np.float32 and np.array_equal(got, want), (dims, c)
        assert not np.array_equal(got, plain.act(obs))
        assert np.array_equal(pi.obs_norm[0], mean) and np.array_equal(pi.obs_norm[1], inv_std) and pi.obs_norm[2] == c
        pi.close()
    plain.close()


def test_nan_and_inf_rows():
    dims = (28, 128, 64, 8)
    ws = pd.synthetic_weights(dims)
    obs = pd.seeded_obs(dims[0], 9, seed=5)
    mean, inv_std = make_norm(dims[0])
    inv_std[3] = 0.0  # inf * 0 = NaN: the one place an inf component does not clamp
    clean = obs.copy()
    obs[2, 7] = np.nan
    obs[4, 1], obs[4, 2], obs[4, 3] = np.inf, -np.inf, np.inf
    obs[6, :] = np.inf
    pi = MLPPolicy(*ws, obs_norm=(mean, inv_std, 5.0))
    plain = MLPPolicy(*ws)
    got = pi.act(obs)
    # NaN: passes through like np.clip and poisons its own row only
    with np.errstate(invalid="ignore"):
        nan_want = plain.act(np.clip((obs[2:3] - mean) * inv_std, np.float32(-5.0), np.float32(5.0)))
    assert np.isnan(nan_want).all() and np.isnan(got[2]).all()
    # inf: the comparison chain spelled out
    xn = chain(obs, mean, inv_std, 5.0)
    assert xn[4, 1] == 5.0 and xn[4, 2] == -5.0 and np.isnan(xn[4, 3])
    assert (xn[6, np.arange(28) != 3] == 5.0).all() and np.isnan(xn[6, 3])
    assert np.array_equal(got, plain.act(xn), equal_nan=True)
    assert np.isnan(got[4]).all() and np.isnan(got[6]).all()
    # the neighbours are what they are without the bad rows
    ok = [0, 1, 3, 5, 7, 8]
    assert np.isfinite(got[ok]).all() and np.array_equal(got[ok], pi.act(clean)[ok])
    pi.close()
    plain.close()


@pytest.mark.parametrize("dims", DIMS[:2], ids=str)
def test_off_equals_never_set(dims):
    ws = pd.synthetic_weights(dims)
    obs = pd.seeded_obs(dims[0], 64, seed=6)
    never = MLPPolicy(*ws)
    want = never.act(obs)
    assert never.obs_norm is None
    toggled = MLPPolicy(*ws, obs_norm=(*make_norm(dims[0]), 5.0))
    assert not np.array_equal(toggled.act(obs), want)
    toggled.set_obs_norm(None)
    assert toggled.obs_norm is None
    assert np.array_equal(toggled.act(obs), want)
    toggled.set_obs_norm(*make_norm(dims[0], seed=1), clip=2.0)   # and on again, with another one
    again = MLPPolicy(*ws, obs_norm=(*make_norm(dims[0], seed=1), 2.0))
    assert np.array_equal(toggled.act(obs), again.act(obs))
    for p in (never, toggled, again):
        p.close()


def test_npz_round_trip(tmp_path):
    dims = (28, 128, 64, 8)
    ws = pd.synthetic_weights(dims)
    obs = pd.seeded_obs(dims[0], 32, seed=7)
    mean, inv_std = make_norm(dims[0])
    with_keys, without = str(tmp_path / "with.npz"), str(tmp_path / "without.npz")
    np.savez(without, **dict(zip(NPZ_KEYS, ws)))
    np.savez(with_keys, **dict(zip(NPZ_KEYS, ws)), obs_mean=mean, obs_inv_std=inv_std, obs_clip=np.float32(2.5))
    a = MLPPolicy.from_npz(without)
    b = MLPPolicy.from_npz(with_keys)
    assert a.obs_norm is None
    assert np.array_equal(b.obs_norm[0], mean) and np.array_equal(b.obs_norm[1], inv_std) and b.obs_norm[2] == 2.5
    plain, normed = MLPPolicy(*ws), MLPPolicy(*ws, obs_norm=(mean, inv_std, 2.5))
    assert np.array_equal(a.act(obs), plain.act(obs))
    assert np.array_equal(b.act(obs), normed.act(obs))
    assert not np.array_equal(a.act(obs), b.act(obs))
    # an existing fixture has no such keys and loads as before
    import os
    fx = MLPPolicy.from_npz(os.path.join(pd.GOLDEN, pd.FIXTURES[0]))
    assert fx.obs_norm is None
    for p in (a, b, plain, normed, fx):
        p.close()


def test_argument_errors_without_a_device():
    L = _native.lib()
    # pbg_obs_stats_create: refused before any HIP call, *out NULL afterwards
    for device, obs_dim, n_slots in ((0, 0, 4), (0, 257, 4), (0, -1, 4), (0, 28, 0), (0, 28, -3), (-1, 28, 4),
                                     (-2, 28, 4)):
        h = ctypes.c_void_p(0x1234)
        assert L.pbg_obs_stats_create(device, obs_dim, n_slots, ctypes.byref(h)) == -1, (device, obs_dim, n_slots)
        assert not h.value
        assert b"pbg_obs_stats_create" in L.pbg_last_error()
    assert L.pbg_obs_stats_create(0, 28, 4, None) == -1
    L.pbg_obs_stats_destroy(None)
    # pbg_policy_set_obs_norm on a host-only policy
    dims = (5, 16, 8, 1)
    pi = MLPPolicy(*pd.synthetic_weights(dims))
    mean, inv_std = make_norm(5)
    m, s = mean.ctypes.data, inv_std.ctypes.data
    for clip in (0.0, -1.0, float("nan")):
        assert L.pbg_policy_set_obs_norm(pi._h, m, s, clip) == -1, clip
        assert b"clip" in L.pbg_last_error()
    assert L.pbg_policy_set_obs_norm(pi._h, m, None, 5.0) == -1
    assert L.pbg_policy_set_obs_norm(pi._h, None, s, 5.0) == -1
    assert L.pbg_policy_set_obs_norm(None, m, s, 5.0) == -1
    assert pi.obs_norm is None
    obs = pd.seeded_obs(5, 8)
    want = pi.act(obs)
    assert L.pbg_policy_set_obs_norm(pi._h, m, s, 5.0) == 0       # a refused call left nothing behind
    assert L.pbg_policy_set_obs_norm(pi._h, None, None, 0.0) == 0  # off: clip is not looked at
    assert np.array_equal(pi.act(obs), want)
    for bad in ((mean[:-1], inv_std[:-1]), (mean, inv_std[:-1]), (mean.reshape(1, 5), inv_std.reshape(1, 5))):
        with pytest.raises(_native.PbgError):
            pi.set_obs_norm(*bad)
    with pytest.raises(_native.PbgError):
        pi.set_obs_norm(mean, inv_std, clip=0.0)
    with pytest.raises(_native.PbgError):
        MLPPolicy(*pd.synthetic_weights(dims), obs_norm=(mean, inv_std, -5.0))
    # the attach entry points and the population setter refuse a NULL actor
    assert L.pbg_policy_attach_obs_stats(None, None) == -1
    assert L.pbg_population_attach_obs_stats(None, None) == -1
    assert L.pbg_population_set_obs_norm(None, None, None, 5.0, None) == -1
    assert L.pbg_policy_attach_obs_stats(pi._h, None) == 0
    pi.close()
    with pytest.raises(_native.PbgError):
        pi.set_obs_norm(mean, inv_std)
