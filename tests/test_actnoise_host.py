"""Gaussian action noise, the parts that need no GPU (include/pbg.h "Stochastic Gaussian actions"):
pbg_action_noise_host against rng.action_noise (both float64 rounded once), the counter structure (global env
index, step count, seed, block of four components, the 0xAC tag that keeps the stream apart from the
evolution strategy's), the moments, and the argument checks that come before any HIP call."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native, rng

ACT_DIMS = (1, 3, 4, 8, 17, 64)  # both edges of a Philox block: 4 b - 1, 4 b, 4 b + 1
SEED = 0x1234_5678_9ABC_DEF0     # both key words in use


def host_noise(act_dim, seed, n, env_offset, step):
    out = np.full((n, act_dim), np.nan, np.float32)
    _native.check(_native.lib().pbg_action_noise_host(act_dim, seed, n, env_offset, step, out.ctypes.data),
                  "pbg_action_noise_host")
    return out


@pytest.mark.parametrize("act_dim", ACT_DIMS)
def test_host_noise_equals_the_numpy_mirror(act_dim):
    for env_offset, step in ((0, 0), (16, 3), (5, 2 ** 32 - 1)):
        a = host_noise(act_dim, SEED, 33, env_offset, step)
        b = rng.action_noise(act_dim, SEED, 33, env_offset, step)
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (33, act_dim)
        assert np.isfinite(a).all()
        print(f"act_dim {act_dim} env_offset {env_offset} step {step}: max |C host - numpy| = "
              f"{np.abs(a.astype(np.float64) - b).max():.3e}")
        assert np.array_equal(a, b)


@pytest.mark.parametrize("noise", [host_noise, rng.action_noise], ids=["c", "numpy"])
def test_prefix_and_shard_properties(noise):
    """The noise of an env depends on its global index only: rows 16..31 of a 32-env call are a 16-env call
    at env_offset 16.  And on the block of four components only, not on act_dim: act_dim 3 is a prefix of
    act_dim 8, row by row."""
    whole = noise(8, SEED, 32, 0, 7)
    part = noise(8, SEED, 16, 16, 7)
    assert np.array_equal(whole[16:], part)
    assert not np.array_equal(whole[:16], part)
    assert np.array_equal(noise(3, SEED, 32, 0, 7), whole[:, :3])
    assert np.array_equal(noise(17, SEED, 32, 0, 7)[:, :8], whole)


@pytest.mark.parametrize("noise", [host_noise, rng.action_noise], ids=["c", "numpy"])
def test_seed_and_step(noise):
    base = noise(8, SEED, 16, 0, 2)
    assert np.array_equal(base, noise(8, SEED, 16, 0, 2))
    for other in (noise(8, SEED, 16, 0, 3), noise(8, SEED + 1, 16, 0, 2), noise(8, SEED + (1 << 32), 16, 0, 2)):
        assert (other != base).any(axis=1).all()  # every env's row changes
        assert (other != base).mean() > 0.99
    assert len({r.tobytes() for r in base}) == 16


def test_the_tag_keeps_the_stream_apart_from_the_es_noise():
    """es_noise's counter is (block, pair0 + i, generation, 0xE5): at the same first three words and key the
    action noise (tag 0xAC) shares no value with it."""
    dims = (1, 1, 1, 4)  # D = 1 + 1 + 1 + 1 + 4 + 4 = 12: three blocks
    es = rng.es_noise(dims, SEED, 5, 3, 8)
    an = rng.action_noise(12, SEED, 8, 3, 5)
    assert es.shape == an.shape == (8, 12)
    assert (es != an).all()
    assert np.array_equal(host_noise(12, SEED, 8, 3, 5), an)


@pytest.mark.parametrize("noise", [host_noise, rng.action_noise], ids=["c", "numpy"])
def test_moments(noise):
    """896 envs x 64 components standard normals (the sample size of the population noise's test): sampling
    bounds at five standard errors (the mean's standard error is 1 / sqrt(N), the variance's sqrt(2 / N)), and
    the contract's hard limit |eps| <= sqrt(48 ln 2)."""
    e = noise(64, SEED, 896, 0, 0).astype(np.float64)
    n = e.size
    assert n == 64 * 896
    print(f"mean {e.mean():+.5f} var {e.var():.5f} max |eps| {np.abs(e).max():.3f}")
    assert abs(e.mean()) <= 5.0 / np.sqrt(n)
    assert abs(e.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert np.abs(e).max() <= 5.77


def test_argument_errors_before_any_hip_call():
    """PBG_E_ARG without a device (this test runs without a GPU); *out NULL after every failure."""
    L = _native.lib()
    buf = np.zeros((4, 8), np.float32)
    for act_dim in (0, -1, 65):
        assert L.pbg_action_noise_host(act_dim, 0, 4, 0, 0, buf.ctypes.data) == -1, act_dim
    for n, env_offset in ((-1, 0), (4, -1), (4, 2 ** 31 - 2)):
        assert L.pbg_action_noise_host(8, 0, n, env_offset, 0, buf.ctypes.data) == -1, (n, env_offset)
    assert L.pbg_action_noise_host(8, 0, 4, 0, 0, None) == -1
    assert not buf.any()
    assert L.pbg_action_noise_host(8, 0, 0, 0, 0, None) == 0  # nothing to write
    assert L.pbg_action_noise_host(8, 0, 4, 0, 0, buf.ctypes.data) == 0 and buf.all()

    def create(device, act_dim):
        h = ctypes.c_void_p(0x1234)  # a stale value: every failure must leave NULL
        return L.pbg_action_noise_create(device, act_dim, 0, ctypes.byref(h)), h.value

    for device, act_dim in ((0, 0), (0, 65), (0, -3), (-1, 8)):
        assert create(device, act_dim) == (-1, None), (device, act_dim)
        assert b"pbg_action_noise_create" in L.pbg_last_error()
    assert L.pbg_action_noise_create(0, 8, 0, None) == -1
    assert create(10 ** 6, 64) == (-3, None)  # PBG_E_HIP: no such device, past the argument checks
    # a NULL object is refused by every entry point that takes one
    assert L.pbg_action_noise_set_std(None, buf.ctypes.data, None) == -1
    assert L.pbg_action_noise_set_counter(None, 0, None) == -1
    assert L.pbg_action_noise_get_counter(None, buf.ctypes.data, None) == -1
    assert L.pbg_action_noise_set_eps2_traj(None, None) == -1
    assert L.pbg_action_noise_fill(None, 4, 0, 0, buf.ctypes.data, None) == -1
    assert L.pbg_policy_attach_action_noise(None, None) == -1
    assert L.pbg_population_attach_action_noise(None, None) == -1
    L.pbg_action_noise_destroy(None)


def test_symbols_are_exported_and_bound():
    assert set(_native.ACTION_NOISE_EXPORTED) <= set(_native.EXPORTED)
    for f in _native.ACTION_NOISE_EXPORTED:
        assert hasattr(_native.lib(), f), f
