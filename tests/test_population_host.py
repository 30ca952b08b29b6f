"""Policy populations, the parts that need no GPU (include/pbg.h pbg_population_*): the evolution-strategy
noise on the host (pbg_population_noise_host against rng.es_noise, both float64 rounded once), its
counter structure (global pair index, generation, seed, block of four parameters), its moments, the flat
parameter layout and the argument checks that come before any HIP call."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native, rng
from pybulletgym_amd.policy import MLPPolicy, pack_theta, param_count, unpack_theta

import policy_data as pd

SMALL = ((3, 5, 7, 2), (2, 5, 7, 3), (7, 33, 17, 3))  # D = 78 (D % 4 = 2), 81 (D % 4 = 1), 896
SEED = 0x1234_5678_9ABC_DEF0  # both key words in use


def host_noise(dims, seed, generation, pair0, n_pairs):
    out = np.full((n_pairs, param_count(dims)), np.nan, np.float32)
    _native.check(_native.lib().pbg_population_noise_host(*dims, seed, generation, pair0, n_pairs, out.ctypes.data),
                  "pbg_population_noise_host")
    return out


def test_param_counts():
    assert [param_count(d) for d in SMALL] == [78, 81, 896]
    assert param_count((28, 128, 64, 8)) == 12488 and rng.es_param_count((28, 128, 64, 8)) == 12488


@pytest.mark.parametrize("dims", SMALL, ids=str)
def test_host_noise_agrees_with_the_numpy_mirror(dims):
    """Both compute the contract in float64 and round once; libm's and numpy's log / cos / sin may differ in
    the last place of the double, far below the 1e-5 the device is held to."""
    for pair0, gen in ((0, 0), (5, 3)):
        a = host_noise(dims, SEED, gen, pair0, 6)
        b = rng.es_noise(dims, SEED, gen, pair0, 6)
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (6, param_count(dims))
        assert np.isfinite(a).all() and np.isfinite(b).all()
        err = np.abs(a.astype(np.float64) - b).max()
        print(f"{dims} pair0 {pair0} generation {gen}: max |C host - numpy| = {err:.3e}")
        assert err <= 1e-5


@pytest.mark.parametrize("noise", [host_noise, rng.es_noise], ids=["c", "numpy"])
def test_prefix_property(noise):
    """The noise of a pair depends on its global index only: pairs 4..7 of an 8-pair call are a 4-pair call
    with pair0 = 4.  And on the block of four parameters only, not on D: the 78 parameters of the D = 78
    shape (whose last block is cut after 2) are the first 78 of a longer vector's."""
    dims = SMALL[2]
    whole = noise(dims, SEED, 7, 0, 8)
    part = noise(dims, SEED, 7, 4, 4)
    assert np.array_equal(whole[4:], part)
    assert not np.array_equal(whole[:4], part)
    short = noise(SMALL[0], SEED, 7, 0, 8)
    assert short.shape == (8, 78)
    assert np.array_equal(short, whole[:, :78])
    assert np.array_equal(noise(SMALL[1], SEED, 7, 0, 8), whole[:, :81])


@pytest.mark.parametrize("noise", [host_noise, rng.es_noise], ids=["c", "numpy"])
def test_seed_and_generation(noise):
    dims = SMALL[0]
    base = noise(dims, SEED, 2, 0, 8)
    assert np.array_equal(base, noise(dims, SEED, 2, 0, 8))
    for other in (noise(dims, SEED, 3, 0, 8), noise(dims, SEED + 1, 2, 0, 8), noise(dims, SEED + (1 << 32), 2, 0, 8)):
        assert (other != base).any(axis=1).all()  # every pair's row changes
        assert (other != base).mean() > 0.99
    # the rows of one call differ from one another too
    assert len({r.tobytes() for r in base}) == 8


@pytest.mark.parametrize("noise", [host_noise, rng.es_noise], ids=["c", "numpy"])
def test_moments(noise):
    """64 pairs x D = 896 standard normals: sampling bounds at five standard errors (the mean's standard
    error is 1 / sqrt(N), the variance's sqrt(2 / N)), and the contract's hard limit |eps| <= sqrt(48 ln 2)."""
    e = noise(SMALL[2], SEED, 0, 0, 64).astype(np.float64)
    n = e.size
    assert n == 64 * 896
    print(f"mean {e.mean():+.5f} var {e.var():.5f} max |eps| {np.abs(e).max():.3f}")
    assert abs(e.mean()) <= 5.0 / np.sqrt(n)
    assert abs(e.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert np.abs(e).max() <= 5.77


@pytest.mark.parametrize("dims", SMALL + ((28, 128, 64, 8),), ids=str)
def test_flat_layout_round_trip(dims):
    """theta is w1, b1, w2, b2, w3, b3 concatenated, row-major and unpadded."""
    ws = pd.synthetic_weights(dims)
    theta = pack_theta(ws)
    assert theta.dtype == np.float32 and theta.shape == (param_count(dims),)
    o, h1, h2, a = dims
    assert theta[0] == ws[0][0, 0] and theta[h1 + 1] == ws[0][1, 1]          # w1 row-major
    assert theta[o * h1] == ws[1][0] and theta[o * h1 + h1] == ws[2][0, 0]    # then b1, then w2
    assert theta[-1] == ws[5][-1] and theta[-a - 1] == ws[4][-1, -1]          # ... w3, b3 last
    back = unpack_theta(dims, theta)
    assert all(np.array_equal(x, y) and x.shape == y.shape for x, y in zip(back, ws))
    # the six arrays are what MLPPolicy takes
    obs = pd.seeded_obs(o, 8)
    p, q = MLPPolicy(*ws), MLPPolicy(*back)
    assert np.array_equal(p.act(obs), q.act(obs))
    p.close()
    q.close()
    with pytest.raises(_native.PbgError):
        unpack_theta(dims, theta[:-1])


BAD_DIMS = [(0, 5, 7, 2), (257, 5, 7, 2), (3, 0, 7, 2), (3, 257, 7, 2), (3, 5, 0, 2), (3, 5, 257, 2), (3, 5, 7, 0),
            (3, 5, 7, 65), (-1, 5, 7, 2)]


def test_population_create_argument_errors():
    """PBG_E_ARG before any HIP call (this test runs without a GPU), *out NULL after every failure."""
    L = _native.lib()

    def create(dims, n_pairs, pair0, device=0):
        h = ctypes.c_void_p(0x1234)  # a stale value: every failure must leave NULL
        rc = L.pbg_population_create(device, *dims, n_pairs, pair0, ctypes.byref(h))
        return rc, h.value

    good = (3, 5, 7, 2)
    for dims in BAD_DIMS:
        assert create(dims, 4, 0) == (-1, None), dims
        assert b"dims" in L.pbg_last_error()
    for n_pairs, pair0 in ((0, 0), (-1, 0), (4, -1), (2 ** 30, 0), (4, 2 ** 31 - 2)):
        assert create(good, n_pairs, pair0) == (-1, None), (n_pairs, pair0)
    assert create(good, 4, 0, device=-1) == (-1, None)  # the members live on a GPU: no host-only population
    assert L.pbg_population_create(0, *good, 4, 0, None) == -1
    # the limits themselves are dims errors for no field
    rc, h = create((256, 256, 256, 64), 1, 0, device=10 ** 6)
    assert rc == -3 and h is None  # PBG_E_HIP: no such device, past the argument checks


def test_noise_host_argument_errors():
    L = _native.lib()
    buf = np.zeros((4, 78), np.float32)
    for dims in BAD_DIMS:
        assert L.pbg_population_noise_host(*dims, 0, 0, 0, 4, buf.ctypes.data) == -1, dims
    good = (3, 5, 7, 2)
    for pair0, n_pairs in ((0, 0), (0, -1), (-1, 4)):
        assert L.pbg_population_noise_host(*good, 0, 0, pair0, n_pairs, buf.ctypes.data) == -1
    assert L.pbg_population_noise_host(*good, 0, 0, 0, 4, None) == -1
    assert not buf.any()
    assert L.pbg_population_noise_host(*good, 0, 0, 0, 4, buf.ctypes.data) == 0 and buf.all()


def test_symbols_are_exported_and_bound():
    assert set(_native.POPULATION_EXPORTED) <= set(_native.EXPORTED)
    for f in _native.POPULATION_EXPORTED:
        assert hasattr(_native.lib(), f), f
