"""Generalised advantage estimation on the host (include/pbg.h pbg_gae_host; no GPU): the float64 scan against
a numpy restatement of the stated order, bit for bit, the lambda = 1 identity with the discounted return, and
the argument checks that come before any HIP call."""
import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import gae

import gae_data as gd


@pytest.mark.parametrize("lam", [0.95, 0.0, 1.0])
@pytest.mark.parametrize("n", gd.NS)
@pytest.mark.parametrize("T", gd.TS)
def test_gae_host_equals_the_numpy_restatement(T, n, lam):
    rew, done, value = gd.case(T, n)
    assert done[T - 1].any() and done[0].any()
    want_adv, want_ret = gd.gae_numpy(rew, done, value, 0.99, lam)
    adv, ret = gae(rew, done, value, 0.99, lam)
    assert adv.dtype == ret.dtype == np.float32 and adv.shape == ret.shape == (T, n)
    assert np.array_equal(adv, want_adv) and np.array_equal(ret, want_ret)
    out_a, out_r = np.full((T, n), np.nan, np.float32), np.full((T, n), np.nan, np.float32)
    got = gae(rew, done, value, 0.99, lam, adv=out_a, ret=out_r)
    assert got[0] is out_a and got[1] is out_r and np.array_equal(out_a, want_adv) and np.array_equal(out_r, want_ret)
    if T > 1:  # a done at t cuts the recursion: the advantage there is r - v, whatever follows
        e = int(np.flatnonzero(done[0])[0])
        assert adv[0, e] == np.float32(np.float64(rew[0, e]) - np.float64(value[0, e]))


def test_lambda_one_without_dones_is_the_discounted_return():
    """ret[t] = sum_k gamma^k r[t + k] + gamma^(T - t) v[T] up to float32 rounding: the float64 recursion's
    own error is some T ulps of a double, far below half a float32 ulp of the result, which is what the bound
    is: one float32 rounding of each side can differ by one ulp of the larger."""
    T, n, gamma = 37, 65, 0.99
    rew, _, value = gd.case(T, n)
    done = np.zeros((T, n), np.uint8)
    _, ret = gae(rew, done, value, gamma, 1.0)
    want = np.zeros((T, n))
    run = value[T].astype(np.float64)
    for t in range(T - 1, -1, -1):
        run = rew[t].astype(np.float64) + gamma * run
        want[t] = run
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(ret.astype(np.float64) - want) <= ulp).all()


def test_argument_errors_before_any_hip_call():
    L = _native.lib()
    rew, done, value = gd.case(2, 4)
    adv, ret = np.zeros((2, 4), np.float32), np.zeros((2, 4), np.float32)
    ptrs = [a.ctypes.data for a in (rew, done, value)]
    for f, tail in ((L.pbg_gae_host, ()), (L.pbg_gae, (None,))):  # the device entry checks before it launches
        for T, n in ((0, 4), (-1, 4), (2, 0), (2, -1)):
            assert f(T, n, *ptrs, 0.99, 0.95, adv.ctypes.data, ret.ctypes.data, *tail) == -1, (T, n)
        for i in range(5):
            args = ptrs + [adv.ctypes.data, ret.ctypes.data]
            args[i] = None
            assert f(2, 4, *args[:3], 0.99, 0.95, *args[3:], *tail) == -1, i
    assert not adv.any() and not ret.any()
    for bad in (rew.astype(np.float64), rew[:, :3], rew[0]):
        with pytest.raises(_native.PbgError):
            gae(bad, done, value)
    with pytest.raises(_native.PbgError):
        gae(rew, done.astype(np.int32), value)
    with pytest.raises(_native.PbgError):
        gae(rew, done, value[:2])
