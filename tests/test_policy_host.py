"""The MLP policy's host path (pbg_policy_create with device -1, pbg_policy_act_host; no GPU).

Its contract (include/pbg.h): every output of a layer is a k-ascending fmaf chain started from the
bias, the hidden layers then `acc < 0 ? 0 : acc`.  The device kernel must give the same floats
(test_policy_gpu.py compares them bit for bit), so what is pinned here pins both."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.policy import MLPPolicy

import policy_data as pd

CASES = [("fixture", f) for f in pd.FIXTURES] + [("synthetic", d) for d in pd.SYNTHETIC]


def case_weights(kind, what):
    return pd.fixture_weights(what) if kind == "fixture" else pd.synthetic_weights(what)


def test_fixtures_present():
    assert len(pd.FIXTURES) == 11, pd.FIXTURES


@pytest.mark.parametrize("kind,what", CASES, ids=[str(w) for _, w in CASES])
def test_host_act_within_apriori_bound(kind, what):
    """512 seeded N(0,1) rows clipped to +-5 against a float64 numpy evaluation, within the bound
    that holds for any rounding of the chain (policy_data.mlp_float64_with_bound)."""
    ws = case_weights(kind, what)
    obs = pd.seeded_obs(ws[0].shape[0])
    pi = MLPPolicy(*ws)
    got = pi.act(obs)
    pi.close()
    assert got.dtype == np.float32 and got.shape == (pd.N_OBS, ws[4].shape[1])
    ref, bound = pd.mlp_float64_with_bound(ws, obs)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"max err / bound = {(err / bound).max():.4f}, max err = {err.max():.3e}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize("dims", [(70, 256, 128, 30), (28, 128, 64, 8), (7, 33, 17, 3), (256, 256, 256, 64)], ids=str)
def test_host_act_exact_on_integers(dims):
    """Weights from {-1,0,1}, obs from {-2..2}: every partial sum is an integer below 2^24
    (|h1| <= 2*70+1, |h2| <= 141*256+1 = 36097, |out| <= 36097*128+1 < 2^23), so every fma is
    exact whatever it rounds like and the result equals the int64 evaluation.
    The widest dims (256, 256, 256, 64) pass that worst case ((513*256+1)*256+1 > 2^24), so for them the
    bound is taken from the (fixed) data: the sum of |term| over a layer bounds every partial sum."""
    ws = pd.integer_weights(dims)
    obs = pd.integer_obs(dims[0])
    x = obs.astype(np.int64)
    for w, b, relu in ((ws[0], ws[1], True), (ws[2], ws[3], True), (ws[4], ws[5], False)):
        assert (np.abs(x) @ np.abs(w.astype(np.int64)) + np.abs(b.astype(np.int64))).max() < 2 ** 24
        x = x @ w.astype(np.int64) + b.astype(np.int64)
        x = np.maximum(x, 0) if relu else x
    pi = MLPPolicy(*ws)
    got = pi.act(obs)
    pi.close()
    ref = pd.mlp_int64(ws, obs)
    assert 10 < np.abs(ref).max() < 2 ** 24  # non-trivial sums, exactly representable
    assert (got.astype(np.float64) == ref).all()
    assert (got.astype(np.int64) == ref).all()


def test_host_act_is_the_k_ascending_fma_chain():
    """The chain itself, one fma per step, in exact rational-free form: an fma's single rounding
    is float32(float64 product + float64 acc) whenever that float64 sum is exact or far from a
    float32 tie -- with 12-bit operands the product has <= 24 significant bits and the sum is
    exact in float64, so numpy reproduces fmaf bit for bit."""
    rng = np.random.default_rng(7)
    dims = (9, 21, 13, 5)

    def q12(a):  # keep 12 significant bits
        m, e = np.frexp(a)
        return np.ldexp(np.round(m * 4096) / 4096, e).astype(np.float32)

    ws = [q12(w) for w in pd.synthetic_weights(dims)]
    obs = q12(rng.standard_normal((64, dims[0])))

    def layer(x, w, b, relu):
        acc = np.broadcast_to(b, (x.shape[0], w.shape[1])).astype(np.float32)
        for k in range(w.shape[0]):
            # products of the 12-bit first-layer operands are exact in float32; later layers' x is a
            # full float32, so the float64 product (<= 36 bits) + acc (24 bits) may round in float64:
            # double rounding can only differ from fmaf at a float32 tie of probability ~2^-29
            acc = (x[:, k:k + 1].astype(np.float64) * w[k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        return np.where(acc < 0, np.float32(0), acc) if relu else acc

    ref = layer(layer(layer(obs, ws[0], ws[1], True), ws[2], ws[3], True), ws[4], ws[5], False)
    pi = MLPPolicy(*ws)
    got = pi.act(obs)
    pi.close()
    assert np.array_equal(got, ref)


def test_rows_are_independent():
    """Row i's output is the same floats for n = 1, 17 and 512 and at any position; a NaN or inf
    row poisons only its own output."""
    ws = pd.fixture_weights("policy_ant.npz")
    obs = pd.seeded_obs(ws[0].shape[0])
    pi = MLPPolicy(*ws)
    full = pi.act(obs)
    for i in (0, 5, 511):
        assert np.array_equal(pi.act(obs[i:i + 1])[0], full[i])
    assert np.array_equal(pi.act(obs[100:117]), full[100:117])
    perm = np.random.default_rng(0).permutation(pd.N_OBS)
    assert np.array_equal(pi.act(obs[perm]), full[perm])
    bad = obs.copy()
    bad[3, 2] = np.nan
    bad[200, :] = np.inf
    bad[201, 0] = -np.inf
    got = pi.act(bad)
    clean = np.ones(pd.N_OBS, bool)
    clean[[3, 200, 201]] = False
    assert np.array_equal(got[clean], full[clean])
    assert np.isnan(got[3]).all()  # the NaN passes the ReLU (acc < 0 ? 0 : acc) and reaches every action
    assert not np.isfinite(got[200]).all() and not np.isfinite(got[201]).all()
    pi.close()


def _create(device, dims, arrays):
    FP = ctypes.POINTER(ctypes.c_float)
    out = ctypes.c_void_p(0x1234)  # a stale value: every failure must leave NULL
    ptrs = [a.ctypes.data_as(FP) if a is not None else None for a in arrays]
    rc = _native.lib().pbg_policy_create(device, *dims, *ptrs, ctypes.byref(out))
    return rc, out


def test_argument_errors_without_gpu():
    L = _native.lib()
    good = (7, 33, 17, 3)
    ws = pd.synthetic_weights((256, 256, 256, 64))  # large enough for every dims below
    for dims in ((0, 33, 17, 3), (7, 0, 17, 3), (7, 33, 0, 3), (7, 33, 17, 0), (257, 33, 17, 3), (7, 257, 17, 3),
                 (7, 33, 257, 3), (7, 33, 17, 65), (-1, 33, 17, 3)):
        rc, out = _create(-1, dims, ws)
        assert rc == -1 and not out.value, dims
        assert b"pbg_policy_create" in L.pbg_last_error()
    for missing in range(6):
        arrays = list(ws)
        arrays[missing] = None
        rc, out = _create(-1, good, arrays)
        assert rc == -1 and not out.value, missing
    # out-of-range dims are refused before any device is looked at, whatever the device argument
    rc, out = _create(0, (7, 33, 17, 65), ws)
    assert rc == -1 and not out.value
    rc, out = _create(-2, good, ws)
    assert rc == -1 and not out.value
    # the limits themselves are legal
    rc, out = _create(-1, (256, 256, 256, 64), ws)
    assert rc == 0 and out.value
    L.pbg_policy_destroy(out)
    # a host-only policy has no device path
    rc, out = _create(-1, good, pd.synthetic_weights(good))
    assert rc == 0 and out.value
    assert L.pbg_policy_act(out, 1, None, None, None) == -1
    assert b"host-only" in L.pbg_last_error()
    io = _native.RolloutIO(n_steps=1)
    assert L.pbg_rollout(None, out, ctypes.byref(io), None) == -1
    L.pbg_policy_destroy(out)
    L.pbg_policy_destroy(None)


def test_python_surface():
    ws = pd.fixture_weights("policy_humanoid.npz")
    import os
    pi = MLPPolicy.from_npz(os.path.join(pd.GOLDEN, "policy_humanoid.npz"))
    assert (pi.obs_dim, pi.h1, pi.h2, pi.act_dim) == (44, 256, 128, 17) and pi.device is None
    obs = pd.seeded_obs(44, 8)
    a = pi.act(obs)
    b = MLPPolicy(*ws).act(obs)
    assert np.array_equal(a, b)
    with pytest.raises(_native.PbgError):
        pi.act(obs[:, :40])
    # a wrong `out` is refused before the native call writes through it (not an assert: python -O keeps it)
    for bad in (np.empty((8, 16), np.float32), np.empty((8, 17), np.float64), np.empty((17, 8), np.float32).T,
                np.empty((7, 17), np.float32), [[0.0] * 17] * 8):
        with pytest.raises(_native.PbgError):
            pi.act(obs, out=bad)
    good = np.empty((8, 17), np.float32)
    assert pi.act(obs, out=good) is good and np.array_equal(good, a)
    pi.close()
    pi.close()  # idempotent
    with pytest.raises(_native.PbgError):
        pi.act(obs)
    with pytest.raises(_native.PbgError):
        MLPPolicy(ws[0], ws[1], ws[2], ws[3], ws[4], ws[5][:-1])
    assert set(("pbg_policy_create", "pbg_policy_destroy", "pbg_policy_act", "pbg_policy_act_host",
                "pbg_rollout")) <= set(_native.EXPORTED)
    assert pybulletgym_amd.MLPPolicy is MLPPolicy
