"""Reward scaling by a running std of the discounted return, on the host (include/pbg.h "Return statistics", the
object created with device -1; no GPU): the walk, the finalize and the scaling against the numpy restatement of the
stated orders, bit for bit; the carry across calls and the totals across iterations; a case by hand with both
branches of the variance floor; non-finite rewards; the clip; slots that compose; the argument checks and reset."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import RetStats

import retstats_data as rd


@pytest.mark.parametrize("T,n,gamma", rd.GRID)
def test_host_twin_equals_the_numpy_restatement(T, n, gamma):
    rew, done = rd.case(T, n)
    assert done[T - 1, 0] and done[0, n - 1]
    obj, ref = RetStats(n, gamma), rd.Restated(n, gamma)
    assert obj.host and obj.n_slots == -(-n // 32)
    obj.update(rew, done)
    obj.finalize()
    ref.update(rew, done)
    ref.finalize()
    rd.assert_state(obj, ref, f"T={T} n={n} gamma={gamma}")
    assert ref.tot_count == T * n
    out = np.full((T, n), np.nan, np.float32)
    assert obj.apply(rew, out=out) is out
    rd.same(out, ref.apply(rew), "scaled rewards")
    assert np.isfinite(out).all()
    if T * n >= 64:
        assert np.abs(out).max() < 10.0   # the clip never engages on these: it has the case of its own below
    obj.close()


@pytest.mark.parametrize("gamma", rd.GAMMAS)
def test_carry_across_calls(gamma):
    T1, T2, n = 5, 9, 65
    rew, done = rd.case(T1 + T2, n, seed=1)
    done[T1 - 1, 3] = 1   # a done at the last step of the first call: the second starts that env from zero
    done[T1 - 1, 4] = 0
    one, two = RetStats(n, gamma), RetStats(n, gamma)
    one.update(rew, done)
    two.update(rew[:T1].copy(), done[:T1].copy())
    mid = two.carry
    assert mid[3] == 0.0 and mid[4] != 0.0
    two.update(rew[T1:].copy(), done[T1:].copy())
    rd.same(two.carry, one.carry, "carry of two walks against one")
    ref = rd.Restated(n, gamma)
    ref.update(rew, done)
    rd.same(one.carry, ref.carry, "carry against the restatement")


def test_two_iterations_totals():
    n, gamma = 65, 0.99
    obj, ref = RetStats(n, gamma), rd.Restated(n, gamma)
    firsts = None
    for it, T in enumerate((7, 4)):
        rew, done = rd.case(T, n, seed=10 + it)
        for o in (obj, ref):
            o.update(rew, done)
            o.finalize()
        rd.assert_state(obj, ref, f"iteration {it}")
        if firsts is None:
            firsts = (ref.tot_count, ref.tot_sums.copy())
    # the second finalize added the second batch's slot sum to the first totals
    _, sums = obj.get_slots()
    b1 = np.float64(0.0)
    for g in range(obj.n_slots):
        b1 = b1 + sums[g, 0]
    assert ref.tot_count == firsts[0] + 4 * n
    assert obj.totals[1][0] == firsts[1][0] + b1


def test_by_hand():
    rew = np.array([[1.0], [1.0], [1.0]], np.float32)
    done = np.array([[0], [1], [0]], np.uint8)
    var = 4.25 / 3.0 - (3.5 / 3.0) * (3.5 / 3.0)   # about 0.0556
    for floor, want in ((1e-2, var), (0.5, 0.5)):   # a floor below the variance, and one above it
        obj = RetStats(1, 0.5)
        obj.update(rew, done)   # R = 1, 1.5 (done: back to 0), 1
        assert obj.carry[0] == 1.0
        counts, sums = obj.get_slots()
        assert counts[0] == 3 and sums[0, 0] == 3.5 and sums[0, 1] == 4.25
        obj.finalize(var_floor=floor)
        count, tsums = obj.totals
        assert count[0] == 3 and tsums[0] == 3.5 and tsums[1] == 4.25
        assert obj.scale[0] == np.float32(1.0 / np.sqrt(want))
        assert (want == var) == (floor < var)


def test_non_finite_rewards():
    rew, done, at = rd.nonfinite_case()
    T, n = rew.shape
    gamma = 0.9
    obj, ref = RetStats(n, gamma), rd.Restated(n, gamma)
    for o in (obj, ref):
        o.update(rew, done)
        o.finalize()
    rd.assert_state(obj, ref, "non-finite rewards")
    count, tsums = obj.totals
    assert count[0] == T * n - len(at)   # exactly the non-finite steps are left out
    assert np.isfinite(tsums).all() and np.isfinite(obj.carry).all() and np.isfinite(obj.scale).all()
    # the carry restarts from zero behind a non-finite step: the env of the last step's -inf ends at 0, and the one whose
    # NaN came at t = 1 carries on from the rewards after it alone
    carry = obj.carry
    assert carry[33] == 0.0
    R = np.float64(0.0)
    for t in range(2, T):
        R = np.float64(gamma) * R + np.float64(rew[t, 0])
    assert carry[0] == R
    out = obj.apply(rew)
    rd.same(out, ref.apply(rew), "scaled non-finite rewards")
    assert np.isnan(out[1, 0]) and np.isnan(out[0, n - 1])         # apply passes the NaN through
    assert out[2, 5] == 10.0 and out[T - 1, 33] == -10.0           # and clips the infinities
    # a batch that is all NaN leaves the scale (and the totals) where they were
    before = obj.scale.copy()
    obj.update(np.full((3, n), np.nan, np.float32), np.zeros((3, n), np.uint8))
    obj.finalize()
    rd.same(obj.scale, before, "scale after an all-NaN batch")
    assert obj.totals[0][0] == count[0]
    fresh = RetStats(n, gamma)
    fresh.update(np.full((3, n), np.nan, np.float32), np.zeros((3, n), np.uint8))
    fresh.finalize()
    assert fresh.totals[0][0] == 0 and fresh.scale[0] == np.float32(1.0)   # empty totals: the initial scale stays


def test_the_clip_engages():
    rew, done, (hi, lo) = rd.clip_case()
    T, n = rew.shape
    obj, ref = RetStats(n, 0.99), rd.Restated(n, 0.99)
    for o in (obj, ref):
        o.update(rew, done)
        o.finalize()
    out = obj.apply(rew, clip=10.0)
    rd.same(out, ref.apply(rew, 10.0), "clipped rewards")
    scale = obj.scale[0]
    with np.errstate(all="ignore"):
        v = rew * scale
    hit = np.abs(v) > 10.0
    assert hit.sum() == 2 and (~hit).sum() == T * n - 2
    assert hit[hi] and hit[lo] and out[hi] == 10.0 and out[lo] == -10.0
    rd.same(out[~hit], v[~hit], "unclipped rewards are r * scale")


def test_slots_compose():
    T, n, gamma = 6, 128, 0.99
    rew, done = rd.case(T, n, seed=5)
    whole = RetStats(n, gamma)
    whole.update(rew, done)
    whole.finalize()
    halves = [RetStats(64, gamma, n_slots=4) for _ in range(2)]
    for r, h in enumerate(halves):
        h.update(rew[:, 64 * r:64 * (r + 1)].copy(), done[:, 64 * r:64 * (r + 1)].copy(), slot_offset=2 * r)
    for r, h in enumerate(halves):   # every object takes the other's slots
        counts, sums = halves[1 - r].get_slots(2 * (1 - r), 2)
        h.set_slots(2 * (1 - r), counts, sums)
    for h in halves:
        h.finalize()
        for a, b in zip(h.totals + (h.scale,), whole.totals + (whole.scale,)):
            rd.same(a, b, "halves against the whole")
        ca, sa = h.get_slots()
        cb, sb = whole.get_slots()
        rd.same(ca, cb, "slot counts")
        rd.same(sa, sb, "slot sums")
    rd.same(np.concatenate([h.carry for h in halves]), whole.carry, "concatenated carry")


def test_reset_and_state():
    n = 40
    rew, done = rd.case(5, n, seed=2)
    obj = RetStats(n, 0.99)
    obj.update(rew, done)
    obj.finalize()
    st = obj.state()
    assert st["count"][0] == 5 * n and st["scale"][0] != np.float32(1.0)
    obj.reset()
    rd.assert_state(obj, rd.Restated(n, 0.99), "after reset")
    other = RetStats(n, 0.99)
    other.load_state(st)
    for k, v in other.state().items():
        rd.same(v, st[k], f"load_state {k}")
    obj.close()
    with pytest.raises(_native.PbgError, match="closed"):
        obj.reset()


def test_argument_errors():
    L = _native.lib()
    assert set(_native.RET_STATS_EXPORTED) <= set(_native.EXPORTED)
    for f in _native.RET_STATS_EXPORTED:
        assert hasattr(L, f), f

    def create(n_envs, n_slots, gamma, device=-1):
        h = ctypes.c_void_p(0x1234)   # a stale value: every failure must leave NULL
        rc = L.pbg_ret_stats_create(device, n_envs, n_slots, gamma, ctypes.byref(h))
        return rc, h

    for args in ((0, 1, 0.99), (33, 1, 0.99), (32, 1, -0.1), (32, 1, 1.5), (32, 1, float("nan")), (32, 1, 0.99, -2)):
        rc, h = create(*args)
        assert rc == -1 and not h.value, args
    assert L.pbg_ret_stats_create(-1, 32, 1, 0.99, None) == -1
    rc, h = create(40, 3, 0.99)
    assert rc == 0 and h.value
    T, n = 2, 40
    rew, out = np.zeros((T, n), np.float32), np.zeros((T, n), np.float32)
    done = np.zeros((T, n), np.uint8)
    r, d, o = rew.ctypes.data, done.ctypes.data, out.ctypes.data
    bad_walks = [(None, T, n, 0, r, d), (h, 0, n, 0, r, d), (h, T, 0, 0, r, d), (h, T, 41, 0, r, d),   # T, n < 1; n > n_envs
                 (h, T, n, -1, r, d), (h, T, n, 2, r, d),                                              # slots outside n_slots
                 (h, T, n, 0, None, d), (h, T, n, 0, r, None)]
    for a in bad_walks:
        assert L.pbg_ret_stats_walk(*a, None) == -1, a
        assert b"pbg_ret_stats_walk" in L.pbg_last_error()
    assert L.pbg_ret_stats_walk(h, T, 32, 2, r, d, None) == 0   # one tile at the last slot is inside
    for a in ((None, 1, 1e-2), (h, -1, 1e-2), (h, 4, 1e-2), (h, 2, 0.0), (h, 2, -1.0), (h, 2, float("nan"))):
        assert L.pbg_ret_stats_finalize(*a, None) == -1, a
    bad_applies = [(None, 8, 10.0, r, o), (h, 0, 10.0, r, o), (h, 8, 0.0, r, o), (h, 8, -1.0, r, o), (h, 8, float("nan"), r, o),
                   (h, 8, 10.0, None, o), (h, 8, 10.0, r, None),
                   (h, 8, 10.0, r, r), (h, 8, 10.0, r, r + 4), (h, 8, 10.0, r + 28, r)]   # aliasing, whole or in part
    for a in bad_applies:
        assert L.pbg_ret_stats_apply(*a, None) == -1, a
    assert L.pbg_ret_stats_apply(h, 8, 10.0, r, r + 32, None) == 0   # adjacent ranges do not overlap
    counts, sums = np.zeros(3, np.int64), np.zeros((3, 2), np.float64)
    c, s = counts.ctypes.data, sums.ctypes.data
    for f in (L.pbg_ret_stats_get_slots, L.pbg_ret_stats_set_slots):
        for a in ((None, 0, 3, c, s), (h, -1, 1, c, s), (h, 1, 3, c, s), (h, 0, -1, c, s), (h, 0, 3, None, s), (h, 0, 3, c, None)):
            assert f(*a, None) == -1, a
        assert f(h, 0, 3, c, s, None) == 0 and f(h, 3, 0, c, s, None) == 0
    for name in ("get_totals", "set_totals"):
        f = getattr(L, "pbg_ret_stats_" + name)
        assert f(None, c, s, None) == -1 and f(h, None, s, None) == -1 and f(h, c, None, None) == -1
    for name in ("get_carry", "set_carry", "get_scale", "set_scale"):
        f = getattr(L, "pbg_ret_stats_" + name)
        assert f(None, s, None) == -1 and f(h, None, None) == -1
    assert L.pbg_ret_stats_reset(None, None) == -1
    L.pbg_ret_stats_destroy(h)
    L.pbg_ret_stats_destroy(None)
    # the Python object refuses what it can see: shapes, dtypes, contiguity, a closed object
    obj = RetStats(40, 0.99)
    with pytest.raises(_native.PbgError, match="rew_traj"):
        obj.update(np.zeros(40, np.float32), np.zeros(40, np.uint8))
    with pytest.raises(_native.PbgError, match="done_traj"):
        obj.update(rew, done.astype(np.int8))
    with pytest.raises(_native.PbgError, match="rew_traj"):
        obj.update(rew.astype(np.float64), done)
    with pytest.raises(_native.PbgError, match="out"):
        obj.apply(rew, out=np.zeros((T, n + 1), np.float32))
    with pytest.raises(_native.PbgError, match="overlaps"):
        obj.apply(rew, out=rew)
    with pytest.raises(_native.PbgError, match="slots"):
        obj.get_slots(1, 2)
    with pytest.raises(_native.PbgError):
        RetStats(40, 1.5)
    with pytest.raises(_native.PbgError):
        RetStats(40, 0.99, n_slots=1)
