"""Shared by the return-statistics tests (include/pbg.h "Return statistics"): seeded cases and
the numpy restatement of the three stated orders -- the per-env walk with its 32-lane tree, the one-lane finalize, and
the scaled, clipped reward.  numpy's float64 add, multiply, divide and sqrt are IEEE and never fused, so the
restatement gives the library's bits."""
import numpy as np

TILE = 32
TS, NS, GAMMAS = (1, 2, 37), (1, 32, 33, 65, 257), (0.99, 0.0, 1.0)
GRID = [(T, n, g) for T in TS for n in NS for g in GAMMAS]


def case(T, n, seed=0, p_done=0.1):
    """``(rew float32 [T, n], done uint8 [T, n])``: rewards 2 N(0, 1), dones with probability ``p_done`` and forced at
    (T - 1, env 0) and (0, env n - 1)."""
    rng = np.random.default_rng([seed, T, n])
    rew = (2.0 * rng.standard_normal((T, n))).astype(np.float32)
    done = (rng.random((T, n)) < p_done).astype(np.uint8)
    done[T - 1, 0] = 1
    done[0, n - 1] = 1
    return rew, done


def nonfinite_case(T=6, n=40):
    """``case`` without dones, with a NaN, a +inf and a -inf reward at chosen steps: ``(rew, done, [(t, e), ...])``."""
    rew, _ = case(T, n, seed=3)
    done = np.zeros((T, n), np.uint8)
    at = [(1, 0), (2, 5), (T - 1, 33), (0, n - 1)]
    for (t, e), v in zip(at, (np.nan, np.inf, -np.inf, np.nan)):
        rew[t, e] = v
    return rew, done, at


def clip_case(T=8, n=64):
    """Unit-variance rewards with an outlier of 1e6 and one of -1e6 at the last step, ``(rew, done, (hi, lo))``.  Each
    outlier enters one return, so the variance is about 2e12 / (T n) and the scaled outliers about sqrt(T n / 2) = 16:
    past a clip of 10, while every other scaled reward is tiny."""
    rng = np.random.default_rng(11)
    rew = rng.standard_normal((T, n)).astype(np.float32)
    done = np.zeros((T, n), np.uint8)
    hi, lo = (T - 1, 7), (T - 1, 40)
    rew[hi] = 1e6
    rew[lo] = -1e6
    return rew, done, (hi, lo)


def walk(rew, done, gamma, carry):
    """The walk over ``rew`` / ``done`` ``[T, n]`` from ``carry`` (float64 ``[n]``): ``(carry_out [n], counts int64
    [tiles], sums float64 [tiles, 2])``.  A column per lane; lanes past n hold (0, +0.0, +0.0)."""
    T, n = rew.shape
    tiles = -(-n // TILE)
    g = np.float64(gamma)
    R = np.array(carry, np.float64)
    c = np.zeros(tiles * TILE, np.int64)
    s1, s2 = np.zeros(tiles * TILE, np.float64), np.zeros(tiles * TILE, np.float64)
    with np.errstate(all="ignore"):
        for t in range(T):
            R = g * R + rew[t].astype(np.float64)   # two ufuncs: the product is rounded before the add
            fin = np.isfinite(R)
            c[:n] += fin
            s1[:n] = np.where(fin, s1[:n] + R, s1[:n])
            s2[:n] = np.where(fin, s2[:n] + R * R, s2[:n])
            R = np.where(~fin | (done[t] != 0), np.float64(0.0), R)
    c, s1, s2 = (x.reshape(tiles, TILE).copy() for x in (c, s1, s2))
    for s in (16, 8, 4, 2, 1):
        for x in (c, s1, s2):
            x[:, :s] += x[:, s:2 * s]
    return R, c[:, 0].copy(), np.stack((s1[:, 0], s2[:, 0]), axis=1)


def finalize(counts, sums, n_used, tot_count, tot_sums, scale, var_floor=1e-2):
    """The one lane's order: ``(tot_count, tot_sums [2], scale float32)`` after adding the slots ``0 .. n_used - 1``."""
    bc, b1, b2 = 0, np.float64(0.0), np.float64(0.0)
    for g in range(n_used):
        bc += int(counts[g])
        b1 = b1 + np.float64(sums[g, 0])
        b2 = b2 + np.float64(sums[g, 1])
    tc = int(tot_count) + bc
    t1, t2 = np.float64(tot_sums[0]) + b1, np.float64(tot_sums[1]) + b2
    if tc == 0:
        return tc, np.array([t1, t2]), np.float32(scale)
    with np.errstate(all="ignore"):
        cnt = np.float64(tc)
        m = t1 / cnt
        mm = m * m
        var = t2 / cnt - mm
        var = var if var > np.float64(var_floor) else np.float64(var_floor)
        return tc, np.array([t1, t2]), np.float32(np.float64(1.0) / np.sqrt(var))


def apply(rew, scale, clip=10.0):
    with np.errstate(all="ignore"):
        v = rew.astype(np.float32) * np.float32(scale)
    c = np.float32(clip)
    return np.where(v < -c, -c, np.where(v > c, c, v)).astype(np.float32)


class Restated:
    """The object's state and its three calls, restated: what ``ppo.RetStats`` must hold bit for bit."""

    def __init__(self, n_envs, gamma, n_slots=None):
        self.n_envs, self.gamma = n_envs, gamma
        self.n_slots = -(-n_envs // TILE) if n_slots is None else n_slots
        self.reset()

    def reset(self):
        self.carry = np.zeros(self.n_envs, np.float64)
        self.counts, self.sums = np.zeros(self.n_slots, np.int64), np.zeros((self.n_slots, 2), np.float64)
        self.tot_count, self.tot_sums, self.scale = 0, np.zeros(2, np.float64), np.float32(1.0)

    def update(self, rew, done, slot_offset=0):
        n = rew.shape[1]
        self.carry[:n], c, s = walk(rew, done, self.gamma, self.carry[:n])
        self.counts[slot_offset:slot_offset + len(c)] = c
        self.sums[slot_offset:slot_offset + len(c)] = s

    def finalize(self, n_used_slots=None, var_floor=1e-2):
        n_used = self.n_slots if n_used_slots is None else n_used_slots
        self.tot_count, self.tot_sums, self.scale = finalize(self.counts, self.sums, n_used, self.tot_count, self.tot_sums,
                                                             self.scale, var_floor)

    def apply(self, rew, clip=10.0):
        return apply(rew, self.scale, clip)


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.ascontiguousarray(np.asarray(a))
    return a.view({np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}.get(a.dtype, a.dtype))


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), g.size)


def assert_state(obj, ref, what=""):
    """``obj`` (a ``ppo.RetStats``, host or device) holds ``ref``'s (a ``Restated``'s, or another ``RetStats``') carry,
    slots, totals and scale bit for bit."""
    if isinstance(ref, Restated):
        rc, rs, rt = ref.carry, (ref.counts, ref.sums), (np.array([ref.tot_count], np.int64), ref.tot_sums)
        rscale = np.array([ref.scale], np.float32)
    else:
        rc, rs, rt, rscale = ref.carry, ref.get_slots(), ref.totals, ref.scale
    same(obj.carry, rc, what + " carry")
    counts, sums = obj.get_slots()
    same(counts, rs[0], what + " slot counts")
    same(sums, rs[1], what + " slot sums")
    count, tsums = obj.totals
    same(count, rt[0], what + " total count")
    same(tsums, rt[1], what + " total sums")
    same(obj.scale, rscale, what + " scale")
