"""Host mirror of the reset RNG of the step kernel (csrc/pbg_math.h philox4x32_10).

The reference draws reset noise with gym's np_random (robot_locomotors.py:18-19:
uniform(-0.1, 0.1) per ordered joint).  The batched kernel draws the same distribution
from Philox4x32-10, key = seed, counter = (global env id, episode index, block, 0x5EED),
so that results do not depend on how envs are sharded over GPUs.  This module
reproduces those draws on the host bit-for-bit (trace replay, sharding tests)."""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: uint32 array [..., 4]; key: (k0, k1).  Returns uint32 [..., 4]."""
    x, y, z, w = [ctr[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0 = M0 * x
        p1 = M1 * z
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        x, y, z, w = (hi1 ^ y ^ k0) & MASK, lo1, (hi0 ^ w ^ k1) & MASK, lo0
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack([x, y, z, w], axis=-1).astype(np.uint32)


def reset_noise(seed: int, global_ids, episode, n_reset_dofs: int) -> np.ndarray:
    """float32 [len(global_ids), n_reset_dofs] = the kernel's U(-0.1, 0.1) reset draws."""
    gid = np.asarray(global_ids, dtype=np.uint32)
    epi = np.broadcast_to(np.asarray(episode, dtype=np.uint32), gid.shape)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.zeros((gid.size, n_reset_dofs), dtype=np.float32)
    for blk in range((n_reset_dofs + 3) // 4):
        ctr = np.stack([gid, epi, np.full_like(gid, blk), np.full_like(gid, 0x5EED)], axis=-1)
        r = philox4x32_10(ctr, key)
        u = (r >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
        # fmaf(0.2f, u, -0.1f): exact in float64, then one rounding to float32
        v = (np.float64(np.float32(0.2)) * u.astype(np.float64) + np.float64(np.float32(-0.1))).astype(np.float32)
        for t in range(4):
            j = 4 * blk + t
            if j < n_reset_dofs:
                out[:, j] = v[:, t]
    return out


def sample_actions(action_dim: int, global_ids, steps, seed: int = 0x5EED) -> np.ndarray:
    """float32 [len(steps), len(global_ids), action_dim] = pbg_sample_actions' U(-1, 1) draws
    (Philox4x32-10, key = seed, counter = (step, global env id, block of 4 actions, 0xAC7))."""
    gid = np.asarray(global_ids, dtype=np.uint32)
    st = np.asarray(steps, dtype=np.uint32)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.zeros((st.size, gid.size, action_dim), dtype=np.float32)
    S, G = np.meshgrid(st, gid, indexing="ij")
    for blk in range((action_dim + 3) // 4):
        ctr = np.stack([S, G, np.full_like(S, blk), np.full_like(S, 0xAC7)], axis=-1)
        r = philox4x32_10(ctr, key)
        u = (r >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
        v = (2.0 * u.astype(np.float64) - 1.0).astype(np.float32)  # fmaf(2, u, -1): exact, one rounding
        for t in range(4):
            j = 4 * blk + t
            if j < action_dim:
                out[..., j] = v[..., t]
    return out


def es_param_count(dims) -> int:
    """D of the flat parameter vector of an MLP dims = (obs_dim, h1, h2, act_dim) (include/pbg.h)."""
    o, h1, h2, a = [int(d) for d in dims]
    return o * h1 + h1 + h1 * h2 + h2 + h2 * a + a


def es_noise(dims, seed: int, generation: int, pair0: int, n_pairs: int) -> np.ndarray:
    """float32 [n_pairs, D]: the evolution-strategy noise of pbg_population_noise (include/pbg.h "Noise
    contract": Philox4x32-10, key = seed, counter = (block of 4 params, pair0 + i, generation, 0xE5), two
    Box-Muller pairs per block), computed in float64 and rounded once like pbg_population_noise_host.
    The device computes the same formula in float32: it agrees within 1e-5 absolute, not bitwise."""
    return _normal_rows(es_param_count(dims), seed, pair0, n_pairs, generation, 0xE5)


def _normal_rows(width: int, seed: int, row0: int, n_rows: int, third: int, tag: int) -> np.ndarray:
    """float32 [n_rows, width]: row i's block b of four normals from counter (b, row0 + i, third, tag)."""
    nb = (width + 3) // 4
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    B, I = np.meshgrid(np.arange(nb, dtype=np.uint32), np.arange(row0, row0 + n_rows, dtype=np.uint32))
    ctr = np.stack([B, I, np.full_like(B, third & 0xFFFFFFFF), np.full_like(B, tag)], axis=-1)
    x = philox4x32_10(ctr, key)
    out = np.empty((n_rows, nb, 4), dtype=np.float32)
    for h in (0, 1):
        u1 = (x[..., 2 * h] >> np.uint32(9)).astype(np.float64) * 2.0 ** -23 + 2.0 ** -24
        u2 = (x[..., 2 * h + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        out[..., 2 * h] = r * np.cos(2.0 * np.pi * u2)
        out[..., 2 * h + 1] = r * np.sin(2.0 * np.pi * u2)
    return np.ascontiguousarray(out.reshape(n_rows, 4 * nb)[:, :width])


def fmix32(h):
    """murmur3's finaliser on a uint32 array (csrc/sim_params.h's contact hash ends with it)."""
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def permutation_keys(seed: int, counter: int) -> np.ndarray:
    """uint32 [8]: the round keys of ``permutation``: the four words of Philox4x32-10 (key = seed) at counter
    (counter, 0, 0, 0x9E), then the four at (counter, 1, 0, 0x9E)."""
    c = int(counter) & 0xFFFFFFFF
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    ctr = np.array([[c, 0, 0, 0x9E], [c, 1, 0, 0x9E]], dtype=np.uint32)
    return philox4x32_10(ctr, key).reshape(8)


def permutation(B: int, seed: int, counter: int) -> np.ndarray:
    """int64 [B]: pbg_perm_fill's permutation of 0 .. B - 1 (include/pbg.h "Counter-based permutations"): an
    eight-round Feistel network on the smallest even number of bits that holds B, keyed by ``permutation_keys``,
    cycle-walked into range.  The same bits as the device and as pbg_perm_host."""
    B = int(B)
    if not 1 <= B <= 2 ** 31 - 1:
        raise ValueError(f"permutation: B = {B} outside 1 .. 2^31 - 1")
    k = max(2, (B - 1).bit_length())
    k += k & 1
    half = np.uint32(k // 2)
    mask = np.uint32((1 << (k // 2)) - 1)
    K = permutation_keys(seed, counter)
    x = np.arange(B, dtype=np.uint32)
    todo = np.arange(B)
    with np.errstate(over="ignore"):
        while todo.size:
            v = x[todo]
            L, R = v >> half, v & mask
            for r in range(8):
                L, R = R, L ^ (fmix32(R + K[r]) & mask)
            v = (L << half) | R
            x[todo] = v
            todo = todo[v >= np.uint32(B)]
    return x.astype(np.int64)


def lr_linear(it: int, n_total: int, lr0: float) -> float:
    """pbg_ppo_lr_linear's value: ``lr0 * (1 - min(it, n_total) / n_total)`` in float64, the same bits."""
    q = np.float64(min(int(it), int(n_total))) / np.float64(int(n_total))
    return float(np.float64(lr0) * (np.float64(1.0) - q))


def action_noise(act_dim: int, seed: int, n: int, env_offset: int, step: int) -> np.ndarray:
    """float32 [n, act_dim]: the action noise of pbg_action_noise_fill (include/pbg.h "Stochastic Gaussian
    actions": the Noise contract's block at counter = (block of 4 components, env_offset + e, step, 0xAC)),
    computed in float64 and rounded once like pbg_action_noise_host.  The device agrees within 1e-5 absolute."""
    return _normal_rows(int(act_dim), seed, int(env_offset), int(n), int(step), 0xAC)
