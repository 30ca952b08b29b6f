"""Shared inputs of the MLP-policy tests (test_policy_host.py, test_policy_gpu.py): the fixtures'
weights, seeded synthetic weights, the seeded observations and the exact-integer data."""
from __future__ import annotations

import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("weights_dense1_w", "weights_dense1_b", "weights_dense2_w", "weights_dense2_b",
        "weights_final_w", "weights_final_b")
FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "policy_*.npz")))
SYNTHETIC = ((7, 33, 17, 3), (5, 64, 32, 1), (256, 256, 256, 64))
N_OBS = 512


def fixture_weights(name: str):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return [np.ascontiguousarray(z[k], dtype=np.float32) for k in KEYS]


def synthetic_weights(dims, seed: int = 1):
    """N(0, 1/K) weights and N(0, 0.01) biases for dims = (obs_dim, h1, h2, act_dim)."""
    rng = np.random.default_rng([seed, *dims])
    d0, d1, d2, d3 = dims
    out = []
    for k, h in ((d0, d1), (d1, d2), (d2, d3)):
        out.append((rng.standard_normal((k, h)) / np.sqrt(k)).astype(np.float32))
        out.append((0.1 * rng.standard_normal(h)).astype(np.float32))
    return out


def seeded_obs(obs_dim: int, n: int = N_OBS, seed: int = 0) -> np.ndarray:
    """n seeded N(0, 1) rows clipped to +-5."""
    rng = np.random.default_rng([seed, obs_dim])
    return np.clip(rng.standard_normal((n, obs_dim)), -5.0, 5.0).astype(np.float32)


def integer_weights(dims, seed: int = 2):
    """Weights and biases from {-1, 0, 1}: seeded, and shifted by the position so that no two
    rows or columns repeat a pattern."""
    rng = np.random.default_rng([seed, *dims])
    d0, d1, d2, d3 = dims
    out = []
    for k, h in ((d0, d1), (d1, d2), (d2, d3)):
        r = rng.integers(0, 3, (k, h))
        pos = np.add.outer(np.arange(k), 2 * np.arange(h))
        out.append(((r + pos) % 3 - 1).astype(np.float32))
        out.append(((rng.integers(0, 3, h) + np.arange(h)) % 3 - 1).astype(np.float32))
    return out


def integer_obs(obs_dim: int, n: int = N_OBS, seed: int = 3) -> np.ndarray:
    """Observations from {-2, ..., 2}, seeded and position-dependent."""
    rng = np.random.default_rng([seed, obs_dim])
    r = rng.integers(0, 5, (n, obs_dim))
    pos = np.add.outer(3 * np.arange(n), np.arange(obs_dim))
    return ((r + pos) % 5 - 2).astype(np.float32)


def mlp_int64(ws, obs) -> np.ndarray:
    w1, b1, w2, b2, w3, b3 = [a.astype(np.int64) for a in ws]
    x = np.maximum(obs.astype(np.int64) @ w1 + b1, 0)
    x = np.maximum(x @ w2 + b2, 0)
    return x @ w3 + b3


def mlp_float64_with_bound(ws, obs):
    """The MLP in float64 and the a-priori bound on what ANY float32 rounding of the contract's chain
    (one rounding per fma, k in any order) can differ from it by: with u = 2^-24 and
    gamma_k = k u / (1 - k u), per layer of fan-in K (K products and the bias: K + 1 terms)
        e1 = gamma_{K1+1} (|x| |W1| + |b1|)
        e2 = gamma_{K2+1} ((h1 + e1) |W2| + |b2|) + e1 |W2|
        e3 = gamma_{K3+1} ((h2 + e2) |W3| + |b3|) + e2 |W3|
    (ReLU is 1-Lipschitz, so a layer's input error passes through it unamplified)."""
    u = 2.0 ** -24

    def gamma(k):
        return k * u / (1.0 - k * u)

    w1, b1, w2, b2, w3, b3 = [a.astype(np.float64) for a in ws]
    x = obs.astype(np.float64)
    z1 = x @ w1 + b1
    e1 = gamma(w1.shape[0] + 1) * (np.abs(x) @ np.abs(w1) + np.abs(b1))
    h1 = np.maximum(z1, 0)
    z2 = h1 @ w2 + b2
    e2 = gamma(w2.shape[0] + 1) * ((h1 + e1) @ np.abs(w2) + np.abs(b2)) + e1 @ np.abs(w2)
    h2 = np.maximum(z2, 0)
    z3 = h2 @ w3 + b3
    e3 = gamma(w3.shape[0] + 1) * ((h2 + e2) @ np.abs(w3) + np.abs(b3)) + e2 @ np.abs(w3)
    return z3, e3
