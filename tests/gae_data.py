"""What the GAE tests share (tests/test_gae_host.py, tests/test_ppo_gpu.py): seeded trajectories and the numpy
restatement of include/pbg.h's scan."""
import numpy as np

TS = (1, 2, 37)
NS = (1, 64, 65)


def case(T, n, seed=0):
    """rew float32 [T, n], done uint8 [T, n] (probability 0.1, and forced in env 0 at t = T - 1 and in env
    n - 1 at t = 0), value float32 [T + 1, n]."""
    r = np.random.default_rng([seed, T, n])
    rew = (r.standard_normal((T, n)) * 2.0).astype(np.float32)
    value = (r.standard_normal((T + 1, n)) * 5.0).astype(np.float32)
    done = (r.random((T, n)) < 0.1).astype(np.uint8)
    done[T - 1, 0] = 1
    done[0, n - 1] = 1
    return rew, done, value


def gae_numpy(rew, done, value, gamma, lam):
    """The stated order in numpy float64 (numpy contracts nothing): every operation one rounding."""
    T, n = rew.shape
    gamma, gl = np.float64(gamma), np.float64(gamma) * np.float64(lam)
    A = np.zeros(n, np.float64)
    adv, ret = np.empty((T, n), np.float32), np.empty((T, n), np.float32)
    for t in range(T - 1, -1, -1):
        nd = np.where(done[t] != 0, 0.0, 1.0)
        v = value[t].astype(np.float64)
        delta = (rew[t].astype(np.float64) + (gamma * value[t + 1].astype(np.float64)) * nd) - v
        A = delta + (gl * nd) * A
        adv[t] = A.astype(np.float32)
        ret[t] = (A + v).astype(np.float32)
    return adv, ret
