"""What the truncation-bootstrapping tests share (tests/test_gae_trunc_host.py, tests/test_trunc_gpu.py): seeded
trajectories with truncation flags and the numpy restatement of include/pbg.h's pbg_gae_trunc scan."""
import numpy as np

import gae_data as gd


def case(T, n, seed=0):
    """gae_data.case's rew, done, value, plus trunc uint8 [T, n], a subset of done (each done a truncation with
    probability 0.5; env 0's forced done at t = T - 1 is one, env n - 1's at t = 0 is not, unless they are the same
    element), and term_value float32 [T, n]: finite where trunc is set, NaN elsewhere (it must not be read there)."""
    rew, done, value = gd.case(T, n, seed)
    r = np.random.default_rng([seed, T, n, 7])
    trunc = ((r.random((T, n)) < 0.5) & (done != 0)).astype(np.uint8)
    trunc[0, n - 1] = 0
    trunc[T - 1, 0] = 1
    term_value = (r.standard_normal((T, n)) * 5.0).astype(np.float32)
    term_value[trunc == 0] = np.nan
    return rew, done, trunc, value, term_value


def gae_trunc_numpy(rew, done, trunc, value, term_value, gamma, lam):
    """The stated order in numpy float64 (numpy contracts nothing): every operation one rounding."""
    T, n = rew.shape
    gamma, gl = np.float64(gamma), np.float64(gamma) * np.float64(lam)
    A = np.zeros(n, np.float64)
    adv, ret = np.empty((T, n), np.float32), np.empty((T, n), np.float32)
    for t in range(T - 1, -1, -1):
        tr = trunc[t] != 0
        nd = np.where(done[t] != 0, 0.0, 1.0)
        v = value[t].astype(np.float64)
        vn = np.where(tr, term_value[t].astype(np.float64), value[t + 1].astype(np.float64))
        nb = np.where(tr, 1.0, nd)
        delta = (rew[t].astype(np.float64) + (gamma * vn) * nb) - v
        A = delta + (gl * nd) * A
        adv[t] = A.astype(np.float32)
        ret[t] = (A + v).astype(np.float32)
    return adv, ret
