"""What the permutation and schedule tests share (tests/test_perm_host.py, tests/test_ppoiter_gpu.py): the cases, the
pins of a numpy restatement of include/pbg.h "Counter-based permutations" (they hold the construction, not merely the
library's agreement with itself) and the uniformity statistic."""
import numpy as np

SEED = 0x123456789ABCDEF0
SEEDS = (0, SEED)
SIZES = (1, 2, 3, 16, 17, 255, 256, 257, 1000, 2048, 65537)
SIZES_GPU = (1, 16, 17, 257, 2048, 65537)
COUNTERS = (0, 7, 2 ** 32 - 1)

# (seed, counter, B, the first eight entries, sum of i * perm[i] mod 2^32 or None)
PINS = ((0, 0, 16, (14, 6, 10, 9, 8, 2, 0, 7), None),
        (SEED, 0, 16, (4, 1, 6, 9, 10, 14, 13, 11), None),
        (SEED, 7, 17, (10, 0, 12, 7, 6, 4, 8, 14), None),
        (SEED, 7, 1000, (657, 574, 827, 229, 497, 104, 272, 38), 250070651),
        (SEED, 2 ** 32 - 1, 2048, (171, 938, 1080, 826, 441, 1105, 1859, 520), 2125032628),
        (SEED, 3, 65537, (42146, 23761, 13973, 2459, 62906, 32569, 43601, 34130), 2340424269))
# the round keys at SEED, counter 7
KEYS_7 = (4235921639, 3205352259, 74246146, 738129923, 3169580653, 1683917794, 874900443, 706937546)

# the schedule's cases
SCHEDULE_N = (1, 3, 1000)
SCHEDULE_LR0 = (3e-4, 1.0, 0.1 + 0.2)


def schedule_its(N):
    return (0, 1, N - 1, N, N + 5, 2 ** 32 - 1)


def weighted_sum(p):
    return int((np.arange(p.shape[0], dtype=np.uint64) * p.astype(np.uint64)).sum() % 2 ** 32)


def chi2_z(counts, expected, dof):
    """z = (chi^2 - dof) / sqrt(2 dof) of a table of counts against one expected count per cell."""
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    return (chi2 - dof) / np.sqrt(2.0 * dof)


def uniformity_z(perms):
    """``perms``: int64 [E, B].  (z of the B x B position-by-value counts, z of the B (B - 1) ordered adjacent pairs
    (perm[i], perm[i + 1])), each against its uniform expectation E / B per cell.  Degrees of freedom: the position
    table has every row and column sum fixed at E, so (B - 1)^2; the pairs' table is one multinomial of E (B - 1)
    draws over B (B - 1) cells with only the total fixed, so B (B - 1) - 1."""
    E, B = perms.shape
    pos = np.zeros((B, B))
    np.add.at(pos, (np.broadcast_to(np.arange(B), (E, B)), perms), 1)
    adj = np.zeros((B, B))
    np.add.at(adj, (perms[:, :-1], perms[:, 1:]), 1)
    off = ~np.eye(B, dtype=bool)           # a value never follows itself: B (B - 1) ordered pairs
    return chi2_z(pos, E / B, (B - 1) ** 2), chi2_z(adj[off], E / B, B * (B - 1) - 1)
