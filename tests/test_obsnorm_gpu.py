"""Running observation normalisation on the device (include/pbg.h "Running observation normalisation",
policy.py ObsStats, es.py obs_norm=True): the stand-alone update and finalize against a numpy restatement
that loops over calls, tile rows and slots in the stated order, the two device actors with a normaliser
against the host policy bit for bit, statistics collected inside rollouts against the restatement applied to
the recorded trajectories, and the evolution strategy under normalisation.

Every float64 sum is compared bitwise: the restatement does the same adds in the same order (the square of
a float32 is exact in float64, so it does not matter whether the device contracts it into the add)."""
import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.es import EvolutionStrategy
from pybulletgym_amd.policy import MLPPolicy, MLPPopulation, ObsStats, pack_theta
from pybulletgym_amd.vec_env import VecEnv

import policies
import policy_data as pd
from test_obsnorm_host import make_norm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ANT = (28, 128, 64, 8)
GUARD = 64
PT = 16  # rows per tile
FIELDS = ("obs", "cur_return", "cur_length", "done_return", "done_length", "done_episodes", "obs_traj", "act_traj",
          "rew_traj", "done_traj")


class Restated:
    """pbg_obs_stats in numpy: the same adds in the same order, vectorised over the components only."""

    def __init__(self, K, n_slots):
        self.K, self.n_slots = K, n_slots
        self.count = np.float64(1e-2)
        self.sum = np.zeros(K, np.float64)
        self.sumsq = np.full(K, 1e-2, np.float64)
        self._zero_slots()

    def _zero_slots(self):
        self.slot_count = np.zeros(self.n_slots, np.int64)
        self.slot_sum = np.zeros((self.n_slots, self.K), np.float64)
        self.slot_sumsq = np.zeros((self.n_slots, self.K), np.float64)

    def update(self, obs, active, G):
        n = obs.shape[0]
        G = G or n
        tpm = (G + PT - 1) // PT
        for m in range(n // G):
            for t in range(tpm):
                slot = m * tpm + t
                for r in range(min(PT, G - t * PT)):     # the tile's rows, ascending
                    e = m * G + t * PT + r
                    if active[e] and np.isfinite(obs[e]).all():
                        x = obs[e].astype(np.float64)
                        self.slot_sum[slot] = self.slot_sum[slot] + x
                        self.slot_sumsq[slot] = self.slot_sumsq[slot] + x * x
                        self.slot_count[slot] += 1

    def finalize(self):
        for s in range(self.n_slots):                    # slot ascending
            self.sum = self.sum + self.slot_sum[s]
            self.sumsq = self.sumsq + self.slot_sumsq[s]
        self.count = self.count + np.float64(int(self.slot_count.sum()))
        self._zero_slots()
        m = self.sum / self.count
        var = np.maximum(self.sumsq / self.count - m * m, 1e-2)
        return m.astype(np.float32), 1.0 / np.sqrt(var)  # inv_std still in float64

    def totals(self):
        return np.concatenate([[self.count], self.sum, self.sumsq])


def _same_totals(stats, ref):
    got = stats.totals.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (1 + 2 * ref.K,)
    assert np.array_equal(got.view(np.uint64), ref.totals().view(np.uint64)), (got[0], ref.count)


def _check_outputs(mean, inv_std, want_mean, want_inv64):
    mean, inv_std = mean.cpu().numpy(), inv_std.cpu().numpy()
    assert mean.dtype == np.float32 and inv_std.dtype == np.float32
    assert np.array_equal(mean, want_mean)
    # the kernel spells the formula uncontracted, and float64 division and sqrt are correctly rounded on both
    # sides, so numpy reproduces it exactly (include/pbg.h would allow the final float32 rounding to differ:
    # the cancellation in sumsq / count - m m is amplified by at most (second moment) / 1e-2 <= 1e8 float64 ulps,
    # far below a float32 ulp)
    want = want_inv64.astype(np.float32)
    ulps = np.abs(inv_std.astype(np.float64) - want_inv64) / np.spacing(want).astype(np.float64)
    print(f"inv_std: max distance from the float64 formula {ulps.max():.3f} float32 ulps")
    assert np.array_equal(inv_std, want), ulps.max()
    assert (inv_std <= 10.0).all() and (inv_std > 0.0).all()


def _synthetic(rng, n, K, call):
    """Magnitudes 1e-3 .. 1e3 of either sign, a NaN row and an inf row (for one row: in calls 1 and 2)."""
    obs = (rng.choice([-1.0, 1.0], (n, K)) * 10.0 ** rng.uniform(-3.0, 3.0, (n, K))).astype(np.float32)
    if n >= 2:
        obs[call % n, call % K] = np.nan
        obs[(call + 1) % n, :] = np.inf if call != 1 else -np.inf
        if n >= 3:
            obs[(call + 2) % n, (call + 1) % K] = np.inf   # one inf component is enough
    elif call == 1:
        obs[0, 0] = np.nan
    elif call == 2:
        obs[0, K - 1] = -np.inf
    active = None if call == 0 else (rng.random(n) < 0.7).astype(np.uint8)
    return obs, active


UPDATE_SHAPES = [(n, g) for n in (1, 16, 17, 33, 85) for g in (0, 1, 5, 16, 17) if g == 0 or n % g == 0]


@pytest.mark.parametrize("K", [1, 5, 28, 256])
def test_update_and_finalize_equal_the_restatement(K):
    """n around the 16-row tile (85 = 5 x 17 so that groups of 5 and of 17 occur), every group size that
    divides n; three updates, finalize, a second round, and a finalize with nothing accumulated."""
    assert {g for _, g in UPDATE_SHAPES} == {0, 1, 5, 16, 17}
    for n, group in UPDATE_SHAPES:
        rng = np.random.default_rng([K, n, group])
        stats = ObsStats(K, n, group=group or None, device=DEV)
        G = group or n
        assert stats.n_slots == (n // G) * ((G + PT - 1) // PT)
        ref = Restated(K, stats.n_slots)
        _same_totals(stats, ref)   # RunningStat(eps = 1e-2)
        for rnd in range(2):
            for call in range(3):
                obs, active = _synthetic(rng, n, K, call)
                ref.update(obs, np.ones(n, bool) if active is None else active, group)
                stats.update(torch.from_numpy(obs).to(DEV), None if active is None else torch.from_numpy(active).to(DEV))
            before = stats.totals.cpu().numpy()
            assert rnd == 1 or before[0] == 1e-2  # the slots are not in the totals before finalize
            mean, inv_std = stats.finalize()
            want_mean, want_inv = ref.finalize()
            _same_totals(stats, ref)
            _check_outputs(mean, inv_std, want_mean, want_inv)
        assert n < 3 or ref.count > 1.0
        first = (mean.clone(), inv_std.clone(), stats.totals.clone())
        mean, inv_std = stats.finalize()   # nothing accumulated: the slots were cleared
        for a, b in zip(first, (mean, inv_std, stats.totals)):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
        # the totals can be assigned (resuming, merging)
        other = ObsStats(K, n, group=group or None, device=DEV)
        other.totals = stats.totals
        _same_totals(other, ref)
        m2, s2 = other.finalize()
        assert np.array_equal(m2.cpu().numpy(), mean.cpu().numpy()) and np.array_equal(s2.cpu().numpy(), inv_std.cpu().numpy())
        other.close()
        stats.close()


def test_update_argument_errors():
    K = 5
    small = ObsStats(K, 16, device=DEV)   # one slot
    obs = torch.zeros((17, K), device=DEV)
    with pytest.raises(_native.PbgError):  # 17 rows are two tiles
        small.update(obs)
    small.update(obs[:16])
    small.update(obs[:3])
    L = _native.lib()
    assert L.pbg_obs_stats_update(small._h, 15, 4, obs.data_ptr(), None, None) == -1   # n no multiple of group
    assert b"multiple" in L.pbg_last_error()
    assert L.pbg_obs_stats_update(small._h, 16, 8, obs.data_ptr(), None, None) == -1   # two groups, two slots
    assert b"slots" in L.pbg_last_error()
    grouped = ObsStats(K, 32, group=16, device=DEV)
    with pytest.raises(_native.PbgError):
        grouped.update(obs)                # 17 is no multiple of 16
    with pytest.raises(_native.PbgError):
        grouped.update(torch.zeros((48, K), device=DEV))
    for bad in (obs[:16].double(), obs[:16].cpu(), torch.zeros((16, K + 1), device=DEV), torch.zeros((K, 16), device=DEV).T):
        with pytest.raises(_native.PbgError):
            small.update(bad)
    for bad in (torch.ones(16, device=DEV), torch.ones(15, dtype=torch.uint8, device=DEV), torch.ones(16, dtype=torch.uint8)):
        with pytest.raises(_native.PbgError):
            small.update(obs[:16], bad)
    with pytest.raises(_native.PbgError):
        ObsStats(K, 30, group=4, device=DEV)
    with pytest.raises(_native.PbgError):
        small.totals = torch.zeros(2 * K, dtype=torch.float64)
    small.close()
    grouped.close()
    with pytest.raises(_native.PbgError):
        small.update(obs[:16])


# ---------------------------------------------------------------------------- actors with a normaliser
def _bad_rows(obs):
    n = obs.shape[0]
    if n >= 3:
        obs[n // 2, 1 % obs.shape[1]] = np.nan
        obs[n - 1, :] = np.inf
    return obs


@pytest.mark.parametrize("dims", [(7, 33, 17, 3), ANT], ids=str)
def test_device_actors_with_a_normaliser_equal_the_host_policy(dims):
    mean, inv_std = make_norm(dims[0])
    pattern = -12345.5
    # the shared-weight actor
    ws = pd.synthetic_weights(dims)
    host = MLPPolicy(*ws, obs_norm=(mean, inv_std, 5.0))
    dev = MLPPolicy(*ws, device=DEV, obs_norm=(mean, inv_std, 5.0))
    for n in (1, 17, 33):
        obs = _bad_rows((3.0 * pd.seeded_obs(dims[0], n, seed=n)).astype(np.float32))
        want = host.act(obs)
        buf = torch.full((GUARD + n + GUARD, dims[3]), pattern, dtype=torch.float32, device=DEV)
        dev.act(torch.from_numpy(obs).to(DEV), out=buf[GUARD:GUARD + n])
        b = buf.cpu().numpy()
        assert np.array_equal(b[GUARD:GUARD + n], want, equal_nan=True), (dims, n)
        assert (b[:GUARD] == pattern).all() and (b[GUARD + n:] == pattern).all(), (dims, n)
    plain = MLPPolicy(*ws)
    obs = pd.seeded_obs(dims[0], 33, seed=2)
    assert not np.array_equal(dev.act(torch.from_numpy(obs).to(DEV)).cpu().numpy(), plain.act(obs))
    dev.set_obs_norm(None)   # off: today's bits
    assert np.array_equal(dev.act(torch.from_numpy(obs).to(DEV)).cpu().numpy(), plain.act(obs))
    for p in (host, dev, plain):
        p.close()
    # the population actor
    pop = MLPPopulation(dims, 3, DEV)
    pop.perturb(torch.from_numpy(pack_theta(ws)).to(DEV), 0.5, 77, 0)
    assert pop.obs_norm is None
    pop.set_obs_norm(torch.from_numpy(mean).to(DEV), torch.from_numpy(inv_std).to(DEV), clip=2.0)
    assert pop.obs_norm[2] == 2.0 and np.array_equal(pop.obs_norm[0].cpu().numpy(), mean)
    P = pop.n_members
    hosts = [MLPPolicy(*pop.member_weights(m), obs_norm=(mean, inv_std, 2.0)) for m in range(P)]
    for G in (1, 5, 16, 17):
        n = P * G
        obs = _bad_rows((3.0 * pd.seeded_obs(dims[0], n, seed=G)).astype(np.float32))
        want = np.concatenate([hosts[m].act(obs[m * G:(m + 1) * G]) for m in range(P)])
        buf = torch.full((GUARD + n + GUARD, dims[3]), pattern, dtype=torch.float32, device=DEV)
        pop.act(torch.from_numpy(obs).to(DEV), out=buf[GUARD:GUARD + n])
        b = buf.cpu().numpy()
        assert np.array_equal(b[GUARD:GUARD + n], want, equal_nan=True), (dims, G)
        assert (b[:GUARD] == pattern).all() and (b[GUARD + n:] == pattern).all(), (dims, G)
    obs = pd.seeded_obs(dims[0], P * 5, seed=3)
    with_norm = pop.act(torch.from_numpy(obs).to(DEV)).cpu().numpy()
    pop.set_obs_norm(None)
    off = pop.act(torch.from_numpy(obs).to(DEV)).cpu().numpy()
    raw = [MLPPolicy(*pop.member_weights(m)) for m in range(P)]
    assert np.array_equal(off, np.concatenate([raw[m].act(obs[m * 5:(m + 1) * 5]) for m in range(P)]))
    assert not np.array_equal(off, with_norm)
    for bad in ((torch.zeros(dims[0]), torch.ones(dims[0])), (torch.zeros(dims[0] + 1, device=DEV), torch.ones(dims[0] + 1, device=DEV)),
                (torch.zeros(dims[0], device=DEV).double(), torch.ones(dims[0], device=DEV).double())):
        with pytest.raises(_native.PbgError):
            pop.set_obs_norm(*bad)
    with pytest.raises(_native.PbgError):
        pop.set_obs_norm(torch.zeros(dims[0], device=DEV), torch.ones(dims[0], device=DEV), clip=0.0)
    for h in hosts + raw:
        h.close()
    pop.close()


# ---------------------------------------------------------------------------- rollouts that collect
def _make(env_id, n, autoreset):
    env = VecEnv(env_id, n, device=DEV, seed=0, autoreset=autoreset, precision=64)
    q0 = policies.reset_draws(n, env.info.reset_dofs, 0).astype(np.float32)
    env.reset(init_q=torch.from_numpy(q0))
    return env


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_fields(res, want, fields=FIELDS):
    for f in fields:
        g, w = _bits(getattr(res, f)), _bits(want[f])
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), f


def _restate_rollout(ref, res, autoreset, G):
    """The restatement on a recorded rollout: a row is active while its action is booked, i.e. always under
    autoreset and otherwise until the env's first done."""
    obs_traj, done_traj = res["obs_traj"].cpu().numpy(), res["done_traj"].cpu().numpy()
    T, n = done_traj.shape
    alive = np.ones(n, bool)
    booked = 0
    for t in range(T):
        active = np.ones(n, bool) if autoreset else alive.copy()
        ref.update(obs_traj[t], active, G)
        booked += int(active.sum())
        alive &= done_traj[t] == 0
    return booked


def _actor(env_id, kind, norm):
    ws = pd.fixture_weights(policies.POLICY_FILES[env_id])
    if kind == "policy":
        pi = MLPPolicy(*ws, device=DEV)
        if norm is not None:
            pi.set_obs_norm(*norm)
        return pi
    pop = MLPPopulation((ws[0].shape[0], ws[0].shape[1], ws[2].shape[1], ws[4].shape[1]), 4, DEV)   # 8 members
    pop.perturb(torch.from_numpy(pack_theta(ws)).to(DEV), 0.05, 99, 0)
    if norm is not None:
        pop.set_obs_norm(torch.from_numpy(norm[0]).to(DEV), torch.from_numpy(norm[1]).to(DEV), clip=norm[2])
    return pop


CASES = {"humanoid-first-episode": ("HumanoidPyBulletEnv-v0", "policy", 64, 56, False, False),
         "ant-autoreset": ("AntPyBulletEnv-v0", "policy", 64, 20, True, True),
         "ant-population": ("AntPyBulletEnv-v0", "population", 64, 20, True, True)}


@pytest.mark.parametrize("case", list(CASES))
def test_rollout_collects_the_restated_statistics(case):
    """The Humanoid runs its own policy raw (so that, as without statistics, about half the 64 envs fall
    inside the 56 steps and both the counted and the skipped branch run); the Ant cases run under a
    normaliser, so the collecting path's in-place normalisation is compared with the plain path's."""
    env_id, kind, n, steps, autoreset, normed = CASES[case]
    K = 44 if "Humanoid" in env_id else 28
    norm = (make_norm(K)[0] * np.float32(0.1), np.clip(make_norm(K)[1], 0.5, 2.0), 5.0) if normed else None
    actor = _actor(env_id, kind, norm)
    G = n // actor.n_members if kind == "population" else None
    # without statistics
    a = _make(env_id, n, autoreset)
    plain = a.rollout(actor, steps, trajectory=True)
    want = {f: getattr(plain, f).clone() for f in FIELDS}
    a.close()
    # with statistics attached: the same ten fields, and the restated totals
    stats = ObsStats(K, n, group=G, device=DEV)
    actor.attach_obs_stats(stats)
    assert actor.obs_stats is stats
    b = _make(env_id, n, autoreset)
    res = b.rollout(actor, steps, trajectory=True)
    _same_fields(res, want)
    ref = Restated(K, stats.n_slots)
    booked = _restate_rollout(ref, want, autoreset, G or 0)
    mean, inv_std = stats.finalize()
    want_mean, want_inv = ref.finalize()
    _same_totals(stats, ref)
    _check_outputs(mean, inv_std, want_mean, want_inv)
    count = float(stats.totals[0])
    assert booked == int((want["done_length"] + want["cur_length"]).sum())
    assert count - 1e-2 == booked, (count, booked)
    if not autoreset:
        finished = int((want["done_episodes"] > 0).sum())
        assert finished >= 8 and n - finished >= 8 and booked < n * steps, finished
    else:
        assert booked == n * steps
    # plain act calls never collect
    actor.act(b.obs)
    before = stats.totals.clone()
    stats.finalize()
    assert np.array_equal(_bits(before), _bits(stats.totals))
    # a call of `steps` steps equals two of half as many (fields and, after one finalize, totals)
    c = _make(env_id, n, autoreset)
    half = ObsStats(K, n, group=G, device=DEV)
    actor.attach_obs_stats(half)
    c.rollout(actor, steps // 2, trajectory=True)
    two = c.rollout(actor, steps // 2, trajectory=True)
    _same_fields(two, want, FIELDS[:6])
    half.finalize()
    _same_totals(half, ref)
    # detached: nothing moves
    actor.attach_obs_stats(None)
    assert actor.obs_stats is None
    c.rollout(actor, 2)
    half.finalize()
    _same_totals(half, ref)
    for e in (b, c):
        e.close()
    for s in (stats, half):
        s.close()
    actor.close()


def test_collecting_rollout_captures_into_a_graph():
    """rollout + finalize + set_obs_norm capture as a plain chain; the replay equals the eager run."""
    env_id, n, steps, K = "AntPyBulletEnv-v0", 64, 8, 28
    q0 = torch.from_numpy(policies.reset_draws(n, 8, 0).astype(np.float32))

    def prepared():
        pop = _actor(env_id, "population", None)
        stats = ObsStats(K, n, group=n // pop.n_members, device=DEV)
        pop.set_obs_norm(*stats.finalize())
        env = _make(env_id, n, True)
        env.rollout(pop, steps)   # allocates the rollout's buffers (nothing attached yet)
        env.reset(init_q=q0)
        env.reset_rollout()
        pop.attach_obs_stats(stats)
        return env, pop, stats

    def run(env, pop, stats):
        res = env.rollout(pop, steps)
        pop.set_obs_norm(*stats.finalize())
        return res

    env, pop, stats = prepared()
    res = run(env, pop, stats)
    eager = {f: getattr(res, f).clone() for f in FIELDS[:6]}
    eager_totals, eager_norm = stats.totals.clone(), [t.clone() for t in pop.obs_norm[:2]]
    assert float(eager_totals[0]) - 1e-2 == n * steps
    env.close()
    pop.close()
    stats.close()

    env, pop, stats = prepared()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        res = run(env, pop, stats)
    torch.cuda.current_stream(DEV).wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    _same_fields(res, eager, FIELDS[:6])
    assert np.array_equal(_bits(stats.totals), _bits(eager_totals))
    for got, want in zip(pop.obs_norm[:2], eager_norm):
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    env.close()
    pop.close()
    stats.close()


def test_rollout_refuses_statistics_that_do_not_fit():
    env = _make("AntPyBulletEnv-v0", 64, True)
    pi = _actor("AntPyBulletEnv-v0", "policy", None)
    pop = _actor("AntPyBulletEnv-v0", "population", None)
    wrong_dim = ObsStats(44, 64, device=DEV)
    too_few = ObsStats(28, 48, device=DEV)           # 3 slots, the policy's launch has 4 workgroups
    per_env = ObsStats(28, 64, device=DEV)           # 4 slots: enough for the policy, not for 8 members x 1 tile
    for actor, bad in ((pi, wrong_dim), (pi, too_few), (pop, wrong_dim), (pop, per_env)):
        actor.attach_obs_stats(bad)
        with pytest.raises(_native.PbgError):
            env.rollout(actor, 2)
        assert b"obs stats" in _native.lib().pbg_last_error()
        actor.attach_obs_stats(None)
        env.rollout(actor, 2)
    pi.attach_obs_stats(per_env)
    env.rollout(pi, 3, fresh=True)
    per_env.finalize()
    assert float(per_env.totals[0]) - 1e-2 == 192
    pi.attach_obs_stats(None)
    for s in (wrong_dim, too_few, per_env):
        s.close()
    with pytest.raises(_native.PbgError):
        pi.attach_obs_stats(per_env)   # closed
    pi.close()
    pop.close()
    env.close()


# ---------------------------------------------------------------------------- evolution strategy
def test_a_generation_under_normalisation_is_its_restatement():
    """AntPyBulletEnv-v0, 4 pairs x 8 envs: EvolutionStrategy(obs_norm=True).step() twice against the same
    generations spelled out (perturb -> rollout with statistics -> finalize -> set_obs_norm -> fitness ->
    ranks -> grad -> theta), bitwise in theta, mean and inv_std; generation 0 acts under (mean 0, inv_std 1),
    generation 1 under generation 0's statistics: every member's recorded actions are its host policy's
    with that normaliser."""
    env_id, n_pairs, G, steps, sigma, lr, seed = "AntPyBulletEnv-v0", 4, 8, 20, 0.1, 0.05, 3
    n, P = 2 * n_pairs * G, 2 * n_pairs
    q0 = policies.reset_draws(n, 8, 0).astype(np.float32)

    env = VecEnv(env_id, n, device=DEV, seed=0, autoreset=True, precision=64)
    pop = MLPPopulation(ANT, n_pairs, DEV)
    es = EvolutionStrategy(env, pop, sigma=sigma, lr=lr, steps=steps, seed=seed, init_q=q0, obs_norm=True, obs_clip=5.0)
    assert np.array_equal(pop.obs_norm[0].cpu().numpy(), np.zeros(28, np.float32))
    assert np.array_equal(pop.obs_norm[1].cpu().numpy(), np.ones(28, np.float32)) and pop.obs_norm[2] == 5.0

    env2 = VecEnv(env_id, n, device=DEV, seed=0, autoreset=True, precision=64)
    pop2 = MLPPopulation(ANT, n_pairs, DEV)
    stats2 = ObsStats(28, n, group=G, device=DEV)
    norm = [t.clone() for t in stats2.finalize()]
    pop2.set_obs_norm(*norm, clip=5.0)
    theta2 = pop2.init_theta(seed)
    centred = torch.arange(P, dtype=torch.float32, device=DEV) / (P - 1) - 0.5
    q0_d = torch.from_numpy(q0).to(DEV)
    for gen in range(2):
        es.step()
        env2.reset(init_q=q0_d)
        pop2.perturb(theta2, sigma, seed, gen)
        pop2.attach_obs_stats(stats2)
        res = env2.rollout(pop2, steps, trajectory=True, fresh=True)
        pop2.attach_obs_stats(None)
        # this generation's actions: each member's host policy under the normaliser in force
        obs0, act0 = res.obs_traj[0].cpu().numpy(), res.act_traj[0].cpu().numpy()
        used = (norm[0].cpu().numpy(), norm[1].cpu().numpy(), 5.0)
        for m in range(P):
            host = MLPPolicy(*pop2.member_weights(m), obs_norm=used)
            assert np.array_equal(host.act(obs0[m * G:(m + 1) * G]), act0[m * G:(m + 1) * G]), (gen, m)
            host.close()
        norm = [t.clone() for t in stats2.finalize()]
        pop2.set_obs_norm(*norm, clip=5.0)
        fit = pop2.fitness(res)
        ranks = torch.zeros(P, dtype=torch.float32, device=DEV)
        ranks[torch.argsort(fit, stable=True)] = centred
        g = pop2.grad((ranks[0::2] - ranks[1::2]).contiguous(), seed, gen)
        theta2.add_(g, alpha=lr / (n_pairs * sigma))
        assert np.array_equal(es.fitness.cpu().numpy(), fit.cpu().numpy())
        assert np.array_equal(es.theta.cpu().numpy(), theta2.cpu().numpy()), gen
        assert np.array_equal(es.obs_stats.mean.cpu().numpy(), norm[0].cpu().numpy()), gen
        assert np.array_equal(es.obs_stats.inv_std.cpu().numpy(), norm[1].cpu().numpy()), gen
        assert np.array_equal(pop.obs_norm[0].cpu().numpy(), norm[0].cpu().numpy())
        assert np.array_equal(_bits(es.obs_stats.totals), _bits(stats2.totals))
        assert float(stats2.totals[0]) - 1e-2 == (gen + 1) * n * steps
    assert np.abs(norm[0].cpu().numpy()).max() > 0.05 and not np.array_equal(norm[1].cpu().numpy(), np.ones(28, np.float32))
    # evaluating does not move the statistics
    before = es.obs_stats.totals.clone()
    es.evaluate()
    es.obs_stats.finalize()
    assert np.array_equal(_bits(before), _bits(es.obs_stats.totals))
    for e in (env, env2):
        e.close()
    for p in (pop, pop2):
        p.close()
    stats2.close()


def _train(generations):
    """test_population_gpu.py's pendulum training, with obs_norm=True."""
    env_id, n_pairs, G, steps = "InvertedPendulumPyBulletEnv-v0", 32, 4, 200
    n = 2 * n_pairs * G
    env = VecEnv(env_id, n, device=DEV, seed=0, autoreset=False, precision=64)
    pop = MLPPopulation((5, 16, 8, 1), n_pairs, DEV)
    q0 = policies.reset_draws(n, env.info.reset_dofs, 0).astype(np.float32)
    es = EvolutionStrategy(env, pop, sigma=0.1, lr=0.2, steps=steps, seed=0, init_q=q0, obs_norm=True)
    before = es.evaluate()[1].cpu().numpy().astype(np.float64)
    for _ in range(generations):
        es.step()
    after = es.evaluate()[1].cpu().numpy().astype(np.float64)
    theta = es.theta.cpu().numpy().copy()
    totals = es.obs_stats.totals.cpu().numpy().copy()
    env.close()
    pop.close()
    return before, after, theta, totals


def test_evolution_strategy_with_normalisation_learns_to_balance_the_pendulum():
    """test_population_gpu.py's training and bar, with obs_norm=True: 32 mirrored pairs x 4 envs, MLP
    5 -> 16 -> 8 -> 1 from init_theta(0), sigma 0.1, lr 0.2, 200-step first-episode rollouts, 60 generations;
    the centre's mean first-episode length must reach 150 of 200 and exceed the untrained centre's by more than
    three of its across-env standard deviations.  A second run gives the same theta and totals bit for bit."""
    before, after, theta, totals = _train(60)
    print(f"untrained centre: mean first-episode length {before.mean():.2f} (std {before.std():.2f}); "
          f"after 60 generations with observation normalisation: {after.mean():.2f} (std {after.std():.2f}) of 200; "
          f"{totals[0] - 1e-2:.0f} observations counted")
    assert after.mean() >= 150.0
    assert after.mean() > before.mean() + 3.0 * before.std()
    before2, after2, theta2, totals2 = _train(60)
    assert np.array_equal(theta, theta2)
    assert np.array_equal(totals.view(np.uint64), totals2.view(np.uint64))
    assert np.array_equal(before, before2) and np.array_equal(after, after2)
