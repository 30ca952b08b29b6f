"""Gaussian action noise on the device (include/pbg.h "Stochastic Gaussian actions", policy.py ActionNoise): the
fill kernel against the host mirror, and rollouts that sample: the recorded actions are mu + std eps on the
device's own bits, eps2 the ascending float64 sum, the bookkeeping the step-by-step loop's, the step counter
advances across calls and graph replays, the noise follows the global env index, and a detached actor computes
what it computed before."""
import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native, rng
from pybulletgym_amd.policy import ActionNoise, MLPPolicy, MLPPopulation, ObsStats, pack_theta, unpack_theta
from pybulletgym_amd.vec_env import VecEnv

import policies
import policy_data as pd
from rollout_checks import check_sampled as _check_sampled, loop_fed as _loop_fed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x1234_5678_9ABC_DEF0
ACT_DIMS = (1, 3, 4, 8, 17, 64)
FIELDS = ("obs", "cur_return", "cur_length", "done_return", "done_length", "done_episodes", "obs_traj", "act_traj",
          "rew_traj", "done_traj")


@pytest.mark.parametrize("act_dim", ACT_DIMS)
def test_fill_within_1e5_of_the_host_mirror(act_dim):
    """1e-5 is the a-priori bound of include/pbg.h's Noise contract (4.5e-6, doubled)."""
    z = ActionNoise(act_dim, SEED, DEV)
    for n in (1, 16, 17, 33):
        for env_offset, step in ((0, 0), (16, 7)):
            buf = torch.full((n + 2, act_dim), -12345.5, dtype=torch.float32, device=DEV)
            got = z.fill(n, env_offset, step, out=buf[1:n + 1])
            assert got.data_ptr() == buf[1].data_ptr()
            b = buf.cpu().numpy()
            want = rng.action_noise(act_dim, SEED, n, env_offset, step)
            err = np.abs(b[1:n + 1].astype(np.float64) - want).max()
            print(f"act_dim {act_dim} n {n} env_offset {env_offset} step {step}: max |device - host| = {err:.3e}")
            assert np.isfinite(b).all() and err <= 1e-5
            assert (b[0] == -12345.5).all() and (b[n + 1] == -12345.5).all()
    assert np.array_equal(z.fill(16, 16, 7).cpu().numpy(), z.fill(32, 0, 7).cpu().numpy()[16:])
    for bad in (torch.empty((4, act_dim + 1), device=DEV), torch.empty((4, act_dim)),
                torch.empty((4, act_dim), device=DEV, dtype=torch.float64)):
        with pytest.raises(_native.PbgError):
            z.fill(4, 0, 0, out=bad)
    with pytest.raises(_native.PbgError):
        z.fill(4, -1, 0)
    z.close()
    with pytest.raises(_native.PbgError):
        z.fill(4, 0, 0)


# ---------------------------------------------------------------------------- rollouts that sample
def _make(env_id, n, autoreset, env_offset=0, rows=None, total=None):
    env = VecEnv(env_id, n, device=DEV, seed=0, autoreset=autoreset, precision=64, env_offset=env_offset)
    q0 = policies.reset_draws(total or n, env.info.reset_dofs, 0).astype(np.float32)
    if rows is not None:
        q0 = q0[rows]
    env.reset(init_q=torch.from_numpy(np.ascontiguousarray(q0)))
    return env


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(res, want, fields=FIELDS):
    for f in fields:
        got = res[f] if isinstance(res, dict) else getattr(res, f)
        assert got is not None, f
        g, w = _bits(got), _bits(want[f])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), f


def _keep(res, fields=FIELDS + ("eps2_traj",)):
    return {f: getattr(res, f).clone() for f in fields if getattr(res, f) is not None}


def _std(act_dim):
    return torch.from_numpy((0.05 + 0.01 * np.arange(act_dim)).astype(np.float32)).to(DEV)  # no exact binary fractions


def _actor(env_id, kind):
    ws = pd.fixture_weights(policies.POLICY_FILES[env_id])
    if kind == "policy":
        return MLPPolicy(*ws, device=DEV)
    pop = MLPPopulation((ws[0].shape[0], ws[0].shape[1], ws[2].shape[1], ws[4].shape[1]), 4, DEV)   # 8 members
    pop.perturb(torch.from_numpy(pack_theta(ws)).to(DEV), 0.05, 99, 0)
    return pop


def _set_norm(actor, K):
    r = np.random.default_rng(K)   # near the identity, so that the pretrained policies still act sensibly
    mean = (0.02 * r.standard_normal(K)).astype(np.float32)
    inv_std = r.uniform(0.9, 1.1, K).astype(np.float32)
    if isinstance(actor, MLPPolicy):
        actor.set_obs_norm(mean, inv_std, 5.0)
    else:
        actor.set_obs_norm(torch.from_numpy(mean).to(DEV), torch.from_numpy(inv_std).to(DEV), clip=5.0)


ROLLOUTS = {"ant": ("AntPyBulletEnv-v0", 64, 20, True), "humanoid": ("HumanoidPyBulletEnv-v0", 64, 56, False)}


@pytest.mark.parametrize("mode", ["plain", "norm", "collect"])
@pytest.mark.parametrize("kind", ["policy", "population"])
@pytest.mark.parametrize("case", list(ROLLOUTS))
def test_rollout_samples_the_stated_actions(case, kind, mode):
    """Ant, 64 envs x 20 steps, auto-reset; Humanoid, 64 envs x 56 steps, first episode (where, without noise,
    about half the envs fall).  A shared-weight policy and an 8-member population; plain, under a normaliser,
    and under a normaliser with statistics attached: the six sampling instantiations, each twice."""
    env_id, n, steps, autoreset = ROLLOUTS[case]
    actor = _actor(env_id, kind)
    K, A = actor.obs_dim, actor.act_dim
    if mode != "plain":
        _set_norm(actor, K)
    stats = None
    if mode == "collect":
        stats = ObsStats(K, n, group=n // actor.n_members if kind == "population" else None, device=DEV)
        actor.attach_obs_stats(stats)
    noise, std, counter0 = ActionNoise(A, SEED, DEV), _std(A), 5
    noise.set_std(std)
    noise.counter = counter0
    actor.attach_action_noise(noise)
    assert actor.action_noise is noise
    env = _make(env_id, n, autoreset)
    res = _keep(env.rollout(actor, steps, trajectory=True))
    assert noise.counter == counter0 + steps
    assert res["eps2_traj"].shape == (steps, n) and res["eps2_traj"].dtype == torch.float64
    _check_sampled(res, actor, noise, std, counter0)
    if stats is not None:
        stats.finalize()
        booked = int((res["done_length"] + res["cur_length"]).sum())
        assert float(stats.totals[0]) - 1e-2 == booked
        actor.attach_obs_stats(None)
    ref = _make(env_id, n, autoreset)
    _same(res, _loop_fed(ref, res["act_traj"]))
    if not autoreset:
        finished = int((res["done_episodes"] > 0).sum())
        print(f"{case} {kind} {mode}: {finished} of {n} envs finished their first episode")
        assert int(res["done_episodes"].max()) <= 1
    for e in (env, ref):
        e.close()
    actor.attach_action_noise(None)
    noise.close()
    actor.close()


def test_logp_traj_is_the_gaussian_log_density():
    env_id, n = "AntPyBulletEnv-v0", 32
    actor = _actor(env_id, "policy")
    noise, std = ActionNoise(8, SEED, DEV), _std(8)
    noise.set_std(std)
    actor.attach_action_noise(noise)
    env = _make(env_id, n, True)
    res = env.rollout(actor, 4, trajectory=True)
    lp = res.logp_traj(std)
    mu = torch.stack([actor.act(res.obs_traj[t].contiguous()) for t in range(4)]).double()
    dist = torch.distributions.Normal(mu, std.double())
    want = dist.log_prob(res.act_traj.double()).sum(-1)
    # the recorded action is mu + std eps rounded to float32: (a - mu) / std differs from eps by a float32
    # rounding of |a| <= ~2 over std >= 0.05, 2^-24 * 2 / 0.05 = 2.4e-6 per component, times |eps| <= 5.77, 8 components
    assert float((lp - want).abs().max()) <= 8 * 5.77 * 2.4e-6
    plain = env.rollout(actor, 4)
    assert plain.eps2_traj is None
    with pytest.raises(_native.PbgError):
        plain.logp_traj(std)
    actor.attach_action_noise(None)
    assert env.rollout(actor, 4, trajectory=True).eps2_traj is None
    env.close()
    noise.close()
    actor.close()


def test_counter_continues_across_calls_and_graph_replays():
    """Two 10-step calls leave what one 20-step call leaves; a captured 10-step rollout replayed twice equals
    two eager calls: the counter lives on the device, so the replay draws fresh noise."""
    env_id, n = "AntPyBulletEnv-v0", 64
    actor = _actor(env_id, "policy")
    noise, std = ActionNoise(8, SEED, DEV), _std(8)
    noise.set_std(std)
    actor.attach_action_noise(noise)

    def prepared(steps):
        """An env whose rollout buffers exist (one call allocates them), back at the seeded start, counter 0."""
        env = _make(env_id, n, True)
        env.rollout(actor, steps, trajectory=True)
        env.reset(init_q=torch.from_numpy(policies.reset_draws(n, env.info.reset_dofs, 0).astype(np.float32)))
        env.reset_rollout()
        noise.counter = 0
        return env

    a = prepared(20)
    whole = _keep(a.rollout(actor, 20, trajectory=True))
    assert noise.counter == 20
    # two eager calls
    b = prepared(10)
    first = _keep(b.rollout(actor, 10, trajectory=True))
    assert noise.counter == 10
    second = _keep(b.rollout(actor, 10, trajectory=True))
    assert noise.counter == 20
    _same(second, whole, FIELDS[:6])
    for f in FIELDS[6:] + ("eps2_traj",):
        assert np.array_equal(_bits(first[f]), _bits(whole[f][:10])), f
        assert np.array_equal(_bits(second[f]), _bits(whole[f][10:])), f
    assert not np.array_equal(_bits(first["eps2_traj"]), _bits(second["eps2_traj"]))
    # a captured call replayed twice
    c = prepared(10)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = c.rollout(actor, 10, trajectory=True)
    torch.cuda.current_stream(DEV).wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    for f in FIELDS[6:] + ("eps2_traj",):
        assert np.array_equal(_bits(getattr(res, f)), _bits(first[f])), f
    assert noise.counter == 10
    graph.replay()
    torch.cuda.synchronize()
    assert noise.counter == 20
    _same(res, second, FIELDS[:6])
    for f in FIELDS[6:] + ("eps2_traj",):
        assert np.array_equal(_bits(getattr(res, f)), _bits(second[f])), f
    for e in (a, b, c):
        e.close()
    actor.attach_action_noise(None)
    noise.close()
    actor.close()


def test_counter_assignment_resumes():
    """From the same start, counter = 7 draws what steps 7.. of a longer run drew: a 3-step call at counter 7
    samples eps(step 7), eps(step 8), eps(step 9)."""
    env_id, n = "AntPyBulletEnv-v0", 32
    actor = _actor(env_id, "policy")
    noise, std = ActionNoise(8, SEED, DEV), _std(8)
    noise.set_std(std)
    noise.counter = 7
    actor.attach_action_noise(noise)
    env = _make(env_id, n, True)
    res = _keep(env.rollout(actor, 3, trajectory=True))
    _check_sampled(res, actor, noise, std, 7)
    noise.counter = 2 ** 32 - 1   # the step count wraps as a uint32
    res = _keep(env.rollout(actor, 2, trajectory=True))
    assert noise.counter == 1
    std64 = std.cpu().numpy().astype(np.float64)
    for t, step in ((0, 2 ** 32 - 1), (1, 0)):
        mu = actor.act(res["obs_traj"][t].contiguous()).cpu().numpy().astype(np.float64)
        eps = noise.fill(n, 0, step).cpu().numpy().astype(np.float64)
        assert np.array_equal(res["act_traj"][t].cpu().numpy(), (mu + std64 * eps).astype(np.float32))
    env.close()
    actor.attach_action_noise(None)
    noise.close()
    actor.close()


@pytest.mark.parametrize("kind", ["policy", "population"])
def test_noise_follows_the_global_env_index(kind):
    """InvertedPendulumPyBulletEnv-v0 (the lane-per-env kernel), auto-reset: a 16-env batch at env_offset 16
    under the same seed reproduces rows 16..31 of a 32-env batch bit for bit, whether the actor is a policy or a
    population of four members that all hold the policy's weights (groups of 8 and of 4 rows per member)."""
    env_id, steps, dims = "InvertedPendulumPyBulletEnv-v0", 30, (5, 16, 8, 1)
    pop = MLPPopulation(dims, 2, DEV)
    theta = pop.init_theta(0)   # section 11's untrained centre: its episodes last about 21 steps, so envs reset
    pop.set_all(theta)
    actor = pop
    if kind == "policy":
        actor = MLPPolicy(*unpack_theta(dims, theta.cpu().numpy()), device=DEV)
        pop.close()
    noise = ActionNoise(dims[3], SEED, DEV)
    std = torch.full((dims[3],), 0.3, dtype=torch.float32, device=DEV)
    noise.set_std(std)
    actor.attach_action_noise(noise)
    whole_env = _make(env_id, 32, True)
    assert whole_env.info.lanes_per_env == 1
    whole = _keep(whole_env.rollout(actor, steps, trajectory=True))
    noise.counter = 0
    part_env = _make(env_id, 16, True, env_offset=16, rows=slice(16, 32), total=32)
    part = _keep(part_env.rollout(actor, steps, trajectory=True))
    _check_sampled(part, actor, noise, std, 0, env_offset=16)
    for f in FIELDS[6:] + ("eps2_traj",):
        assert np.array_equal(_bits(part[f]), _bits(whole[f][:, 16:])), f
    for f in FIELDS[:6]:
        assert np.array_equal(_bits(part[f]), _bits(whole[f][16:])), f
    assert int(whole["done_episodes"].sum()) > 0   # resets happened: the reset draws follow the global index too
    assert not np.array_equal(_bits(whole["eps2_traj"][:, :16]), _bits(whole["eps2_traj"][:, 16:]))
    for e in (whole_env, part_env):
        e.close()
    actor.attach_action_noise(None)
    noise.close()
    actor.close()


@pytest.mark.parametrize("kind", ["policy", "population"])
def test_detached_actor_computes_the_plain_rollout(kind):
    env_id, n, steps = "AntPyBulletEnv-v0", 64, 12
    actor = _actor(env_id, kind)
    a = _make(env_id, n, True)
    plain = _keep(a.rollout(actor, steps, trajectory=True))
    assert "eps2_traj" not in plain
    noise = ActionNoise(8, SEED, DEV)
    noise.set_std(_std(8))
    actor.attach_action_noise(noise)
    b = _make(env_id, n, True)
    sampled = _keep(b.rollout(actor, steps, trajectory=True))
    assert not np.array_equal(_bits(sampled["act_traj"]), _bits(plain["act_traj"]))
    assert np.array_equal(_bits(sampled["obs_traj"][0]), _bits(plain["obs_traj"][0]))
    # std = 0 (a fresh object): mu + 0 eps = mu, the plain actions, with eps2 still recorded
    zero = ActionNoise(8, SEED, DEV)
    actor.attach_action_noise(zero)
    c = _make(env_id, n, True)
    res = _keep(c.rollout(actor, steps, trajectory=True))
    _same(res, plain)
    assert float(res["eps2_traj"].min()) > 0.0
    # plain act never samples
    assert np.array_equal(actor.act(plain["obs_traj"][0].contiguous()).cpu().numpy(), plain["act_traj"][0].cpu().numpy())
    actor.attach_action_noise(None)
    assert actor.action_noise is None
    d = _make(env_id, n, True)
    _same(d.rollout(actor, steps, trajectory=True), plain)
    assert noise.counter == steps and zero.counter == steps
    for e in (a, b, c, d):
        e.close()
    for o in (noise, zero, actor):
        o.close()


def test_rollout_refuses_noise_that_does_not_fit():
    env = _make("AntPyBulletEnv-v0", 32, True)
    pi = _actor("AntPyBulletEnv-v0", "policy")
    pop = _actor("AntPyBulletEnv-v0", "population")
    wrong = ActionNoise(17, SEED, DEV)
    for actor in (pi, pop):
        actor.attach_action_noise(wrong)
        with pytest.raises(_native.PbgError, match="action noise"):
            env.rollout(actor, 2)
        with pytest.raises(_native.PbgError, match="action noise"):
            env.rollout(actor, 2, trajectory=True)
        actor.attach_action_noise(None)
        env.rollout(actor, 2)
    if torch.cuda.device_count() > 1:   # an object on another device than the handle and the actor
        other = ActionNoise(8, SEED, "cuda:1")
        pi.attach_action_noise(other)
        with pytest.raises(_native.PbgError, match="action noise"):
            env.rollout(pi, 2)
        pi.attach_action_noise(None)
        other.close()
    ok = ActionNoise(8, SEED, DEV)
    for bad in (torch.zeros(9, device=DEV), torch.zeros(8), torch.zeros(8, device=DEV, dtype=torch.float64)):
        with pytest.raises(_native.PbgError):
            ok.set_std(bad)
    for bad in (torch.zeros((2, 32), device=DEV), torch.zeros((2, 32), dtype=torch.float64),
                torch.zeros(64, dtype=torch.float64, device=DEV)):
        with pytest.raises(_native.PbgError):
            ok.bind_eps2_traj(bad)
    with pytest.raises(_native.PbgError):
        ActionNoise(65, SEED, DEV)
    with pytest.raises(_native.PbgError):
        ActionNoise(8, SEED, "cpu")
    ok.close()
    with pytest.raises(_native.PbgError):   # closed
        pi.attach_action_noise(ok)
    for o in (wrong, pi, pop, env):
        o.close()
