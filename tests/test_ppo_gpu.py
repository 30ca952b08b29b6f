"""Generalised advantage estimation on the device (include/pbg.h pbg_gae, ppo.gae) against the host loop and the
numpy restatement, bit for bit; and the PPO trainer (ppo.py): its collection half repeats bit for bit, and it
learns to balance the pendulum."""
import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import PPO, gae, mlp_forward
from pybulletgym_amd.policy import MLPPopulation
from pybulletgym_amd.vec_env import VecEnv

import gae_data as gd
import policies

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("n", gd.NS + (257,))
@pytest.mark.parametrize("T", gd.TS)
def test_gae_equals_the_host_loop_and_numpy(T, n):
    """One lane per env: n = 257 needs a second workgroup with one live lane."""
    rew, done, value = gd.case(T, n)
    for lam in (0.95, 0.0, 1.0):
        want = gd.gae_numpy(rew, done, value, 0.99, lam)
        host = gae(rew, done, value, 0.99, lam)
        buf = torch.full((2, T + 2, n), np.nan, dtype=torch.float32, device=DEV)  # a guard row after each output
        got = gae(torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV), torch.from_numpy(value).to(DEV), 0.99, lam,
                  adv=buf[0, :T], ret=buf[1, :T])
        assert got[0].data_ptr() == buf[0].data_ptr()
        b = buf.cpu().numpy()
        for k in (0, 1):
            assert np.array_equal(b[k, :T], host[k]) and np.array_equal(b[k, :T], want[k]), (T, n, lam, k)
            assert np.isnan(b[k, T:]).all()
    fresh = gae(torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV), torch.from_numpy(value).to(DEV), 0.99, 1.0)
    assert np.array_equal(fresh[0].cpu().numpy(), want[0]) and np.array_equal(fresh[1].cpu().numpy(), want[1])


def test_gae_argument_errors():
    rew, done, value = (torch.from_numpy(a).to(DEV) for a in gd.case(2, 4))
    for bad in ((rew.double(), done, value), (rew, done.int(), value), (rew, done, value[:2]), (rew.cpu(), done, value),
                (rew.T.contiguous().T, done, value), (rew, done[:, :3], value)):
        with pytest.raises(_native.PbgError):
            gae(*bad)
    with pytest.raises(_native.PbgError):
        gae(rew, done, value, adv=torch.zeros((2, 5), device=DEV))


def test_torch_forward_is_the_actors_mlp():
    """The update differentiates mlp_forward; the rollout runs the HIP actor.  They are the same function up to
    the summation order: a float32 dot product of at most 64 terms of magnitude <= ~10 differs from the
    k-ascending fma chain by far less than 1e-4."""
    dims = (5, 64, 64, 3)
    pop = MLPPopulation(dims, 1, DEV)
    theta = pop.init_theta(3)
    pop.set_all(theta)
    obs = torch.from_numpy(np.random.default_rng(0).standard_normal((64, 5)).astype(np.float32)).to(DEV)
    mean, inv_std = obs.mean(0).contiguous(), (1.0 / obs.std(0)).contiguous()
    for norm in (None, (mean, inv_std, 1.5)):
        pop.set_obs_norm(*(norm or (None,)))
        assert float((pop.act(obs) - mlp_forward(theta, dims, obs, norm)).abs().max()) <= 1e-4
    pop.close()


# ---------------------------------------------------------------------------- the trainer
ENV_ID, EVAL_N, EVAL_STEPS = "InvertedPendulumPyBulletEnv-v0", 256, 200
HP = dict(hidden=(64, 64), steps=32, lr=3e-3, epochs=4, minibatches=4, log_std=-0.5)
TRAIN_N = 256
# Measured on the MI355X: the mean length is 182 of 200 after 5 iterations (the bar is first
# met there), dips to 174 at 10 and is 200 of 200 from iteration 20 on; 20 is the count the test builds on.
MEASURED = 20


def _trainer(hp=HP, n=TRAIN_N, seed=0):
    env = VecEnv(ENV_ID, n, device=DEV, seed=seed, autoreset=True, precision=64)
    return env, PPO(env, seed=seed, **hp)


def _evaluate(ppo, test):
    """The noise-free mean policy on section 11's 256 fixed initial states: first-episode lengths of 200 steps."""
    q0 = torch.from_numpy(policies.reset_draws(EVAL_N, test.info.reset_dofs, 0).astype(np.float32))
    return ppo.evaluate(test, EVAL_STEPS, init_q=q0)[1].cpu().numpy().astype(np.float64)


def _train(iterations, hp=HP, n=TRAIN_N, seed=0, every=0):
    env, ppo = _trainer(hp, n, seed)
    test = VecEnv(ENV_ID, EVAL_N, device=DEV, seed=0, autoreset=False, precision=64)
    before = _evaluate(ppo, test)
    curve = [(0, before.mean())]
    for it in range(1, iterations + 1):
        ppo.iterate()
        if every and it % every == 0:
            curve.append((it, _evaluate(ppo, test).mean()))
    after = _evaluate(ppo, test)
    ppo.close()
    env.close()
    test.close()
    return before, after, curve


def test_collection_repeats_bit_for_bit():
    """Two fresh trainers: the first iteration's trajectories, eps2, log-probabilities, values, advantages and
    returns are the same bits (the rollout, the critic and the advantage scan have no atomics and no
    host-dependent order); so is the second collection after one detached copy of the parameters, i.e. the
    device step counter moved on by the first."""
    runs = []
    for _ in range(2):
        env, ppo = _trainer(n=64)
        first = {k: v.clone() for k, v in vars(ppo.collect()).items()}
        assert ppo.noise.counter == HP["steps"]
        second = {k: v.clone() for k, v in vars(ppo.collect()).items()}
        assert ppo.noise.counter == 2 * HP["steps"]
        runs.append((first, second))
        ppo.close()
        env.close()
    for a, b in zip(runs[0], runs[1]):
        for k in a:
            x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    first, second = runs[0]
    assert float(first["eps2"].min()) > 0.0 and float(first["adv"].abs().max()) > 0.0
    assert not np.array_equal(first["eps2"].cpu().numpy(), second["eps2"].cpu().numpy())
    std = np.exp(np.float32(HP["log_std"]))
    want = -0.5 * first["eps2"].cpu().numpy() - np.log(np.float64(std)) - 0.5 * np.log(2.0 * np.pi)
    assert np.abs(first["logp"].cpu().numpy() - want).max() <= 1e-6  # std = expf(log_std) on the device: a few float32 ulps


def test_obs_norm_follows_section_12s_schedule():
    """obs_norm=True: iteration 0 acts under the initial totals' normaliser (mean 0, inv_std 1), the statistics
    count exactly the rollout's T n observations (auto-reset: every row is booked), and after the update both
    networks hold the normaliser finalized from them, which the next collection's critic values then use."""
    T, n = HP["steps"], 64
    env = VecEnv(ENV_ID, n, device=DEV, seed=0, autoreset=True, precision=64)
    ppo = PPO(env, seed=0, obs_norm=True, **HP)
    mean0, inv0, clip = ppo.actor.obs_norm
    assert clip == 5.0 and float(mean0.abs().max()) == 0.0 and float((inv0 - 1.0).abs().max()) == 0.0
    b = ppo.collect()
    obs = b.obs.clone()
    assert float(ppo.actor.obs_norm[0].abs().max()) == 0.0   # the update still sees the normaliser of its data
    ppo.update(b)
    ppo._set_norm()
    assert float(ppo.obs_stats.totals[0]) - 1e-2 == T * n
    mean, inv_std, _ = ppo.actor.obs_norm
    want_mean = obs.double().sum((0, 1)) / (T * n + 1e-2)
    assert float((mean.double() - want_mean).abs().max()) <= 1e-6   # float32 rounding of a mean of order one
    assert float(mean.abs().max()) > 0.0 and float(inv_std.min()) > 0.0 and float(inv_std.max()) <= 10.0
    for a, c in zip(ppo.actor.obs_norm[:2], ppo.critic.obs_norm[:2]):
        assert torch.equal(a, c)
    # the critic's device values are the torch forward's under that normaliser
    b2 = ppo.collect()
    v = mlp_forward(ppo.critic_theta.data, ppo.critic_dims, b2.obs.reshape(T * n, -1), ppo.critic.obs_norm).squeeze(1)
    assert float((v - b2.value[:T].reshape(-1)).abs().max()) <= 1e-4
    assert float(ppo.obs_stats.totals[0]) - 1e-2 == T * n   # collect() leaves the new rows in the slots
    ppo.close()
    env.close()


def test_ppo_learns_to_balance_the_pendulum():
    """InvertedPendulumPyBulletEnv-v0, float64, 256 auto-reset training envs x 32 steps per iteration, MLPs
    5 -> 64 -> 64 -> 1, Adam 3e-3, 4 epochs x 4 minibatches.  Evaluation: the noise-free mean policy on section
    11's 256 fixed initial states, first episode, 200 steps.  The bar is section 11's: mean length >= 150 of 200
    and more than three untrained standard deviations above the untrained mean (21.46, std 6.74, for the
    evolution strategy's initial centre).  The run takes the measured iteration count plus half again."""
    assert MEASURED > 0
    before, after, _ = _train(MEASURED + MEASURED // 2)
    print(f"untrained mean policy: mean first-episode length {before.mean():.2f} (std {before.std():.2f}); "
          f"after {MEASURED + MEASURED // 2} iterations: {after.mean():.2f} (std {after.std():.2f}) of 200")
    assert after.mean() >= 150.0
    assert after.mean() > 21.46 + 3.0 * 6.74
    assert after.mean() > before.mean() + 3.0 * before.std()
