"""What the tests of sampling rollouts share (tests/test_actnoise_gpu.py, tests/test_learner_invariance_gpu.py): the
step-by-step loop fed recorded actions, and the check of recorded actions against mu + std eps."""
import numpy as np
import torch


def loop_fed(env, act_traj):
    """The step-by-step loop fed the recorded actions; torch float64 accumulation in include/pbg.h's order."""
    n, kw = env.num_envs, dict(device=env.device)
    cur_return = torch.zeros(n, dtype=torch.float64, **kw)
    done_return = torch.zeros(n, dtype=torch.float64, **kw)
    cur_length = torch.zeros(n, dtype=torch.int32, **kw)
    done_length = torch.zeros(n, dtype=torch.int32, **kw)
    done_episodes = torch.zeros(n, dtype=torch.int32, **kw)
    traj = dict(obs_traj=[], rew_traj=[], done_traj=[])
    for a in act_traj:
        traj["obs_traj"].append(env.obs.clone())
        r = env.step(a.contiguous(), want_reward64=True)
        traj["rew_traj"].append(r.reward.clone())
        traj["done_traj"].append(r.done.clone())
        alive = torch.ones(n, dtype=torch.bool, **kw) if env.autoreset else done_episodes == 0
        cur_return = torch.where(alive, cur_return + env.reward64, cur_return)
        cur_length = cur_length + alive.to(torch.int32)
        fin = alive & (r.done != 0)
        done_return = torch.where(fin, done_return + cur_return, done_return)
        done_length = torch.where(fin, done_length + cur_length, done_length)
        done_episodes = done_episodes + fin.to(torch.int32)
        cur_return = torch.where(fin, torch.zeros_like(cur_return), cur_return)
        cur_length = torch.where(fin, torch.zeros_like(cur_length), cur_length)
    out = dict(obs=env.obs.clone(), cur_return=cur_return, cur_length=cur_length, done_return=done_return,
               done_length=done_length, done_episodes=done_episodes, act_traj=act_traj)
    out.update({k: torch.stack(v) for k, v in traj.items()})
    return out


def check_sampled(res, actor, noise, std, counter0, env_offset=0):
    """act_traj = float32(float64(mu) + float64(std) float64(eps)) with mu the noise-free actor on the recorded
    observations and eps the fill kernel's bits at the matching steps; eps2_traj the ascending float64 sum."""
    T, n, A = res["act_traj"].shape
    std64 = std.cpu().numpy().astype(np.float64)
    for t in range(T):
        mu = actor.act(res["obs_traj"][t].contiguous()).cpu().numpy().astype(np.float64)
        eps = noise.fill(n, env_offset, counter0 + t).cpu().numpy().astype(np.float64)
        want = (mu + std64 * eps).astype(np.float32)  # the product of two float32 values is exact in float64
        assert np.array_equal(res["act_traj"][t].cpu().numpy(), want, equal_nan=True), t
        q = np.zeros(n, np.float64)
        for j in range(A):
            q = q + eps[:, j] * eps[:, j]
        assert np.array_equal(res["eps2_traj"][t].cpu().numpy().view(np.uint64), q.view(np.uint64)), t
        assert (eps != 0.0).any()
