"""ppo.ShardedPPO over several processes (tests/test_sharding_gpu.py's pattern: fresh spawned children, gloo, every rank
on cuda:0): after each of two iterations every rank holds the bits of the one-process
PPO(backward="hip", optimizer="hip", permutation="device") on VecEnv(n_global) -- parameters, Adam's moments and step
count, the noise / permutation / iteration counters and, with obs_norm, the statistics' totals and the normaliser --
and the ranks' env states, concatenated in rank order, are the one-process env's."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pybulletgym_amd  # noqa: F401

from poison import assert_same_bits

pytestmark = pytest.mark.gpu

ENV, DEV, ITERATIONS = "InvertedPendulumPyBulletEnv-v0", "cuda:0", 2
HP = dict(hidden=(16, 8), steps=8, epochs=2, seed=3, lr=3e-3, lr_schedule="linear", schedule_iterations=5)
# (world, global envs, minibatches, the ranks' workgroups of G); the last: 272 rows a minibatch, G = 17 cut 9 / 8, an odd
# share of an odd Dtot (483), so rank 1's gathered block lies at an odd multiple of 4 bytes before its padding
W2, W3, W2_ODD = (2, 128, 4, (8, 8)), (3, 96, 3, (6, 5, 5)), (2, 68, 2, (9, 8))


def snapshot(ppo, env):
    """What a trainer and its env hold, as numpy: a synchronising read."""
    m, v, t = ppo.adam.state()
    out = dict(actor=ppo.actor_theta.data, critic=ppo.critic_theta.data, log_std=ppo.log_std.data, adam_t=t, it=ppo._it_dev)
    out.update({f"m{i}": a for i, a in enumerate(m)}, **{f"v{i}": a for i, a in enumerate(v)})
    if ppo.obs_stats is not None:
        out.update(totals=ppo.obs_stats.totals, mean=ppo.actor.obs_norm[0], inv_std=ppo.actor.obs_norm[1])
    phys, aux = env.get_state()
    out.update(env_phys=phys, env_aux=aux)
    out = {k: a.detach().cpu().numpy().copy() for k, a in out.items()}
    out["counters"] = np.array([ppo.noise.counter, ppo.perm.counter, ppo.iteration], np.int64)
    return out


def _worker(rank, world, port, n_global, minibatches, obs_norm, grad_path, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pybulletgym_amd.distributed import ShardedVecEnv
    from pybulletgym_amd.ppo import ShardedPPO
    shard = ShardedVecEnv(ENV, n_global, rank, world, device=DEV, seed=3, autoreset=True, precision=64)
    ppo = ShardedPPO(shard, minibatches=minibatches, obs_norm=obs_norm, grad_path=grad_path, **HP)
    snaps = []
    for _ in range(ITERATIONS):
        ppo.iterate()
        snaps.append(snapshot(ppo, shard.env))
    q.put((rank, (ppo._G, ppo._wg0, ppo._wgn), snaps))
    dist.barrier()
    ppo.close()
    shard.env.close()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("case,obs_norm,grad_path", [(W2, False, "fma"), (W2, True, "fma"), (W3, False, "fma"), (W3, True, "fma"),
                                                     (W2, True, "mfma"), (W2_ODD, False, "fma")],
                         ids=("w2-raw", "w2-obs_norm", "w3-raw", "w3-obs_norm", "w2-obs_norm-mfma", "w2-odd-share"))
def test_every_rank_holds_the_one_process_trainers_bits(case, obs_norm, grad_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pybulletgym_amd.ppo import PPO
    from pybulletgym_amd.vec_env import VecEnv
    world, n_global, minibatches, wgs = case
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_global, minibatches, obs_norm, grad_path, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        # the one-process trainer, while the children start
        env = VecEnv(ENV, n_global, device=DEV, seed=3, autoreset=True, precision=64)
        one = PPO(env, backward="hip", optimizer="hip", permutation="device", minibatches=minibatches, obs_norm=obs_norm,
                  grad_path=grad_path, **HP)
        want = []
        for _ in range(ITERATIONS):
            one.iterate()
            want.append(snapshot(one, env))
        one.close()
        env.close()
        results = sorted((q.get(timeout=100) for _ in range(world)), key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=60)
        for p in procs:
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert [r for r, _, _ in results] == list(range(world))
    at = 0
    for rank, (G, wg0, wgn), _ in results:
        assert (G, wg0, wgn) == (sum(wgs), at, wgs[rank])
        at += wgn
    for it in range(ITERATIONS):
        for rank, _, snaps in results:
            got = snaps[it]
            assert set(got) == set(want[it])
            for k in got:
                if not k.startswith("env_"):
                    assert_same_bits(got[k], want[it][k], f"iteration {it} rank {rank} {k}")
        for k in ("env_phys", "env_aux"):
            assert_same_bits(np.concatenate([snaps[it][k] for _, _, snaps in results]), want[it][k], f"iteration {it} {k}")
        assert list(want[it]["counters"]) == [8 * (it + 1), 2 * (it + 1), it + 1]
    assert np.abs(want[1]["actor"] - want[0]["actor"]).max() > 0.0
