"""distributed.gather_traj over gloo on CPU tensors (world 2 and 3): every rank's [T, n_rank, C] shard lands at its
global columns of one [T, n, C] array on every rank, one collective per call; uneven shards are refused, by gather_traj
and by ShardedPPO."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import distributed as pd
from pybulletgym_amd import _native

SHAPES = [(T, C) for T in (1, 5) for C in (1, 7)]


def known(T, n, C):
    """Element (t, e, c) = 1e4 t + 10 e + c, exact in float32."""
    t, e, c = np.meshgrid(np.arange(T), np.arange(n), np.arange(C), indexing="ij")
    return (1e4 * t + 10 * e + c).astype(np.float32)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pybulletgym_amd.ppo import ShardedPPO
    n = 6 * world
    out = {}
    for T, C in SHAPES:
        whole = known(T, n, C)
        off, cnt = pd.shard_range(n, rank, world)
        # a strided view: the shard as it lies inside a larger trajectory
        local = torch.from_numpy(whole)[:, off:off + cnt]
        got = pd.gather_traj(local, n)
        out[(T, C)] = (tuple(got.shape), got.is_contiguous(), bool(np.array_equal(got.numpy(), whole)))
    refused = []
    for bad_local, bad_global in ((torch.zeros((2, 6, 3)), n + 1), (torch.zeros((2, 6 + (rank == 0), 3)), n)):
        # n + 1 envs: no multiple of the world; then rank 0 a row longer than its equal share of n
        try:
            if bad_global == n and rank != 0:
                raise ValueError("this rank's shard is the equal one: only rank 0 can tell")
            pd.gather_traj(bad_local, bad_global)
            refused.append(False)
        except ValueError:
            refused.append(True)
    try:
        ShardedPPO(types.SimpleNamespace(num_global=2 * world + 1, world=world, rank=rank, env=None))
        refused.append(False)
    except _native.PbgError as e:
        refused.append("no multiple of world" in str(e))
    q.put((rank, out, refused))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 3])
def test_gather_traj_places_every_shard_at_its_global_columns(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        results = [q.get(timeout=60) for _ in range(world)]
    finally:
        for p in procs:
            p.join(timeout=30)
        for p in procs:
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert sorted(r for r, _, _ in results) == list(range(world))
    for rank, out, refused in results:
        for T, C in SHAPES:
            assert out[(T, C)] == ((T, 6 * world, C), True, True), (rank, T, C, out[(T, C)])
        assert refused == [True, True, True], (rank, refused)

