"""The KL gate on the device (include/pbg.h "Value clipping and the KL gate": pbg_ppo_gate, pbg_ppo_gate_reset and the
gate that both paths' tile kernels, the reduction and the optimiser's two launches obey; ppo.KLGate, PPO(target_kl=...),
ShardedPPO): the gated chain of tests/ppo_klgate_data.py against the device's own ungated chain cut at the step that
trips -- eager, on a side stream and as a captured graph replayed twice --, stopped launches that read and write
nothing, and the trainers."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import PPO, AdamClip, KLGate, PPOGrad, ShardedPPO, adv_norm
from pybulletgym_amd.vec_env import VecEnv

import ppo_grad_data as pd
import ppo_klgate_data as kd
import ppo_opt_data as od
from test_ppograd_gpu import DEV, GUARD, Outputs, dev, tensors
from test_ppoopt_gpu import HP, TRAIN_N
from test_sharded_ppo_gpu import _free_port

pytestmark = pytest.mark.gpu

PATHS = ("fma", "mfma")
ENV_ID = "InvertedPendulumPyBulletEnv-v0"


class Chain:
    """The chain of ppo_klgate_data on the device: the batch, the parameters' storage, one PPOGrad and one AdamClip."""

    def __init__(self, path, first_seed=0):
        self.c, self.seed = kd.batch(first_seed)
        self.t = tensors(self.c)
        self.perm = dev(kd.permutations(self.seed))
        self.g = PPOGrad(kd.DIMS, kd.BM, DEV, path=path)
        self.opt = AdamClip(od.sizes_of(kd.DIMS), DEV)
        self.start = [self.t[k].clone() for k in ("theta_actor", "theta_critic", "log_std")]
        self.params = [p.clone() for p in self.start]
        self.grads = [torch.full_like(p, np.nan) for p in self.params]
        self.stats = torch.full((4,), np.nan, dtype=torch.float64, device=DEV)
        self.an = torch.zeros(2, dtype=torch.float32, device=DEV)
        self.gate = KLGate(DEV)

    def rewind(self):
        """The parameters and the optimiser as they were; the gate shut with a count, for the chain's reset to undo."""
        for p, s in zip(self.params, self.start):
            p.copy_(s)
        self.opt.reset()
        self.stats.fill_(np.nan)
        self.gate.gate.copy_(torch.tensor([1, 99], dtype=torch.int32))

    def launches(self, kl_limit=None, record=None):
        """Every launch of the chain on the current stream; ``record``: a list that takes a snapshot after each step
        (clones on the stream)."""
        t, kw = self.t, {}
        if kl_limit is not None:
            self.gate.reset()
            kw = dict(gate=self.gate.gate)
        for e in range(kd.EPOCHS):
            for idx in self.perm[e]:
                adv_norm(t["adv"], idx, out=self.an)
                self.g.run(*self.params, t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"], idx=idx, adv_norm=self.an,
                           clip_eps=pd.CLIP_EPS, vf_coef=pd.VF_COEF, ent_coef=kd.ENT_COEF, grad_actor=self.grads[0],
                           grad_critic=self.grads[1], grad_log_std=self.grads[2], stats=self.stats, **kw)
                if kl_limit is not None:
                    self.gate.check(self.stats, kl_limit)
                self.opt.step(self.params, self.grads, kd.LR, kd.BETAS, kd.EPS, kd.MAX_GRAD_NORM, **kw)
                if record is not None:
                    record.append((self.stats.clone(), self.snapshot()))

    def snapshot(self):
        m, v, t = self.opt.state()
        return [p.clone() for p in self.params] + m + v + [t]

    def close(self):
        self.g.close()
        self.opt.close()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("path", PATHS)
def test_the_gated_chain_is_the_devices_ungated_chain_cut_at_the_step_that_trips(path):
    ch = Chain(path)
    ch.rewind()
    free = []
    ch.launches(record=free)   # the parent's function: no gate anywhere
    kl = torch.stack([s for s, _ in free])[:, 3].cpu().numpy()
    assert int(free[-1][1][-1].item()) == kd.K and np.isfinite(kl).all()
    stops = kd.stops(kl)
    print(f"{path}: batch seed {ch.seed}; kl per step {kl.tolist()}; stops {stops}")
    side = torch.cuda.Stream(DEV)
    for j, limit in stops:
        want_stats, want = free[j][0], free[j - 1][1]

        def check(what):
            assert ch.gate.state.cpu().tolist() == [1, j], (what, j)
            assert _same(ch.snapshot(), want), (what, j)
            assert torch.equal(ch.stats, want_stats), (what, j)
            assert int(want[-1].item()) == j and not _same(ch.params, ch.start)

        ch.rewind()
        ch.launches(limit)
        check("eager")
        ch.rewind()
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            ch.launches(limit)
        torch.cuda.current_stream(DEV).wait_stream(side)
        check("side stream")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ch.launches(limit)
        for replay in range(2):
            ch.rewind()
            graph.replay()
            check(f"replay {replay}")
        del graph
    # a limit nothing reaches: every step applied and counted, the ungated chain's bits
    ch.rewind()
    ch.launches(1e9)
    assert ch.gate.state.cpu().tolist() == [0, kd.K] and _same(ch.snapshot(), free[-1][1]) and torch.equal(ch.stats, free[-1][0])
    ch.close()


@pytest.mark.parametrize("path", PATHS)
def test_stopped_launches_read_and_write_nothing(path):
    """gate[0] = 1: the parameters and the observations are NaN, idx is in range but not the case's, every output is
    NaN-filled between guards: after run, run_part and reduce all of them still are, and a stopped optimiser step leaves
    the parameters, the moments, the step count and info."""
    dims, B, Bm, seed = pd.CASES[3]
    c = pd.case(dims, B, Bm, seed, True)
    g, t = PPOGrad(dims, Bm, DEV, path=path), tensors(c)
    shut = torch.tensor([1, 5], dtype=torch.int32, device=DEV)
    nan = lambda x: torch.full_like(x, np.nan)  # noqa: E731
    idx = torch.arange(Bm, device=DEV).flip(0).contiguous()
    args = (nan(t["theta_actor"]), nan(t["theta_critic"]), nan(t["log_std"]), nan(t["obs"]), t["act"], t["logp_old"], t["adv"],
            t["ret"])
    kw = dict(idx=idx, adv_norm=t["adv_norm"], obs_norm=(t["mean"], t["inv_std"], c["clip"]), clip_eps=pd.CLIP_EPS,
              vf_coef=pd.VF_COEF, ent_coef=0.01, gate=shut)
    out = Outputs(g, Bm)
    G, dtot = g.geometry(Bm)
    part = torch.full((G * dtot + GUARD,), np.nan, dtype=torch.float32, device=DEV)
    part_stats = torch.full((G * 4 + GUARD,), np.nan, dtype=torch.float64, device=DEV)
    pv, sv = part[:G * dtot].view(G, dtot), part_stats[:G * 4].view(G, 4)
    g.run(*args, **kw, **out.kw)
    g.run_part(*args, 0, G, pv, sv, **kw, logp_out=out.kw["logp_out"], v_out=out.kw["v_out"])
    g.reduce(*args, G, pv, sv, **kw, **out.kw)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(x).all()) for x in list(out.full.values()) + [part, part_stats])
    assert shut.cpu().tolist() == [1, 5]
    # an open gate writes every output (the inputs are the case's again)
    open_, ref = Outputs(g, Bm), Outputs(g, Bm)
    args = tuple(t[k] for k in ("theta_actor", "theta_critic", "log_std", "obs", "act", "logp_old", "adv", "ret"))
    g.run(*args, **dict(kw, gate=torch.zeros(2, dtype=torch.int32, device=DEV)), **open_.kw)
    g.run(*args, **dict(kw, gate=None), **ref.kw)
    a, b = open_.numpy(), ref.numpy()
    assert all(np.isfinite(a[k]).all() and a[k].tobytes() == b[k].tobytes() for k in a)
    g.close()

    sizes = od.SIZES[3]
    opt = AdamClip(sizes, DEV)
    p = [dev(a) for a in od.params0(sizes)]
    opt.step(p, [dev(a) for a in od.grads_of(sizes, 0)], od.LR, od.BETAS, od.EPS, 0.5)
    before = [x.clone() for x in p] + sum((list(x) for x in opt.state()), [])
    info = torch.full((2 + GUARD,), np.nan, dtype=torch.float64, device=DEV)
    opt.step(p, [nan(x) for x in p], od.LR, od.BETAS, od.EPS, 0.5, info=info[:2], gate=shut)
    after = [x.clone() for x in p] + sum((list(x) for x in opt.state()), [])
    assert _same(before, after) and int(after[-1].item()) == 1 and bool(torch.isnan(info).all())
    opt.close()


def test_wrapper_strictness():
    g = KLGate(DEV)
    assert g.gate.dtype == torch.int32 and g.gate.cpu().tolist() == [0, 0] and g.state.data_ptr() != g.gate.data_ptr()
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    for bad in (stats.float(), stats[:3], stats.cpu(), stats.cpu().numpy()):
        with pytest.raises(_native.PbgError):
            g.check(bad, 0.1)
    dims, B, Bm, seed = pd.CASES[2]
    c = pd.case(dims, B, Bm, seed, False)
    gr, t = PPOGrad(dims, Bm, DEV), tensors(c)
    args = tuple(t[k] for k in ("theta_actor", "theta_critic", "log_std", "obs", "act", "logp_old", "adv", "ret"))
    for bad in (g.gate.cpu(), g.gate.long(), torch.zeros(3, dtype=torch.int32, device=DEV), np.zeros(2, np.int32)):
        with pytest.raises(_native.PbgError):
            gr.run(*args, idx=t["idx"], gate=bad)
    for kw in (dict(value_old=t["ret"]), dict(vf_clip=0.2), dict(value_old=t["ret"].double(), vf_clip=0.2),
               dict(value_old=t["ret"].cpu(), vf_clip=0.2), dict(value_old=t["ret"][:-1], vf_clip=0.2),
               dict(value_old=t["ret"], vf_clip=-0.2)):
        with pytest.raises(_native.PbgError):
            gr.run(*args, idx=t["idx"], **kw)
    gr.close()


# ---------------------------------------------------------------------------- the trainers
def _trainer(hp=HP, seed=0, n=TRAIN_N, **kw):
    env = VecEnv(ENV_ID, n, device=DEV, seed=seed, autoreset=True, precision=64)
    kw = dict(dict(backward="hip", optimizer="hip"), **kw)
    return env, PPO(env, seed=seed, **dict(hp, **kw))


def _state(ppo):
    m, v, t = ppo.adam.state()
    return [x.clone() for x in (ppo.actor_theta.data, ppo.critic_theta.data, ppo.log_std.data)] + m + v + [t]


def _iterations(n_iter, **kw):
    env, ppo = _trainer(**kw)
    stats = [ppo.iterate() for _ in range(n_iter)]
    state = _state(ppo)
    stats = [{k: float(v) for k, v in s.items()} for s in stats]
    ppo.close()
    env.close()
    return state, stats


def test_target_kl_needs_the_hip_optimiser_and_positive_values():
    env = VecEnv(ENV_ID, 64, device=DEV, seed=0, autoreset=True, precision=64)
    for kw in (dict(target_kl=0.01), dict(target_kl=0.01, backward="hip"), dict(target_kl=0.0, backward="hip", optimizer="hip"),
               dict(vf_clip=0.0), dict(vf_clip=-1.0, backward="hip"), dict(vf_clip=float("nan"))):
        with pytest.raises(_native.PbgError):
            PPO(env, **dict(HP, **kw))
    env.close()


def test_a_target_nothing_reaches_holds_the_bits_of_no_target():
    steps = HP["epochs"] * HP["minibatches"]
    want, wstats = _iterations(2)
    got, gstats = _iterations(2, target_kl=1e9)
    assert _same(got, want)
    assert set(gstats[-1]) == set(wstats[-1]) | {"updates", "kl_stop"}
    for s, w in zip(gstats, wstats):
        assert s["updates"] == steps and s["kl_stop"] == 0 and all(s[k] == w[k] for k in w)


def test_the_trainer_stops_early_and_every_graph_mode_holds_the_eager_bits():
    """K0: the last minibatch's kl of the ungated trainer's iteration 0 (seed 0: positive on the device, asserted).
    target_kl = K0 / 3 puts kl_limit at K0 / 2, which that minibatch at the latest exceeds: iteration 0 stops."""
    steps = HP["epochs"] * HP["minibatches"]
    _, free = _iterations(1)
    K0 = free[0]["kl"]
    assert K0 > 0.0, K0
    want, stats = _iterations(4, target_kl=K0 / 3.0, vf_clip=0.2)
    print(f"K0 {K0:.6f}; updates per iteration {[s['updates'] for s in stats]}; kl {[s['kl'] for s in stats]}")
    _, stats0 = _iterations(1, target_kl=K0 / 3.0)
    assert stats0[0]["updates"] < steps and stats0[0]["kl_stop"] == 1 and stats0[0]["kl"] > 0.5 * K0
    assert any(s["kl_stop"] == 1 and s["updates"] < steps for s in stats)
    for s in stats:
        assert (s["updates"] < steps) == (s["kl_stop"] == 1) and (s["kl_stop"] == 0 or s["kl"] > 0.5 * K0)
    ref, rstats = _iterations(4, target_kl=K0 / 3.0, vf_clip=0.2, permutation="device")
    for graph in (True, "iteration"):
        got, gstats = _iterations(4, target_kl=K0 / 3.0, vf_clip=0.2, graph=graph, permutation="device")
        assert _same(got, ref), graph
        assert [(s["updates"], s["kl_stop"]) for s in gstats] == [(s["updates"], s["kl_stop"]) for s in rstats], graph
    assert any(s["kl_stop"] == 1 for s in rstats)


SMALL = dict(hidden=(16, 8), steps=8, epochs=2, seed=3, lr=3e-3, minibatches=4)   # tests/test_sharded_ppo_gpu.py's smallest
SMALL_N, SMALL_KL = 128, 1e-4


def _small_snapshot(ppo):
    out = [x.cpu().numpy().copy() for x in _state(ppo)]
    return out, ppo.kl_gate.state.cpu().tolist()


def _one_process(iterations=2, **kw):
    env = VecEnv(ENV_ID, SMALL_N, device=DEV, seed=3, autoreset=True, precision=64)
    ppo = PPO(env, backward="hip", optimizer="hip", permutation="device", vf_clip=0.2, target_kl=SMALL_KL, **dict(SMALL, **kw))
    snaps = []
    for _ in range(iterations):
        ppo.iterate()
        snaps.append(_small_snapshot(ppo))
    ppo.close()
    env.close()
    return snaps


def test_sharded_world_one_is_the_trainer_bit_for_bit():
    from pybulletgym_amd.distributed import ShardedVecEnv
    want = _one_process()
    shard = ShardedVecEnv(ENV_ID, SMALL_N, 0, 1, device=DEV, seed=3, autoreset=True, precision=64)
    ppo = ShardedPPO(shard, vf_clip=0.2, target_kl=SMALL_KL, **SMALL)
    for it in range(2):
        stats = ppo.iterate()
        got, gate = _small_snapshot(ppo)
        assert gate == want[it][1] == [int(stats["kl_stop"]), int(stats["updates"])]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want[it][0])), it
    print(f"gate per iteration {[g for _, g in want]}")
    assert any(g[0] == 1 and 0 < g[1] < SMALL["epochs"] * SMALL["minibatches"] for _, g in want)
    ppo.close()
    shard.env.close()


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pybulletgym_amd.distributed import ShardedVecEnv
    shard = ShardedVecEnv(ENV_ID, SMALL_N, rank, world, device=DEV, seed=3, autoreset=True, precision=64)
    ppo = ShardedPPO(shard, vf_clip=0.2, target_kl=SMALL_KL, **SMALL)
    snaps = []
    for _ in range(2):
        ppo.iterate()
        snaps.append(_small_snapshot(ppo))
    q.put((rank, snaps))
    dist.barrier()
    ppo.close()
    shard.env.close()
    dist.destroy_process_group()


def test_two_ranks_hold_the_one_process_bits_and_stop_at_the_same_step():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        want = _one_process()   # while the children start
        results = sorted((q.get(timeout=100) for _ in range(2)), key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=60)
        for p in procs:
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    for rank, snaps in results:
        for it in range(2):
            assert snaps[it][1] == want[it][1], (rank, it, snaps[it][1], want[it][1])
            assert all(a.tobytes() == b.tobytes() for a, b in zip(snaps[it][0], want[it][0])), (rank, it)
    assert any(g[0] == 1 for _, g in want)
