"""The PPO gradient on the device (include/pbg.h "PPO gradient", pbg_ppo_grad_run, ppo.PPOGrad) against torch
float64 autograd under the bound of tests/ppo_grad_data.py, against the host twin and the critic's actor; its
repeatability on streams and in a replayed graph; and the trainer with backward="hip"."""
import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd.policy import MLPPopulation
from pybulletgym_amd.ppo import PPO, PPOGrad
from pybulletgym_amd.vec_env import VecEnv

import policies
import ppo_grad_data as pd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 8  # NaN elements behind every output


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


class Outputs:
    """The six outputs, each followed by GUARD NaNs."""

    def __init__(self, g, Bm):
        sizes = dict(grad_actor=g.Da, grad_critic=g.Dc, grad_log_std=g.dims[3], logp_out=Bm, v_out=Bm)
        self.full = {k: torch.full((n + GUARD,), np.nan, dtype=torch.float32, device=DEV) for k, n in sizes.items()}
        self.full["stats"] = torch.full((4 + GUARD,), np.nan, dtype=torch.float64, device=DEV)
        self.kw = {k: t[:t.shape[0] - GUARD] for k, t in self.full.items()}

    def numpy(self):
        """The outputs as numpy, after checking the guards."""
        for k, t in self.full.items():
            assert bool(torch.isnan(t[-GUARD:]).all()), f"{k}: a guard element was written"
        return {k: t.cpu().numpy() for k, t in self.kw.items()}


def tensors(c):
    return {k: dev(c[k]) for k in ("theta_actor", "theta_critic", "log_std", "obs", "act", "logp_old", "adv", "ret", "idx",
                                   "adv_norm", "mean", "inv_std")}


def run(g, c, t, adv_norm, ent_coef, out, idx="case", rows=None):
    norm = (t["mean"], t["inv_std"], c["clip"]) if c["mean"] is not None else None
    g.run(t["theta_actor"], t["theta_critic"], t["log_std"], t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"],
          idx=t["idx"] if isinstance(idx, str) else idx, rows=rows, adv_norm=t["adv_norm"] if adv_norm else None,
          obs_norm=norm, clip_eps=pd.CLIP_EPS, vf_coef=pd.VF_COEF, ent_coef=ent_coef, **out.kw)


def host_run(c, adv_norm, ent_coef):
    norm = (c["mean"], c["inv_std"], c["clip"]) if c["mean"] is not None else None
    return PPOGrad(c["dims"], c["Bm"]).run(
        c["theta_actor"], c["theta_critic"], c["log_std"], c["obs"], c["act"], c["logp_old"], c["adv"], c["ret"], idx=c["idx"],
        adv_norm=c["adv_norm"] if adv_norm else None, obs_norm=norm, clip_eps=pd.CLIP_EPS, vf_coef=pd.VF_COEF,
        ent_coef=ent_coef)


def critic_values(c, t):
    """The critic's actor on the gathered rows: a population of one pair, each member given all the rows."""
    pop = MLPPopulation(pd.critic_dims(c["dims"]), 1, DEV)
    pop.set_all(t["theta_critic"])
    if c["mean"] is not None:
        pop.set_obs_norm(t["mean"], t["inv_std"], clip=c["clip"])
    rows = t["obs"][t["idx"]]
    v = pop.act(torch.cat((rows, rows)).contiguous())[:c["Bm"], 0].cpu().numpy()
    pop.close()
    return v


def check_case(c, refs, adv_norm, ent_coef, what):
    (g64, _, _, _), (g32, _, _, _) = refs
    dims, Bm = c["dims"], c["Bm"]
    g, t = PPOGrad(dims, Bm, DEV), tensors(c)
    out = Outputs(g, Bm)
    run(g, c, t, adv_norm, ent_coef, out)
    o = out.numpy()
    g.close()
    got = pd.blocks(dims, o["grad_actor"], o["grad_critic"], o["grad_log_std"])
    worst = pd.check_grads(got, g64, g32, what)
    print(f"{what}: worst err / err_torch32 {worst:.3f}")
    # the forward is the actor's: the critic's values bit for bit
    assert np.array_equal(o["v_out"], critic_values(c, t)), what
    # the host twin: the same function, its backward summed in another order
    ha, hc, hl, _ = host_run(c, adv_norm, ent_coef)
    host = pd.blocks(dims, ha, hc, hl)
    for (name, a), (_, h), (_, r64), (_, r32) in zip(pd.flat_blocks(got), pd.flat_blocks(host), pd.flat_blocks(g64),
                                                     pd.flat_blocks(g32)):
        assert pd.err(a, h) <= max(4.0 * pd.err(r32, r64), 1e-5), (what, name)
    return o


@pytest.mark.parametrize("norm,adv_norm,ent_coef", pd.OPTIONS)
@pytest.mark.parametrize("dims,B,Bm,seed", pd.CASES)
def test_device_gradient_against_float64_autograd(dims, B, Bm, seed, norm, adv_norm, ent_coef):
    c = pd.case(dims, B, Bm, seed, norm)
    check_case(c, pd.references(dims, B, Bm, seed, norm, adv_norm, ent_coef), adv_norm, ent_coef,
               f"dims {dims} Bm {Bm} norm {norm} adv_norm {adv_norm} ent {ent_coef}")


@pytest.mark.parametrize("norm,adv_norm,ent_coef", pd.OPTIONS)
@pytest.mark.parametrize("dims,B,Bm,seed", pd.CASES)
def test_device_stats_and_logp_against_float64(dims, B, Bm, seed, norm, adv_norm, ent_coef):
    """stats within 1e-5 relative of the float64 values, logp_out within 1e-5 max(1, |logp|).  The device
    twin of tests/test_ppograd_host.py's test: the float64 forward for the stats is a code path of the kernel."""
    c = pd.case(dims, B, Bm, seed, norm)
    (_, s64, logp64, _), _ = pd.references(dims, B, Bm, seed, norm, adv_norm, ent_coef)
    g, t = PPOGrad(dims, Bm, DEV), tensors(c)
    out = Outputs(g, Bm)
    run(g, c, t, adv_norm, ent_coef, out)
    o = out.numpy()
    g.close()
    print(f"dims {dims} Bm {Bm} norm {norm} adv_norm {adv_norm}: stats rel err {np.abs(o['stats'] - s64) / np.abs(s64)}")
    pd.check_stats(o["stats"], o["logp_out"], s64, logp64, (dims, Bm, norm, adv_norm))


@pytest.mark.parametrize("dims,B,Bm,seed", pd.CASES)
def test_idx_null_is_an_explicit_arange(dims, B, Bm, seed):
    c = pd.case(dims, B, Bm, seed, True)
    g, t = PPOGrad(dims, Bm, DEV), tensors(c)
    a, b = Outputs(g, Bm), Outputs(g, Bm)
    run(g, c, t, True, 0.01, a, idx=None, rows=Bm)
    run(g, c, t, True, 0.01, b, idx=torch.arange(Bm, device=DEV))
    a, b = a.numpy(), b.numpy()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.isfinite(a["grad_actor"]).all() and np.isfinite(a["stats"]).all()
    g.close()


def test_many_workgroups_and_many_tiles_per_workgroup():
    """8,209 rows are 514 tiles of 16 rows (the last one of a single row).  An object never launches more than 512
    workgroups, and workgroup b owns the tiles b, b + 512, ...: workgroups 0 and 1 own two tiles each, the other
    510 one, and the reduction adds 512 partials.  (5, 16, 8, 1) takes the register path for the sums over a
    workgroup's tiles, (5, 65, 16, 1) the path through the workgroup's partial in memory."""
    for dims, B, Bm in (((5, 16, 8, 1), 8300, 8209), ((5, 65, 16, 1), 8300, 8209)):
        c = pd.case(dims, B, Bm, 0, False)
        (g64, _, logp64, _), (g32, _, _, _) = pd.references(dims, B, Bm, 0, False, True, 0.01)
        t = tensors(c)
        g = PPOGrad(dims, Bm, DEV)
        out = Outputs(g, Bm)
        run(g, c, t, True, 0.01, out)
        o = out.numpy()
        g.close()
        worst = pd.check_grads(pd.blocks(dims, o["grad_actor"], o["grad_critic"], o["grad_log_std"]), g64, g32, dims)
        print(f"dims {dims} Bm {Bm}: worst err / err_torch32 {worst:.3f}")
        assert (np.abs(o["logp_out"] - logp64) <= 1e-5 * np.maximum(1.0, np.abs(logp64))).all()
        assert np.array_equal(o["v_out"], critic_values(c, t))
        # the stats' sums over tiles, slots and workgroups against the host twin's over rows: the same float64 terms
        # (up to exp's last bit) in another order, 8,209 of them: 8209 * 2^-53 ~ 1e-12 of sum |term|, which is at
        # most some 1e3 times the |sum| of the cancelling ones
        hstats = host_run(c, True, 0.01)[3]
        assert (np.abs(o["stats"] - hstats) <= 1e-8 * np.abs(hstats)).all(), (o["stats"], hstats)


def test_the_same_bits_twice_on_a_side_stream_and_in_a_replayed_graph():
    dims, B, Bm, seed = pd.CASES[3]
    c = pd.case(dims, B, Bm, seed, True)
    g, t = PPOGrad(dims, Bm, DEV), tensors(c)
    outs = [Outputs(g, Bm) for _ in range(5)]
    run(g, c, t, True, 0.01, outs[0])
    run(g, c, t, True, 0.01, outs[1])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        run(g, c, t, True, 0.01, outs[2])
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(g, c, t, True, 0.01, outs[3])
    graph.replay()
    torch.cuda.synchronize()
    first = outs[3].numpy()
    for t_ in outs[3].kw.values():
        t_.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    second = outs[3].numpy()
    want = outs[0].numpy()
    assert np.abs(want["grad_actor"]).max() > 0.0
    for other in (outs[1].numpy(), outs[2].numpy(), first, second):
        for k in want:
            assert want[k].tobytes() == other[k].tobytes(), k
    g.close()


# ---------------------------------------------------------------------------- the trainer
ENV_ID, EVAL_N, EVAL_STEPS = "InvertedPendulumPyBulletEnv-v0", 256, 200
HP = dict(hidden=(64, 64), steps=32, lr=3e-3, epochs=4, minibatches=4, log_std=-0.5)   # tests/test_ppo_gpu.py's
TRAIN_N = 256


def _trainer(backward, hp=HP, seed=0):
    env = VecEnv(ENV_ID, TRAIN_N, device=DEV, seed=seed, autoreset=True, precision=64)
    return env, PPO(env, seed=seed, backward=backward, **hp)


def test_trainer_gradients_agree_with_torch():
    """One epoch of one minibatch without gradient clipping leaves the first (and only) minibatch's raw gradient in
    the parameters' .grad.  Torch float64 autograd on the device is g64, the torch trainer's float32 gradient the
    yardstick."""
    hp = dict(HP, epochs=1, minibatches=1, max_grad_norm=0)
    runs = {}
    for mode in ("torch", "hip"):
        env, ppo = _trainer(mode, hp)
        b = ppo.collect()
        batch = {k: v.clone() for k, v in vars(b).items()}
        params = [p.data.clone() for p in (ppo.actor_theta, ppo.critic_theta, ppo.log_std)]
        ppo.update(b)
        runs[mode] = (batch, params, [p.grad.clone() for p in (ppo.actor_theta, ppo.critic_theta, ppo.log_std)], ppo.actor_dims)
        ppo.close()
        env.close()
    bt, bh = runs["torch"][0], runs["hip"][0]
    for k in bt:
        assert bt[k].cpu().numpy().tobytes() == bh[k].cpu().numpy().tobytes(), k
    for a, b in zip(runs["torch"][1], runs["hip"][1]):
        assert torch.equal(a, b)
    dims = runs["hip"][3]
    B = TRAIN_N * HP["steps"]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    idx = torch.randperm(B, device=DEV, generator=gen)
    a_mb = bt["adv"].reshape(B)[idx]
    n = lambda x: x.cpu().numpy()  # noqa: E731
    c = dict(dims=dims, theta_actor=n(runs["hip"][1][0]), theta_critic=n(runs["hip"][1][1]), log_std=n(runs["hip"][1][2]),
             mean=None, obs=n(bt["obs"].reshape(B, -1)), act=n(bt["act"].reshape(B, -1)), logp_old=n(bt["logp"].reshape(B).float()),
             adv=n(bt["adv"].reshape(B)), ret=n(bt["ret"].reshape(B)), idx=n(idx),
             adv_norm=n(torch.stack((a_mb.mean(), 1.0 / (a_mb.std() + 1e-8)))))
    g64 = pd.reference(c, True, 0.0, torch.float64, device=DEV)[0]
    worst = pd.check_grads(pd.blocks(dims, *(n(g) for g in runs["hip"][2])), g64,
                           pd.blocks(dims, *(n(g) for g in runs["torch"][2])), "trainer")
    print(f"trainer, 8192 rows: worst err / err_torch32 {worst:.3f}")


def test_two_hip_trainers_hold_the_same_bits_after_two_iterations():
    finals = []
    for _ in range(2):
        env, ppo = _trainer("hip")
        stats = [ppo.iterate() for _ in range(2)]
        assert set(stats[-1]) == {"pg", "vf", "clipfrac", "kl"}
        finals.append([p.data.cpu().numpy().copy() for p in (ppo.actor_theta, ppo.critic_theta, ppo.log_std)])
        ppo.close()
        env.close()
    for a, b in zip(*finals):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


def test_the_hip_trainer_learns_to_balance_the_pendulum():
    """tests/test_ppo_gpu.py's learning test with backward="hip": the same hyperparameters, 30 iterations, the
    noise-free mean policy on section 11's 256 fixed initial states, first episode, 200 steps; section 11's bar."""
    env, ppo = _trainer("hip")
    test = VecEnv(ENV_ID, EVAL_N, device=DEV, seed=0, autoreset=False, precision=64)
    q0 = torch.from_numpy(policies.reset_draws(EVAL_N, test.info.reset_dofs, 0).astype(np.float32))
    length = lambda: ppo.evaluate(test, EVAL_STEPS, init_q=q0)[1].cpu().numpy().astype(np.float64)  # noqa: E731
    before, curve = length(), []
    for it in range(1, 31):
        ppo.iterate()
        if it % 5 == 0:
            curve.append((it, float(length().mean())))
    after = length()
    ppo.close()
    env.close()
    test.close()
    print(f"untrained {before.mean():.2f} (std {before.std():.2f}); curve {curve}; after 30: {after.mean():.2f}")
    assert after.mean() >= 150.0
    assert after.mean() > 21.46 + 3.0 * 6.74
    assert after.mean() > before.mean() + 3.0 * before.std()
