"""The matrix-core path of the PPO gradient on the device (include/pbg.h "PPO gradient", "The matrix-core path";
ppo.PPOGrad(path="mfma"), PPO(grad_path="mfma")): against torch float64 autograd under the bound of
tests/ppo_grad_data.py, its forward against the FMA path and the critic's actor bit for bit, its repeatability on
streams, in a replayed graph and after other work, its independence of uninitialised memory, and the trainer."""
import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd.ppo import PPO, PPOGrad
from pybulletgym_amd.vec_env import VecEnv

import poison
import policies
import ppo_grad_data as gd
from poison import RUNS, surrounded
from test_learner_invariance_gpu import GRAD_KEYS, GradOutputs
from test_ppograd_gpu import DEV, Outputs, critic_values, run, tensors

pytestmark = pytest.mark.gpu

# tests/ppo_grad_data.py's cases (widths 1, 3, 5, 8, 17 below a block, 65 and 129 one past an edge, the maxima 256 and
# 64; 1 to 257 rows; 8,209 and 1,921 rows: several tiles per workgroup, the second through the workgroup's partial) and
# the two shipped shapes at 40 rows of 64, each with the smallest seed gd.case accepts with and without a normaliser
SHIPPED = (((28, 128, 64, 8), 64, 40, 0), ((44, 256, 128, 17), 64, 40, 0))
CASES = gd.CASES + SHIPPED


@pytest.mark.parametrize("dims,B,Bm,seed", CASES)
def test_gradient_stats_forward_and_guards(dims, B, Bm, seed):
    """Every option of a case: the gradient within max(4 err(torch float32), 1e-5) per block of float64 autograd and the
    stats and logp within 1e-5 (gd.check_grads, gd.check_stats); v_out and logp_out the FMA path's bits and v_out the
    critic's actor's; every output between NaN guards that stay NaN."""
    worst = 0.0
    fma, mfma = PPOGrad(dims, Bm, DEV), PPOGrad(dims, Bm, DEV, path="mfma")
    for norm in (False, True):
        c = gd.case(dims, B, Bm, seed, norm)
        t = tensors(c)
        v_actor = critic_values(c, t)
        for n_, adv_norm, ent_coef in gd.OPTIONS:
            if n_ != norm:
                continue
            what = f"mfma dims {dims} Bm {Bm} norm {norm} adv_norm {adv_norm} ent {ent_coef}"
            (g64, s64, logp64, _), (g32, _, _, _) = gd.references(dims, B, Bm, seed, norm, adv_norm, ent_coef)
            out, ref = Outputs(mfma, Bm), Outputs(fma, Bm)
            run(mfma, c, t, adv_norm, ent_coef, out)
            run(fma, c, t, adv_norm, ent_coef, ref)
            o, r = out.numpy(), ref.numpy()
            ratio = gd.check_grads(gd.blocks(dims, o["grad_actor"], o["grad_critic"], o["grad_log_std"]), g64, g32, what)
            worst = max(worst, ratio)
            gd.check_stats(o["stats"], o["logp_out"], s64, logp64, what)
            assert np.array_equal(o["v_out"], r["v_out"]) and np.array_equal(o["logp_out"], r["logp_out"]), what
            assert np.array_equal(o["v_out"], v_actor), what
    fma.close()
    mfma.close()
    print(f"mfma dims {dims} Bm {Bm}: worst err / err_torch32 {worst:.3f}")


def _bits_equal(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("dims,B,Bm,seed", (gd.CASES[3], SHIPPED[1], gd.CASES[5]))
def test_the_same_bits_twice_on_a_side_stream_and_in_a_replayed_graph(dims, B, Bm, seed):
    c = gd.case(dims, B, Bm, seed, True)
    g, t = PPOGrad(dims, Bm, DEV, path="mfma"), tensors(c)
    outs = [Outputs(g, Bm) for _ in range(4)]
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
    for i, other in enumerate((outs[1].numpy(), outs[2].numpy(), first, second)):
        _bits_equal(want, other, (dims, i))
    g.close()


@pytest.mark.parametrize("dims,B,Bm,seed", (gd.CASES[8], gd.CASES[9]))
def test_a_used_object_gives_a_fresh_ones_bits(dims, B, Bm, seed):
    """Many rows leave every workgroup's partial in the workspace (the widest MLP: the running sums of the route
    through it); a minibatch of 33 rows then runs 3 workgroups and must see none of it."""
    c = gd.case(dims, B, Bm, seed, False)
    t = tensors(c)
    small = t["idx"][:33].contiguous()
    used, fresh = PPOGrad(dims, Bm, DEV, path="mfma"), PPOGrad(dims, Bm, DEV, path="mfma")
    big = Outputs(used, Bm)
    run(used, c, t, True, 0.01, big)
    assert np.abs(big.numpy()["grad_actor"]).max() > 0.0
    a, b = Outputs(used, 33), Outputs(fresh, 33)
    run(used, c, t, True, 0.01, a, idx=small)
    run(fresh, c, t, True, 0.01, b, idx=small)
    a, b = a.numpy(), b.numpy()
    _bits_equal(a, b, dims)
    assert np.isfinite(b["grad_actor"]).all() and np.abs(b["grad_actor"]).max() > 0.0
    used.close()
    fresh.close()


# below a block, a shipped shape (the on-chip route) and the widest (the route through the partial); 13 rows: one ragged
# tile, 48: three tiles; the smallest seeds gd.case accepts
INVARIANCE = [(dims, 64, Bm, seed) for dims, seed in (((7, 33, 17, 3), 0), ((44, 256, 128, 17), 0), ((256, 256, 256, 64), 1))
              for Bm in (13, 48)]


@pytest.mark.parametrize("dims,B,Bm,seed", INVARIANCE)
def test_the_gradient_is_invariant_to_uninitialised_memory(dims, B, Bm, seed):
    """tests/test_learner_invariance_gpu.py's protocol: a fresh object per run, every input inside a buffer of the
    run's pattern, LDS and register files poisoned before the call, every output between guards; the four runs agree
    on every output."""
    c = gd.case(dims, B, Bm, seed, True)
    what = f"mfma gradient {dims} Bm {Bm}"
    runs = []
    for r in RUNS:
        t = {k: None if c[k] is None else surrounded(c[k], r, DEV) for k in GRAD_KEYS}
        g = PPOGrad(dims, Bm, DEV, path="mfma")
        out = GradOutputs(g, Bm)
        poison.poison_run(r, None, DEV)
        run(g, c, t, True, 0.01, out)
        runs.append(out.numpy(what))
        g.close()
    poison.assert_runs_agree(runs, what)
    (g64, s64, logp64, _), (g32, _, _, _) = gd.references(dims, B, Bm, seed, True, True, 0.01)
    o = runs[0]
    gd.check_grads(gd.blocks(dims, o["grad_actor"], o["grad_critic"], o["grad_log_std"]), g64, g32, what)
    gd.check_stats(o["stats"], o["logp_out"], s64, logp64, what)


@pytest.mark.parametrize("dims,B,Bm,seed", (gd.CASES[2], gd.CASES[4], SHIPPED[1], gd.CASES[7]))
def test_idx_null_is_an_explicit_arange_and_a_permuted_idx_is_accepted(dims, B, Bm, seed):
    c = gd.case(dims, B, Bm, seed, True)
    g, t = PPOGrad(dims, Bm, DEV, path="mfma"), tensors(c)
    a, b, p = Outputs(g, Bm), Outputs(g, Bm), Outputs(g, Bm)
    run(g, c, t, True, 0.01, a, idx=None, rows=Bm)
    run(g, c, t, True, 0.01, b, idx=torch.arange(Bm, device=DEV))
    perm = torch.from_numpy(np.random.default_rng(Bm).permutation(Bm)).to(DEV)
    run(g, c, t, True, 0.01, p, idx=perm)
    a, b, p = a.numpy(), b.numpy(), p.numpy()
    _bits_equal(a, b, dims)
    assert np.isfinite(a["grad_actor"]).all() and np.isfinite(a["stats"]).all()
    # the same rows in another order: the per-row outputs move with their rows
    perm = perm.cpu().numpy()
    assert np.array_equal(p["v_out"], a["v_out"][perm]) and np.array_equal(p["logp_out"], a["logp_out"][perm])
    assert np.isfinite(p["grad_actor"]).all() and np.abs(p["grad_actor"]).max() > 0.0
    g.close()


# ---------------------------------------------------------------------------- the trainer
ENV_ID, EVAL_N, EVAL_STEPS = "InvertedPendulumPyBulletEnv-v0", 256, 200
SMALL = dict(hidden=(16, 8), steps=8, lr=3e-3, epochs=2, minibatches=2, log_std=-0.5)
SMALL_N = 64


def _small(seed=3, **kw):
    env = VecEnv(ENV_ID, SMALL_N, device=DEV, seed=seed, autoreset=True, precision=64)
    return env, PPO(env, seed=seed, backward="hip", optimizer="hip", grad_path="mfma", **dict(SMALL, **kw))


def _iterate(n, **kw):
    env, ppo = _small(**kw)
    assert ppo.grad_path == "mfma" and ppo.grad.path == "mfma"
    for _ in range(n):
        ppo.iterate()
    torch.cuda.synchronize()
    m, v, t = ppo.adam.state()
    out = dict(actor=ppo.actor_theta.data, critic=ppo.critic_theta.data, log_std=ppo.log_std.data, m=torch.cat(m), v=torch.cat(v), t=t)
    out = {k: x.cpu().numpy().copy() for k, x in out.items()}
    ppo.close()
    env.close()
    return out


def test_two_trainers_hold_the_same_bits_after_two_iterations():
    a, b = _iterate(2), _iterate(2)
    for k in a:
        assert np.isfinite(a[k]).all()
        poison.assert_same_bits(a[k], b[k], k)


def test_the_iteration_graph_trainer_holds_the_eager_trainers_bits():
    eager = _iterate(3, permutation="device")
    graph = _iterate(3, permutation="device", graph="iteration")
    for k in eager:
        poison.assert_same_bits(graph[k], eager[k], k)


def test_a_hopper_trainers_first_gradient_agrees_with_float64_autograd():
    """tests/test_ppograd_gpu.py's trainer test at hidden = (128, 64) on Hopper, 64 envs x 8 steps: one epoch of one
    minibatch without clipping leaves the raw gradient in .grad; torch float64 autograd on the device is the truth, the
    torch trainer's float32 gradient the yardstick."""
    env_id, n, hp = "HopperPyBulletEnv-v0", 64, dict(hidden=(128, 64), steps=8, lr=3e-3, epochs=1, minibatches=1,
                                                       log_std=-0.5, max_grad_norm=0)
    runs = {}
    for mode, kw in (("torch", dict(backward="torch")), ("mfma", dict(backward="hip", grad_path="mfma"))):
        env = VecEnv(env_id, n, device=DEV, seed=0, autoreset=True, precision=64)
        ppo = PPO(env, seed=0, **hp, **kw)
        b = ppo.collect()
        batch = {k: v.clone() for k, v in vars(b).items()}
        params = [p.data.clone() for p in (ppo.actor_theta, ppo.critic_theta, ppo.log_std)]
        ppo.update(b)
        runs[mode] = (batch, params, [p.grad.clone() for p in (ppo.actor_theta, ppo.critic_theta, ppo.log_std)], ppo.actor_dims)
        ppo.close()
        env.close()
    bt, bh = runs["torch"][0], runs["mfma"][0]
    for k in bt:
        assert bt[k].cpu().numpy().tobytes() == bh[k].cpu().numpy().tobytes(), k
    dims = runs["mfma"][3]
    assert dims[1:3] == (128, 64)
    B = n * hp["steps"]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    idx = torch.randperm(B, device=DEV, generator=gen)
    a_mb = bt["adv"].reshape(B)[idx]
    f = lambda x: x.cpu().numpy()  # noqa: E731
    c = dict(dims=dims, theta_actor=f(runs["mfma"][1][0]), theta_critic=f(runs["mfma"][1][1]), log_std=f(runs["mfma"][1][2]),
             mean=None, obs=f(bt["obs"].reshape(B, -1)), act=f(bt["act"].reshape(B, -1)), logp_old=f(bt["logp"].reshape(B).float()),
             adv=f(bt["adv"].reshape(B)), ret=f(bt["ret"].reshape(B)), idx=f(idx),
             adv_norm=f(torch.stack((a_mb.mean(), 1.0 / (a_mb.std() + 1e-8)))))
    g64 = gd.reference(c, True, 0.0, torch.float64, device=DEV)[0]
    worst = gd.check_grads(gd.blocks(dims, *(f(g) for g in runs["mfma"][2])), g64,
                           gd.blocks(dims, *(f(g) for g in runs["torch"][2])), "hopper trainer")
    print(f"hopper trainer, {B} rows, dims {dims}: worst err / err_torch32 {worst:.3f}")


def test_the_trainer_learns_to_balance_the_pendulum():
    """Section 13's run with grad_path="mfma": tests/test_ppograd_gpu.py's hyperparameters, 20 + 10 iterations, the
    noise-free mean policy on section 11's 256 fixed initial states, first episode, 200 steps; section 11's bar."""
    hp = dict(hidden=(64, 64), steps=32, lr=3e-3, epochs=4, minibatches=4, log_std=-0.5)
    env = VecEnv(ENV_ID, 256, device=DEV, seed=0, autoreset=True, precision=64)
    ppo = PPO(env, seed=0, backward="hip", grad_path="mfma", **hp)
    test = VecEnv(ENV_ID, EVAL_N, device=DEV, seed=0, autoreset=False, precision=64)
    q0 = torch.from_numpy(policies.reset_draws(EVAL_N, test.info.reset_dofs, 0).astype(np.float32))
    length = lambda: ppo.evaluate(test, EVAL_STEPS, init_q=q0)[1].cpu().numpy().astype(np.float64)  # noqa: E731
    before = length()
    for _ in range(20 + 10):
        ppo.iterate()
    after = length()
    ppo.close()
    env.close()
    test.close()
    print(f"untrained {before.mean():.2f} (std {before.std():.2f}); after 30: {after.mean():.2f}")
    assert after.mean() >= 150.0
    assert after.mean() > 21.46 + 3.0 * 6.74
    assert after.mean() > before.mean() + 3.0 * before.std()
