"""Value clipping in the PPO gradient on the device (include/pbg.h "Value clipping and the KL gate"; ppo.PPOGrad.run with
value_old on both paths, PPO(vf_clip=...)): against torch float64 autograd over PPO.update's expression with vf_clip
under the bound of tests/ppo_grad_data.py and against the host twin, v_out still the critic's actor's bits, the new
struct with the option off against the first version's, and the trainer's two backward paths against each other."""
import ctypes

import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import PPO, PPOGrad
from pybulletgym_amd.vec_env import VecEnv

import ppo_grad_data as pd
import ppo_vclip_data as vd
from test_ppograd_gpu import DEV, ENV_ID, HP, TRAIN_N, Outputs, critic_values, dev, tensors

pytestmark = pytest.mark.gpu

PATHS = ("fma", "mfma")


def run(g, c, t, adv_norm, ent_coef, out, **kw):
    norm = (t["mean"], t["inv_std"], c["clip"]) if c["mean"] is not None else None
    g.run(t["theta_actor"], t["theta_critic"], t["log_std"], t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"], idx=t["idx"],
          adv_norm=t["adv_norm"] if adv_norm else None, obs_norm=norm, clip_eps=pd.CLIP_EPS, vf_coef=pd.VF_COEF,
          ent_coef=ent_coef, **out.kw, **kw)


def check_case(g, c, refs, adv_norm, ent_coef, what):
    """tests/test_ppograd_gpu.py's check_case with value_old: the float64 reference under check_grads, the stats, v_out
    the critic's actor's bits, the guards, and the host twin at the same bound."""
    (g64, s64, logp64, _), (g32, _, _, _) = refs
    dims, Bm = c["dims"], c["Bm"]
    t = tensors(c)
    out = Outputs(g, Bm)
    run(g, c, t, adv_norm, ent_coef, out, value_old=dev(c["value_old"]), vf_clip=c["vf_clip"])
    o = out.numpy()   # asserts the guards
    got = pd.blocks(dims, o["grad_actor"], o["grad_critic"], o["grad_log_std"])
    worst = pd.check_grads(got, g64, g32, what)
    print(f"{what}: worst err / err_torch32 {worst:.3f}; stats {o['stats']} (float64 {s64})")
    pd.check_stats(o["stats"], o["logp_out"], s64, logp64, what)
    assert np.array_equal(o["v_out"], critic_values(c, t)), what
    (ha, hc, hl, hst), _, hv = vd.host_run(PPOGrad(dims, Bm), c, adv_norm, ent_coef)
    assert np.array_equal(o["v_out"], hv), what
    host = pd.blocks(dims, ha, hc, hl)
    for (name, a), (_, h), (_, r64), (_, r32) in zip(pd.flat_blocks(got), pd.flat_blocks(host), pd.flat_blocks(g64),
                                                     pd.flat_blocks(g32)):
        assert pd.err(a, h) <= max(4.0 * pd.err(r32, r64), 1e-5), (what, name)
    return o


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dims,B,Bm,seed", vd.CASES)
def test_device_gradient_with_value_old(dims, B, Bm, seed, path):
    g = PPOGrad(dims, Bm, DEV, path=path)
    for norm, adv_norm, ent_coef in vd.OPTIONS:
        c = vd.case(dims, B, Bm, seed, norm)
        check_case(g, c, vd.references(dims, B, Bm, seed, norm, adv_norm, ent_coef), adv_norm, ent_coef,
                   f"{path} dims {dims} Bm {Bm} norm {norm} adv_norm {adv_norm}")
    g.close()


@pytest.mark.parametrize("path", PATHS)
def test_workgroups_that_own_two_tiles_clip_too(path):
    """8,209 rows are 514 tiles: on either path workgroups 0 and 1 (and, under the matrix-core path's cap of 256, every
    workgroup) own more than one."""
    dims, B, Bm, seed = vd.TWO_TILES
    c = vd.case(dims, B, Bm, seed, False)
    g = PPOGrad(dims, Bm, DEV, path=path)
    o = check_case(g, c, vd.references(dims, B, Bm, seed, False, True, 0.01), True, 0.01, f"{path} dims {dims} Bm {Bm}")
    g.close()
    # the value loss against the host twin's sum over rows: the same float64 terms in another order
    (_, _, _, hst), _, _ = vd.host_run(PPOGrad(dims, Bm), c, True, 0.01)
    assert abs(o["stats"][1] - hst[1]) <= 1e-8 * abs(hst[1])
    print(f"{path}: generator seed {c['vclip_seed']}, the clipped term wins in {c['vclip_share']:.3f} of the batch")


@pytest.mark.parametrize("path", PATHS)
def test_the_new_struct_with_both_options_off_is_the_first_version(path):
    """value_old NULL and gate NULL through the 200-byte struct against the 176-byte one: torch.equal outputs."""
    for dims, B, Bm, seed in (vd.CASES[2], vd.CASES[3]):
        c = vd.case(dims, B, Bm, seed, True)
        g, t = PPOGrad(dims, Bm, DEV, path=path), tensors(c)
        old, new = Outputs(g, Bm), Outputs(g, Bm)
        run(g, c, t, True, 0.01, old)
        io = g._io("run", t["theta_actor"], t["theta_critic"], t["log_std"], t["obs"], t["act"], t["logp_old"], t["adv"],
                   t["ret"], t["idx"], None, t["adv_norm"], (t["mean"], t["inv_std"], c["clip"]), pd.CLIP_EPS, pd.VF_COEF, 0.01,
                   [new.kw[k] for k in ("grad_actor", "grad_critic", "grad_log_std", "stats")], new.kw["logp_out"],
                   new.kw["v_out"])
        assert type(io) is _native.PPOGradIO and io.struct_size == 176
        io2 = _native.PPOGradIO2(**{n: getattr(io, n) for n, _ in _native.PPOGradIO._fields_ if n != "struct_size"})
        assert io2.struct_size == 200 and not io2.value_old and not io2.gate
        g._launch("pbg_ppo_grad_run", g._open("run"), ctypes.byref(io2))
        new.numpy()
        for k in old.kw:
            assert torch.equal(old.kw[k], new.kw[k]) and bool(torch.isfinite(new.kw[k]).all()), (path, dims, k)
        g.close()


def _trainer(backward, hp, seed=0, **kw):
    env = VecEnv(ENV_ID, TRAIN_N, device=DEV, seed=seed, autoreset=True, precision=64)
    return env, PPO(env, seed=seed, backward=backward, **dict(hp, **kw))


def test_trainer_gradients_with_vf_clip_agree_with_torch():
    """tests/test_ppograd_gpu.py's test_trainer_gradients_agree_with_torch with vf_clip=0.2: one epoch of one minibatch
    without gradient clipping leaves the minibatch's raw gradient in the parameters' .grad.  Torch float64 autograd on
    the device over the clipped expression is g64, the torch trainer's float32 gradient the yardstick."""
    hp = dict(HP, epochs=1, minibatches=1, max_grad_norm=0)
    runs = {}
    for mode in ("torch", "hip"):
        env, ppo = _trainer(mode, hp, vf_clip=0.2)
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
    dims = runs["hip"][3]
    T, B = HP["steps"], TRAIN_N * HP["steps"]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    idx = torch.randperm(B, device=DEV, generator=gen)
    a_mb = bt["adv"].reshape(B)[idx]
    n = lambda x: x.cpu().numpy()  # noqa: E731
    c = dict(dims=dims, theta_actor=n(runs["hip"][1][0]), theta_critic=n(runs["hip"][1][1]), log_std=n(runs["hip"][1][2]),
             mean=None, obs=n(bt["obs"].reshape(B, -1)), act=n(bt["act"].reshape(B, -1)), logp_old=n(bt["logp"].reshape(B).float()),
             adv=n(bt["adv"].reshape(B)), ret=n(bt["ret"].reshape(B)), idx=n(idx), value_old=n(bt["value"][:T].reshape(B)),
             vf_clip=0.2, adv_norm=n(torch.stack((a_mb.mean(), 1.0 / (a_mb.std() + 1e-8)))))
    # the first minibatch runs under the parameters the batch was collected with: v == value_old and no row is clamped,
    # so this pins the plumbing (the value buffer's rows against the batch's) and the unclipped branch's derivative
    g64 = vd.reference(c, True, 0.0, torch.float64, device=DEV)[0]
    worst = pd.check_grads(pd.blocks(dims, *(n(g) for g in runs["hip"][2])), g64,
                           pd.blocks(dims, *(n(g) for g in runs["torch"][2])), "trainer with vf_clip")
    print(f"trainer with vf_clip, {B} rows: worst err / err_torch32 {worst:.3f}")
