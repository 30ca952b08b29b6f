"""The advantage normaliser and the clip + Adam step on the device (include/pbg.h "PPO optimiser step", pbg_adv_norm,
pbg_ppo_opt_step, ppo.adv_norm, ppo.AdamClip) bit for bit against their host twins, between guard elements, on
streams and in a replayed graph; and the trainer with optimizer="hip" and graph=True."""
import ctypes

import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import PPO, AdamClip, Permutation, PPOGrad, RetStats, adv_norm
from pybulletgym_amd.vec_env import VecEnv

import policies
import ppo_opt_data as od

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 8  # NaN elements before and after every block


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("Bm", od.ADV_ROWS + (8209,))
def test_adv_norm_device_is_the_host_twin(Bm):
    rng = np.random.default_rng(Bm)
    B = 2 * Bm + 5
    adv = (0.3 + 2.0 * rng.standard_normal(B)).astype(np.float32)
    idx = rng.permutation(B)[:Bm].astype(np.int64)
    out = torch.full((2 + 2 * GUARD,), np.nan, dtype=torch.float32, device=DEV)
    for a, i in ((adv[:Bm].copy(), None), (adv, idx)):
        want = adv_norm(a, i)
        out.fill_(np.nan)
        adv_norm(dev(a), None if i is None else dev(i), out=out[GUARD:GUARD + 2])
        got = out.cpu().numpy()
        assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + 2:]).all()
        assert bits(got[GUARD:GUARD + 2], want), (Bm, got[GUARD:GUARD + 2], want)
        assert bits(want, od.adv_norm_ref(a, i))


@pytest.mark.parametrize("Bm,value", od.CONSTANT)
def test_adv_norm_device_of_constant_advantages(Bm, value):
    const = np.full(Bm, value, np.float32)
    got = adv_norm(dev(const)).cpu().numpy()
    assert bits(got, adv_norm(const)) and got[0] == np.float32(value) and got[1] == np.float32(1e8)
    assert ((const - got[0]) * got[1] == 0.0).all()


class Guarded:
    """The blocks of ``arrays`` on the device, each between GUARD NaNs (``shift`` further elements in front: 1 breaks
    the 16-byte alignment, so the element-wise path runs)."""

    def __init__(self, arrays, shift):
        self.full, self.view = [], []
        for a in arrays:
            f = torch.full((GUARD + shift + a.shape[0] + GUARD,), np.nan, dtype=torch.float32, device=DEV)
            v = f[GUARD + shift:GUARD + shift + a.shape[0]]
            v.copy_(dev(a))
            assert v.data_ptr() % 16 == (4 * shift) % 16
            self.full.append(f)
            self.view.append(v)
        self.lo = GUARD + shift

    def numpy(self):
        for f, v in zip(self.full, self.view):
            assert bool(torch.isnan(f[:self.lo]).all()) and bool(torch.isnan(f[self.lo + v.shape[0]:]).all()), "a guard was written"
        return [v.cpu().numpy() for v in self.view]


def device_state(opt):
    """m, v, t through the raw call, into buffers with guards before and after."""
    n = sum(opt.sizes)
    m, v = (torch.full((n + 2 * GUARD,), np.nan, dtype=torch.float32, device=DEV) for _ in range(2))
    t = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _native.check(_native.lib().pbg_ppo_opt_get_state(opt._h, m[GUARD:].data_ptr(), v[GUARD:].data_ptr(), t[1:].data_ptr(),
                                                      stream), "pbg_ppo_opt_get_state")
    m, v, t = m.cpu().numpy(), v.cpu().numpy(), t.cpu().numpy()
    for a in (m, v):
        assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + n:]).all()
    assert t[0] == -7 and t[2] == -7
    cuts = np.cumsum(opt.sizes)[:-1]
    return np.split(m[GUARD:GUARD + n], cuts), np.split(v[GUARD:GUARD + n], cuts), int(t[1])


@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("max_grad_norm", (0.0, 0.5))
@pytest.mark.parametrize("sizes", od.SIZES_GPU)
def test_opt_step_device_is_the_host_twin(sizes, max_grad_norm, shift):
    host, hp = AdamClip(sizes), od.params0(sizes)
    opt, p = AdamClip(sizes, DEV), Guarded(od.params0(sizes), shift)
    info = torch.full((2 + GUARD,), np.nan, dtype=torch.float64, device=DEV)
    hinfo = np.zeros(2)
    for s in range(3):
        g = od.grads_of(sizes, s, zero_block=(len(sizes) - 1) if s == 1 and len(sizes) > 1 else None)
        host.step(hp, g, od.LR, od.BETAS, od.EPS, max_grad_norm, info=hinfo)
        gd = Guarded(g, shift)
        opt.step(p.view, gd.view, od.LR, od.BETAS, od.EPS, max_grad_norm, info=info[:2])
        got, (m, v, t) = p.numpy(), device_state(opt)
        hm, hv, ht = host.state()
        assert t == s + 1 == int(ht[0])
        i = info.cpu().numpy()
        assert np.isnan(i[2:]).all() and bits(i[:2], hinfo), (s, i[:2], hinfo)
        for b in range(len(sizes)):
            assert bits(got[b], hp[b]), (s, b, "param", int((got[b] != hp[b]).sum()))
            assert bits(m[b], hm[b]) and bits(v[b], hv[b]), (s, b, "state")
            assert bits(gd.numpy()[b], g[b])
    m, v, t = opt.state()
    assert int(t.cpu()[0]) == 3 and all(bits(a.cpu().numpy(), b) for a, b in zip(m, host.state()[0]))
    opt.reset()
    m, v, t = device_state(opt)
    assert t == 0 and not any(a.any() for a in m + v)
    opt.close()


def test_the_same_bits_twice_on_a_side_stream_and_in_a_replayed_graph():
    sizes = od.SIZES[3]
    g = [dev(a) for a in od.grads_of(sizes, 1)]

    def fresh():
        return AdamClip(sizes, DEV), [dev(a) for a in od.params0(sizes)]

    def final(opt, p):
        torch.cuda.synchronize()
        m, v, t = opt.state()
        out = [a.cpu().numpy() for a in p + m + v] + [t.cpu().numpy()]
        opt.close()
        return out

    def two_steps(opt, p):
        for _ in range(2):
            opt.step(p, g, od.LR, od.BETAS, od.EPS, 0.5)

    # the host twin's two steps
    host, hp = AdamClip(sizes), od.params0(sizes)
    hg = od.grads_of(sizes, 1)
    for _ in range(2):
        host.step(hp, hg, od.LR, od.BETAS, od.EPS, 0.5)
    runs = []
    for _ in range(2):   # twice from equal states
        opt, p = fresh()
        two_steps(opt, p)
        runs.append(final(opt, p))
    opt, p = fresh()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        two_steps(opt, p)
    torch.cuda.current_stream(DEV).wait_stream(side)
    runs.append(final(opt, p))
    # one captured step replayed twice: the step count and the betas' powers advance on the device
    opt, p = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(p, g, od.LR, od.BETAS, od.EPS, 0.5)
    torch.cuda.synchronize()
    assert int(opt.state()[2].cpu()[0]) == 0 and all(bits(a.cpu().numpy(), b) for a, b in zip(p, od.params0(sizes)))
    graph.replay()
    graph.replay()
    runs.append(final(opt, p))
    want = runs[0]
    assert int(want[-1][0]) == 2 and all(bits(a, b) for a, b in zip(want[:3], hp))
    for other in runs[1:]:
        for a, b in zip(want, other):
            assert bits(a, b)


# ---------------------------------------------------------------------------- the trainer
ENV_ID, EVAL_N, EVAL_STEPS = "InvertedPendulumPyBulletEnv-v0", 256, 200
HP = dict(hidden=(64, 64), steps=32, lr=3e-3, epochs=4, minibatches=4, log_std=-0.5)   # tests/test_ppo_gpu.py's
TRAIN_N = 256


def _trainer(hp=HP, seed=0, **kw):
    env = VecEnv(ENV_ID, TRAIN_N, device=DEV, seed=seed, autoreset=True, precision=64)
    return env, PPO(env, seed=seed, backward="hip", **dict(hp, **kw))


def _params(ppo):
    return [p.data.cpu().numpy().copy() for p in (ppo.actor_theta, ppo.critic_theta, ppo.log_std)]


def test_trainer_first_step_agrees_with_the_torch_optimiser():
    """One epoch of one minibatch is one optimiser step.  Truth: torch.optim.Adam + clip_grad_norm_ in float64 on the
    raw gradient of the optimizer="hip" trainer (its step leaves .grad as pbg_ppo_grad wrote it); yardstick: the
    optimizer="torch" trainer's float32 parameters; tests/ppo_opt_data.py's bound on the movement."""
    hp = dict(HP, epochs=1, minibatches=1)
    res = {}
    for mode in ("torch", "hip"):
        env, ppo = _trainer(hp, optimizer=mode)
        p0 = _params(ppo)
        stats = ppo.iterate()
        res[mode] = (p0, _params(ppo), [p.grad.cpu().numpy().copy() for p in (ppo.actor_theta, ppo.critic_theta, ppo.log_std)],
                     {k: float(v) for k, v in stats.items()})
        ppo.close()
        env.close()
    p0, got, grad, stats = res["hip"]
    assert all(bits(a, b) for a, b in zip(p0, res["torch"][0]))
    assert set(stats) == {"pg", "vf", "clipfrac", "kl", "grad_norm"}
    norm = np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in grad))
    assert abs(stats["grad_norm"] - norm) <= 1e-12 * norm
    ps = [torch.nn.Parameter(torch.from_numpy(p).double()) for p in p0]
    opt = torch.optim.Adam(ps, lr=hp["lr"], eps=1e-5)
    for p, g in zip(ps, grad):
        p.grad = torch.from_numpy(g).double()
    torch.nn.utils.clip_grad_norm_(ps, 0.5)
    opt.step()
    for b, (g, p64, p32, z) in enumerate(zip(got, ps, res["torch"][1], p0)):
        e, e32 = od.movement_err(g, p64.detach().numpy(), z), od.movement_err(p32, p64.detach().numpy(), z)
        print(f"trainer block {b}: err {e:.3e}, the torch optimiser's {e32:.3e}")
        assert e <= max(4.0 * e32, 1e-5), (b, e, e32)


def test_two_hip_optimiser_trainers_hold_the_same_bits_after_two_iterations():
    finals = []
    for _ in range(2):
        env, ppo = _trainer(optimizer="hip")
        for _ in range(2):
            ppo.iterate()
        finals.append(_params(ppo))
        ppo.close()
        env.close()
    for a, b in zip(*finals):
        assert np.isfinite(a).all() and bits(a, b)


@pytest.mark.parametrize("obs_norm", (False, True))
def test_the_graph_trainer_holds_the_eager_trainers_bits(obs_norm):
    finals = []
    for graph in (False, True):
        env, ppo = _trainer(optimizer="hip", graph=graph, obs_norm=obs_norm)
        stats = [ppo.iterate() for _ in range(2)]
        finals.append(_params(ppo) + [np.array([float(stats[-1][k]) for k in ("pg", "vf", "clipfrac", "kl", "grad_norm")])])
        assert (ppo._graph is not None) == graph
        ppo.close()
        env.close()
    for a, b in zip(*finals):
        assert np.isfinite(a).all()
        assert bits(a, b)


def test_refused_argument_combinations():
    env = VecEnv(ENV_ID, TRAIN_N, device=DEV, seed=0, autoreset=True, precision=64)
    for kw in (dict(optimizer="hip"), dict(optimizer="hip", backward="torch"), dict(backward="hip", graph=True),
               dict(graph=True), dict(backward="hip", optimizer="torch", graph=True), dict(backward="hip", optimizer="adam")):
        with pytest.raises(_native.PbgError):
            PPO(env, **dict(HP, **kw))
    env.close()


@pytest.mark.parametrize("make,use", [
    (lambda: PPOGrad((3, 4, 4, 1), 8, DEV), lambda o: o.geometry(8)),
    (lambda: AdamClip([5], DEV), lambda o: o.reset()),
    (lambda: Permutation(0, DEV), lambda o: o.fill(4)),
    (lambda: RetStats(32, 0.99, DEV), lambda o: o.reset())], ids=["PPOGrad", "AdamClip", "Permutation", "RetStats"])
def test_every_native_wrapper_closes_once_and_refuses_use_after_close(make, use):
    obj = make()
    use(obj)          # open: the call goes through
    obj.close()
    obj.close()       # twice is harmless
    assert not obj._h
    with pytest.raises(_native.PbgError, match="closed"):
        use(obj)


def test_the_graph_trainer_learns_to_balance_the_pendulum():
    """tests/test_ppo_gpu.py's learning test with optimizer="hip", graph=True: the same hyperparameters, 30
    iterations, the noise-free mean policy on section 11's 256 fixed initial states, first episode, 200 steps;
    section 11's bar."""
    env, ppo = _trainer(optimizer="hip", graph=True)
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
