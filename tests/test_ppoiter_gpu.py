"""Device-side permutations, the optimiser's learning rate from device memory and the whole-iteration PPO graph
(include/pbg.h "Counter-based permutations and an on-device learning rate"): pbg_perm_fill bit
for bit against its host twin between guard rows, on streams and in a replayed graph; ``AdamClip.step`` with an ``lr``
tensor; the ``permutation="device"`` / ``lr_schedule="linear"`` / ``graph="iteration"`` trainers bit for bit against
one another and against the numpy mirrors; the uninitialised-memory invariance of the new launches."""
import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native, rng
from pybulletgym_amd.ppo import PPO, AdamClip, Permutation, lr_linear
from pybulletgym_amd.vec_env import VecEnv

import perm_data as pd
import poison
import policies
import ppo_opt_data as od
from poison import RUNS, Guarded, surrounded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64, I64 = torch.float32, torch.float64, torch.int64
SEED = pd.SEED


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host_perm(counter, B, n_perms, seed=SEED):
    p = Permutation(seed)
    p.counter = counter
    return p.fill(B, n_perms)


# ---------------------------------------------------------------------------- pbg_perm_fill
@pytest.mark.parametrize("n_perms", (1, 3))
@pytest.mark.parametrize("B", pd.SIZES_GPU)
def test_perm_fill_is_the_host_twin(B, n_perms):
    p = Permutation(SEED, DEV)
    assert p.counter == 0
    for c in (0, 7):
        p.counter = c
        out = Guarded((n_perms, B), I64, DEV)
        p.fill(B, n_perms, out=out.view)
        got = out.numpy(f"fill B {B} x {n_perms}")
        assert np.array_equal(got, host_perm(c, B, n_perms)), (B, n_perms, c)
        assert p.counter == c + n_perms
    p.close()


def test_two_fills_of_two_leave_what_one_fill_of_four_leaves():
    B = 257
    a, b = Permutation(SEED, DEV), Permutation(SEED, DEV)
    two = torch.cat([a.fill(B, 2), a.fill(B, 2)])
    four = b.fill(B, 4)
    assert torch.equal(two, four) and a.counter == b.counter == 4
    assert np.array_equal(four.cpu().numpy(), host_perm(0, B, 4))
    a.close()
    b.close()


def test_a_captured_fill_replayed_twice_equals_two_eager_fills():
    B = 2048
    p, out = Permutation(SEED, DEV), torch.zeros((2, B), dtype=I64, device=DEV)
    p.counter = 5
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p.fill(B, 2, out=out)
    torch.cuda.synchronize()
    assert p.counter == 5 and not out.any()   # the capture ran nothing
    want = host_perm(5, B, 4)
    graph.replay()
    assert np.array_equal(out.cpu().numpy(), want[:2]) and p.counter == 7
    graph.replay()
    assert np.array_equal(out.cpu().numpy(), want[2:]) and p.counter == 9
    p.close()


def test_an_assigned_counter_the_wrap_and_a_side_stream():
    B = 17
    p = Permutation(SEED, DEV)
    p.counter = 2 ** 32 - 1
    got = p.fill(B, 3).cpu().numpy()
    assert p.counter == 2   # 2^32 - 1, 0, 1
    for j, c in enumerate((2 ** 32 - 1, 0, 1)):
        assert np.array_equal(got[j], rng.permutation(B, SEED, c))
    p.counter = 2 ** 32 - 1
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = p.fill(B, 3)
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert np.array_equal(other.cpu().numpy(), got) and p.counter == 2
    for bad in (dict(B=0), dict(B=5, n_perms=0), dict(B=5, n_perms=65536), dict(B=5, out=torch.zeros((1, 5), dtype=I64)),
                dict(B=5, out=torch.zeros((1, 5), dtype=torch.int32, device=DEV))):
        with pytest.raises(_native.PbgError):
            p.fill(**bad)
    p.close()
    with pytest.raises(_native.PbgError):
        p.fill(5)


# ---------------------------------------------------------------------------- AdamClip.step with a device lr
def _final(opt, p):
    m, v, t = opt.state()
    return [a.cpu().numpy() for a in p + m + v] + [t.cpu().numpy()]


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_device_lr_gives_the_bits_of_the_float():
    sizes = od.SIZES[3]
    runs = []
    for as_tensor in (False, True):
        opt, p = AdamClip(sizes, DEV), [dev(a) for a in od.params0(sizes)]
        lr = torch.zeros(1, dtype=F64, device=DEV)
        for s in range(3):
            value = od.LR * (1.0 - s / 7.0)
            lr.fill_(value)
            opt.step(p, [dev(a) for a in od.grads_of(sizes, s)], lr if as_tensor else value, od.BETAS, od.EPS, 0.5)
        runs.append(_final(opt, p))
        opt.close()
    assert _same(*runs)
    host, hp = AdamClip(sizes), od.params0(sizes)
    for s in range(3):
        host.step(hp, od.grads_of(sizes, s), od.LR * (1.0 - s / 7.0), od.BETAS, od.EPS, 0.5)
    assert _same(runs[0][:3], hp)
    opt = AdamClip(sizes, DEV)
    p, g = [dev(a) for a in od.params0(sizes)], [dev(a) for a in od.grads_of(sizes, 0)]
    for bad in (torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F32, device=DEV), torch.zeros(2, dtype=F64, device=DEV),
                np.zeros(1)):
        with pytest.raises(_native.PbgError):
            opt.step(p, g, bad)
    opt.close()


def test_a_captured_step_follows_its_lr_tensor():
    sizes = od.SIZES[3]
    g = [dev(a) for a in od.grads_of(sizes, 1)]
    old, new = od.LR, 0.25 * od.LR

    def eager(second):
        opt, p = AdamClip(sizes, DEV), [dev(a) for a in od.params0(sizes)]
        opt.step(p, g, old, od.BETAS, od.EPS, 0.5)
        opt.step(p, g, second, od.BETAS, od.EPS, 0.5)
        out = _final(opt, p)
        opt.close()
        return out

    opt, p = AdamClip(sizes, DEV), [dev(a) for a in od.params0(sizes)]
    lr = torch.full((1,), old, dtype=F64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(p, g, lr, od.BETAS, od.EPS, 0.5)
    graph.replay()
    lr.fill_(new)
    graph.replay()
    got = _final(opt, p)
    opt.close()
    assert _same(got, eager(new))
    assert not _same(got[:3], eager(old)[:3])


# ---------------------------------------------------------------------------- the trainers
ENV_ID = "InvertedPendulumPyBulletEnv-v0"
SMALL = dict(hidden=(16, 8), steps=8, lr=3e-3, epochs=2, minibatches=2, log_std=-0.5)
SMALL_N, N_SCHED = 64, 5


def _trainer(n=SMALL_N, hp=SMALL, seed=3, **kw):
    env = VecEnv(ENV_ID, n, device=DEV, seed=seed, autoreset=True, precision=64)
    return env, PPO(env, seed=seed, backward="hip", optimizer="hip", **dict(hp, **kw))


def _snapshot(ppo):
    """What an iteration leaves: the parameters, the optimiser's state, the statistics' totals, the three counters and
    the env's state."""
    m, v, t = ppo.adam.state()
    phys, aux = ppo.env.get_state()
    out = dict(actor=ppo.actor_theta.data, critic=ppo.critic_theta.data, log_std=ppo.log_std.data, m=torch.cat(m),
               v=torch.cat(v), t=t, phys=phys, aux=aux)
    out = {k: x.cpu().numpy().copy() for k, x in out.items()}
    out["noise_counter"] = np.array([ppo.noise.counter])
    out["perm_counter"] = np.array([ppo.perm.counter])
    if ppo._it_dev is not None:
        out["iteration"] = ppo._it_dev.cpu().numpy().copy()
    if ppo.obs_stats is not None:
        out["totals"] = ppo.obs_stats.totals.cpu().numpy()
    return out


def _assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        poison.assert_same_bits(a[k], b[k], f"{what}: {k}")


def _three_iterations(obs_norm, **kw):
    """Per iteration: the snapshot, the learning rate the update used and the indices it used."""
    env, ppo = _trainer(obs_norm=obs_norm, permutation="device", lr_schedule="linear", schedule_iterations=N_SCHED, **kw)
    out = []
    for _ in range(3):
        ppo.iterate()
        out.append((_snapshot(ppo), ppo._lr_dev.cpu().numpy().copy(), ppo._perm.cpu().numpy().copy()))
    graphs = (ppo._graph is not None, ppo._iter_graph is not None)
    ppo.close()
    env.close()
    return out, graphs


@pytest.fixture(scope="module", params=(False, True), ids=("plain", "obs_norm"))
def eager_run(request):
    out, graphs = _three_iterations(request.param)
    assert graphs == (False, False)
    return request.param, out


def test_the_eager_device_trainer_uses_the_numpy_permutations_and_schedule(eager_run):
    obs_norm, out = eager_run
    B, E, M = SMALL_N * SMALL["steps"], SMALL["epochs"], SMALL["minibatches"]
    for i, (snap, lr, perm) in enumerate(out):
        assert lr.tobytes() == np.float64(rng.lr_linear(i, N_SCHED, SMALL["lr"])).tobytes(), i
        assert perm.shape == (E, M, B // M)
        for e in range(E):
            assert np.array_equal(perm[e].reshape(B), rng.permutation(B, 3, i * E + e)), (i, e)
        assert int(snap["perm_counter"][0]) == (i + 1) * E and int(snap["iteration"][0]) == i + 1
        assert int(snap["noise_counter"][0]) == (i + 1) * SMALL["steps"] and int(snap["t"][0]) == (i + 1) * E * M
        assert all(np.isfinite(snap[k]).all() for k in ("actor", "critic", "log_std"))
    assert out[0][1][0] == SMALL["lr"] and out[2][1][0] < out[1][1][0] < out[0][1][0]
    assert not np.array_equal(out[0][0]["actor"], out[1][0]["actor"])


@pytest.mark.parametrize("graph", (True, "iteration"))
def test_the_graph_trainers_hold_the_eager_trainers_bits(eager_run, graph):
    obs_norm, want = eager_run
    got, graphs = _three_iterations(obs_norm, graph=graph)
    assert graphs == (graph is True, graph == "iteration")
    for i, ((snap, lr, perm), (wsnap, wlr, wperm)) in enumerate(zip(got, want)):
        _assert_same(snap, wsnap, f"graph={graph!r} obs_norm {obs_norm} iteration {i}")
        assert lr.tobytes() == wlr.tobytes() and np.array_equal(perm, wperm), i


def test_evaluate_between_two_replays_changes_nothing():
    test = VecEnv(ENV_ID, 16, device=DEV, seed=0, autoreset=False, precision=64)
    finals = []
    for evaluates in (False, True):
        env, ppo = _trainer(obs_norm=True, permutation="device", lr_schedule="linear", schedule_iterations=N_SCHED,
                            graph="iteration")
        for _ in range(2):
            ppo.iterate()
        if evaluates:
            before = _snapshot(ppo)
            ret, length = ppo.evaluate(test, 20)
            assert np.isfinite(ret.cpu().numpy()).all()
            _assert_same(_snapshot(ppo), before, "evaluate")
        ppo.iterate()
        finals.append(_snapshot(ppo))
        ppo.close()
        env.close()
    test.close()
    _assert_same(finals[1], finals[0], "the iteration after evaluate")


def test_refused_combinations():
    env = VecEnv(ENV_ID, SMALL_N, device=DEV, seed=0, autoreset=True, precision=64)
    hip = dict(backward="hip", optimizer="hip")
    for kw in (dict(hip, graph="iteration"), dict(hip, graph="iteration", permutation="torch"),
               dict(backward="hip", permutation="device"), dict(permutation="device"),
               dict(backward="hip", lr_schedule="linear", schedule_iterations=5),
               dict(lr_schedule="linear", schedule_iterations=5),
               dict(hip, lr_schedule="cosine", schedule_iterations=5), dict(hip, lr_schedule="linear"),
               dict(hip, lr_schedule="linear", schedule_iterations=0), dict(hip, permutation="numpy"),
               dict(hip, graph="update"), dict(backward="hip", graph="iteration", permutation="device")):
        with pytest.raises(_native.PbgError):
            PPO(env, **dict(SMALL, **kw))
    env.close()


def test_a_moved_baked_buffer_raises():
    env, ppo = _trainer(permutation="device", graph="iteration")
    for _ in range(2):
        ppo.iterate()
    io, traj = env._ro_io[(SMALL["steps"], True)]
    traj["act_traj"] = traj["act_traj"].clone()   # what another owner of the env's buffers might do
    with pytest.raises(_native.PbgError, match="moved"):
        ppo.iterate()
    ppo.close()
    env.close()


def test_the_iteration_graph_trainer_learns_to_balance_the_pendulum():
    """tests/test_ppoopt_gpu.py's learning test with permutation="device", graph="iteration" and no schedule: the same
    hyperparameters, 30 iterations, the noise-free mean policy on section 11's 256 fixed initial states, first episode,
    200 steps; section 13's bar."""
    hp = dict(hidden=(64, 64), steps=32, lr=3e-3, epochs=4, minibatches=4, log_std=-0.5)
    env, ppo = _trainer(256, hp, seed=0, permutation="device", graph="iteration")
    test = VecEnv(ENV_ID, 256, device=DEV, seed=0, autoreset=False, precision=64)
    q0 = torch.from_numpy(policies.reset_draws(256, test.info.reset_dofs, 0).astype(np.float32))
    length = lambda: ppo.evaluate(test, 200, init_q=q0)[1].cpu().numpy().astype(np.float64)  # noqa: E731
    before, curve = length(), []
    for it in range(1, 31):
        ppo.iterate()
        if it % 5 == 0:
            curve.append((it, float(length().mean())))
    after = length()
    assert ppo._iter_graph is not None and ppo.perm.counter == 30 * 4
    ppo.close()
    env.close()
    test.close()
    print(f"untrained {before.mean():.2f} (std {before.std():.2f}); curve {curve}; after 30: {after.mean():.2f}")
    assert after.mean() >= 150.0
    assert after.mean() > 21.46 + 3.0 * 6.74
    assert after.mean() > before.mean() + 3.0 * before.std()


# ---------------------------------------------------------------------------- uninitialised-memory invariance
@pytest.mark.parametrize("B", (17, 65537))
def test_perm_fill_is_invariant(B):
    runs = []
    for run in RUNS:
        p, out = Permutation(SEED, DEV), Guarded((3, B), I64, DEV)
        p.counter = 2 ** 32 - 2
        poison.poison_run(run, None, DEV)
        p.fill(B, 3, out=out.view)
        runs.append(dict(perm=out.numpy("fill"), counter=np.array([p.counter])))
        p.close()
    poison.assert_runs_agree(runs, f"perm fill B {B}")
    poison.assert_same_bits(runs[0]["perm"], host_perm(2 ** 32 - 2, B, 3), "perm fill against the host twin")
    assert int(runs[0]["counter"][0]) == 1


def test_lr_linear_is_invariant():
    N, lr0 = 1000, 0.1 + 0.2
    for it in (0, 7, 999, 1005):
        runs = []
        for run in RUNS:
            i, out = surrounded(np.array([it], np.int32), run, DEV), Guarded(1, F64, DEV)
            poison.poison_run(run, None, DEV)
            lr_linear(i, N, lr0, out=out.view)
            runs.append(dict(lr=out.numpy("lr_linear")))
        poison.assert_runs_agree(runs, f"lr_linear it {it}")
        poison.assert_same_bits(runs[0]["lr"], lr_linear(np.array([it], np.uint32), N, lr0), "lr_linear against the host twin")


@pytest.mark.parametrize("shift", (0, 1))
def test_the_lr_ptr_step_is_invariant(shift):
    """tests/test_learner_invariance_gpu.py's optimiser case with the learning rate read from device memory."""
    sizes = od.SIZES[3]
    lrs = [od.LR * (1.0 - s / 7.0) for s in range(3)]
    runs = []
    for run in RUNS:
        opt = AdamClip(sizes, DEV)
        params = [Guarded(s, F32, DEV, shift=shift, init=p) for s, p in zip(sizes, od.params0(sizes))]
        out = {}
        for s in range(3):
            grads = [surrounded(g, run, DEV, shift=shift) for g in od.grads_of(sizes, s)]
            lr, info = surrounded(np.array([lrs[s]]), run, DEV), Guarded(2, F64, DEV)
            poison.poison_run(run, None, DEV)
            opt.step([p.view for p in params], grads, lr, od.BETAS, od.EPS, 0.5, info=info.view)
            out[f"info{s}"] = info.numpy("info")
            out[f"params{s}"] = np.concatenate([p.numpy("params") for p in params])
            m, v, t = opt.state()
            out[f"m{s}"], out[f"v{s}"] = (torch.cat(x).cpu().numpy() for x in (m, v))
        runs.append(out)
        opt.close()
    what = f"AdamClip with lr_ptr, shift {shift}"
    poison.assert_runs_agree(runs, what)
    host, hp = AdamClip(sizes), od.params0(sizes)
    for s in range(3):
        info = np.zeros(2)
        host.step(hp, od.grads_of(sizes, s), np.array([lrs[s]]), od.BETAS, od.EPS, 0.5, info=info)
        poison.assert_same_bits(runs[0][f"info{s}"], info, f"{what} info, step {s}")
        poison.assert_same_bits(runs[0][f"params{s}"], np.concatenate(hp), f"{what} params, step {s}")
        m, v, _ = host.state()
        poison.assert_same_bits(runs[0][f"m{s}"], np.concatenate(m), f"{what} m, step {s}")
        poison.assert_same_bits(runs[0][f"v{s}"], np.concatenate(v), f"{what} v, step {s}")
