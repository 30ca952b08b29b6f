"""Bootstrapping through TimeLimit truncations on the device (include/pbg.h "Truncation bootstrapping", DESIGN.md
section 19): the rollout's truncation records (pbg_rollout_io_t version 2) against the step-by-step loop, the masked
actor launch (pbg_population_act_where) against the dense actor bit for bit, pbg_gae_trunc against its host twin, the
uninitialised-memory invariance of both new kernels, and the trainer's ``truncation="bootstrap"``."""
import ctypes

import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.distributed import ShardedVecEnv
from pybulletgym_amd.policy import MLPPopulation
from pybulletgym_amd.ppo import PPO, ShardedPPO, gae
from pybulletgym_amd.vec_env import VecEnv

import gae_data as gd
import poison
import policies
import trunc_data as td
from poison import RUNS, Guarded, assert_same_bits, surrounded
from test_policy_gpu import FIELDS, _assert_same
from test_obsnorm_host import make_norm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, U8 = torch.float32, torch.uint8


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


# ---------------------------------------------------------------------------- the rollout's records
def _env(env_id, n, precision, elapsed, autoreset=True):
    """A fresh env on the shared reset draws; ``elapsed(e)``: (mask, value) for the elapsed-steps word aux[:, 2]."""
    env = VecEnv(env_id, n, device=DEV, seed=0, autoreset=autoreset, precision=precision)
    env.reset(init_q=torch.from_numpy(policies.reset_draws(n, env.info.reset_dofs, 0).astype(np.float32)))
    if elapsed is not None:
        phys, aux = env.get_state()
        mask, value = elapsed(torch.arange(n, device=DEV))
        aux[:, 2] = torch.where(mask, value.to(aux.dtype), aux[:, 2])
        env.set_state(phys, aux)
    return env


def _constant_actor(env):
    """One pair with all weights zero and b3 = +1 (member 0, the first half of the envs) / -1 (member 1)."""
    pi = MLPPopulation((env.info.obs_dim, 4, 4, env.info.action_dim), 1, DEV)
    for m, b3 in ((0, 1.0), (1, -1.0)):
        theta = torch.zeros(pi.n_params, dtype=F32, device=DEV)
        theta[-env.info.action_dim:] = b3
        pi.set_member(m, theta)
    return pi


def _loop(env, pi, steps):
    """``pi.act`` then ``env.step``, step by step: what each step reports."""
    out = dict(done=[], truncated=[], terminal_obs=[])
    for _ in range(steps):
        r = env.step(pi.act(env.obs))
        out["done"].append(r.done.clone())
        out["truncated"].append(r.truncated.clone())
        out["terminal_obs"].append(r.terminal_obs.clone())
    return {k: torch.stack(v).cpu().numpy() for k, v in out.items()}


def _recording_case(env_id, n, precision, T, elapsed):
    a, b, c = (_env(env_id, n, precision, elapsed) for _ in range(3))
    pi = _constant_actor(a)
    want = _loop(a, pi, T)
    res = b.rollout(pi, T, trajectory=True, truncation=True)
    plain = c.rollout(pi, T, trajectory=True)
    assert plain.trunc_traj is None and plain.term_obs_traj is None
    torch.cuda.synchronize()
    done, trunc, tobs = (t.cpu().numpy() for t in (res.done_traj, res.trunc_traj, res.term_obs_traj))
    assert trunc.dtype == np.uint8 and trunc.shape == (T, n) and tobs.dtype == np.float32
    assert tobs.shape == (T, n, a.info.obs_dim)
    assert np.array_equal(done, want["done"])
    assert np.array_equal(trunc, want["truncated"])
    assert not (trunc & (done == 0)).any()
    # the step-by-step env keeps the last terminal observation of every env; the trajectory holds row (t, e) where done
    # is set (the other rows were never written: the buffer's initial zeros)
    for t in range(T):
        at = done[t] != 0
        assert_same_bits(tobs[t][at], want["terminal_obs"][t][at], f"{env_id} term_obs_traj[{t}]")
        assert not tobs[t][~at].any(), t
    # nothing else the rollout produces changes
    _assert_same(res, {f: getattr(plain, f) for f in FIELDS})
    for e in (a, b, c):
        e.close()
    pi.close()
    return done, trunc


def test_rollout_records_truncations_and_terminal_observations_pendulum():
    """InvertedPendulumPyBulletEnv-v0 (lane kernel), 96 envs, float64, 12 steps under a constant +-1 action: the envs
    with e % 3 == 1 start at elapsed 999 - (e % 5) and are truncated at steps 0 .. 4, every env falls at a step in
    5 .. 10 (and the restarted ones again later), so the window holds both kinds of done and some 16-env tile holds
    both (at their own steps: no step of the window has both, the truncations come first)."""
    done, trunc = _recording_case("InvertedPendulumPyBulletEnv-v0", 96, 64, 12,
                                  lambda e: (e % 3 == 1, 999 - (e % 5)))
    term = (done != 0) & (trunc == 0)
    print(f"truncated pairs {int(trunc.sum())}, terminated pairs {int(term.sum())}")
    assert int(trunc.sum()) >= 24 and int(term.sum()) >= 48
    tiles_trunc, tiles_term = trunc.reshape(12, 6, 16).any(axis=(0, 2)), term.reshape(12, 6, 16).any(axis=(0, 2))
    assert (tiles_trunc & tiles_term).any()


def test_rollout_records_truncations_gang_kernel_hopper():
    """HopperPyBulletEnv-v0 (gang kernel), 32 envs, float32, 6 steps: the odd envs are truncated at steps 0 .. 2, the
    envs of the member that pushes with -1 fall at step 3."""
    done, trunc = _recording_case("HopperPyBulletEnv-v0", 32, 32, 6, lambda e: (e % 2 == 1, 999 - (e % 3)))
    term = (done != 0) & (trunc == 0)
    print(f"truncated pairs {int(trunc.sum())}, terminated pairs {int(term.sum())}")
    assert int(trunc.sum()) >= 16 and int(term.sum()) >= 8


def test_rollout_truncation_refusals():
    env = _env("InvertedPendulumPyBulletEnv-v0", 32, 64, None)
    pi = _constant_actor(env)
    with pytest.raises(_native.PbgError):
        env.rollout(pi, 2, truncation=True)                      # no trajectories
    off = _env("InvertedPendulumPyBulletEnv-v0", 32, 64, None, autoreset=False)
    with pytest.raises(_native.PbgError):
        off.rollout(pi, 2, trajectory=True, truncation=True)     # nothing resets: nothing to record
    assert (2, True, True) not in env._ro_io and (2, True, True) not in off._ro_io
    env.rollout(pi, 2, trajectory=True, truncation=True)
    io, traj = env._ro_io[(2, True, True)]
    assert io.struct_size == ctypes.sizeof(_native.RolloutIO2) == ctypes.sizeof(_native.RolloutIO) + 16
    # the C struct: one of the pair, or the pair without autoreset, is PBG_E_ARG before any launch
    L, before = _native.lib(), env.get_state()[1].clone()
    call = lambda: L.pbg_rollout_population(env._h, pi._h, ctypes.byref(io), _stream())  # noqa: E731
    both = (io.trunc_traj, io.term_obs_traj)
    for keep in (0, 1):
        io.trunc_traj, io.term_obs_traj = (both[0], None) if keep == 0 else (None, both[1])
        assert call() == -1
        with pytest.raises(_native.PbgError):
            env.rollout(pi, 2, trajectory=True, truncation=True)
    io.trunc_traj, io.term_obs_traj = both
    io.autoreset = 0
    assert call() == -1
    # a size that is neither version's
    io.autoreset = 1
    io.struct_size -= 8
    assert call() == -1
    io.struct_size += 8
    torch.cuda.synchronize()
    assert torch.equal(env.get_state()[1], before)               # no refused call stepped the env
    assert call() == 0
    # the same buffers every call, and the plain key keeps its own
    again = env.rollout(pi, 2, trajectory=True, truncation=True)
    assert again.term_obs_traj.data_ptr() == traj["term_obs_traj"].data_ptr()
    plain = env.rollout(pi, 2, trajectory=True)
    assert plain.obs_traj.data_ptr() != again.obs_traj.data_ptr() and set(env._ro_io) == {(2, True, True), (2, True)}
    assert env._ro_io[(2, True)][0].struct_size == ctypes.sizeof(_native.RolloutIO)
    for o in (pi, env, off):
        o.close()


# ---------------------------------------------------------------------------- the masked launch
WHERE_DIMS = ((5, 64, 64, 1), (11, 33, 17, 3), (28, 128, 64, 1))
WHERE_SIZES = ((3, 40), (2, 96))   # (T, n): 20 rows a member (a partly filled last tile), and 48
PATTERNS = ("none", "all", "one row", "one step", "random")


def _flags(pattern, T, n):
    f = np.zeros((T, n), np.uint8)
    if pattern == "all":
        f[:] = 1
    elif pattern == "one row":
        f[T - 1, n // 2 + 3] = 1
    elif pattern == "one step":
        f[T // 2] = 1
    elif pattern == "random":
        f[:] = np.random.default_rng([T, n]).random((T, n)) < 0.1
        assert f.any() and not f.all()
    return f


def _population(dims, normed):
    pop = MLPPopulation(dims, 1, DEV)
    pop.perturb(pop.init_theta(dims[1]), 0.5, 77, 0)   # two different members
    if normed:
        mean, inv_std = make_norm(dims[0])
        pop.set_obs_norm(dev(mean), dev(inv_std), clip=5.0)
    return pop


def _where_obs(dims, T, n, flags, word=0x7FC00000):
    """Seeded rows (3 sigma, so that a normaliser's clip acts); every unflagged row is filled with ``word``."""
    obs = (3.0 * np.random.default_rng([T, n, dims[0]]).standard_normal((T, n, dims[0]))).astype(np.float32)
    obs.view(np.uint32)[flags == 0] = word
    return obs


def _dense_reference(pop, flags, obs):
    """``pop.act`` on the flagged rows gathered into a dense batch, each member's rows in its half (padded with zero
    rows to equal halves); +0.0 everywhere else."""
    T, n = flags.shape
    G, A = n // 2, pop.act_dim
    want = np.zeros((T, n, A), np.float32)
    at = [np.argwhere((flags != 0) & ((np.arange(n) // G) == m)[None, :]) for m in (0, 1)]
    L = max(len(at[0]), len(at[1]))
    if L == 0:
        return want
    batch = np.zeros((2, L, pop.obs_dim), np.float32)
    for m in (0, 1):
        batch[m, :len(at[m])] = obs[at[m][:, 0], at[m][:, 1]]
    out = pop.act(dev(batch.reshape(2 * L, -1))).cpu().numpy().reshape(2, L, A)
    for m in (0, 1):
        want[at[m][:, 0], at[m][:, 1]] = out[m, :len(at[m])]
    return want


@pytest.mark.parametrize("normed", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("size", WHERE_SIZES, ids=str)
@pytest.mark.parametrize("dims", WHERE_DIMS, ids=str)
def test_act_where_equals_the_dense_actor_on_the_flagged_rows(dims, size, normed):
    T, n = size
    pop = _population(dims, normed)
    for pattern in PATTERNS:
        flags = _flags(pattern, T, n)
        obs = _where_obs(dims, T, n, flags)
        want = _dense_reference(pop, flags, obs)
        assert np.isfinite(want).all() and (pattern == "none" or want.any())
        out = Guarded((T, n, dims[3]), F32, DEV)
        got = pop.act_where(dev(flags), dev(obs), out=out.view)
        assert got.data_ptr() == out.view.data_ptr()
        what = f"act_where {dims} {size} {pattern}"
        got = out.numpy(what)
        assert_same_bits(got, want, what)   # the flagged rows' bits, +0.0 bits elsewhere, every element written
    fresh = pop.act_where(dev(flags), dev(obs))
    assert_same_bits(fresh, want, "a fresh out")
    pop.close()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("normed", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("dims", WHERE_DIMS, ids=str)
def test_act_where_is_invariant(dims, normed, shift):
    """Once as it is and once under each poison pattern (LDS and register file), the unflagged obs rows filled with
    the run's pattern, flags and obs inside pattern-filled buffers (shift 1: off the 16-byte alignment): the same
    bits, which are the dense actor's."""
    T, n = WHERE_SIZES[0]
    pop = _population(dims, normed)
    flags = _flags("random", T, n)
    flags[0, :16], flags[1, 16:20] = 0, 1   # a tile without a flag, and a partly filled tile with every row flagged
    runs = []
    for run in RUNS:
        obs = _where_obs(dims, T, n, flags, poison.PATTERNS[0][0] if run is None else run[0])
        f, x = surrounded(flags, run, DEV, shift=shift), surrounded(obs, run, DEV, shift=shift)
        out = Guarded((T, n, dims[3]), F32, DEV, shift=shift)
        poison.poison_run(run, None, DEV)
        pop.act_where(f, x, out=out.view)
        runs.append(dict(out=out.numpy(f"act_where {dims} under {run}")))
    poison.assert_runs_agree(runs, f"act_where {dims}")
    assert_same_bits(runs[0]["out"], _dense_reference(pop, flags, obs), f"act_where {dims}")
    pop.close()


def test_act_where_on_a_side_stream_and_in_a_replayed_graph():
    dims, (T, n) = WHERE_DIMS[1], WHERE_SIZES[1]
    pop = _population(dims, True)
    flags = _flags("random", T, n)
    obs = _where_obs(dims, T, n, flags)
    f, x = dev(flags), dev(obs)
    want = pop.act_where(f, x).cpu().numpy()
    assert want.any()
    out = torch.full((T, n, dims[3]), np.nan, dtype=F32, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        pop.act_where(f, x, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert_same_bits(out, want, "side stream")
    out.fill_(np.nan)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pop.act_where(f, x, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())   # the capture ran nothing
    for _ in range(2):
        graph.replay()
        assert_same_bits(out, want, "replay")
        out.fill_(np.nan)
    pop.close()


def test_act_where_argument_errors():
    """PBG_E_ARG before any HIP call.  (A host-only population cannot be built: pbg_population_create refuses it, so
    that check of the entry point has no caller to test it with.)"""
    dims, T, n = WHERE_DIMS[0], 2, 32
    pop = _population(dims, False)
    L = _native.lib()
    f, x = torch.ones((T, n), dtype=U8, device=DEV), torch.zeros((T, n, dims[0]), dtype=F32, device=DEV)
    out = torch.full((T, n, dims[3]), np.nan, dtype=F32, device=DEV)
    ptrs = [pop._h, f.data_ptr(), x.data_ptr(), out.data_ptr()]
    call = lambda p, T, n, f, x, o: L.pbg_population_act_where(p, T, n, f, x, o, _stream())  # noqa: E731
    for i in range(4):
        args = list(ptrs)
        args[i] = None
        assert call(args[0], T, n, *args[1:]) == -1, i
    for bad_T, bad_n in ((0, n), (-1, n), (T, 0), (T, -2), (T, 31), (2 ** 30, n)):   # the last: 2^31 workgroups
        assert call(ptrs[0], bad_T, bad_n, *ptrs[1:]) == -1, (bad_T, bad_n)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    for bad in (dict(flags=f.to(torch.int32)), dict(flags=f[:, :31]), dict(flags=f.cpu()), dict(obs=x[:1]), dict(obs=x.double()),
                dict(obs=x[:, :, :4]), dict(out=out[:, :, 0]), dict(out=torch.empty((T, n, 2), device=DEV)), dict(flags=f[0])):
        kw = dict(flags=f, obs=x, out=out)
        kw.update(bad)
        with pytest.raises(_native.PbgError):
            pop.act_where(kw["flags"], kw["obs"], out=kw["out"])
    assert call(*ptrs[:1], T, n, *ptrs[1:]) == 0
    pop.close()
    with pytest.raises(_native.PbgError):
        pop.act_where(f, x)


# ---------------------------------------------------------------------------- pbg_gae_trunc
@pytest.mark.parametrize("n", gd.NS + (257,))
@pytest.mark.parametrize("T", gd.TS)
def test_gae_trunc_equals_the_host_twin_and_is_invariant(T, n):
    """One lane per env: n = 257 needs a second workgroup with one live lane.  The inputs inside pattern-filled
    buffers, the outputs between guards, the LDS and register file poisoned: the host twin's bits every time."""
    rew, done, trunc, value, term_value = td.case(T, n)
    want = gae(rew, done, value, 0.99, 0.95, trunc_traj=trunc, term_value=term_value)
    runs = []
    for run in RUNS:
        args = [surrounded(a, run, DEV) for a in (rew, done, value)]
        tr, tv = surrounded(trunc, run, DEV), surrounded(term_value, run, DEV)
        adv, ret = Guarded((T, n), F32, DEV), Guarded((T, n), F32, DEV)
        poison.poison_run(run, None, DEV)
        gae(*args, 0.99, 0.95, adv=adv.view, ret=ret.view, trunc_traj=tr, term_value=tv)
        runs.append(dict(adv=adv.numpy(f"gae_trunc adv {T} x {n}"), ret=ret.numpy(f"gae_trunc ret {T} x {n}")))
    poison.assert_runs_agree(runs, f"gae_trunc {T} x {n}")
    assert_same_bits(runs[0]["adv"], want[0], "adv")
    assert_same_bits(runs[0]["ret"], want[1], "ret")
    # without truncations: pbg_gae's bits
    zero = torch.zeros((T, n), dtype=U8, device=DEV)
    plain = gae(dev(rew), dev(done), dev(value), 0.99, 0.95)
    same = gae(dev(rew), dev(done), dev(value), 0.99, 0.95, trunc_traj=zero, term_value=dev(term_value))
    assert_same_bits(same[0], plain[0], "adv without truncations")
    assert_same_bits(same[1], plain[1], "ret without truncations")


def test_gae_trunc_argument_errors():
    rew, done, trunc, value, term_value = (dev(a) for a in td.case(2, 4))
    for kw in (dict(trunc_traj=trunc), dict(term_value=term_value), dict(trunc_traj=trunc.int(), term_value=term_value),
               dict(trunc_traj=trunc, term_value=term_value[:1]), dict(trunc_traj=trunc.cpu(), term_value=term_value)):
        with pytest.raises(_native.PbgError):
            gae(rew, done, value, **kw)


# ---------------------------------------------------------------------------- the trainer
ENV_ID, N, STEPS = "InvertedPendulumPyBulletEnv-v0", 64, 8
KW = dict(hidden=(16, 16), steps=STEPS, seed=0, backward="hip", optimizer="hip", permutation="device")


def _age(env):
    """The elapsed word to 1000 - 12 - (e % 8): an env that stays up is truncated at step 11 + (e % 8) of the run,
    inside iterations 1 and 2 (0-based) of 8 steps."""
    phys, aux = env.get_state()
    aux[:, 2] = (1000 - 12 - (torch.arange(env.num_envs, device=DEV) % 8)).to(aux.dtype)
    env.set_state(phys, aux)


def _trainer(cls=PPO, **kw):
    if cls is PPO:
        env = holder = VecEnv(ENV_ID, N, device=DEV, seed=0, autoreset=True, precision=64)
    else:
        holder = ShardedVecEnv(ENV_ID, N, 0, 1, DEV, seed=0, autoreset=True, precision=64)
        env = holder.env
    ppo = cls(holder, **dict(KW, **kw))
    _age(env)
    return env, ppo


def _params(ppo):
    torch.cuda.synchronize()
    return {k: getattr(ppo, k).data.cpu().numpy().copy() for k in ("actor_theta", "critic_theta", "log_std")}


def _run(iterations, cls=PPO, **kw):
    env, ppo = _trainer(cls, **kw)
    for _ in range(iterations):
        ppo.iterate()
    out = _params(ppo)
    ppo.close()
    env.close()
    return out


def _assert_same_params(a, b, what):
    for k in a:
        assert_same_bits(a[k], b[k], f"{what} {k}")


def test_collect_bootstraps_through_the_truncations():
    """Three iterations spelled out (collect, checks, update): adv and ret are the numpy restatement of the batch's
    own trajectories and values, term_value is the critic on the flagged terminal observations and +0.0 elsewhere;
    iterations 1 and 2 hold truncations."""
    env, ppo = _trainer(truncation="bootstrap")
    counts = []
    for it in range(3):
        b = ppo.collect()
        res_io, traj = env._ro_io[(STEPS, True, True)]
        rew, done, trunc, value, term_value, adv, ret = (t.cpu().numpy() for t in (b.rew, b.done, b.trunc, b.value, b.term_value,
                                                                                  b.adv, b.ret))
        counts.append(int(trunc.sum()))
        assert not (trunc & (done == 0)).any()
        want_adv, want_ret = td.gae_trunc_numpy(rew, done, trunc, value, term_value, ppo.gamma, ppo.lam)
        assert_same_bits(adv, want_adv, f"iteration {it} adv")
        assert_same_bits(ret, want_ret, f"iteration {it} ret")
        at = np.argwhere(trunc != 0)
        want_tv = np.zeros((STEPS, N), np.float32)
        if len(at):
            rows = traj["term_obs_traj"].cpu().numpy()[at[:, 0], at[:, 1]]
            rows = np.concatenate([rows, np.zeros((len(rows) % 2, rows.shape[1]), np.float32)])   # an even batch
            want_tv[at[:, 0], at[:, 1]] = ppo.critic.act(dev(rows)).cpu().numpy()[:len(at), 0]
            plain = gae(b.rew, b.done, b.value, ppo.gamma, ppo.lam)[0].cpu().numpy()
            assert (plain[trunc != 0] != adv[trunc != 0]).any()
        assert_same_bits(term_value, want_tv, f"iteration {it} term_value")
        ppo.update(b)
        ppo.iteration += 1
    print(f"truncated pairs per iteration: {counts}")
    assert counts[0] == 0 and counts[1] >= 1 and counts[2] >= 1
    ppo.close()
    env.close()


def test_terminal_is_the_default_and_bootstrap_differs():
    spelled, omitted = _run(3, truncation="terminal"), _run(3)
    _assert_same_params(spelled, omitted, "terminal against the default")
    boot = _run(3, truncation="bootstrap")
    assert any(not np.array_equal(boot[k], omitted[k]) for k in boot)
    with pytest.raises(_native.PbgError):
        _trainer(truncation="bootstrapped")


@pytest.mark.parametrize("graph", [True, "iteration"], ids=["update-graph", "iteration-graph"])
def test_bootstrap_under_a_graph_holds_the_eager_bits(graph):
    """Four iterations: the truncations of iterations 1 and 2 lie inside replayed graphs."""
    _assert_same_params(_run(4, truncation="bootstrap", graph=graph), _run(4, truncation="bootstrap"), f"graph={graph}")


def test_sharded_world_one_holds_the_trainers_bits():
    _assert_same_params(_run(3, ShardedPPO, truncation="bootstrap"), _run(3, truncation="bootstrap"), "ShardedPPO")


def test_bootstrap_learns_to_balance_the_pendulum():
    """tests/test_ppo_gpu.py's configuration and iteration count with ``truncation="bootstrap"``: the mean
    first-episode length must exceed the untrained policy's mean by three of its standard deviations, that test's
    relative criterion.  (Its absolute 150 of 200 is not asserted here: nobody had measured this mode when the test
    was written; DESIGN.md section 19 holds the number.)"""
    import test_ppo_gpu as tp
    iterations = tp.MEASURED + tp.MEASURED // 2
    before, after, _ = tp._train(iterations, hp=dict(tp.HP, truncation="bootstrap"))
    print(f"untrained mean policy: mean first-episode length {before.mean():.2f} (std {before.std():.2f}); "
          f"after {iterations} iterations with truncation='bootstrap': {after.mean():.2f} (std {after.std():.2f}) of 200")
    assert after.mean() > before.mean() + 3.0 * before.std()
