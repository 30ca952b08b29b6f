"""The uninitialised-memory invariance of tests/test_gpu.py's step kernels, extended to the
learner: the actors (pbg_policy.hip, pbg_population.hip), the observation statistics (pbg_obsnorm.hip), the action
noise and GAE (pbg_actnoise.hip), the PPO gradient (pbg_ppograd.hip) and the optimiser step (pbg_ppoopt.hip).

Every case runs once as it is and once under each of tests/poison.py's three patterns, the poison (every CU's LDS,
the env handle's workspace where there is one, every SIMD's register file) applied right before every library call
that launches.  Every input lies inside a larger buffer filled with the run's pattern, every output between NaN
guards.  (a) The four results are the same bits; (b) the guards are untouched; (c) the unpoisoned result meets the
operation's own reference: the host twins and numpy restatements bit for bit where include/pbg.h promises bits, the
float64 autograd bound of tests/ppo_grad_data.py for the gradient.  No tolerance is new.

The second half is about an object's history: one that served another call first gives the bits of a fresh one."""
import ctypes
import types

import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native, rng
from pybulletgym_amd.policy import ActionNoise, MLPPolicy, MLPPopulation, ObsStats, pack_theta
from pybulletgym_amd.ppo import AdamClip, PPOGrad, adv_norm, gae
from pybulletgym_amd.vec_env import VecEnv

import gae_data
import poison
import policies
import policy_data
import ppo_grad_data as gd
import ppo_opt_data as od
from poison import RUNS, Guarded, surrounded
from rollout_checks import check_sampled, loop_fed
from test_obsnorm_gpu import Restated, _check_outputs, _restate_rollout
from test_obsnorm_host import make_norm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x1234_5678_9ABC_DEF0
F32, F64 = torch.float32, torch.float64
ACTOR_DIMS = ((7, 33, 17, 3), (28, 128, 64, 8), (256, 256, 256, 64))   # `layer`'s 4-, 8- and 16-row splits


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


# ---------------------------------------------------------------------------- the witness
@pytest.mark.parametrize("words", [8192, 18432])
def test_the_lds_poison_lands(words):
    """What the poison is worth: after it, 8 workgroups per CU that take the actor's 32 KiB (8,192 words) or the
    gradient kernel's 72 KiB (18,432 words) of LDS find the pattern in every word of it."""
    _need_gpu()
    n_wg = 8 * torch.cuda.get_device_properties(DEV).multi_processor_count
    for pat, reg in poison.PATTERNS:
        poison.poison(None, pat, reg, DEV)
        got = poison.lds_peek(words, n_wg, DEV)
        assert got.shape == (n_wg, words)
        bad = got != np.uint32(pat)
        assert not bad.any(), (hex(pat), int(bad.sum()), np.argwhere(bad)[0], hex(int(got[bad][0])))


# ---------------------------------------------------------------------------- actors, plain calls
def _actor_obs(K, n):
    """Seeded rows (3 sigma, so that a normaliser's clip acts); row 7 holds a NaN and row 40 is all inf where n
    reaches them, as in tests/test_policy_gpu.py."""
    obs = (3.0 * policy_data.seeded_obs(K, n, seed=n)).astype(np.float32)
    if n > 7:
        obs[7, 1 % K] = np.nan
    if n > 40:
        obs[40, :] = np.inf
    return obs


def _act_four_times(actor, obs, what):
    A = actor.act_dim
    runs = []
    for run in RUNS:
        x, out = surrounded(obs, run, DEV), Guarded((obs.shape[0], A), F32, DEV)
        poison.poison_run(run, None, DEV)
        actor.act(x, out=out.view)
        runs.append(dict(act=out.numpy(what)))
    poison.assert_runs_agree(runs, what)
    return runs[0]["act"]


@pytest.mark.parametrize("normed", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("dims", ACTOR_DIMS, ids=str)
def test_actor_calls_are_invariant(dims, normed):
    """MLPPolicy.act at n = 1 and 17, MLPPopulation.act of 2 pairs at G = 1, 5 and 17; the truth is
    pbg_policy_act_host, per member."""
    _need_gpu()
    K = dims[0]
    norm = make_norm(K) + (5.0,) if normed else None
    ws = policy_data.synthetic_weights(dims)
    host, dev = MLPPolicy(*ws, obs_norm=norm), MLPPolicy(*ws, device=DEV, obs_norm=norm)
    for n in (1, 17):
        obs = _actor_obs(K, n)
        got = _act_four_times(dev, obs, f"policy {dims} n {n}")
        assert np.array_equal(got, host.act(obs), equal_nan=True), (dims, n)
    host.close()
    dev.close()
    pop = MLPPopulation(dims, 2, DEV)
    pop.perturb(torch.from_numpy(pack_theta(ws)).to(DEV), 0.5, 77, 0)
    if normed:
        pop.set_obs_norm(torch.from_numpy(norm[0]).to(DEV), torch.from_numpy(norm[1]).to(DEV), clip=norm[2])
    P = pop.n_members
    hosts = [MLPPolicy(*pop.member_weights(m), obs_norm=norm) for m in range(P)]
    for G in (1, 5, 17):
        obs = _actor_obs(K, P * G)
        got = _act_four_times(pop, obs, f"population {dims} G {G}")
        want = np.concatenate([hosts[m].act(obs[m * G:(m + 1) * G]) for m in range(P)])
        assert np.array_equal(got, want, equal_nan=True), (dims, G)
    for h in hosts:
        h.close()
    pop.close()


# ---------------------------------------------------------------------------- rollout steps
ENV_ID, N_ENVS, STEPS, COUNTER0 = "HopperPyBulletEnv-v0", 20, 4, 5
ACC = ("obs", "cur_return", "cur_length", "done_return", "done_length", "done_episodes")
TRAJ = ("obs_traj", "act_traj", "rew_traj", "done_traj")


def _hopper_env():
    env = VecEnv(ENV_ID, N_ENVS, device=DEV, seed=0, autoreset=True, precision=64)
    q0 = policies.reset_draws(N_ENVS, env.info.reset_dofs, 0).astype(np.float32)
    env.reset(init_q=torch.from_numpy(q0))
    return env


def _hopper_actor(kind, mode):
    ws = policy_data.fixture_weights(policies.POLICY_FILES[ENV_ID])
    K = ws[0].shape[0]
    r = np.random.default_rng(K)   # near the identity, so that the pretrained policy still acts sensibly
    mean, inv_std = (0.02 * r.standard_normal(K)).astype(np.float32), r.uniform(0.9, 1.1, K).astype(np.float32)
    if kind == "policy":
        actor = MLPPolicy(*ws, device=DEV)
        if mode != "plain":
            actor.set_obs_norm(mean, inv_std, 5.0)
        return actor
    actor = MLPPopulation((K, ws[0].shape[1], ws[2].shape[1], ws[4].shape[1]), 2, DEV)   # 4 members of 5 envs
    actor.perturb(torch.from_numpy(pack_theta(ws)).to(DEV), 0.05, 99, 0)
    if mode != "plain":
        actor.set_obs_norm(torch.from_numpy(mean).to(DEV), torch.from_numpy(inv_std).to(DEV), clip=5.0)
    return actor


@pytest.mark.parametrize("noisy", [False, True], ids=["mean", "sampled"])
@pytest.mark.parametrize("mode", ["plain", "norm", "collect"])
@pytest.mark.parametrize("kind", ["policy", "population"])
def test_rollout_steps_are_invariant(kind, mode, noisy):
    """The six actor_kernel<MODE, SAMPLE> instantiations and book_kernel: Hopper (15 observations, 3 actions: the
    last block of four normals is ragged), 20 envs: a shared-weight policy (its second tile has 4 rows) and a
    population of 4 members x 5 envs.  Four one-step rollouts, each behind a poison, against one unpoisoned
    four-step rollout from the same reset: test_rollout_split_continues_the_accumulators states that the split is
    exact."""
    _need_gpu()
    actor = _hopper_actor(kind, mode)
    K, A = actor.obs_dim, actor.act_dim
    assert (K, A) == (15, 3)
    group = N_ENVS // actor.n_members if kind == "population" else None
    noise, std = None, None
    if noisy:
        noise = ActionNoise(A, SEED, DEV)
        std = torch.from_numpy((0.05 + 0.01 * np.arange(A)).astype(np.float32)).to(DEV)
        noise.set_std(std)
        actor.attach_action_noise(noise)

    def start():
        env = _hopper_env()
        stats = None
        if mode == "collect":
            stats = ObsStats(K, N_ENVS, group=group, device=DEV)
            actor.attach_obs_stats(stats)
        if noisy:
            noise.counter = COUNTER0
        return env, stats

    def finish(env, stats, out):
        if noisy:
            out["counter"] = np.array([noise.counter])
        if stats is not None:
            out["mean"], out["inv_std"] = (t.cpu().numpy().copy() for t in (stats.mean, stats.inv_std))
            out["totals"] = stats.totals.cpu().numpy()
            actor.attach_obs_stats(None)
            stats.close()
        env.close()
        return out

    # the reference: one unpoisoned call of four steps
    env, stats = start()
    res = env.rollout(actor, STEPS, trajectory=True)
    whole = {f: getattr(res, f).clone() for f in ACC + TRAJ + (("eps2_traj",) if noisy else ())}
    if stats is not None:
        stats.finalize()
    want = finish(env, stats, {f: t.cpu().numpy() for f, t in whole.items()})

    runs = []
    for run in RUNS:
        env, stats = start()
        steps = []
        for _ in range(STEPS):
            poison.poison_run(run, env._h, DEV)
            res = env.rollout(actor, 1, trajectory=True)
            steps.append({f: getattr(res, f).clone() for f in TRAJ + (("eps2_traj",) if noisy else ())})
        out = {f: torch.cat([s[f] for s in steps]).cpu().numpy() for f in steps[0]}
        out.update({f: getattr(res, f).cpu().numpy() for f in ACC})
        if stats is not None:
            poison.poison_run(run, env._h, DEV)
            stats.finalize()
        runs.append(finish(env, stats, out))
    what = f"rollout {kind} {mode} {'sampled' if noisy else 'mean'}"
    poison.assert_runs_agree(runs, what)
    assert set(runs[0]) == set(want)
    for f in want:
        poison.assert_same_bits(runs[0][f], want[f], f"{what} {f}: four calls against one")

    # the reference against the stated semantics
    if noisy:
        assert int(want["counter"][0]) == COUNTER0 + STEPS
        actor.attach_action_noise(None)   # check_sampled's actor is the noise-free one
        check_sampled(whole, actor, noise, std, COUNTER0)
    else:
        for t in range(STEPS):
            mu = actor.act(whole["obs_traj"][t].contiguous())
            poison.assert_same_bits(whole["act_traj"][t], mu, f"{what} act_traj[{t}]")
    ref = _hopper_env()
    fed = loop_fed(ref, whole["act_traj"])
    for f in ACC + TRAJ:
        g, w = poison.bits(whole[f]), poison.bits(fed[f])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, f)
    ref.close()
    if mode == "collect":
        restated = Restated(K, (N_ENVS // (group or N_ENVS)) * (((group or N_ENVS) + 15) // 16))
        booked = _restate_rollout(restated, whole, True, group or 0)
        want_mean, want_inv = restated.finalize()
        assert booked == N_ENVS * STEPS
        poison.assert_same_bits(want["totals"], restated.totals(), f"{what} totals against the restatement")
        _check_outputs(torch.from_numpy(want["mean"]), torch.from_numpy(want["inv_std"]), want_mean, want_inv)
    if noise is not None:
        noise.close()
    actor.close()


# ---------------------------------------------------------------------------- observation statistics
@pytest.mark.parametrize("n,group", [(17, 0), (20, 5)])
@pytest.mark.parametrize("K", [1, 28, 256])
def test_obs_stats_update_and_finalize_are_invariant(K, n, group):
    """Two updates (the second under an `active` mask; each batch with one NaN row) and a finalize, against the numpy
    restatement of tests/test_obsnorm_gpu.py."""
    _need_gpu()
    r = np.random.default_rng([K, n, group])
    batches = []
    for call in range(2):
        obs = (r.choice([-1.0, 1.0], (n, K)) * 10.0 ** r.uniform(-3.0, 3.0, (n, K))).astype(np.float32)
        obs[3 + call, call % K] = np.nan
        batches.append((obs, None if call == 0 else (r.random(n) < 0.7).astype(np.uint8)))
    runs = []
    for run in RUNS:
        stats = ObsStats(K, n, group=group or None, device=DEV)
        for obs, active in batches:
            x = surrounded(obs, run, DEV)
            a = None if active is None else surrounded(active, run, DEV)
            poison.poison_run(run, None, DEV)
            stats.update(x, a)
        poison.poison_run(run, None, DEV)
        mean, inv_std = stats.finalize()
        runs.append(dict(mean=mean.cpu().numpy().copy(), inv_std=inv_std.cpu().numpy().copy(), totals=stats.totals.cpu().numpy()))
        n_slots = stats.n_slots
        stats.close()
    what = f"obs stats K {K} n {n} group {group}"
    poison.assert_runs_agree(runs, what)
    ref = Restated(K, n_slots)
    for obs, active in batches:
        ref.update(obs, np.ones(n, bool) if active is None else active, group)
    want_mean, want_inv = ref.finalize()
    poison.assert_same_bits(runs[0]["totals"], ref.totals(), what)
    _check_outputs(torch.from_numpy(runs[0]["mean"]), torch.from_numpy(runs[0]["inv_std"]), want_mean, want_inv)
    assert ref.count > 10.0


# ---------------------------------------------------------------------------- population kernels, noise fill, GAE
def test_population_kernels_are_invariant():
    """noise, perturb (read back through get_member: copy_rows_kernel), grad and fitness of 3 pairs of
    (7, 33, 17, 3); fitness over G = 5 envs per member.  References as in tests/test_population_gpu.py."""
    _need_gpu()
    dims, n_pairs, G, gen = (7, 33, 17, 3), 3, 5, 2
    theta = pack_theta(policy_data.synthetic_weights(dims))
    sigma = np.float32(0.1)
    r = np.random.default_rng(5)
    w = r.standard_normal(n_pairs).astype(np.float32)
    P = 2 * n_pairs
    cur = r.standard_normal(P * G) * 10.0 ** r.integers(-3, 4, P * G)
    done = r.standard_normal(P * G) * 10.0 ** r.integers(-3, 4, P * G)
    runs = []
    for run in RUNS:
        pop = MLPPopulation(dims, n_pairs, DEV, pair0=2)
        D = pop.n_params
        o_noise, o_grad, o_fit = Guarded((n_pairs, D), F32, DEV), Guarded(D, F32, DEV), Guarded(P, F64, DEV)
        o_members = [Guarded(D, F32, DEV) for _ in range(P)]
        poison.poison_run(run, None, DEV)
        pop.noise(SEED, gen, out=o_noise.view)
        th = surrounded(theta, run, DEV)
        poison.poison_run(run, None, DEV)
        pop.perturb(th, float(sigma), SEED, gen)
        for m in range(P):
            poison.poison_run(run, None, DEV)
            pop.get_member(m, out=o_members[m].view)
        wd = surrounded(w, run, DEV)
        poison.poison_run(run, None, DEV)
        pop.grad(wd, SEED, gen, out=o_grad.view)
        acc = types.SimpleNamespace(cur_return=surrounded(cur, run, DEV), done_return=surrounded(done, run, DEV))
        poison.poison_run(run, None, DEV)
        pop.fitness(acc, out=o_fit.view)
        runs.append(dict(noise=o_noise.numpy("noise"), grad=o_grad.numpy("grad"), fitness=o_fit.numpy("fitness"),
                         members=np.stack([o.numpy("member") for o in o_members])))
        pop.close()
    poison.assert_runs_agree(runs, "population")
    got = runs[0]
    host = rng.es_noise(dims, SEED, gen, 2, n_pairs)
    assert np.isfinite(got["noise"]).all() and np.abs(got["noise"].astype(np.float64) - host).max() <= 1e-5   # pbg.h's bound
    eps, th64 = got["noise"].astype(np.float64), theta.astype(np.float64)
    acc = np.zeros(theta.shape[0], np.float64)
    for i in range(n_pairs):
        assert np.array_equal(got["members"][2 * i], (th64 + np.float64(sigma) * eps[i]).astype(np.float32)), i
        assert np.array_equal(got["members"][2 * i + 1], (th64 - np.float64(sigma) * eps[i]).astype(np.float32)), i
        acc += np.float64(w[i]) * eps[i]
    assert np.array_equal(got["grad"], acc.astype(np.float32))
    want = np.zeros(P)
    for m in range(P):
        s = np.float64(0.0)
        for e in range(m * G, (m + 1) * G):
            s = s + (done[e] + cur[e])
        want[m] = s / np.float64(G)
    poison.assert_same_bits(got["fitness"], want, "fitness")


@pytest.mark.parametrize("act_dim", [3, 17])
def test_action_noise_fill_is_invariant(act_dim):
    _need_gpu()
    n, env_offset, step = 17, 16, 7
    runs = []
    for run in RUNS:
        z, out = ActionNoise(act_dim, SEED, DEV), Guarded((n, act_dim), F32, DEV)
        poison.poison_run(run, None, DEV)
        z.fill(n, env_offset, step, out=out.view)
        runs.append(dict(eps=out.numpy("fill")))
        z.close()
    poison.assert_runs_agree(runs, f"fill act_dim {act_dim}")
    want = rng.action_noise(act_dim, SEED, n, env_offset, step)
    assert np.isfinite(runs[0]["eps"]).all() and np.abs(runs[0]["eps"].astype(np.float64) - want).max() <= 1e-5   # pbg.h's bound


def test_gae_is_invariant():
    _need_gpu()
    T, n, gamma, lam = 37, 65, 0.99, 0.95
    rew, done, value = gae_data.case(T, n)
    runs = []
    for run in RUNS:
        ins = [surrounded(a, run, DEV) for a in (rew, done, value)]
        adv, ret = Guarded((T, n), F32, DEV), Guarded((T, n), F32, DEV)
        poison.poison_run(run, None, DEV)
        gae(*ins, gamma, lam, adv=adv.view, ret=ret.view)
        runs.append(dict(adv=adv.numpy("adv"), ret=ret.numpy("ret")))
    poison.assert_runs_agree(runs, "gae")
    want_adv, want_ret = gae_data.gae_numpy(rew, done, value, gamma, lam)
    poison.assert_same_bits(runs[0]["adv"], want_adv, "gae adv")
    poison.assert_same_bits(runs[0]["ret"], want_ret, "gae ret")


# ---------------------------------------------------------------------------- the optimiser's half
@pytest.mark.parametrize("Bm", [17, 1025])
def test_adv_norm_is_invariant(Bm):
    _need_gpu()
    r = np.random.default_rng(Bm)
    B = 2 * Bm + 5
    a = (0.3 + 2.0 * r.standard_normal(B)).astype(np.float32)
    idx = r.permutation(B)[:Bm].astype(np.int64)
    runs = []
    for run in RUNS:
        ad, ix, out = surrounded(a, run, DEV), surrounded(idx, run, DEV), Guarded(2, F32, DEV)
        poison.poison_run(run, None, DEV)
        adv_norm(ad, ix, out=out.view)
        runs.append(dict(pair=out.numpy("adv_norm")))
    poison.assert_runs_agree(runs, f"adv_norm Bm {Bm}")
    poison.assert_same_bits(runs[0]["pair"], od.adv_norm_ref(a, idx), "adv_norm against the restatement")
    poison.assert_same_bits(runs[0]["pair"], adv_norm(a, idx), "adv_norm against the host twin")


@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("sizes", od.SIZES[2:4], ids=str)
def test_adam_clip_steps_are_invariant(sizes, shift):
    """Three steps with max_grad_norm 0.5 (the clip is active on the second), the blocks 16-byte aligned and one
    element off; parameters, moments, step count and info against ppo_opt_data.opt_step_ref."""
    _need_gpu()
    runs = []
    for run in RUNS:
        opt = AdamClip(sizes, DEV)
        params = [Guarded(s, F32, DEV, shift=shift, init=p) for s, p in zip(sizes, od.params0(sizes))]
        out = {}
        for s in range(3):
            grads = [surrounded(g, run, DEV, shift=shift) for g in od.grads_of(sizes, s)]
            info = Guarded(2, F64, DEV)
            poison.poison_run(run, None, DEV)
            opt.step([p.view for p in params], grads, od.LR, od.BETAS, od.EPS, 0.5, info=info.view)
            out[f"info{s}"] = info.numpy("info")
            out[f"params{s}"] = np.concatenate([p.numpy("params") for p in params])
            m, v, t = opt.state()
            out[f"m{s}"], out[f"v{s}"] = (torch.cat(x).cpu().numpy() for x in (m, v))
            out[f"t{s}"] = t.cpu().numpy()
        runs.append(out)
        opt.close()
    what = f"AdamClip {sizes} shift {shift}"
    poison.assert_runs_agree(runs, what)
    state, hp = od.new_state(sizes), od.params0(sizes)
    for s in range(3):
        norm, coef = od.opt_step_ref(state, hp, od.grads_of(sizes, s), max_grad_norm=0.5)
        poison.assert_same_bits(runs[0][f"info{s}"], np.array([norm, coef]), f"{what} info, step {s}")
        poison.assert_same_bits(runs[0][f"params{s}"], np.concatenate(hp), f"{what} params, step {s}")
        poison.assert_same_bits(runs[0][f"m{s}"], np.concatenate(state["m"]), f"{what} m, step {s}")
        poison.assert_same_bits(runs[0][f"v{s}"], np.concatenate(state["v"]), f"{what} v, step {s}")
        assert int(runs[0][f"t{s}"][0]) == s + 1 == state["t"]
    assert runs[0]["info1"][1] < 1.0   # the clip was active


# ---------------------------------------------------------------------------- the gradient
GRAD_KEYS = ("theta_actor", "theta_critic", "log_std", "obs", "act", "logp_old", "adv", "ret", "idx", "adv_norm", "mean", "inv_std")
GRAD_CASES = (gd.CASES[2], gd.CASES[4], gd.CASES[5]) + gd.CASES[6:]
GRAD_OPTIONS = ((True, True, 0.01), (False, False, 0.0))


class GradOutputs:
    """pbg_ppo_grad_run's six outputs between guards."""

    def __init__(self, g, Bm):
        sizes = dict(grad_actor=g.Da, grad_critic=g.Dc, grad_log_std=g.dims[3], logp_out=Bm, v_out=Bm)
        self.g = {k: Guarded(n, F32, DEV) for k, n in sizes.items()}
        self.g["stats"] = Guarded(4, F64, DEV)
        self.kw = {k: o.view for k, o in self.g.items()}

    def numpy(self, what):
        return {k: o.numpy(f"{what} {k}") for k, o in self.g.items()}


def _grad_run(g, c, t, adv_norm_on, ent_coef, out, idx=None):
    norm = (t["mean"], t["inv_std"], c["clip"]) if c["mean"] is not None else None
    g.run(t["theta_actor"], t["theta_critic"], t["log_std"], t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"],
          idx=t["idx"] if idx is None else idx, adv_norm=t["adv_norm"] if adv_norm_on else None, obs_norm=norm,
          clip_eps=gd.CLIP_EPS, vf_coef=gd.VF_COEF, ent_coef=ent_coef, **out.kw)


@pytest.mark.parametrize("norm,adv_norm_on,ent_coef", GRAD_OPTIONS)
@pytest.mark.parametrize("dims,B,Bm,seed", GRAD_CASES)
def test_ppo_gradient_is_invariant(dims, B, Bm, seed, norm, adv_norm_on, ent_coef):
    """ppograd_tiles_kernel<true> ((5, 16, 8, 1): the register path, into the AGPR half) and <false>, and
    ppograd_reduce_kernel, a fresh object per run; the unpoisoned run under tests/ppo_grad_data.py's bound."""
    _need_gpu()
    if (dims, Bm) == ((256, 256, 256, 64), 1921):
        # more tiles than the workgroups the workspace cap allows: workgroups 0 and 1 own two tiles each
        assert gd.WIDEST_TILES == 121 and gd.WIDEST_WGS == 119
    c = gd.case(dims, B, Bm, seed, norm)
    what = f"gradient {dims} Bm {Bm} norm {norm} adv_norm {adv_norm_on} ent {ent_coef}"
    runs = []
    for run in RUNS:
        t = {k: None if c[k] is None else surrounded(c[k], run, DEV) for k in GRAD_KEYS}
        g = PPOGrad(dims, Bm, DEV)
        out = GradOutputs(g, Bm)
        poison.poison_run(run, None, DEV)
        _grad_run(g, c, t, adv_norm_on, ent_coef, out)
        runs.append(out.numpy(what))
        g.close()
    poison.assert_runs_agree(runs, what)
    (g64, s64, logp64, _), (g32, _, _, _) = gd.references(dims, B, Bm, seed, norm, adv_norm_on, ent_coef)
    o = runs[0]
    gd.check_grads(gd.blocks(dims, o["grad_actor"], o["grad_critic"], o["grad_log_std"]), g64, g32, what)
    gd.check_stats(o["stats"], o["logp_out"], s64, logp64, what)


# ---------------------------------------------------------------------------- an object's history
@pytest.mark.parametrize("dims", [(5, 16, 8, 1), (5, 129, 16, 1)], ids=str)
def test_a_used_gradient_object_gives_a_fresh_ones_bits(dims):
    """8,209 rows leave 512 workgroups' partials in the workspace; a minibatch of 33 rows then runs 3 workgroups
    and must not see the other 509, nor what its own three held."""
    _need_gpu()
    c = gd.case(dims, 8300, 8209, 0, False)
    t = {k: None if c[k] is None else torch.from_numpy(np.array(c[k])).to(DEV) for k in GRAD_KEYS}
    small = t["idx"][:33].contiguous()
    used, fresh = PPOGrad(dims, 8209, DEV), PPOGrad(dims, 8209, DEV)
    big = GradOutputs(used, 8209)
    _grad_run(used, c, t, True, 0.01, big)
    assert np.abs(big.numpy("8,209 rows")["grad_actor"]).max() > 0.0
    a, b = GradOutputs(used, 33), GradOutputs(fresh, 33)
    _grad_run(used, c, t, True, 0.01, a, idx=small)
    _grad_run(fresh, c, t, True, 0.01, b, idx=small)
    a, b = a.numpy("used"), b.numpy("fresh")
    for k in a:
        poison.assert_same_bits(a[k], b[k], f"{dims} {k}: a used object against a fresh one")
    assert np.isfinite(b["grad_actor"]).all() and np.abs(b["grad_actor"]).max() > 0.0
    used.close()
    fresh.close()


def test_used_obs_stats_give_a_fresh_objects_bits():
    """20 rows in groups of 5 fill four slots; after finalize and the initial totals put back, 17 rows as one
    group (two tiles) must count as in a fresh object."""
    _need_gpu()
    K = 28
    r = np.random.default_rng(K)
    first = torch.from_numpy(r.standard_normal((20, K)).astype(np.float32)).to(DEV)
    second = torch.from_numpy(r.standard_normal((17, K)).astype(np.float32)).to(DEV)

    def update17(stats):   # the object's wrapper passes its own group: 17 rows as one group through the library
        _native.check(_native.lib().pbg_obs_stats_update(stats._h, 17, 0, second.data_ptr(), None, _stream()), "pbg_obs_stats_update")
        mean, inv_std = stats.finalize()
        return dict(mean=mean.cpu().numpy().copy(), inv_std=inv_std.cpu().numpy().copy(), totals=stats.totals.cpu().numpy())

    used, fresh = ObsStats(K, 20, group=5, device=DEV), ObsStats(K, 20, group=5, device=DEV)
    initial = used.totals.clone()
    used.update(first)
    used.finalize()
    assert float(used.totals[0]) == 20.0 + 1e-2
    used.totals = initial
    a, b = update17(used), update17(fresh)
    for k in a:
        poison.assert_same_bits(a[k], b[k], f"obs stats {k}: a used object against a fresh one")
    assert float(b["totals"][0]) == 17.0 + 1e-2
    used.close()
    fresh.close()


def test_a_reset_adam_clip_gives_a_fresh_objects_bits():
    _need_gpu()
    sizes = od.SIZES[3]

    def first_step(opt):
        p = [torch.from_numpy(a).to(DEV) for a in od.params0(sizes)]
        info = torch.zeros(2, dtype=F64, device=DEV)
        opt.step(p, [torch.from_numpy(a).to(DEV) for a in od.grads_of(sizes, 1)], od.LR, od.BETAS, od.EPS, 0.5, info=info)
        m, v, t = opt.state()
        return dict(params=torch.cat(p).cpu().numpy(), m=torch.cat(m).cpu().numpy(), v=torch.cat(v).cpu().numpy(),
                    t=t.cpu().numpy(), info=info.cpu().numpy())

    used, fresh = AdamClip(sizes, DEV), AdamClip(sizes, DEV)
    p = [torch.from_numpy(a).to(DEV) for a in od.params0(sizes)]
    for s in range(3):
        used.step(p, [torch.from_numpy(a).to(DEV) for a in od.grads_of(sizes, s)], od.LR, od.BETAS, od.EPS, 0.5)
    used.reset()
    a, b = first_step(used), first_step(fresh)
    for k in a:
        poison.assert_same_bits(a[k], b[k], f"AdamClip {k}: a reset object against a fresh one")
    assert int(b["t"][0]) == 1
    used.close()
    fresh.close()


def test_a_used_population_gives_a_fresh_ones_bits():
    """act at G = 17 (two tiles per member), then at G = 5, against a fresh population holding the same members."""
    _need_gpu()
    dims = (7, 33, 17, 3)
    used, fresh = MLPPopulation(dims, 2, DEV), MLPPopulation(dims, 2, DEV)
    used.perturb(torch.from_numpy(pack_theta(policy_data.synthetic_weights(dims))).to(DEV), 0.5, 77, 0)
    for m in range(used.n_members):
        fresh.set_member(m, used.get_member(m))
    P = used.n_members
    used.act(torch.from_numpy(_actor_obs(dims[0], P * 17)).to(DEV))
    obs = torch.from_numpy(_actor_obs(dims[0], P * 5)).to(DEV)
    poison.assert_same_bits(used.act(obs), fresh.act(obs), "population act: a used object against a fresh one")
    used.close()
    fresh.close()
