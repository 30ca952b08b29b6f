"""The gradient as parts on the device (include/pbg.h "The PPO gradient as parts, and the statistics' slots";
ppo.PPOGrad.geometry / run_part / reduce, policy.ObsStats.get_slots / set_slots, ppo.ShardedPPO with no process
group): for every cut of a gradient's workgroups into consecutive ranges the parts, written into one buffer and
reduced, are pbg_ppo_grad_run's bits, on both paths, on a side stream, in a replayed graph and whatever uninitialised
memory holds; slots moved between objects finalize to the whole batch's bits; the world-1 sharded trainer holds PPO's
bits."""
import functools

import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd.distributed import ShardedVecEnv
from pybulletgym_amd.policy import ObsStats
from pybulletgym_amd.ppo import PPO, PPOGrad, ShardedPPO
from pybulletgym_amd.vec_env import VecEnv

import poison
import ppo_grad_data as gd
from poison import RUNS, Guarded, assert_same_bits, surrounded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SHIPPED1 = ((44, 256, 128, 17), 64, 40, 0)   # tests/test_ppograd_mfma_gpu.py's SHIPPED[1]
SENTINEL = -12345.0
KEYS = ("theta_actor", "theta_critic", "log_std", "obs", "act", "logp_old", "adv", "ret", "idx", "adv_norm", "mean", "inv_std")
OUT = ("grad_actor", "grad_critic", "grad_log_std", "stats", "logp_out", "v_out")

# (case, path, G, cuts): the cuts are workgroup counts of consecutive ranges, empty ones included
PART_CASES = ((gd.CASES[1], "fma", 2, ((1, 1), (2, 0), (0, 1, 1))),
              (gd.CASES[3], "fma", 17, ((17,), (9, 8), (6, 6, 5), (1, 16))),
              (gd.CASES[8], "fma", 512, ((256, 256), (1, 511))),      # workgroups 0 and 1 own two tiles
              (SHIPPED1, "mfma", 3, ((2, 1), (1, 1, 1))),
              (gd.CASES[9], "mfma", gd.WIDEST_WGS, ((60, 59),)))      # the memory-resident chain, two-tile workgroups
IDS = [f"{path}-{c[0]}-{c[2]}" for c, path, _, _ in PART_CASES]


def _args(c, t, adv_norm, ent_coef):
    norm = (t["mean"], t["inv_std"], c["clip"]) if c["mean"] is not None else None
    pos = (t["theta_actor"], t["theta_critic"], t["log_std"], t["obs"], t["act"], t["logp_old"], t["adv"], t["ret"])
    kw = dict(idx=t["idx"], adv_norm=t["adv_norm"] if adv_norm else None, obs_norm=norm, clip_eps=gd.CLIP_EPS, vf_coef=gd.VF_COEF,
              ent_coef=ent_coef)
    return pos, kw


class Out:
    """The six outputs between guards; logp_out and v_out start as the sentinel."""

    def __init__(self, g, Bm):
        sizes = dict(grad_actor=g.Da, grad_critic=g.Dc, grad_log_std=g.dims[3])
        self.g = {k: Guarded(n, F32, DEV) for k, n in sizes.items()}
        self.g["stats"] = Guarded(4, F64, DEV)
        for k in ("logp_out", "v_out"):
            self.g[k] = Guarded(Bm, F32, DEV, init=np.full(Bm, SENTINEL, np.float32))
        self.kw = {k: o.view for k, o in self.g.items()}

    def numpy(self, what=""):
        return {k: o.numpy(f"{what} {k}") for k, o in self.g.items()}


class Rows:
    """A [G, width] buffer of NaN with one whole guard row of NaN before it and one behind."""
    mark = float("nan")

    def __init__(self, G, width, dtype):
        self.full = torch.full((G + 2, width), self.mark, dtype=dtype, device=DEV)
        self.view = self.full[1:G + 1]

    def numpy(self, what=""):
        assert bool(torch.isnan(self.full[0]).all()) and bool(torch.isnan(self.full[-1]).all()), f"{what}: a guard row was written"
        return self.view.cpu().numpy()


class Parts:
    """One [G, Dtot] / [G, 4] pair, guard-rowed."""

    def __init__(self, G, dtot):
        self.part, self.stats = Rows(G, dtot, F32), Rows(G, 4, F64)

    def check(self, what):
        p, s = self.part.numpy(f"{what} part"), self.stats.numpy(f"{what} part_stats")
        assert not np.isnan(p).any() and not np.isnan(s).any(), f"{what}: a partial's element was not written"


def rows_of(wg_first, wg_count, G, Bm):
    """The minibatch rows of the tiles the workgroups wg_first .. wg_first + wg_count - 1 own."""
    own = np.zeros(Bm, bool)
    for b in range(wg_first, wg_first + wg_count):
        for t in range(b, -(-Bm // 16), G):
            own[16 * t:16 * t + 16] = True
    return own


def run_cut(g, pos, kw, cut, G, dtot, Bm, what, fwd_want=None):
    """The parts of ``cut`` into one buffer, each with fresh sentinel-filled logp_out / v_out, then the reduction: the six
    outputs (the forward ones assembled from the parts' own rows) as numpy."""
    assert sum(cut) == G
    buf, out = Parts(G, dtot), Out(g, Bm)
    logp, v = np.full(Bm, SENTINEL, np.float32), np.full(Bm, SENTINEL, np.float32)
    at = 0
    for cnt in cut:
        part_out = Out(g, Bm)
        g.run_part(*pos, at, cnt, buf.part.view[at:at + cnt], buf.stats.view[at:at + cnt], logp_out=part_out.kw["logp_out"],
                   v_out=part_out.kw["v_out"], **kw)
        own = rows_of(at, cnt, G, Bm)
        for name, dst in (("logp_out", logp), ("v_out", v)):
            got = part_out.g[name].numpy(f"{what} part at {at} {name}")
            assert (got[~own] == np.float32(SENTINEL)).all(), f"{what}: the part at {at} wrote {name} outside its tiles"
            assert (got[own] != np.float32(SENTINEL)).all(), f"{what}: the part at {at} left {name} rows of its tiles"
            dst[own] = got[own]
        at += cnt
    buf.check(what)
    kwr = {k: t for k, t in out.kw.items() if k not in ("logp_out", "v_out")}
    g.reduce(*pos, G, buf.part.view, buf.stats.view, **kwr, **kw)
    buf.check(what)   # the reduction writes no partial
    o = out.numpy(what)
    o["logp_out"], o["v_out"] = logp, v
    return o


def same(got, want, what):
    for k in OUT:
        assert_same_bits(got[k], want[k], f"{what} {k}")


@functools.lru_cache(maxsize=None)
def tensors(dims, B, Bm, seed, norm):
    c = gd.case(dims, B, Bm, seed, norm)
    return c, {k: None if c[k] is None else torch.from_numpy(np.array(c[k])).to(DEV) for k in KEYS}


@pytest.mark.parametrize("case,path,G,cuts", PART_CASES, ids=IDS)
def test_every_cut_reduces_to_the_whole_gradients_bits(case, path, G, cuts):
    dims, B, Bm, seed = case
    g = PPOGrad(dims, Bm, DEV, path=path)
    assert g.geometry(Bm) == (G, g.Da + g.Dc + dims[3])
    dtot = g.geometry(Bm)[1]
    for norm, adv_norm, ent_coef in gd.OPTIONS:
        c, t = tensors(dims, B, Bm, seed, norm)
        pos, kw = _args(c, t, adv_norm, ent_coef)
        what = f"{path} {dims} Bm {Bm} norm {norm} adv_norm {adv_norm} ent {ent_coef}"
        whole = Out(g, Bm)
        g.run(*pos, **whole.kw, **kw)
        want = whole.numpy(what)
        assert np.abs(want["grad_actor"]).max() > 0.0 and (want["logp_out"] != np.float32(SENTINEL)).all()
        for cut in cuts:
            same(run_cut(g, pos, kw, cut, G, dtot, Bm, f"{what} cut {cut}"), want, f"{what} cut {cut}")
    g.close()


@pytest.mark.parametrize("case,path,G,cuts", PART_CASES, ids=IDS)
def test_the_same_bits_on_a_side_stream_and_in_a_replayed_graph(case, path, G, cuts):
    dims, B, Bm, seed = case
    c, t = tensors(dims, B, Bm, seed, True)
    pos, kw = _args(c, t, True, 0.01)
    g = PPOGrad(dims, Bm, DEV, path=path)
    dtot, cut, what = g.geometry(Bm)[1], cuts[-1], f"{path} {dims} Bm {Bm}"
    whole = Out(g, Bm)
    g.run(*pos, **whole.kw, **kw)
    want = whole.numpy(what)

    def parts(buf, out):
        at = 0
        for cnt in cut:
            g.run_part(*pos, at, cnt, buf.part.view[at:at + cnt], buf.stats.view[at:at + cnt], logp_out=out.kw["logp_out"],
                       v_out=out.kw["v_out"], **kw)
            at += cnt
        g.reduce(*pos, G, buf.part.view, buf.stats.view, **{k: out.kw[k] for k in OUT[:4]}, **kw)

    side = torch.cuda.Stream(DEV)
    buf, out = Parts(G, dtot), Out(g, Bm)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        parts(buf, out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    same(out.numpy(what), want, f"{what} on a side stream")
    buf.check(what)

    buf, out = Parts(G, dtot), Out(g, Bm)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        parts(buf, out)
    for n in range(2):
        for o in list(out.g.values()) + [buf.part, buf.stats]:
            o.view.fill_(o.mark)
        graph.replay()
        torch.cuda.synchronize()
        same(out.numpy(what), want, f"{what} replay {n}")
        buf.check(what)
    g.close()


@pytest.mark.parametrize("case,path,G,cut", [(gd.CASES[3], "fma", 17, (9, 8)), (gd.CASES[8], "fma", 512, (1, 511)),
                                             (SHIPPED1, "mfma", 3, (2, 1)), (gd.CASES[9], "mfma", gd.WIDEST_WGS, (60, 59))],
                         ids=("fma-257", "fma-8209", "mfma-40", "mfma-1921"))
def test_the_parts_are_invariant_to_uninitialised_memory(case, path, G, cut):
    """tests/test_learner_invariance_gpu.py's protocol for run_part and reduce: a fresh object per run, every input
    inside a buffer of the run's pattern, LDS and register files poisoned before the calls, every output and the
    partials between guards; the four runs agree on every output and on the partials."""
    dims, B, Bm, seed = case
    c = gd.case(dims, B, Bm, seed, True)
    what = f"parts {path} {dims} Bm {Bm}"
    runs = []
    for r in RUNS:
        t = {k: None if c[k] is None else surrounded(c[k], r, DEV) for k in KEYS}
        pos, kw = _args(c, t, True, 0.01)
        g = PPOGrad(dims, Bm, DEV, path=path)
        buf, out = Parts(G, g.geometry(Bm)[1]), Out(g, Bm)
        at = 0
        for cnt in cut:
            poison.poison_run(r, None, DEV)
            g.run_part(*pos, at, cnt, buf.part.view[at:at + cnt], buf.stats.view[at:at + cnt], logp_out=out.kw["logp_out"],
                       v_out=out.kw["v_out"], **kw)
            at += cnt
        poison.poison_run(r, None, DEV)
        g.reduce(*pos, G, buf.part.view, buf.stats.view, **{k: out.kw[k] for k in OUT[:4]}, **kw)
        o = out.numpy(what)
        o["part"], o["part_stats"] = buf.part.numpy(what), buf.stats.numpy(what)
        runs.append(o)
        g.close()
    poison.assert_runs_agree(runs, what)
    g = PPOGrad(dims, Bm, DEV, path=path)
    whole = Out(g, Bm)
    pos, kw = _args(*tensors(dims, B, Bm, seed, True), True, 0.01)
    g.run(*pos, **whole.kw, **kw)
    same(runs[0], whole.numpy(what), what)
    g.close()


def test_bad_ranges_and_a_wrong_G_are_refused_on_the_device_object():
    from pybulletgym_amd import _native
    dims, B, Bm, seed = gd.CASES[3]
    c, t = tensors(dims, B, Bm, seed, False)
    pos, kw = _args(c, t, False, 0.0)
    g = PPOGrad(dims, Bm, DEV)
    G, dtot = g.geometry(Bm)
    part, st = torch.zeros((G, dtot), device=DEV), torch.zeros((G, 4), dtype=F64, device=DEV)
    for first, cnt in ((-1, 1), (0, G + 1), (G, 1), (3, -1)):
        with pytest.raises(_native.PbgError, match="outside 0"):
            g.run_part(*pos, first, cnt, part[:max(cnt, 0)], st[:max(cnt, 0)], **kw)
    with pytest.raises(_native.PbgError, match="part_out"):
        g.run_part(*pos, 0, 2, part[:1], st[:2], **kw)
    with pytest.raises(_native.PbgError, match="is not the 17 workgroups"):
        g.reduce(*pos, G - 1, part[:G - 1], st[:G - 1], **kw)
    with pytest.raises(_native.PbgError):
        g.geometry(Bm + 1)       # beyond max_rows
    g.run_part(*pos, G, 0, part[:0], st[:0], **kw)   # an empty range at the end is valid
    torch.cuda.synchronize()
    assert not part.any() and not st.any()
    g.close()


# ---------------------------------------------------------------------------- the statistics' slots
def _stats_bits(s):
    mean, inv_std = s.finalize()
    return dict(totals=s.totals.cpu().numpy(), mean=mean.cpu().numpy().copy(), inv_std=inv_std.cpu().numpy().copy())


def test_slots_moved_between_objects_finalize_to_the_whole_batchs_bits():
    K = 5
    obs = np.random.default_rng(7).standard_normal((64, K)).astype(np.float32) * 3.0 + 1.0
    obs[5, 2] = np.nan    # an uncounted row: the counts differ between tiles
    runs = []
    for r in RUNS:
        x = surrounded(obs, r, DEV)
        whole, third = ObsStats(K, 64, group=16, device=DEV), ObsStats(K, 64, group=16, device=DEV)
        halves = [ObsStats(K, 64, group=16, device=DEV) for _ in range(2)]
        assert whole.n_slots == 4
        whole.update(x)
        for h, s in enumerate(halves):
            s.update(x[32 * h:32 * h + 32])
            poison.poison_run(r, None, DEV)
            counts, sums = s.get_slots(0, 2)
            assert counts.shape == (2,) and sums.shape == (2, 2 * K)
            poison.poison_run(r, None, DEV)
            third.set_slots(2 * h, counts, sums)
        c_all, s_all = third.get_slots(0, 4)
        c_one, s_one = whole.get_slots(0, 4)
        got, want = _stats_bits(third), _stats_bits(whole)
        assert int(c_all.sum()) == 63 == int(c_one.sum())
        assert_same_bits(c_all, c_one, "slot counts")
        assert_same_bits(s_all, s_one, "slot sums")
        for k in want:
            assert_same_bits(got[k], want[k], f"moved slots: {k}")
        # get zeroes nothing, finalize does
        assert int(halves[0].get_slots(0, 2)[0].sum()) > 0 and not third.get_slots(0, 4)[1].any()
        runs.append(dict(got, counts=c_all.cpu().numpy(), sums=s_all.cpu().numpy()))
        for s in [whole, third] + halves:
            s.close()
    poison.assert_runs_agree(runs, "obs stats slots")


# ---------------------------------------------------------------------------- the trainer with no process group
ENV = "InvertedPendulumPyBulletEnv-v0"
HP = dict(hidden=(16, 8), steps=8, epochs=2, minibatches=2, seed=3, lr=3e-3, lr_schedule="linear", schedule_iterations=5)


def trainer_bits(ppo):
    """What a trainer holds after an iteration, as numpy."""
    m, v, t = ppo.adam.state()
    out = dict(actor=ppo.actor_theta.data, critic=ppo.critic_theta.data, log_std=ppo.log_std.data, adam_t=t, it=ppo._it_dev)
    out.update({f"m{i}": a for i, a in enumerate(m)}, **{f"v{i}": a for i, a in enumerate(v)})
    if ppo.obs_stats is not None:
        out.update(totals=ppo.obs_stats.totals, mean=ppo.actor.obs_norm[0], inv_std=ppo.actor.obs_norm[1])
    out = {k: a.detach().cpu().numpy().copy() for k, a in out.items()}
    out["counters"] = np.array([ppo.noise.counter, ppo.perm.counter, ppo.iteration], np.int64)
    return out


@pytest.mark.parametrize("obs_norm", (False, True), ids=("raw", "obs_norm"))
@pytest.mark.parametrize("grad_path", ("fma", "mfma"))
def test_sharded_ppo_without_a_process_group_holds_ppos_bits(grad_path, obs_norm):
    n = 64
    env = VecEnv(ENV, n, device=DEV, seed=3, autoreset=True, precision=64)
    one = PPO(env, backward="hip", optimizer="hip", permutation="device", obs_norm=obs_norm, grad_path=grad_path, **HP)
    shard = ShardedVecEnv(ENV, n, 0, 1, DEV, seed=3, autoreset=True, precision=64)
    assert (shard.rank, shard.world, shard.offset, shard.count) == (0, 1, 0, n)
    sh = ShardedPPO(shard, obs_norm=obs_norm, grad_path=grad_path, **HP)
    assert (sh.world, sh.rank, sh._G) == (1, 0, 16)   # 8 x 64 rows in 2 minibatches: 256 rows, 16 tiles
    for it in range(2):
        s1, s2 = one.iterate(), sh.iterate()
        a, b = trainer_bits(one), trainer_bits(sh)
        assert set(a) == set(b)
        for k in a:
            assert_same_bits(b[k], a[k], f"iteration {it} {k}")
        for k in s1:
            assert_same_bits(s2[k], s1[k], f"iteration {it} stats {k}")
        assert list(a["counters"]) == [8 * (it + 1), 2 * (it + 1), it + 1]
    st1, st2 = env.get_state(), shard.env.get_state()
    for x, y in zip(st1, st2):
        assert_same_bits(y, x, "env state")
    for o in (sh, one):
        o.close()
    env.close()
    shard.env.close()
