"""Reward scaling by a running std of the discounted return on the device (include/pbg.h "Return statistics",
DESIGN.md section 20): the three launches against the host twin bit for bit, a misaligned input against the aligned
path, a side stream and a replayed graph against eager rounds, the uninitialised-memory invariance of the three
kernels, and slots that compose."""
import numpy as np
import pytest
import torch

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import RetStats

import poison
import retstats_data as rd
from poison import RUNS, Guarded, assert_same_bits, surrounded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _round(obj, rew, done, out=None, **kw):
    obj.update(rew, done)
    obj.finalize()
    return obj.apply(rew, out=out, **kw)


def _host_round(n, gamma, rew, done, rounds=1, **kw):
    """The host twin after ``rounds`` rounds over the same batch: ``(object, the last round's scaled rewards)``."""
    host = RetStats(n, gamma)
    for _ in range(rounds):
        out = _round(host, rew, done, **kw)
    return host, out


@pytest.mark.parametrize("T,n,gamma", rd.GRID)
def test_device_equals_the_host_twin(T, n, gamma):
    """n = 1: one lane; 32: a full tile; 33 and 65: a partial last tile, in the first and in the second workgroup; 257:
    a fifth workgroup with one live lane.  Two rounds, so the second starts from a carry and adds to totals."""
    rew, done = rd.case(T, n)
    obj = RetStats(n, gamma, DEV)
    r, d = dev(rew), dev(done)
    for rounds in (1, 2):
        host, want = _host_round(n, gamma, rew, done, rounds)
        out = Guarded((T, n), torch.float32, DEV)
        _round(obj, r, d, out=out.view)
        assert_same_bits(out.numpy(f"apply {T} x {n}"), want, f"scaled rewards, round {rounds}")
        rd.assert_state(obj, host, f"T={T} n={n} gamma={gamma} round {rounds}")
    assert_same_bits(r, rew, "the raw rewards stay as they are")
    obj.close()


@pytest.mark.parametrize("which", ["non-finite", "clip"])
def test_device_equals_the_host_twin_on_the_special_cases(which):
    rew, done = rd.nonfinite_case()[:2] if which == "non-finite" else rd.clip_case()[:2]
    T, n = rew.shape
    host, want = _host_round(n, 0.9, rew, done)
    obj = RetStats(n, 0.9, DEV)
    got = _round(obj, dev(rew), dev(done))
    assert_same_bits(got, want, which)
    rd.assert_state(obj, host, which)
    if which == "non-finite":
        assert np.isnan(want).sum() == 2 and bool(torch.isfinite(obj.carry).all())
        # a batch that is all NaN leaves the scale where it was
        before = obj.scale.clone()
        nan = torch.full((3, n), float("nan"), dtype=torch.float32, device=DEV)
        obj.update(nan, torch.zeros((3, n), dtype=torch.uint8, device=DEV))
        obj.finalize()
        assert_same_bits(obj.scale, before, "scale after an all-NaN batch")
    else:
        assert (np.abs(want) == 10.0).sum() == 2
    obj.close()


@pytest.mark.parametrize("n", [65, 256])
def test_a_misaligned_input_gives_the_aligned_bits(n):
    """``apply`` takes float4 loads and stores where both pointers are 16-byte aligned and single elements otherwise: a
    rew_in one float off, a rew_out one float off and both off give the aligned call's bits.  T n = 455 leaves a
    three-element tail behind the float4 groups, 1792 none."""
    T = 7
    rew, done = rd.case(T, n, seed=4)
    host, want = _host_round(n, 0.99, rew, done)
    obj = RetStats(n, 0.99, DEV)
    obj.update(dev(rew), dev(done))
    obj.finalize()
    for shift_in, shift_out in ((0, 0), (1, 0), (0, 1), (1, 1)):
        r = surrounded(rew, None, DEV, shift=shift_in)
        assert (r.data_ptr() % 16 == 0) == (shift_in == 0)
        out = Guarded((T, n), torch.float32, DEV, shift=shift_out)
        assert (out.view.data_ptr() % 16 == 0) == (shift_out == 0)
        obj.apply(r, out=out.view)
        assert_same_bits(out.numpy(f"apply shifts {shift_in}, {shift_out}"), want, f"shifts {shift_in}, {shift_out}")
    obj.close()


def test_a_side_stream_and_a_replayed_graph_hold_the_eager_bits():
    T, n, gamma = 5, 65, 0.99
    rew, done = rd.case(T, n, seed=6)
    r, d = dev(rew), dev(done)
    eager = RetStats(n, gamma, DEV)
    first = _round(eager, r, d).clone()
    first_state = eager.state()
    second = _round(eager, r, d).clone()   # from the first round's carry, onto its totals
    assert not np.array_equal(first.cpu().numpy(), second.cpu().numpy())
    # a side stream
    side_obj, side = RetStats(n, gamma, DEV), torch.cuda.Stream(DEV)
    out = torch.full((T, n), float("nan"), dtype=torch.float32, device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        _round(side_obj, r, d, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert_same_bits(out, first, "side stream")
    for k, v in side_obj.state().items():
        assert_same_bits(v, first_state[k], f"side stream {k}")
    # a captured round, replayed twice: the state lives on the device, so the second replay is a second eager round
    obj = RetStats(n, gamma, DEV)
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _round(obj, r, d, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and int(obj.totals[0][0]) == 0   # the capture ran nothing
    graph.replay()
    assert_same_bits(out, first, "first replay")
    graph.replay()
    assert_same_bits(out, second, "second replay")
    rd.assert_state(obj, eager, "after two replays")
    for o in (eager, side_obj, obj):
        o.close()


def test_the_three_launches_are_invariant():
    """n = 65, T = 2: the inputs inside pattern-filled buffers, the scaled rewards between guards, every CU's LDS and
    every SIMD's register file poisoned before the round: the unpoisoned run's bits under each pattern, and the host
    twin's.  The walk's lanes past n, the tree's upper lanes and finalize's LDS slots past the used ones hold
    whatever the poison left there."""
    T, n, gamma = 2, 65, 0.99
    rew, done = rd.case(T, n, seed=7)
    host, want = _host_round(n, gamma, rew, done)
    runs = []
    for run in RUNS:
        obj = RetStats(n, gamma, DEV)
        r, d = surrounded(rew, run, DEV), surrounded(done, run, DEV)
        out = Guarded((T, n), torch.float32, DEV)
        poison.poison_run(run, None, DEV)
        obj.update(r, d)
        poison.poison_run(run, None, DEV)
        obj.finalize()
        poison.poison_run(run, None, DEV)
        obj.apply(r, out=out.view)
        counts, sums = obj.get_slots()
        count, tsums = obj.totals
        runs.append(dict(out=out.numpy(f"apply under {run}"), carry=obj.carry, counts=counts, sums=sums, count=count,
                         tsums=tsums, scale=obj.scale))
        obj.close()
    poison.assert_runs_agree(runs, "return statistics")
    assert_same_bits(runs[0]["out"], want, "scaled rewards")
    for k, v in host.state().items():
        assert_same_bits(runs[0][dict(count="count", sums="tsums", carry="carry", scale="scale")[k]], v, k)


def test_slots_compose_on_the_device():
    T, n, gamma = 6, 128, 0.99
    rew, done = rd.case(T, n, seed=5)
    whole = RetStats(n, gamma, DEV)
    _round(whole, dev(rew), dev(done))
    halves = [RetStats(64, gamma, DEV, n_slots=4) for _ in range(2)]
    for r, h in enumerate(halves):
        h.update(dev(rew[:, 64 * r:64 * (r + 1)]), dev(done[:, 64 * r:64 * (r + 1)]), slot_offset=2 * r)
    for r, h in enumerate(halves):
        counts, sums = halves[1 - r].get_slots(2 * (1 - r), 2)
        h.set_slots(2 * (1 - r), counts, sums)
    for h in halves:
        h.finalize()
        for a, b in zip(h.totals + (h.scale,) + h.get_slots(), whole.totals + (whole.scale,) + whole.get_slots()):
            assert_same_bits(a, b, "halves against the whole")
    assert_same_bits(torch.cat([h.carry for h in halves]), whole.carry, "concatenated carry")
    host, _ = _host_round(n, gamma, rew, done)
    rd.assert_state(whole, host, "the whole against the host twin")
    for o in halves + [whole]:
        o.close()


def test_device_argument_errors():
    obj = RetStats(64, 0.99, DEV)
    rew = torch.zeros((2, 64), dtype=torch.float32, device=DEV)
    done = torch.zeros((2, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(_native.PbgError, match="rew_traj"):
        obj.update(rew.cpu().numpy(), done)   # a host array for a device object
    with pytest.raises(_native.PbgError, match="rew_traj"):
        obj.update(rew.t(), done.t())         # not contiguous
    with pytest.raises(_native.PbgError, match="overlaps"):
        obj.apply(rew, out=rew)
    with pytest.raises(_native.PbgError, match="n = 64"):
        RetStats(32, 0.99, DEV).update(rew, done)   # more envs than the object has
    with pytest.raises(_native.PbgError):
        RetStats(64, 0.99, "cpu:0")
    obj.close()
    with pytest.raises(_native.PbgError, match="closed"):
        obj.finalize()
