"""The measurement protocol of the tools/bench_*.py scripts, in one place.

A figure is a median over `windows` timed windows with [min, max] beside it.  A window is `calls` calls of one leg
between two synchronises; the legs are alternated per window (A B A B, not A A B B), so that a drift of the clocks or
of the machine lands on every leg alike.  Launches are timed by device events in us per call (device_windows), whole
trainer iterations by a host clock around a synchronise in ms per call (wall_windows; pendulum_windows is that loop
on the pendulum trainer every learner benchmark shares).  A library is loaded once per process, so two builds of
libpbg_amd.so are compared by one child process per library (use_library, run_child), whose last stdout line is its
result as JSON.  A function lives here when at least two scripts call it; the legs, shapes, result keys and printed
lines are each script's own.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# the pendulum trainer of profiles/ppo_*.json: 256 envs x 32 steps, 4 epochs x 4 minibatches
ENV_ID, ENVS = "InvertedPendulumPyBulletEnv-v0", 256
HP = dict(hidden=(64, 64), steps=32, lr=3e-3, epochs=4, minibatches=4, log_std=-0.5)


def summary(w):
    """{leg: [window, ...]} with its medians, minima and maxima."""
    return {"windows": w, "median": {k: statistics.median(v) for k, v in w.items()}, "min": {k: min(v) for k, v in w.items()},
            "max": {k: max(v) for k, v in w.items()}}


class DeviceEvents:
    """The stopwatch of device_windows: us between two events on `dev`'s current stream."""

    def __init__(self, dev):
        import torch
        self.sync = lambda: torch.cuda.synchronize(dev)
        self.stream = torch.cuda.current_stream(dev)
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def start(self):
        self.e0.record(self.stream)

    def stop(self):
        self.e1.record(self.stream)
        self.sync()
        return self.e0.elapsed_time(self.e1) * 1e3


class WallClock:
    """The stopwatch of wall_windows: ms of `clock` (seconds) up to the end of a `sync`."""

    def __init__(self, sync, clock=time.perf_counter):
        self.sync, self.clock = sync, clock

    def start(self):
        self.t0 = self.clock()

    def stop(self):
        self.sync()
        return (self.clock() - self.t0) * 1e3


def warm_up(legs, n):
    for _ in range(n):
        for f in legs.values():
            f()


def _windows(watch, legs, windows, calls, per=1, once=(), after=None):
    w = {leg: [] for leg in legs}
    for _ in range(windows):
        for leg, f in legs.items():
            watch.sync()
            watch.start()
            for _ in range(1 if leg in once else calls):
                f()
            w[leg].append(watch.stop() / (calls * per))
            if after:
                after(leg)
    return w


def device_windows(dev, legs, windows, calls, warmup=0, per=1, once=(), watch=None):
    """{leg: [us per call]} of the callables `legs` after `warmup` untimed rounds over them.  per: what a call holds
    (the steps of a replayed graph).  once: legs whose callable already holds `calls` calls, run once per window."""
    warm_up(legs, warmup)
    return _windows(watch or DeviceEvents(dev), legs, windows, calls, per, once)


def wall_windows(sync, legs, windows, calls, clock=time.perf_counter, after=None):
    """{leg: [ms per call]} of the callables `legs` by `clock` around `sync`, the device's synchronise.  after(leg)
    runs behind each window, untimed."""
    return _windows(WallClock(sync, clock), legs, windows, calls, after=after)


def pendulum_windows(dev, legs, windows, iterations, base=None, after=None):
    """One pendulum trainer PPO(**HP, **base, **kw) per leg of `legs` (leg -> kw), each on a VecEnv of its own and
    three iterations old: ({leg: [ms per PPO.iterate()]}, {leg: whether its actor's parameters are still finite}).
    after(leg, ppo) runs behind each window, untimed."""
    import torch
    from pybulletgym_amd.ppo import PPO
    from pybulletgym_amd.vec_env import VecEnv
    tr = {}
    for leg, kw in legs.items():
        env = VecEnv(ENV_ID, ENVS, device=dev, seed=0, autoreset=True, precision=64)
        tr[leg] = (env, PPO(env, seed=0, **HP, **(base or {}), **kw))
        for _ in range(3):
            tr[leg][1].iterate()
    w = wall_windows(lambda: torch.cuda.synchronize(dev), {leg: ppo.iterate for leg, (_, ppo) in tr.items()}, windows,
                     iterations, after=after and (lambda leg: after(leg, tr[leg][1])))
    finite = {leg: bool(torch.isfinite(ppo.actor_theta.data).all()) for leg, (_, ppo) in tr.items()}
    for env, ppo in tr.values():
        ppo.close()
        env.close()
    return w, finite


def capture(fn, dev):
    """fn's launches as a graph, captured on a side stream."""
    import torch
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    torch.cuda.current_stream(dev).wait_stream(s)
    return g


def use_library(path):
    """Make this process load another build of libpbg_amd.so (None: this tree's); before the first native call."""
    import pybulletgym_amd  # noqa: F401
    from pybulletgym_amd import _native
    if path:
        _native.LIB_PATH = os.path.abspath(path)


def child_cmd(script, what, args, lib=None):
    """The command of `script --child what` under the protocol options of the parsed `args`."""
    cmd = [sys.executable, os.path.abspath(script), "--child", what]
    for k in ("warmup", "windows", "calls", "iterations"):
        cmd += ["--" + k, str(getattr(args, k))]
    if hasattr(args, "shapes"):
        cmd += ["--shapes"] + list(args.shapes)
    return cmd + (["--lib", lib] if lib else [])


def last_json(cmd, returncode, stdout, stderr):
    """A child's result: the last line of its stdout; a failed child raises with the end of its stderr."""
    if returncode:
        raise RuntimeError(f"{' '.join(cmd)} failed ({returncode}):\n{stderr[-3000:]}")
    return json.loads(stdout.strip().splitlines()[-1])


def run_child(script, what, args, lib=None, timeout=600):
    """One process, one library: `script --child what` [--lib lib], and the JSON line it ends with."""
    cmd = child_cmd(script, what, args, lib)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return last_json(cmd, p.returncode, p.stdout, p.stderr)


def parser(out, warmup=5, calls=None, calls_help=None, iterations_help=None, rounds=None):
    """The options every script has (--out under profiles/, --warmup, --windows), with --calls and --iterations
    where a help text is given, and with --lib, --rounds and the hidden --child where `rounds` (the default) is."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=out and os.path.join(REPO, "profiles", out))
    if rounds:
        ap.add_argument("--lib", default=None, help="another build of libpbg_amd.so (the parent commit's, to alternate with)")
        ap.add_argument("--rounds", type=int, default=rounds, help="child processes per library")
        ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--windows", type=int, default=5)
    if calls_help:
        ap.add_argument("--calls", type=int, default=calls, help=calls_help)
    if iterations_help:
        ap.add_argument("--iterations", type=int, default=5, help=iterations_help)
    return ap


def finish(res, out, done=True):
    """Write the result and print the line a caller waits for."""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"done": done, "out": out}))
