"""tools/benchlib.py, the measurement protocol of the tools/bench_*.py scripts, without a GPU: the summary, the
alternation and the per-call division of both window loops under an injected clock and synchronise, and a child
process's result line."""
import argparse
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import benchlib  # noqa: E402

ARGS = argparse.Namespace(warmup=1, windows=2, calls=3, iterations=4)


def test_summary_of_hand_made_windows():
    w = {"a": [3.0, 1.0, 2.0], "b": [4.0, 10.0]}
    s = benchlib.summary(w)
    assert s == {"windows": w, "median": {"a": 2.0, "b": 7.0}, "min": {"a": 1.0, "b": 4.0}, "max": {"a": 3.0, "b": 10.0}}


class Script:
    """Legs that log their calls and advance a fake clock by a cost of their own; the clock's other readers log too."""

    def __init__(self, costs):
        self.now, self.log = 0.0, []
        self.legs = {leg: (lambda leg=leg, c=c: self.call(leg, c)) for leg, c in costs.items()}

    def call(self, leg, cost):
        self.log.append(leg)
        self.now += cost

    def sync(self):
        self.log.append("sync")

    def clock(self):
        return self.now


def test_wall_windows_alternate_the_legs_and_divide_by_the_calls():
    s = Script({"A": 0.002, "B": 0.005})
    after = []
    w = benchlib.wall_windows(s.sync, s.legs, windows=3, calls=4, clock=s.clock, after=after.append)
    assert s.log == (["sync"] + ["A"] * 4 + ["sync"] + ["sync"] + ["B"] * 4 + ["sync"]) * 3   # A B A B A B, a sync each side
    assert after == ["A", "B"] * 3
    assert w == {"A": [pytest.approx(2.0)] * 3, "B": [pytest.approx(5.0)] * 3}   # ms per call


def test_device_windows_alternate_the_legs_and_divide_by_the_calls():
    s = Script({"A": 6.0, "B": 9.0, "G": 30.0})

    class Watch:   # DeviceEvents' three methods on the fake clock, in us
        sync = s.sync

        def start(self):
            self.t0 = s.now

        def stop(self):
            s.sync()
            return s.now - self.t0

    w = benchlib.device_windows(None, s.legs, windows=2, calls=5, warmup=2, per=3, once=("G",), watch=Watch())
    warm = ["A", "B", "G"] * 2                                     # untimed, and alternated as well
    window = ["sync"] + ["A"] * 5 + ["sync"] + ["sync"] + ["B"] * 5 + ["sync"] + ["sync", "G", "sync"]
    assert s.log == warm + window * 2
    # us per call and per step: G's one call holds the 5 calls of a window
    assert w == {"A": [pytest.approx(6.0 / 3)] * 2, "B": [pytest.approx(9.0 / 3)] * 2, "G": [pytest.approx(30.0 / 15)] * 2}


def test_run_child_takes_the_last_json_line(tmp_path):
    script = tmp_path / "child.py"
    script.write_text("import sys\nprint('loading')\nprint('{\"not\": \"this\"}')\nprint(sys.argv[1:])\n"
                      "print('{\"windows\": [1.5, 2.5], \"argv\": %s}' % str(sys.argv[1:]).replace(\"'\", '\"'))\n")
    got = benchlib.run_child(str(script), "legA,legB", ARGS, lib="/some/lib.so", timeout=60)
    assert got["windows"] == [1.5, 2.5]
    assert got["argv"] == ["--child", "legA,legB", "--warmup", "1", "--windows", "2", "--calls", "3", "--iterations", "4",
                           "--lib", "/some/lib.so"]


def test_run_child_raises_with_the_end_of_stderr(tmp_path):
    script = tmp_path / "child.py"
    script.write_text("import sys\nprint('{\"fine\": true}')\nsys.stderr.write('x' * 5000 + 'the reason')\nsys.exit(3)\n")
    with pytest.raises(RuntimeError) as e:
        benchlib.run_child(str(script), "leg", ARGS, timeout=60)
    msg = str(e.value)
    assert "failed (3)" in msg and msg.endswith("the reason") and len(msg.split("\n", 1)[1]) == 3000
