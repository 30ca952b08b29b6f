"""The kernel plan of every robot x precision x kernel x gang_lanes x gang_dist x n_envs against the table
recorded from the commit the host-side launcher refactor started from (tests/golden/plan_table.json,
tools/record_plan_table.py): pbg_create_v2's return code and, on success, pbg_info's robot_id,
lanes_per_env, block, lds_bytes and lds_rows.  Handles are created and destroyed; nothing is launched."""
import ctypes
import itertools
import json
import os

import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native, robots

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_table.json")
AXES = [["precision", [32, 64]], ["kernel", [-1, 0, 2]], ["gang_lanes", [-1, 16, 32]], ["gang_dist", [-1, 0, 1]],
        ["n_envs", [64, 16384]]]
FIELDS = ["rc", "robot_id", "lanes_per_env", "block", "lds_bytes", "lds_rows"]


with open(TABLE) as _f:
    T = json.load(_f)  # read once, never modified


def test_table_covers_every_case():
    """CPU: the recorded file holds the whole product of the axes for every robot of the registry."""
    assert T["env_ids"] == [s.env_id for s in robots.BY_ID]
    assert T["axes"] == AXES and T["fields"] == FIELDS
    assert len(T["index"]) == len(T["env_ids"]) * 2 * 3 * 3 * 3 * 2
    assert set(T["index"]) == set(range(len(T["rows"])))
    assert T["parent"] and T["cus"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("precision", T["axes"][0][1])
@pytest.mark.parametrize("robot", range(len(T["env_ids"])), ids=T["env_ids"])
def test_plans_match_the_recorded_table(robot, precision):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == T["cus"], (f"the plan depends on the CU count: the table was recorded on {T['cus']} CUs "
                             f"({T['device']}, commit {T['parent']}), this device has {cus}")
    L = _native.lib()
    bad = []
    # this (robot, precision)'s slice of the table: the cases run robot-major, precision next
    per = len(T["index"]) // (len(T["env_ids"]) * len(T["axes"][0][1]))
    first = (robot * len(T["axes"][0][1]) + T["axes"][0][1].index(precision)) * per
    cases = itertools.product([T["env_ids"][robot]], [precision], *(v for _, v in T["axes"][1:]))
    for (env_id, _, kernel, gang_lanes, gang_dist, n_envs), row in zip(cases, T["index"][first:first + per]):
        o = _native.CreateOpts(precision=precision, kernel=kernel, gang_lanes=gang_lanes, gang_dist=gang_dist)
        h = ctypes.c_void_p()
        got = [L.pbg_create_v2(env_id.encode(), n_envs, 0, 0, 0, None, ctypes.byref(o), ctypes.byref(h))]
        if got[0] == 0:
            info = _native.Info()
            assert L.pbg_info(h, ctypes.byref(info)) == 0
            got += [getattr(info, f) for f in FIELDS[1:]]
            L.pbg_destroy(h)
        else:
            assert not h.value
        if got != T["rows"][row]:
            bad.append(((env_id, precision, kernel, gang_lanes, gang_dist, n_envs), got, T["rows"][row]))
    assert not bad, (len(bad), bad[:8])
