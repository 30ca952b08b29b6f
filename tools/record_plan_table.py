#!/usr/bin/env python3
"""Record the kernel-plan table tests/test_plan_table.py compares against (tests/golden/plan_table.json).

For every robot x precision x kernel x gang_lanes x gang_dist x n_envs it creates a handle with
pbg_create_v2 and notes the return code and, on success, pbg_info's robot_id, lanes_per_env, block,
lds_bytes and lds_rows; nothing is launched.  The table is the behaviour of the commit whose library it
loads: record it from a build of the commit a host-side change starts from (its hash goes into the
file), never from the tree under test.

    python tools/record_plan_table.py --parent $(git rev-parse --short HEAD~) --out tests/golden/plan_table.json
"""
import argparse
import ctypes
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pybulletgym_amd  # noqa: E402,F401
from pybulletgym_amd import _native  # noqa: E402

AXES = (("precision", (32, 64)), ("kernel", (-1, 0, 2)), ("gang_lanes", (-1, 16, 32)), ("gang_dist", (-1, 0, 1)),
        ("n_envs", (64, 16384)))
FIELDS = ("rc", "robot_id", "lanes_per_env", "block", "lds_bytes", "lds_rows")


def outcome(L, env_id, precision, kernel, gang_lanes, gang_dist, n_envs):
    """The FIELDS of one pbg_create_v2 call (a failed create: the return code alone)."""
    o = _native.CreateOpts(precision=precision, kernel=kernel, gang_lanes=gang_lanes, gang_dist=gang_dist)
    h = ctypes.c_void_p()
    rc = L.pbg_create_v2(env_id.encode(), n_envs, 0, 0, 0, None, ctypes.byref(o), ctypes.byref(h))
    if rc != 0:
        assert not h.value
        return [rc]
    info = _native.Info()
    assert L.pbg_info(h, ctypes.byref(info)) == 0
    L.pbg_destroy(h)
    return [rc] + [getattr(info, f) for f in FIELDS[1:]]


def cases(env_ids):
    """Every (env_id, precision, kernel, gang_lanes, gang_dist, n_envs), the last axis fastest."""
    return itertools.product(env_ids, *(v for _, v in AXES))


def record(L, env_ids):
    """(distinct outcome rows, one row index per case in cases() order)."""
    rows, index = [], []
    for c in cases(env_ids):
        r = outcome(L, *c)
        if r not in rows:
            rows.append(r)
        index.append(rows.index(r))
    return rows, index


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", required=True, help="hash of the commit whose build is loaded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    env_ids = sorted(_native.ROBOT_IDS, key=_native.ROBOT_IDS.get)
    rows, index = record(_native.lib(), env_ids)
    props = torch.cuda.get_device_properties(0)
    doc = {"parent": a.parent, "device": props.name, "cus": props.multi_processor_count, "env_ids": env_ids,
           "axes": [[k, list(v)] for k, v in AXES], "fields": list(FIELDS), "rows": rows, "index": index}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(index)} cases, {len(rows)} distinct outcomes, {doc['cus']} CUs -> {a.out}")


if __name__ == "__main__":
    main()
