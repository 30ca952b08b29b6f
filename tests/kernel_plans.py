"""One list of kernel plans for the tests that must reach every kernel instantiation, taken from the
recorded plan table (tests/golden/plan_table.json, tests/test_plan_table.py), and the float64 scene
variants of tests/test_f64.py.  No GPU and no torch: the CPU tests read the same lists.

A plan is an env id and the VecEnv options that select one kernel instantiation.  ``plans(precision)``
returns one for every distinct successful row of the table at 64 envs -- distinct: another
(lanes_per_env, block, lds_bytes, lds_rows) of the same env id -- and, where the table creates a handle
with gang_dist = 0 and with gang_dist = 1 under otherwise the same options, one for each: replicated and
distributed gang dynamics are two kernels with one geometry.  A plan added to the table later is in the
list, and in every test parametrised by it, without an edit here (tests/test_kernel_plans_host.py checks that)."""
import itertools
import json
import os

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_table.json")
N_ENVS = 64
GEOMETRY = ("lanes_per_env", "block", "lds_bytes", "lds_rows")
OPTS = ("kernel", "gang_lanes", "gang_dist")

with open(TABLE) as _f:
    T = json.load(_f)  # read once, never modified


def table_rows(precision, n_envs=N_ENVS):
    """Every successful case of the table at this precision and env count, in the table's order:
    (env_id, {kernel, gang_lanes, gang_dist}, (lanes_per_env, block, lds_bytes, lds_rows))."""
    names = [a for a, _ in T["axes"]]
    assert names == ["precision"] + list(OPTS) + ["n_envs"] and T["fields"][0] == "rc"
    geo = [T["fields"].index(f) for f in GEOMETRY]
    out = []
    for case, row in zip(itertools.product(T["env_ids"], *(v for _, v in T["axes"])), T["index"]):
        env_id, prec, n = case[0], case[1], case[-1]
        r = T["rows"][row]
        if prec == precision and n == n_envs and r[0] == 0:
            out.append((env_id, dict(zip(OPTS, case[2:5])), tuple(r[i] for i in geo)))
    return out


def _explicit(opts):
    return sum(v != -1 for v in opts.values())


def plans(precision):
    """[(env_id, opts, geometry)]: opts holds only the options that differ from the default (-1), the
    fewest that reach the geometry; a gang_dist entry only where both values are honoured."""
    groups = {}
    for env_id, opts, geo in table_rows(precision):
        groups.setdefault((env_id, geo), []).append(opts)
    out = []
    for (env_id, geo), cases in groups.items():  # dicts keep the table's order
        base = min((o for o in cases if o["gang_dist"] == -1), key=_explicit)  # ties: the table's first
        opts = {k: v for k, v in base.items() if v != -1}
        if all(dict(base, gang_dist=d) in cases for d in (0, 1)):
            out += [(env_id, dict(opts, gang_dist=d), geo) for d in (0, 1)]
        else:
            out.append((env_id, opts, geo))
    return out


def plan_id(env_id, opts):
    return "-".join([env_id] + [f"{k}={v}" for k, v in opts.items()]) if opts else env_id


def params(precision):
    """pytest.param(env_id, opts) per plan, with readable ids."""
    import pytest
    return [pytest.param(e, o, id=plan_id(e, o)) for e, o, _ in plans(precision)]


def lanes_of(precision, env_id, opts):
    """lanes_per_env the table records for these options (64 envs); None where it records a refusal."""
    want = dict({k: -1 for k in OPTS}, **opts)
    for e, o, geo in table_rows(precision):
        if e == env_id and o == want:
            return geo[0]
    return None


# ------------------------------------------------------------------ float64 scene variants
# (env id, scene overrides, [(options, lanes_per_env they select)]): every float64 kernel family --
# lane, quad, 16- and 32-lane gangs, replicated and distributed dynamics -- under a scene that changes
# timestep, frame_skip, both ERPs, gravity and the sweep count, and the documented edges: gravity 0,
# ERP 0 and 1, one PGS sweep, frame_skip 1.  tests/test_kernel_plans_host.py checks on the CPU that
# each scene leaves the default scene's trajectory and that the options select the stated kernel.
_P = "PyBulletEnv-v0"
_M = "MuJoCoEnv-v0"
F64_SCENE_VARIANTS = [
    ("InvertedPendulum" + _P, {"gravity": 3.7, "timestep": 0.01}, [({}, 1)]),
    ("InvertedDoublePendulum" + _P, {"frame_skip": 3, "timestep": 0.0055, "joint_limit_erp": 0.5}, [({}, 1)]),
    ("Hopper" + _P, {"contact_erp": 0.0}, [({}, 16), ({"gang_dist": 1}, 16), ({"kernel": 0}, 1)]),
    ("Hopper" + _P, {"contact_erp": 1.0, "joint_limit_erp": 1.0}, [({}, 16)]),
    ("Hopper" + _M, {"timestep": 0.002, "frame_skip": 6}, [({}, 16), ({"gang_dist": 1}, 16)]),
    ("HalfCheetah" + _P, {"gravity": 12.0, "joint_limit_erp": 0.4, "solver_iterations": 3}, [({}, 16)]),
    ("HalfCheetah" + _M, {"solver_iterations": 1}, [({}, 16)]),
    ("Walker2D" + _P, {"joint_limit_erp": 0.0}, [({}, 16), ({"kernel": 0}, 1)]),
    ("Walker2D" + _M, {"solver_iterations": 20}, [({}, 16)]),
    ("Ant" + _P, {"frame_skip": 1, "timestep": 0.0165}, [({}, 4), ({"kernel": 2}, 16), ({"kernel": 0}, 1)]),
    ("Ant" + _P, {"contact_erp": 0.5, "frame_skip": 8, "timestep": 0.0165 / 8}, [({}, 4)]),
    ("Ant" + _M, {"gravity": 0.0}, [({}, 4)]),
    ("Humanoid" + _P, {"timestep": 0.0165 / 5, "frame_skip": 5, "contact_erp": 0.3},
     [({}, 32), ({"gang_lanes": 16}, 16), ({"kernel": 0}, 1)]),
    ("Humanoid" + _M, {"gravity": 0.0}, [({}, 32)]),
    ("HumanoidFlagrun" + _P, {"frame_skip": 7, "timestep": 0.0165 / 7}, [({}, 32)]),
    ("HumanoidFlagrunHarder" + _P, {"gravity": 9.0, "solver_iterations": 6}, [({}, 32), ({"gang_lanes": 16}, 16)]),
    ("Atlas" + _P, {"frame_skip": 4, "timestep": 0.0165 / 4, "solver_iterations": 8}, [({}, 16)]),
]
# the float32 edge rows of tests/test_gpu.py's SIM_VARIANTS
F32_EDGE_VARIANTS = [("Ant" + _M, {"gravity": 0.0}), ("Hopper" + _P, {"contact_erp": 0.0}),
                     ("Walker2D" + _P, {"joint_limit_erp": 0.0}), ("HalfCheetah" + _M, {"solver_iterations": 1})]


def scene_size(env_id):
    """(envs, steps) of a float64 scene-variant case."""
    return (32, 12) if env_id.startswith("Atlas") else (64, 20)


def f64_scene_cases():
    """(env_id, overrides, opts) per float64 scene-variant case."""
    return [(e, over, opts) for e, over, kernels in F64_SCENE_VARIANTS for opts, _ in kernels]


def scene_id(env_id, over, opts=None):
    s = env_id + "-" + ",".join(f"{k}={v:.6g}" for k, v in over.items())
    return s + ("-" + plan_id("", opts)[1:] if opts else "")
