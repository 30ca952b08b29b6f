"""CPU: tests/kernel_plans.py's lists are what the GPU tests parametrised by them take them for.

  * The plan list covers the recorded plan table: every distinct successful instantiation at 64 envs, both
    gang dynamics where both exist.  A plan added to the table is then inside the poison-invariance and the
    sub-step composition tests.
  * The float64 scene variants select the kernels they name (by the table), between them reach every float64
    kernel family and every scene field and edge, and none is a no-op: the oracle under the variant's scene
    leaves the default scene's trajectory in at least 95 % of the envs within the steps the GPU test runs."""
import numpy as np
import pytest

import kernel_plans as kp
import oracle
import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native

MOVED = 1e-6
MOVED_SHARE = 0.95


@pytest.mark.parametrize("precision", [32, 64])
def test_plan_list_covers_the_table(precision):
    rows = kp.table_rows(precision)
    listed = kp.plans(precision)
    want = {}  # (env id, geometry) -> every option set of the table that reaches it
    for e, o, g in rows:
        want.setdefault((e, g), []).append(o)
    # every distinct (env id, geometry) of the table is listed, and nothing else
    assert set(want) == {(e, g) for e, _, g in listed}
    # ... twice where some option set is honoured with gang_dist = 0 and with gang_dist = 1
    both = {k for k, cases in want.items() if any(all(dict(o, gang_dist=d) in cases for d in (0, 1)) for o in cases)}
    assert len(listed) == len(want) + len(both)
    for e, o, g in listed:
        # each entry's options are a successful row of the table with that geometry
        assert (e, dict({k: -1 for k in kp.OPTS}, **o), g) in rows, (e, o)
        assert ("gang_dist" in o) == ((e, g) in both), (e, o)
    for k in both:
        assert sorted(o["gang_dist"] for e, o, g in listed if (e, g) == k) == [0, 1], k
    assert len({kp.plan_id(e, o) for e, o, _ in listed}) == len(listed)
    assert {e for e, _, _ in listed} == set(kp.T["env_ids"])


def test_f64_scene_variants_reach_every_family_field_and_edge():
    fams = set()
    for env_id, over, kernels in kp.F64_SCENE_VARIANTS:
        assert set(over) <= set(oracle.SIM_PARAM_FIELDS)
        for opts, lanes in kernels:
            assert kp.lanes_of(64, env_id, opts) == lanes, (env_id, opts)
            has_repl = any(e == env_id and o == dict(opts, gang_dist=0) for e, o, _ in kp.plans(64))
            fams.add((lanes, has_repl and opts.get("gang_dist", 0) == 0))  # (width, replicated gang dynamics)
    assert fams == {(1, False), (4, False), (16, False), (16, True), (32, False)}
    assert {k for _, over, _ in kp.F64_SCENE_VARIANTS for k in over} == set(oracle.SIM_PARAM_FIELDS)
    edges = [{"gravity": 0.0}, {"contact_erp": 0.0}, {"contact_erp": 1.0}, {"joint_limit_erp": 0.0},
             {"joint_limit_erp": 1.0}, {"solver_iterations": 1}, {"frame_skip": 1}]
    for edge in edges:
        assert any(edge.items() <= over.items() for _, over, _ in kp.F64_SCENE_VARIANTS), edge
    assert len(kp.f64_scene_cases()) == sum(len(k) for _, _, k in kp.F64_SCENE_VARIANTS)
    for env_id, over in kp.F32_EDGE_VARIANTS:
        assert any(e == env_id and over.items() <= o.items() for e, o, _ in kp.F64_SCENE_VARIANTS), (env_id, over)


def _oracle_states(env_id, n, steps, sim):
    """The oracle's float64 state after each of ``steps`` env steps from the same U(-0.1, 0.1) reset under the
    same U(-1, 1) actions, in the scene ``sim`` (None: the reference's)."""
    oracle.set_sim_params(sim)
    try:
        e = oracle.OracleEnvs(env_id, n, nthreads=16, seed=3)
        r = np.random.default_rng(3)
        e.reset(r.uniform(-0.1, 0.1, (n, e.info.NR)).astype(np.float32))
        out = []
        for _ in range(steps):
            e.step(r.uniform(-1, 1, (n, e.info.NA)).astype(np.float32))
            out.append(e.state.copy())
        return np.stack(out)
    finally:
        oracle.set_sim_params(None)


@pytest.fixture(scope="module")
def default_states():
    cache = {}

    def get(env_id):
        if env_id not in cache:
            cache[env_id] = _oracle_states(env_id, *kp.scene_size(env_id), None)
            cache[env_id].setflags(write=False)
        return cache[env_id]
    return get


@pytest.mark.parametrize("env_id,over", [pytest.param(e, o, id=kp.scene_id(e, o)) for e, o, _ in kp.F64_SCENE_VARIANTS])
def test_scene_variant_leaves_the_default_trajectory(env_id, over, default_states):
    n, steps = kp.scene_size(env_id)
    base = default_states(env_id)
    sp = _native.default_sim_params(env_id).as_dict()
    assert any(sp[k] != v for k, v in over.items())
    sp.update(over)
    var = _oracle_states(env_id, n, steps, sp)
    assert np.isfinite(var).all() and np.isfinite(base).all()
    moved = np.abs(var - base).max(axis=(0, 2)) > MOVED  # per env: any state word at any step
    assert moved.mean() >= MOVED_SHARE, (env_id, over, float(moved.mean()))
