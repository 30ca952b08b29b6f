"""Sub-step composition, bit for bit: one env step at frame_skip = K leaves the state that K env steps at
frame_skip = 1 leave, with the same timestep and the same action repeated -- for every kernel plan of the
recorded table (tests/kernel_plans.py) at both precisions.

The step kernels run their K sub-steps inside one launch and keep the state in registers and LDS between them;
the record in HBM is all that crosses a launch boundary.  A value that survives from one sub-step to the next
outside the record -- a stale contact row, a solver impulse, a wait that let an old word through -- reads as a
small oracle-parity error at most.  Here it is a different bit: handle B (frame_skip 1) crosses a launch
boundary after every sub-step, handle A (the reference scene, K = 4; Atlas 8; the pendulums, whose scene has
one sub-step, run frame_skip 2 against 2 x 1) never does.

Compared after every env step of A: the physical state words [0, 13 + 2 NJ) as uint64, the last sub-step's
contact count, and the float32 observation as uint32 -- outside the feet-contact columns of the
PyBullet-observation walkers, which hold the previous env step's contacts (the MuJoCo-observation ids and the
pendulums compare every column).  Rewards, contact-set signatures and the aux record depend on Scene.dt and on
the sub-step index by design and are not compared.  The float32 kernels store float32 values exactly in the
float64 record, so bitwise equality is the expectation at both precisions; the oracle composes exactly in its
float64 and its IEEE-float32 instantiation (tests/test_substep_composition_host.py).  First run on an MI355X:
every plan of both precisions is bitwise, so no family carries a value and none has a relaxed bound.
HumanoidFlagrunHarder's cube launches after frame 100, counted in env steps: B reaches 80; the cube's words lie
past the compared range."""
import numpy as np
import pytest
import torch

import kernel_plans
import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import robots
from pybulletgym_amd.vec_env import VecEnv, sample_actions

pytestmark = pytest.mark.gpu

SEED = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _size(env_id):
    """(envs, env steps of A, K, A's scene overrides)."""
    if env_id.startswith("Atlas"):
        return 32, 12, 8, None
    if robots.spec_for(env_id).kind == robots.KIND_PENDULUM:
        return 64, 20, 2, {"frame_skip": 2}
    return 64, 20, 4, None


CASES = [pytest.param(p, e, o, id=f"f{p}-" + kernel_plans.plan_id(e, o)) for p in (64, 32)
         for e, o, _ in kernel_plans.plans(p)]


@pytest.mark.parametrize("precision,env_id,opts", CASES)
def test_one_step_of_k_substeps_equals_k_steps_of_one(precision, env_id, opts):
    n, steps, K, scene = _size(env_id)
    spec = robots.spec_for(env_id)
    kw = dict(seed=SEED, autoreset=False, precision=precision, **opts)
    A = VecEnv(env_id, n, sim_params=scene, **kw)
    B = VecEnv(env_id, n, sim_params={"frame_skip": 1}, **kw)
    assert A.info.substeps == K and B.info.substeps == 1
    assert A.sim_params.timestep == B.sim_params.timestep
    q0 = np.random.default_rng(SEED).uniform(-0.1, 0.1, (n, A.info.reset_dofs)).astype(np.float32)
    A.reset(init_q=torch.from_numpy(q0))
    B.set_state(*A.get_state())
    acts = sample_actions(A.info.action_dim, n, steps, seed=SEED)
    words = 13 + 2 * A.info.n_joints
    cols = A.info.obs_dim - (A.info.n_feet if spec.kind == robots.KIND_WALKER else 0)
    assert 0 < words <= A.info.state_words and cols > 0
    most = 0
    for t in range(steps):
        ra = A.step(acts[t], want_contacts=True)
        for _ in range(K):
            rb = B.step(acts[t], want_contacts=True)
        sa, sb = (e.get_state()[0][:, :words].cpu().numpy().view(np.uint64) for e in (A, B))
        np.testing.assert_array_equal(sa, sb, err_msg=f"state, env step {t}")
        ca, cb = A.ncontact.cpu().numpy(), B.ncontact.cpu().numpy()
        np.testing.assert_array_equal(ca, cb, err_msg=f"ncontact, env step {t}")
        oa, ob = (r.obs[:, :cols].cpu().numpy().view(np.uint32) for r in (ra, rb))
        np.testing.assert_array_equal(oa, ob, err_msg=f"obs, env step {t}")
        most = max(most, int(ca.max()))
    assert np.isfinite(A.get_state()[0][:, :words].cpu().numpy()).all()
    if spec.kind != robots.KIND_PENDULUM:
        assert most > 0  # the contact path ran
    A.close()
    B.close()
