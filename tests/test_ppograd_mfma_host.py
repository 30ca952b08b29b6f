"""The matrix-core path of the PPO gradient without a GPU (include/pbg.h "PPO gradient", "The matrix-core path"):
what pbg_ppo_grad_create_ex refuses before any HIP call, what ppo.PPOGrad and ppo.PPO refuse, and the host twin, which
serves both paths."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import PPO, PPOGrad

import ppo_grad_data as gd

E_ARG = -1  # PBG_E_ARG


def create_ex(device, dims, max_rows, path=None, struct_size=None):
    """(return code, the handle's value) of pbg_ppo_grad_create_ex; ``path`` None: opts NULL.  The handle starts as a
    non-NULL marker, so that a NULL afterwards was written by the call."""
    h = ctypes.c_void_p(0xDEAD0)
    opts = None
    if path is not None:
        opts = _native.PPOGradOpts(path=path)
        if struct_size is not None:
            opts.struct_size = struct_size
        opts = ctypes.byref(opts)
    rc = _native.lib().pbg_ppo_grad_create_ex(device, *dims, max_rows, opts, ctypes.byref(h))
    return rc, h.value


def test_the_constants_and_the_symbol():
    assert (_native.PPO_GRAD_FMA, _native.PPO_GRAD_MFMA) == (0, 1)
    assert ctypes.sizeof(_native.PPOGradOpts) == 8
    assert set(_native.PPO_GRAD_EX_EXPORTED) <= set(_native.EXPORTED)
    assert hasattr(_native.lib(), "pbg_ppo_grad_create_ex")


@pytest.mark.parametrize("path,struct_size", [(2, None), (-1, None), (1, 0), (1, ctypes.sizeof(_native.PPOGradOpts) + 4),
                                              (0, 0), (0, ctypes.sizeof(_native.PPOGradOpts) + 4)])
def test_create_ex_refuses_an_unknown_path_and_a_bad_struct_size(path, struct_size):
    rc, h = create_ex(0, (5, 16, 8, 1), 64, path, struct_size)
    assert rc == E_ARG and h is None, (rc, h)


@pytest.mark.parametrize("device,dims,max_rows", [(-1, (5, 16, 8, 1), 64), (0, (5, 16, 8, 1), 0), (0, (5, 16, 8, 1), -3),
                                                  (0, (0, 16, 8, 1), 64), (0, (257, 16, 8, 1), 64), (0, (5, 257, 8, 1), 64),
                                                  (0, (5, 16, 0, 1), 64), (0, (5, 16, 8, 65), 64), (0, (5, 16, 8, 0), 64)])
@pytest.mark.parametrize("path", [None, 0, 1])
def test_create_ex_refuses_what_create_refuses(device, dims, max_rows, path):
    """device < 0, max_rows < 1 and dims out of pbg_policy_create's ranges: PBG_E_ARG before any HIP call (this test
    runs without a GPU), for opts NULL and for both paths."""
    rc, h = create_ex(device, dims, max_rows, path)
    assert rc == E_ARG and h is None, (rc, h)


def test_create_ex_refuses_a_null_out():
    opts = _native.PPOGradOpts(path=1)
    assert _native.lib().pbg_ppo_grad_create_ex(0, 5, 16, 8, 1, 64, ctypes.byref(opts), None) == E_ARG


def test_ppograd_refuses_an_unknown_path():
    for bad in ("x", "MFMA", None, 1):
        with pytest.raises(_native.PbgError):
            PPOGrad((5, 16, 8, 1), 4, path=bad)
    with pytest.raises(_native.PbgError):
        PPOGrad((5, 16, 8, 1), 4, "cuda:0", path="x")   # refused before the device is looked at


class _Env:
    """What PPO's constructor reads before it refuses."""
    num_envs, device, autoreset = 4, "cpu", True


def test_ppo_refuses_the_matrix_core_path_without_the_hip_backward():
    with pytest.raises(_native.PbgError, match="backward"):
        PPO(_Env(), backward="torch", grad_path="mfma")
    with pytest.raises(_native.PbgError, match="grad_path"):
        PPO(_Env(), backward="hip", grad_path="x")


def test_the_host_twin_serves_both_paths():
    dims, B, Bm, seed = gd.CASES[4]
    c = gd.case(dims, B, Bm, seed, True)
    outs = []
    for path in ("fma", "mfma"):
        g = PPOGrad(dims, Bm, path=path)
        assert g.host and g.path == path
        logp, v = np.zeros(Bm, np.float32), np.zeros(Bm, np.float32)
        res = g.run(c["theta_actor"], c["theta_critic"], c["log_std"], c["obs"], c["act"], c["logp_old"], c["adv"], c["ret"],
                    idx=c["idx"], adv_norm=c["adv_norm"], obs_norm=(c["mean"], c["inv_std"], c["clip"]), clip_eps=gd.CLIP_EPS,
                    vf_coef=gd.VF_COEF, ent_coef=0.01, logp_out=logp, v_out=v)
        outs.append(tuple(res) + (logp, v))
        g.close()
    assert np.abs(outs[0][0]).max() > 0.0
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
