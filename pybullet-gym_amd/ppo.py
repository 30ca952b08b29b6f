"""Proximal policy optimisation on the device (Schulman et al. 2017) and generalised advantage estimation
(Schulman et al. 2016).

The per-step path is HIP: ``VecEnv.rollout`` with an ``ActionNoise`` attached acts ``a = mu(obs) + std eps``
inside the actor launch and records ``sum eps^2`` for the log-probability (include/pbg.h "Stochastic Gaussian
actions"), the critic's values are one ``MLPPopulation.act`` over the whole trajectory, and ``gae`` is one
launch (pbg_gae).  The backward pass is torch autograd by default (``PPO(backward="torch")``); with
``backward="hip"`` each minibatch's gradient is ``PPOGrad.run``: two launches (pbg_ppo_grad, include/pbg.h "PPO
gradient"), and with ``optimizer="hip"`` the advantage normaliser, the gradient clipping and Adam are ``adv_norm`` and
``AdamClip`` (pbg_adv_norm, pbg_ppo_opt, include/pbg.h "PPO optimiser step"): three more launches, optionally
the whole update as one captured graph.  The collection half of an iteration has no host work between its launches.
``Permutation`` (pbg_perm, include/pbg.h "Counter-based permutations") draws the minibatch permutations on the device,
``lr_linear`` (pbg_ppo_lr_linear) writes a scheduled learning rate that ``AdamClip.step`` reads from device memory, and
with both an iteration can be one captured graph (``PPO(graph="iteration")``).  ``RetStats`` (pbg_ret_stats, include/pbg.h
"Return statistics") keeps a running standard deviation of the discounted return on the device and scales the rewards
``gae`` sees by it (``PPO(reward_norm=True)``): three launches more, inside the captured iteration too.  ``PPOGrad.run(...,
value_old=, vf_clip=)`` is PPO2's clipped value loss inside the gradient's kernels, and ``KLGate`` (pbg_ppo_gate, include/pbg.h
"Value clipping and the KL gate") an early stop of the update that lives on the device: one more launch per minibatch writes
a word that the gradient's and the optimiser's launches read and obey (``PPO(vf_clip=, target_kl=)``).

Who owns what.  ``policy._NativeObject`` is the base of every wrapper here (``PPOGrad``, ``AdamClip``, ``Permutation``,
``RetStats``, ``KLGate``): the handle, ``close``, the closed guard, the device, and ``_ptr`` / ``_new`` / ``_launch``, which are
``policy.check_array`` / ``new_array`` / ``launch`` on the object's side (its GPU, or the host twin's numpy arrays).  The
free functions ``gae``, ``adv_norm`` and ``lr_linear`` call the same three directly.  In the trainer ``PPO._grad_args`` is
the one place that knows what ``PPOGrad.run`` takes, ``PPO._gradient`` the one call of it (``ShardedPPO._gradient``: of
``run_part`` and ``reduce``), and ``PPO._chain`` the one ``epochs x minibatches`` loop of ``optimizer="hip"``, called,
captured or called after ``ShardedPPO``'s gather.  ``update`` (torch autograd) and ``_update_hip`` (torch optimiser) keep
loops of their own: they are what the other paths are tested against."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _native
from .policy import ActionNoise, MLPPopulation, ObsStats, _NativeObject, check_array, launch, new_array


def _side(t, who, name):
    """Where a free function runs, read off its first array: ``None`` (the host) for a numpy array, its GPU for a
    tensor.  ``check_array`` then holds every array of the call, that one included, to this side."""
    if isinstance(t, np.ndarray):
        return None
    if isinstance(t, torch.Tensor) and t.is_cuda:
        return t.device
    raise _native.PbgError(f"{who}: {name} must be a numpy array or a GPU tensor")


def gae(rew_traj, done_traj, value, gamma: float = 0.99, lam: float = 0.95, adv=None, ret=None, trunc_traj=None,
        term_value=None):
    """``(adv, ret)``, float32 ``[T, n]``: pbg_gae, one launch, a lane per env, float64 arithmetic in the order
    include/pbg.h states.  ``rew_traj`` float32 ``[T, n]``, ``done_traj`` uint8 ``[T, n]``, ``value`` float32
    ``[T + 1, n]`` (row T: the value of the observation after the last step), contiguous tensors on one GPU.
    ``done`` includes the TimeLimit truncation, and without the two arguments below a truncated episode is treated
    as terminal: nothing bootstraps through it.  ``trunc_traj`` (uint8 ``[T, n]``) and ``term_value`` (float32
    ``[T, n]``: the critic's value of the observation the episode was cut at, read only where ``trunc_traj`` is
    set), both or neither: pbg_gae_trunc, which bootstraps ``term_value`` through a truncated step; with
    ``trunc_traj`` all zero it gives pbg_gae's bits.  numpy arrays instead of tensors run the same loop on the host
    (pbg_gae_host, pbg_gae_trunc_host: the same bits)."""
    if not hasattr(_native.lib(), "pbg_gae"):
        raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_gae: a build without advantage estimation")
    if (trunc_traj is None) != (term_value is None):
        raise _native.PbgError("gae: trunc_traj and term_value go together (both or neither)")
    trunc = trunc_traj is not None
    if trunc and not hasattr(_native.lib(), "pbg_gae_trunc"):
        raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_gae_trunc: a build without truncation bootstrapping")
    dev = _side(rew_traj, "gae", "rew_traj")
    if rew_traj.ndim != 2 or min(rew_traj.shape) < 1:
        raise _native.PbgError(f"gae: rew_traj must be [T, n] (T, n >= 1), got shape {tuple(rew_traj.shape)}")
    T, n = (int(d) for d in rew_traj.shape)
    adv = new_array((T, n), np.float32, dev) if adv is None else adv
    ret = new_array((T, n), np.float32, dev) if ret is None else ret
    # the entry points' pointer order: the two truncation arrays follow done_traj and value
    arrays = [("rew_traj", rew_traj, (T, n), np.float32), ("done_traj", done_traj, (T, n), np.uint8),
              ("trunc_traj", trunc_traj, (T, n), np.uint8), ("value", value, (T + 1, n), np.float32),
              ("term_value", term_value, (T, n), np.float32), ("adv", adv, (T, n), np.float32), ("ret", ret, (T, n), np.float32)]
    p = [check_array(t, "gae", name, shape, dt, dev) for name, t, shape, dt in arrays if trunc or name not in
         ("trunc_traj", "term_value")]
    launch(dev, "pbg_gae" + "_trunc" * trunc + "_host" * (dev is None), T, n, *p[:-2], float(gamma), float(lam), *p[-2:])
    return adv, ret


def mlp_forward(theta, dims, x, obs_norm=None):
    """The MLP of the flat parameter vector ``theta`` (include/pbg.h "Flat parameter layout", ``unpack_theta``'s
    slicing as views, so autograd reaches ``theta``) on ``x [B, obs_dim]``; ``obs_norm = (mean, inv_std, clip)``:
    the actor's normaliser expression first."""
    o, h1, h2, a = dims
    if obs_norm is not None:
        mean, inv_std, clip = obs_norm
        x = torch.clamp((x - mean) * inv_std, -clip, clip)
    at = 0
    for k, h, relu in ((o, h1, True), (h1, h2, True), (h2, a, False)):
        w = theta[at:at + k * h].view(k, h)
        b = theta[at + k * h:at + k * h + h]
        at += k * h + h
        x = x @ w + b
        if relu:
            x = torch.relu(x)
    return x


class PPOGrad(_NativeObject):
    """The gradient of the clipped-surrogate loss of one minibatch as two HIP launches (include/pbg.h "PPO
    gradient", pbg_ppo_grad).  ``dims = (obs_dim, h1, h2, act_dim)``: the actor's; the critic is obs_dim -> h1 -> h2
    -> 1.  ``device``: a GPU, or ``None`` / ``"cpu"`` for the host twin (pbg_ppo_grad_host, numpy arrays, no GPU).
    ``max_rows``: the largest minibatch ``run`` will see (it sizes the reduction's workspace).  ``path``: ``"fma"``
    (pbg_ppo_grad_create) or ``"mfma"``, the matrix-core path for wide networks (pbg_ppo_grad_create_ex with
    PBG_PPO_GRAD_MFMA: the same forward bits, another order of the backward's sums); the host twin serves both and
    computes the same thing for either."""
    _DESTROY, _HOST_HANDLE = "pbg_ppo_grad_destroy", False

    PATHS = {"fma": _native.PPO_GRAD_FMA, "mfma": _native.PPO_GRAD_MFMA}

    def __init__(self, dims, max_rows: int, device=None, path: str = "fma"):
        if not hasattr(_native.lib(), "pbg_ppo_grad_create"):
            raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_ppo_grad_create: a build without the PPO gradient")
        if path not in self.PATHS:
            raise _native.PbgError(f"PPOGrad: path must be 'fma' or 'mfma', got {path!r}")
        self.path = path
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 4:
            raise _native.PbgError(f"PPOGrad: dims must be (obs_dim, h1, h2, act_dim), got {dims!r}")
        o, h1, h2, a = self.dims
        self.Da = o * h1 + h1 + h1 * h2 + h2 + h2 * a + a
        self.Dc = o * h1 + h1 + h1 * h2 + h2 + h2 + 1
        self.max_rows = int(max_rows)
        index = self._set_device(device, "a GPU or None", host=True)
        if self.host:
            if self.max_rows < 1 or not (1 <= o <= _native.POLICY_MAX_DIM and 1 <= h1 <= _native.POLICY_MAX_DIM and
                                         1 <= h2 <= _native.POLICY_MAX_DIM and 1 <= a <= _native.POLICY_MAX_ACT):
                raise _native.PbgError(f"PPOGrad: dims {self.dims} or max_rows {max_rows} out of range")
            return
        h = ctypes.c_void_p()
        if path == "fma":
            _native.check(_native.lib().pbg_ppo_grad_create(index, o, h1, h2, a, self.max_rows, ctypes.byref(h)),
                          "pbg_ppo_grad_create")
        else:
            if not hasattr(_native.lib(), "pbg_ppo_grad_create_ex"):
                raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_ppo_grad_create_ex: a build without the matrix-core path")
            opts = _native.PPOGradOpts(path=self.PATHS[path])
            _native.check(_native.lib().pbg_ppo_grad_create_ex(index, o, h1, h2, a, self.max_rows, ctypes.byref(opts),
                                                               ctypes.byref(h)), "pbg_ppo_grad_create_ex")
        self._h = h

    def _outputs(self, grad_actor, grad_critic, grad_log_std, stats):
        """The four output arrays of ``run`` and ``reduce``: new ones where none were given."""
        given = ((grad_actor, self.Da, np.float32), (grad_critic, self.Dc, np.float32), (grad_log_std, self.dims[3], np.float32),
                 (stats, 4, np.float64))
        return tuple(self._new(n, dt) if t is None else t for t, n, dt in given)

    def _io(self, who, theta_actor, theta_critic, log_std, obs, act, logp_old, adv, ret, idx, rows, adv_norm, obs_norm, clip_eps,
            vf_coef, ent_coef, out, logp_out, v_out, value_old=None, vf_clip=None, gate=None):
        """The checked pbg_ppo_grad_io_t of ``run``, ``run_part`` and ``reduce``.  ``out``: the four output arrays
        (``_outputs``), or four ``None`` for ``run_part``, which writes no gradient.  The struct's first version while
        neither ``value_old`` nor ``gate`` is given."""
        o, h1, h2, A = self.dims
        f32, f64 = np.float32, np.float64
        if getattr(obs, "ndim", 0) != 2:
            raise _native.PbgError(f"PPOGrad.{who}: obs must be [B, obs_dim]")
        B = int(obs.shape[0])
        Bm = int(idx.shape[0]) if idx is not None and getattr(idx, "ndim", 0) == 1 else (B if rows is None else int(rows))
        mean, inv_std, clip = obs_norm if obs_norm is not None else (None, None, 0.0)
        # (the struct's field, the array, its shape and dtype, whether it may be None: a null pointer then)
        arrays = (("theta_actor", theta_actor, (self.Da,), f32, False), ("theta_critic", theta_critic, (self.Dc,), f32, False),
                  ("log_std", log_std, (A,), f32, False), ("obs", obs, (B, o), f32, False), ("act", act, (B, A), f32, False),
                  ("logp_old", logp_old, (B,), f32, False), ("adv", adv, (B,), f32, False), ("ret", ret, (B,), f32, False),
                  ("grad_actor", out[0], (self.Da,), f32, True), ("grad_critic", out[1], (self.Dc,), f32, True),
                  ("grad_log_std", out[2], (A,), f32, True), ("stats", out[3], (4,), f64, True),
                  ("idx", idx, (Bm,), np.int64, True), ("adv_norm", adv_norm, (2,), f32, True), ("mean", mean, (o,), f32, True),
                  ("inv_std", inv_std, (o,), f32, True), ("logp_out", logp_out, (Bm,), f32, True), ("v_out", v_out, (Bm,), f32, True))
        if value_old is not None or gate is not None:
            arrays += (("value_old", value_old, (B,), f32, True), ("gate", gate, (2,), np.int32, True))
        at, dev = (self, who), self.device   # _ptr's check, without a call in between: eighteen pointers per minibatch
        p = {name: None if t is None and optional else check_array(t, at, name, shape, dt, dev)
             for name, t, shape, dt, optional in arrays}
        if Bm < 1 or Bm > self.max_rows or (idx is None and Bm > B):
            raise _native.PbgError(f"PPOGrad.{who}: {Bm} minibatch rows outside 1 .. max_rows = {self.max_rows} (or the batch's {B})")
        if (mean is None) != (inv_std is None):
            raise _native.PbgError(f"PPOGrad.{who}: obs_norm needs both mean and inv_std")
        if (value_old is None) != (vf_clip is None):
            raise _native.PbgError(f"PPOGrad.{who}: value_old and vf_clip go together (both or neither)")
        IO, more = _native.PPOGradIO, {}
        if value_old is not None or gate is not None:
            if not hasattr(_native.lib(), "pbg_ppo_gate"):
                raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_ppo_gate: a build without value clipping and the KL gate")
            IO, more = _native.PPOGradIO2, dict(vf_clip=0.0 if vf_clip is None else float(vf_clip))
        return IO(batch_rows=B, mb_rows=Bm, clip=float(clip), clip_eps=float(clip_eps), vf_coef=float(vf_coef),
                  ent_coef=float(ent_coef), **p, **more)

    def run(self, theta_actor, theta_critic, log_std, obs, act, logp_old, adv, ret, idx=None, rows=None, adv_norm=None,
            obs_norm=None, clip_eps: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0, grad_actor=None,
            grad_critic=None, grad_log_std=None, stats=None, logp_out=None, v_out=None, value_old=None, vf_clip=None, gate=None):
        """``(grad_actor [Da], grad_critic [Dc], grad_log_std [A], stats float64 [4])`` of the minibatch ``idx`` (int64
        ``[Bm]`` rows of the batch; ``None``: the first ``rows`` rows, default all) of the batch ``obs [B, obs_dim]``,
        ``act [B, A]``, ``logp_old``, ``adv``, ``ret`` ``[B]``: contiguous float32 tensors on the object's GPU (numpy
        arrays on the host).  ``adv_norm``: float32 ``[2]`` (shift, scale) or ``None``; ``obs_norm``: ``(mean, inv_std,
        clip)`` or ``None``.  The outputs are written into the given tensors, or into new ones.  ``stats``: pg loss, vf
        loss, clipped fraction, mean(logp_old - logp).  ``logp_out``, ``v_out``: optional float32 ``[Bm]``.  The indices
        are not validated on a GPU.  ``value_old`` (float32 ``[B]``, the values the batch was collected under) with
        ``vf_clip > 0``: PPO2's clipped value loss (include/pbg.h "Value clipping").  ``gate``: an int32 ``[2]`` array
        (``KLGate.gate``); while its first word is not 0 both launches return at entry and every output keeps what it
        held."""
        out = self._outputs(grad_actor, grad_critic, grad_log_std, stats)
        io = self._io("run", theta_actor, theta_critic, log_std, obs, act, logp_old, adv, ret, idx, rows, adv_norm, obs_norm,
                      clip_eps, vf_coef, ent_coef, out, logp_out, v_out, value_old, vf_clip, gate)
        if self.host:
            self._launch("pbg_ppo_grad_host", *self.dims, ctypes.byref(io))
        else:
            self._launch("pbg_ppo_grad_run", self._open("run"), ctypes.byref(io))
        return out

    def _parts(self, who):
        if not hasattr(_native.lib(), "pbg_ppo_grad_run_part"):
            raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_ppo_grad_run_part: a build without the gradient as parts")
        if self.host:
            raise _native.PbgError(f"PPOGrad.{who}: needs an open object on a GPU")
        return self._open(who)

    def geometry(self, mb_rows: int):
        """``(G, Dtot)``: the workgroups ``run`` launches for a minibatch of ``mb_rows`` rows and the floats of one
        workgroup's partial (pbg_ppo_grad_geometry, no GPU work)."""
        h = self._parts("geometry")
        G, dtot = ctypes.c_int(), ctypes.c_int64()
        _native.check(_native.lib().pbg_ppo_grad_geometry(h, int(mb_rows), ctypes.byref(G), ctypes.byref(dtot)),
                      "pbg_ppo_grad_geometry")
        return G.value, dtot.value

    def run_part(self, theta_actor, theta_critic, log_std, obs, act, logp_old, adv, ret, wg_first, wg_count, part_out,
                 part_stats_out, idx=None, rows=None, adv_norm=None, obs_norm=None, clip_eps: float = 0.2, vf_coef: float = 0.5,
                 ent_coef: float = 0.0, logp_out=None, v_out=None, value_old=None, vf_clip=None, gate=None):
        """``run``'s tile launch for the workgroups ``wg_first .. wg_first + wg_count - 1`` of the minibatch's ``G``
        (``geometry``): their partials into ``part_out`` (float32 ``[wg_count, Dtot]``) and ``part_stats_out`` (float64
        ``[wg_count, 4]``), contiguous tensors (or row ranges of ones) on the object's GPU.  No gradient is written;
        ``logp_out`` / ``v_out`` get the rows of these workgroups' tiles.  ``wg_count = 0`` launches nothing.  The other
        arguments and their checks are ``run``'s."""
        h = self._parts("run_part")
        io = self._io("run_part", theta_actor, theta_critic, log_std, obs, act, logp_old, adv, ret, idx, rows, adv_norm, obs_norm,
                      clip_eps, vf_coef, ent_coef, (None,) * 4, logp_out, v_out, value_old, vf_clip, gate)
        wg_first, wg_count = int(wg_first), int(wg_count)
        G, dtot = self.geometry(io.mb_rows)
        if wg_first < 0 or wg_count < 0 or wg_first + wg_count > G:
            raise _native.PbgError(f"PPOGrad.run_part: workgroups {wg_first} .. {wg_first} + {wg_count} outside 0 .. {G}")
        self._launch("pbg_ppo_grad_run_part", h, ctypes.byref(io), wg_first, wg_count,
                     self._ptr(part_out, "run_part", "part_out", (wg_count, dtot)),
                     self._ptr(part_stats_out, "run_part", "part_stats_out", (wg_count, 4), np.float64))

    def reduce(self, theta_actor, theta_critic, log_std, obs, act, logp_old, adv, ret, G, part, part_stats, idx=None, rows=None,
               adv_norm=None, obs_norm=None, clip_eps: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0, grad_actor=None,
               grad_critic=None, grad_log_std=None, stats=None, logp_out=None, v_out=None, value_old=None, vf_clip=None,
               gate=None):
        """``run``'s reduction over the ``G`` partials of ``part`` (float32 ``[G, Dtot]``) and ``part_stats`` (float64
        ``[G, 4]``): ``(grad_actor, grad_critic, grad_log_std, stats)`` as ``run`` returns them.  ``G`` must be
        ``geometry``'s for the minibatch; the other arguments and their checks are ``run``'s (of them the launch reads
        the minibatch's size and ``ent_coef``)."""
        h = self._parts("reduce")
        out = self._outputs(grad_actor, grad_critic, grad_log_std, stats)
        io = self._io("reduce", theta_actor, theta_critic, log_std, obs, act, logp_old, adv, ret, idx, rows, adv_norm, obs_norm,
                      clip_eps, vf_coef, ent_coef, out, logp_out, v_out, value_old, vf_clip, gate)
        G = int(G)
        Gq, dtot = self.geometry(io.mb_rows)
        if G != Gq:
            raise _native.PbgError(f"PPOGrad.reduce: G = {G} is not the {Gq} workgroups of {io.mb_rows} minibatch rows")
        self._launch("pbg_ppo_grad_reduce", h, ctypes.byref(io), G, self._ptr(part, "reduce", "part", (G, dtot)),
                     self._ptr(part_stats, "reduce", "part_stats", (G, 4), np.float64))
        return out


def _need_opt():
    if not hasattr(_native.lib(), "pbg_ppo_opt_create"):
        raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_ppo_opt_create: a build without the PPO optimiser step")
    return _native.lib()


def adv_norm(adv, idx=None, out=None):
    """``out``, float32 ``[2]``: the ``(shift, scale) = (mean, 1 / (std + 1e-8))`` pair of the advantages ``adv[idx]``
    (``adv`` float32 ``[B]``; ``idx`` int64 ``[Bm]``, ``None``: all of ``adv``; Bessel's correction, ``Tensor.std()``)
    that ``PPOGrad.run`` takes as ``adv_norm``: pbg_adv_norm, one launch, float64 sums in the order include/pbg.h
    states.  Contiguous tensors on one GPU run the launch (the indices are not validated there); numpy arrays run
    the same sums on the host (pbg_adv_norm_host, the same bits, the indices validated)."""
    _need_opt()
    dev = _side(adv, "adv_norm", "adv")
    if adv.ndim != 1:
        raise _native.PbgError("adv_norm: adv must be a float32 [B] array or GPU tensor")
    B = int(adv.shape[0])
    Bm = int(idx.shape[0]) if idx is not None and getattr(idx, "ndim", 0) == 1 else B
    out = new_array(2, np.float32, dev) if out is None else out
    launch(dev, "pbg_adv_norm" + "_host" * (dev is None), B, Bm, check_array(adv, "adv_norm", "adv", (B,), np.float32, dev),
           None if idx is None else check_array(idx, "adv_norm", "idx", (Bm,), np.int64, dev),
           check_array(out, "adv_norm", "out", (2,), np.float32, dev))
    return out


class AdamClip(_NativeObject):
    """Adam with global-norm gradient clipping over up to 8 flat float32 blocks as two HIP launches (include/pbg.h
    "PPO optimiser step", pbg_ppo_opt).  ``sizes``: the blocks' element counts.  ``device``: a GPU, whose object then
    owns the moments, the step count and the running powers of the betas on the device (so a captured step that is
    replayed advances like an eager one), or ``None`` / ``"cpu"`` for the host twin (pbg_ppo_opt_host: numpy arrays,
    no GPU, the state kept here as numpy arrays; the same bits)."""
    _DESTROY, _HOST_HANDLE = "pbg_ppo_opt_destroy", False

    def __init__(self, sizes, device=None):
        L = _need_opt()
        self.sizes = tuple(int(s) for s in sizes)
        if not 1 <= len(self.sizes) <= _native.PPO_OPT_MAX_BLOCKS or min(self.sizes) < 1:
            raise _native.PbgError(f"AdamClip: 1 .. {_native.PPO_OPT_MAX_BLOCKS} blocks of at least one element, got {sizes!r}")
        self._sizes = (ctypes.c_int64 * len(self.sizes))(*self.sizes)
        index = self._set_device(device, "a GPU or None", host=True)
        if self.host:
            self.reset()
            return
        h = ctypes.c_void_p()
        _native.check(L.pbg_ppo_opt_create(index, len(self.sizes), self._sizes, ctypes.byref(h)), "pbg_ppo_opt_create")
        self._h = h

    def step(self, params, grads, lr, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float = 0.0, info=None, gate=None):
        """One step on ``params`` (updated in place) with ``grads``: sequences of contiguous float32 ``[sizes[b]]``
        tensors on the object's GPU (numpy arrays on the host).  ``max_grad_norm`` 0 (or None): no clipping.  ``info``:
        optional float64 ``[2]`` that receives the gradient's global norm and the clipping coefficient.  ``lr``: a
        float, a launch argument like the other scalars (a captured step keeps the value it was captured with), or a
        float64 ``[1]`` tensor on the object's GPU (a numpy ``[1]`` array on the host) that the step reads where it
        lies: the bits of the same value passed as a float, and a captured step follows the tensor.  ``gate``: an int32
        ``[2]`` array (``KLGate.gate``); while its first word is not 0 the step changes nothing: no parameter, no moment,
        not the step count and not ``info``."""
        h = self._open("step")
        params, grads = list(params), list(grads)
        lr_t = lr if isinstance(lr, (np.ndarray, torch.Tensor)) else None
        if len(params) != len(self.sizes) or len(grads) != len(self.sizes):
            raise _native.PbgError(f"AdamClip.step: {len(self.sizes)} blocks expected, got {len(params)} params and "
                                   f"{len(grads)} grads")
        kw = dict(param=[self._ptr(t, "step", f"params[{b}]", (s,)) for b, (t, s) in enumerate(zip(params, self.sizes))],
                  grad=[self._ptr(t, "step", f"grads[{b}]", (s,)) for b, (t, s) in enumerate(zip(grads, self.sizes))],
                  lr=0.0 if lr_t is not None else float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps),
                  max_grad_norm=float(max_grad_norm or 0.0),
                  info=None if info is None else self._ptr(info, "step", "info", (2,), np.float64))
        # the struct's first version while no lr tensor is given: a library from before lr_ptr keeps working
        IO = _native.PPOOptIO
        if lr_t is not None:
            _need_perm()
            IO, kw["lr_ptr"] = _native.PPOOptIO2, self._ptr(lr_t, "step", "lr", (1,), np.float64)
        if gate is not None:
            _need_gate()
            IO, kw["gate"] = _native.PPOOptIO3, self._ptr(gate, "step", "gate", (2,), np.int32)
        if self.host:
            io = IO(m=[t.ctypes.data for t in self._m], v=[t.ctypes.data for t in self._v], t=self._t.ctypes.data,
                    bpow=self._bpow.ctypes.data, **kw)
            self._launch("pbg_ppo_opt_host", len(self.sizes), self._sizes, ctypes.byref(io))
            return
        io = IO(**kw)
        self._launch("pbg_ppo_opt_step", h, ctypes.byref(io))

    def reset(self):
        """Zero moments, step count 0 (stream order on a GPU)."""
        if self.host:
            self._m = [np.zeros(s, np.float32) for s in self.sizes]
            self._v = [np.zeros(s, np.float32) for s in self.sizes]
            self._t, self._bpow = np.zeros(1, np.uint32), np.ones(2, np.float64)
            return
        self._launch("pbg_ppo_opt_reset", self._open("reset"))

    def state(self):
        """``(m, v, t)``: the two moments as lists of float32 ``[sizes[b]]`` and the step count (``[1]``: int32 bits of
        the uint32 on a GPU, uint32 on the host): fresh device tensors, copied on the stream (copies of the numpy state on
        the host)."""
        if self.host:
            return [a.copy() for a in self._m], [a.copy() for a in self._v], self._t.copy()
        h, n = self._open("state"), sum(self.sizes)
        m, v = self._new(n), self._new(n)
        t = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._launch("pbg_ppo_opt_get_state", h, m.data_ptr(), v.data_ptr(), t.data_ptr())
        return list(m.split(self.sizes)), list(v.split(self.sizes)), t


def _need_perm():
    if not hasattr(_native.lib(), "pbg_perm_create"):
        raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_perm_create: a build without counter-based permutations")
    return _native.lib()


class Permutation(_NativeObject):
    """Counter-based permutations of ``0 .. B - 1`` (include/pbg.h "Counter-based permutations", pbg_perm): an
    eight-round Feistel network keyed by Philox words of ``(seed, counter)``, cycle-walked into range; ``rng.permutation``
    is the numpy mirror with the same bits.  ``device``: a GPU, whose object owns the counter on the device (so a
    captured fill that is replayed draws the next permutations like an eager one), or ``None`` / ``"cpu"`` for the host
    twin (pbg_perm_host on numpy arrays, the counter kept here)."""
    _DESTROY, _HOST_HANDLE = "pbg_perm_destroy", False

    def __init__(self, seed: int, device=None):
        L = _need_perm()
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._counter = 0
        index = self._set_device(device, "a GPU or None", host=True)
        if self.host:
            return
        h = ctypes.c_void_p()
        _native.check(L.pbg_perm_create(index, self.seed, ctypes.byref(h)), "pbg_perm_create")
        self._h = h

    def fill(self, B: int, n_perms: int = 1, out=None):
        """``out``, int64 ``[n_perms, B]``: row j is the permutation at ``counter + j``; the counter then advances by
        ``n_perms`` (uint32, it wraps).  On a GPU: two launches on the current stream, no host work."""
        h = self._open("fill")
        B, n_perms = int(B), int(n_perms)
        if B < 1 or not 1 <= n_perms <= 65535:
            raise _native.PbgError(f"Permutation.fill: B = {B} must be >= 1 and n_perms = {n_perms} in 1 .. 65535")
        out = self._new((n_perms, B), np.int64) if out is None else out
        p = self._ptr(out, "fill", "out", (n_perms, B), np.int64)
        if self.host:
            self._launch("pbg_perm_host", self.seed, self._counter, B, n_perms, p)
            self._counter = (self._counter + n_perms) & 0xFFFFFFFF
        else:
            self._launch("pbg_perm_fill", h, B, n_perms, p)
        return out

    @property
    def counter(self) -> int:
        """Permutations drawn so far, modulo 2^32 (on a GPU it synchronises to read it); assignable."""
        if self.host:
            return self._counter
        h = self._open("counter")
        out = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._launch("pbg_perm_get_counter", h, out.data_ptr())
        return int(out.item()) & 0xFFFFFFFF

    @counter.setter
    def counter(self, value):
        if self.host:
            self._counter = int(value) & 0xFFFFFFFF
            return
        self._launch("pbg_perm_set_counter", self._open("counter"), int(value) & 0xFFFFFFFF)


def lr_linear(it, n_total: int, lr0: float, out=None):
    """``out``, float64 ``[1]`` = ``lr0 * (1 - min(it, n_total) / n_total)``: pbg_ppo_lr_linear, one launch of one lane,
    float64 in that order (``rng.lr_linear`` gives the same bits).  ``it``: an int32 ``[1]`` tensor on a GPU (read as
    uint32), or a numpy uint32 ``[1]`` array for the host twin (pbg_ppo_lr_linear_host)."""
    _need_perm()
    n_total = int(n_total)
    if not 1 <= n_total <= 0xFFFFFFFF:
        raise _native.PbgError(f"lr_linear: n_total = {n_total} outside 1 .. 2^32 - 1")
    dev = _side(it, "lr_linear", "it")
    out = new_array(1, np.float64, dev) if out is None else out
    launch(dev, "pbg_ppo_lr_linear" + "_host" * (dev is None),
           check_array(it, "lr_linear", "it", (1,), np.uint32 if dev is None else np.int32, dev), n_total, float(lr0),
           check_array(out, "lr_linear", "out", (1,), np.float64, dev))
    return out


def _need_gate():
    if not hasattr(_native.lib(), "pbg_ppo_gate"):
        raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_ppo_gate: a build without value clipping and the KL gate")
    return _native.lib()


class KLGate(_NativeObject):
    """The device-side early stop of a PPO update (include/pbg.h "Value clipping and the KL gate"): an int32 ``[2]``
    array ``gate`` = (stopped, minibatch steps applied since the last ``reset``), on a GPU or, with ``device`` ``None`` /
    ``"cpu"``, a numpy array for the host twin.  ``check(stats, kl_limit)`` is one launch of one lane (pbg_ppo_gate): while
    not stopped, ``stats[3] > kl_limit`` stops, anything else (a NaN included) counts one more step.  ``PPOGrad.run`` /
    ``run_part`` / ``reduce`` and ``AdamClip.step`` take ``gate`` and do nothing while it is stopped.  Only ``check`` and
    ``reset`` write the two words, in launches of their own, so a chain of them captures as a plain chain."""
    _HOST_HANDLE = False   # no native object on either side: the array is the state

    def __init__(self, device=None):
        _need_gate()
        self._set_device(device, "a GPU or None", host=True)
        self.gate = np.zeros(2, np.int32) if self.host else torch.zeros(2, dtype=torch.int32, device=self.device)

    def reset(self):
        """Both words to 0 (stream order on a GPU)."""
        if self.host:
            self.gate[:] = 0
        else:
            self._launch("pbg_ppo_gate_reset", self.gate.data_ptr())

    def check(self, stats, kl_limit: float):
        """``stats``: ``PPOGrad.run``'s float64 ``[4]``, read where it lies."""
        self._launch("pbg_ppo_gate" + "_host" * self.host, self._ptr(stats, "check", "stats", (4,), np.float64), float(kl_limit),
                     self._ptr(self.gate, "check", "gate", (2,), np.int32))

    @property
    def state(self):
        """A copy of ``gate`` (a device tensor on a GPU, made on the stream: nothing is read back)."""
        return self.gate.copy() if self.host else self.gate.clone()


class RetStats(_NativeObject):
    """Reward scaling by a running standard deviation of the discounted return (include/pbg.h "Return statistics",
    pbg_ret_stats), what VecNormalize does to rewards.  ``n_envs`` envs each keep a running return
    ``R <- gamma R + r``, reset where ``done`` is set and carried from one ``update`` to the next; ``finalize`` folds the
    walk's per-tile partials (one slot per 32 consecutive envs) into the running totals and sets ``scale = 1 /
    sqrt(max(var, var_floor))``; ``apply`` multiplies rewards by it and clips.  ``device``: a GPU, whose object owns all
    of that on the device (three launches, no atomics, nothing read back: a captured round that is replayed advances
    like an eager one), or ``None`` / ``"cpu"`` for the host twin (the same entry points on numpy arrays, no GPU, the
    same bits).  ``n_slots``: default ``ceil(n_envs / 32)``; more when the object also finalizes other shards' slots."""
    _DESTROY = "pbg_ret_stats_destroy"   # the host twin is a native object too

    TILE = 32

    def __init__(self, n_envs: int, gamma: float, device=None, n_slots=None):
        if not hasattr(_native.lib(), "pbg_ret_stats_create"):
            raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_ret_stats_create: a build without return statistics")
        self.n_envs, self.gamma = int(n_envs), float(gamma)
        self.n_slots = -(-self.n_envs // self.TILE) if n_slots is None else int(n_slots)
        index = self._set_device(device, "a GPU or None", host=True)
        h = ctypes.c_void_p()
        _native.check(_native.lib().pbg_ret_stats_create(index, self.n_envs, self.n_slots, self.gamma, ctypes.byref(h)),
                      "pbg_ret_stats_create")
        self._h = h

    def _call(self, name, *args):
        """``pbg_ret_stats_<name>(handle, *args, stream)`` on the current stream of the object's GPU; the host twin
        goes through the same entry points with no stream."""
        self._launch("pbg_ret_stats_" + name, self._open(name), *args, *((None,) if self.host else ()))

    def update(self, rew_traj, done_traj, slot_offset: int = 0):
        """Walk ``rew_traj`` (float32 ``[T, n]``) and ``done_traj`` (uint8 ``[T, n]``), ``n <= n_envs``: every env's
        return advances ``T`` steps from its carry, and the tiles' partials overwrite the slots ``slot_offset ..``."""
        if getattr(rew_traj, "ndim", 0) != 2:
            raise _native.PbgError("RetStats.update: rew_traj must be [T, n]")
        T, n = (int(d) for d in rew_traj.shape)
        self._call("walk", T, n, int(slot_offset), self._ptr(rew_traj, "update", "rew_traj", (T, n), np.float32),
                   self._ptr(done_traj, "update", "done_traj", (T, n), np.uint8))

    def finalize(self, n_used_slots=None, var_floor: float = 1e-2):
        """Add the slots ``0 .. n_used_slots - 1`` (default: all) in ascending order, then that sum onto the totals, and
        set the scale from them (left as it is while the totals are empty)."""
        self._call("finalize", self.n_slots if n_used_slots is None else int(n_used_slots), float(var_floor))

    def apply(self, rew, out=None, clip: float = 10.0):
        """``out = clamp(rew * scale, -clip, clip)`` (float32, any shape, contiguous; a NaN passes); ``out`` may not
        overlap ``rew``."""
        shape = tuple(getattr(rew, "shape", ()))
        count = int(np.prod(shape)) if shape else 0
        if out is None:
            out = self._new(shape, np.float32)
        self._call("apply", count, float(clip), self._ptr(rew, "apply", "rew", shape, np.float32),
                   self._ptr(out, "apply", "out", shape, np.float32))
        return out

    def _slot_range(self, what, first, count):
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > self.n_slots:
            raise _native.PbgError(f"RetStats.{what}: slots {first} .. {first} + {count} are outside the object's 0 .. "
                                   f"{self.n_slots}")
        return first, count

    def get_slots(self, first: int = 0, count=None):
        """``(counts int64 [count], sums float64 [count, 2])`` of the slots ``first .. first + count - 1`` (default: to
        the last), per slot ``s1, s2``: fresh arrays; the slots stay as they are."""
        first, count = self._slot_range("get_slots", first, self.n_slots - int(first) if count is None else count)
        counts, sums = self._new(count, np.int64), self._new((count, 2), np.float64)
        self._call("get_slots", first, count, self._ptr(counts, "get_slots", "counts", (count,), np.int64),
                   self._ptr(sums, "get_slots", "sums", (count, 2), np.float64))
        return counts, sums

    def set_slots(self, first: int, counts, sums):
        """Overwrite the slots ``first .. first + len(counts) - 1`` (``get_slots``' layout).  Slots gathered from equal
        shards of a multiple of 32 envs in shard order and finalized here give the unsharded object's bits."""
        first, count = self._slot_range("set_slots", first, counts.shape[0] if getattr(counts, "ndim", 0) == 1 else -1)
        self._call("set_slots", first, count, self._ptr(counts, "set_slots", "counts", (count,), np.int64),
                   self._ptr(sums, "set_slots", "sums", (count, 2), np.float64))
        self._src = (counts, sums)   # alive until the stream has copied them

    def _get(self, name, *shapes_dts):
        outs = [self._new(s, d) for s, d in shapes_dts]
        self._call("get_" + name, *(self._ptr(o, name, name, s, d) for o, (s, d) in zip(outs, shapes_dts)))
        return outs

    @property
    def totals(self):
        """``(count int64 [1], sums float64 [2])`` over every finalized batch: fresh arrays (device tensors on a GPU)."""
        return tuple(self._get("totals", ((1,), np.int64), ((2,), np.float64)))

    @property
    def carry(self):
        """float64 ``[n_envs]``: every env's running return (a fresh array)."""
        return self._get("carry", ((self.n_envs,), np.float64))[0]

    @property
    def scale(self):
        """float32 ``[1]``: what ``apply`` multiplies by (a fresh array; a device tensor on a GPU, nothing is read back)."""
        return self._get("scale", ((1,), np.float32))[0]

    def reset(self):
        """Carry, slots and totals to zero, the scale to 1."""
        self._call("reset")

    def state(self) -> dict:
        """Everything a checkpoint needs, as fresh arrays: ``count``, ``sums``, ``carry``, ``scale`` (the slots are one
        walk's scratch)."""
        count, sums = self.totals
        return dict(count=count, sums=sums, carry=self.carry, scale=self.scale)

    def load_state(self, state: dict):
        """``state()``'s dict back into the object (arrays on its side, of ``state()``'s shapes and dtypes)."""
        shapes = dict(count=((1,), np.int64), sums=((2,), np.float64), carry=((self.n_envs,), np.float64),
                      scale=((1,), np.float32))
        p = {k: self._ptr(state[k], "load_state", k, *shapes[k]) for k in shapes}
        self._call("set_totals", p["count"], p["sums"])
        self._call("set_carry", p["carry"])
        self._call("set_scale", p["scale"])
        self._src = dict(state)   # alive until the stream has copied them


@dataclass
class Batch:
    """One iteration's data (views of the env's rollout buffers and this object's own): ``[T, n, ...]``."""
    obs: torch.Tensor
    act: torch.Tensor
    rew: torch.Tensor
    done: torch.Tensor
    eps2: torch.Tensor      # float64
    logp: torch.Tensor      # float64, under the policy that acted
    value: torch.Tensor     # [T + 1, n]
    adv: torch.Tensor
    ret: torch.Tensor
    # truncation="bootstrap" sets these two on the batch; in terminal mode they are the class's None and no field, so
    # that ``vars(batch)`` stays the nine tensors it was
    trunc = None        # uint8 [T, n]: truncated and not terminated
    term_value = None   # float32 [T, n]: the critic on the terminal observations, +0.0 where trunc is 0
    # reward_norm=True sets this one the same way; ``rew`` stays the raw rewards
    rew_scaled = None   # float32 [T, n]: the rewards ``adv`` and ``ret`` were computed from


class PPO:
    """``env``: a ``VecEnv`` (auto-reset on, an even ``num_envs``).  The actor (obs -> h1 -> h2 -> act) and the
    critic (obs -> h1 -> h2 -> 1) are two ``MLPPopulation``s of one pair each, given their weights by
    ``set_all(theta)`` on the stream; ``actor_theta``, ``critic_theta`` (flat float32, section 11's layout) and
    ``log_std`` are the torch parameters Adam moves.  ``iterate()`` is one iteration: rollout of ``steps`` env
    steps with Gaussian action noise, values, GAE, then ``epochs`` x ``minibatches`` clipped-surrogate updates.
    ``obs_norm=True``: running observation normalisation on section 12's schedule: statistics are attached
    during the rollout and finalized into both networks' normaliser after the update, which uses the normaliser
    its data was collected under.  ``backward="hip"``: every minibatch's gradient comes from ``PPOGrad.run`` (two
    launches, written straight into the parameters' ``.grad``) instead of torch autograd; the permutation, the
    gradient clipping and Adam are the same, and ``update``'s stats gain ``clipfrac`` and ``kl``.
    ``optimizer="hip"`` (needs ``backward="hip"``): the advantage normaliser, the gradient clipping and Adam are the
    library's too (``adv_norm``, ``AdamClip``: the torch path's lr, betas (0.9, 0.999), eps 1e-5 and ``max_grad_norm``), a
    minibatch is at most five launches and no torch kernel, and the stats gain ``grad_norm``; the permutation stays
    ``torch.randperm``.  ``graph=True`` (needs ``optimizer="hip"``): the whole ``epochs x minibatches`` chain is one
    captured graph, replayed every iteration; ``lr`` is a launch argument, so the graph keeps the captured value unless a
    schedule is set (below).

    ``permutation="device"`` (needs ``optimizer="hip"``): the minibatch permutations come from a ``Permutation(seed)``
    (pbg_perm_fill, one fill of ``epochs`` rows per update) instead of ``torch.randperm``: iteration i, epoch e uses
    ``rng.permutation(B, seed, i * epochs + e)``, which numpy restates and no torch version changes; with ``graph=True``
    the fill is part of the captured update.  ``lr_schedule="linear", schedule_iterations=N`` (needs ``optimizer="hip"``):
    the trainer keeps its iteration count in a device int32 ``[1]`` (``_it_dev``, advanced on the stream at the end of
    ``iterate``), every update starts with pbg_ppo_lr_linear into a device float64 ``[1]`` (``_lr_dev``: ``lr * (1 -
    min(i, N) / N)``, ``rng.lr_linear``) and ``AdamClip.step`` reads that tensor, so the schedule advances under a
    replayed graph too.  ``graph="iteration"`` (needs ``optimizer="hip"`` and ``permutation="device"``): the first
    ``iterate()`` runs eagerly as iteration 0 (so every kernel has been launched once) and then captures the whole
    iteration -- ``set_all``, the std, the rollout with its statistics, the critic, ``gae``, ``logp_old``, the schedule
    launch, the permutation fill, the ``epochs x minibatches`` steps, the normaliser's ``finalize`` / ``set_obs_norm`` and
    the iteration count's increment -- as one graph; every later ``iterate()`` is one replay and returns device tensors
    without synchronising.  The actor kernel takes the statistics and the noise as launch arguments, so the graph bakes
    them: what is attached on the host at replay time does not matter, and ``evaluate()`` between two replays (which
    detaches the noise on the host and never attaches the statistics) changes nothing the replay does.  The pointers the
    graph baked are compared before each replay; a moved one raises ``PbgError``.

    ``grad_path="mfma"`` (needs ``backward="hip"``): the gradient object is ``PPOGrad(path="mfma")``, the matrix-core
    path for networks wider than 64; it works with every optimizer, graph and permutation setting above.

    ``truncation="terminal"`` (the default): ``done`` includes the TimeLimit truncation and ``gae`` treats it as a
    death.  ``truncation="bootstrap"``: the rollout also records ``trunc_traj`` and
    ``term_obs_traj``, one more launch (``critic.act_where``) values the terminal observations of the truncated rows
    under the normaliser the batch was collected under, and ``gae`` bootstraps them through the truncation; the
    observation statistics do not see the terminal observations.  It works with every setting above, a captured
    iteration included.

    ``reward_norm=True``: the rewards ``gae`` sees are the rollout's divided by a running
    standard deviation of the discounted return and clipped to ``+-reward_clip``: ``collect`` runs ``RetStats.update ->
    finalize -> apply`` (three launches) on the rollout's ``rew_traj`` / ``done_traj`` into a buffer of its own, so the
    batch of iteration i is scaled by the statistics of iterations 0 .. i.  ``Batch.rew`` and ``evaluate()`` stay in the
    robot's units, ``Batch.rew_scaled`` is what the advantages were computed from, and the value loss is then in scaled
    units.  ``iterate()``'s stats gain ``rew_scale`` (a device tensor).  It works with every setting above, a captured
    iteration included.

    ``vf_clip=e``: PPO2's clipped value loss, ``1/2 mean(max((v - ret)^2, (vc - ret)^2))`` with
    ``vc`` the value clamped to within ``e`` of the value the batch was collected under (``Batch.value``).  It works with
    every ``backward``: the torch path adds the same expression, the HIP paths pass the trainer's own value buffer to
    ``PPOGrad.run``.  ``target_kl=k`` (needs ``optimizer="hip"``): every update starts by resetting a ``KLGate``, every
    minibatch's gradient is followed by the gate's launch with ``kl_limit = 1.5 k`` on ``mean(logp_old - logp)``, and once
    it trips the rest of the update's launches return at entry: the tripping step is not applied.  Nothing is read back,
    so it works eager, under ``graph=True`` and inside a captured iteration.  The stats gain ``updates`` (minibatch steps
    applied) and ``kl_stop`` (0 or 1), device tensors; after a stop ``pg``, ``vf``, ``clipfrac`` and ``kl`` are the tripping
    minibatch's."""

    def __init__(self, env, hidden=(64, 64), steps: int = 64, seed: int = 0, gamma: float = 0.99, lam: float = 0.95,
                 clip: float = 0.2, lr: float = 3e-4, epochs: int = 4, minibatches: int = 4, vf_coef: float = 0.5,
                 ent_coef: float = 0.0, log_std: float = -0.5, max_grad_norm: float = 0.5, norm_adv: bool = True,
                 obs_norm: bool = False, obs_clip: float = 5.0, backward: str = "torch", optimizer: str = "torch",
                 graph=False, permutation: str = "torch", lr_schedule=None, schedule_iterations=None,
                 grad_path: str = "fma", truncation: str = "terminal", reward_norm: bool = False,
                 reward_clip: float = 10.0, vf_clip=None, target_kl=None):
        n, dev = env.num_envs, env.device
        nb = self._batch_envs(env)   # the envs whose rows make one update's batch: the env's own
        if truncation not in ("terminal", "bootstrap"):
            raise _native.PbgError(f"PPO: truncation must be 'terminal' or 'bootstrap', got {truncation!r}")
        self.truncation = truncation
        if backward not in ("torch", "hip"):
            raise _native.PbgError(f"PPO: backward must be 'torch' or 'hip', got {backward!r}")
        if optimizer not in ("torch", "hip"):
            raise _native.PbgError(f"PPO: optimizer must be 'torch' or 'hip', got {optimizer!r}")
        if optimizer == "hip" and backward != "hip":
            raise _native.PbgError("PPO: optimizer='hip' takes its gradient from pbg_ppo_grad: it needs backward='hip'")
        if graph and optimizer != "hip":
            raise _native.PbgError("PPO: graph=True captures the library's launches alone: it needs optimizer='hip'")
        if not isinstance(graph, bool) and graph != "iteration":
            raise _native.PbgError(f"PPO: graph must be False, True or 'iteration', got {graph!r}")
        if permutation not in ("torch", "device"):
            raise _native.PbgError(f"PPO: permutation must be 'torch' or 'device', got {permutation!r}")
        if permutation == "device" and optimizer != "hip":
            raise _native.PbgError("PPO: permutation='device' fills the index buffer of the library's update: it needs "
                                   "optimizer='hip'")
        if graph == "iteration" and permutation != "device":
            raise _native.PbgError("PPO: graph='iteration' captures the permutation's draw: it needs permutation='device'")
        if lr_schedule not in (None, "linear"):
            raise _native.PbgError(f"PPO: lr_schedule must be None or 'linear', got {lr_schedule!r}")
        if lr_schedule is not None and optimizer != "hip":
            raise _native.PbgError("PPO: lr_schedule is read from device memory by the library's optimiser: it needs "
                                   "optimizer='hip'")
        if lr_schedule is not None and (schedule_iterations is None or int(schedule_iterations) < 1):
            raise _native.PbgError(f"PPO: lr_schedule needs schedule_iterations >= 1, got {schedule_iterations!r}")
        if grad_path not in PPOGrad.PATHS:
            raise _native.PbgError(f"PPO: grad_path must be 'fma' or 'mfma', got {grad_path!r}")
        if grad_path != "fma" and backward != "hip":
            raise _native.PbgError("PPO: grad_path selects a path of pbg_ppo_grad: it needs backward='hip'")
        if vf_clip is not None and not float(vf_clip) > 0.0:
            raise _native.PbgError(f"PPO: vf_clip must be None or > 0, got {vf_clip!r}")
        if target_kl is not None and optimizer != "hip":
            raise _native.PbgError("PPO: target_kl is a gate the library's launches read on the device: it needs optimizer='hip'")
        if target_kl is not None and not float(target_kl) > 0.0:
            raise _native.PbgError(f"PPO: target_kl must be None or > 0, got {target_kl!r}")
        self.vf_clip = None if vf_clip is None else float(vf_clip)
        self.target_kl = None if target_kl is None else float(target_kl)
        self.backward, self.grad_path = backward, grad_path
        if n % 2 != 0 or not env.autoreset:
            raise _native.PbgError("PPO: the env must have an even number of envs (the actors are populations of one "
                                   "pair) and autoreset=True")
        if int(steps) < 1 or int(epochs) < 1 or int(minibatches) < 1 or (int(steps) * nb) % int(minibatches) != 0:
            raise _native.PbgError("PPO: steps, epochs, minibatches must be >= 1 and steps * num_envs a multiple of minibatches")
        self.env, self.steps, self.seed = env, int(steps), int(seed)
        self.gamma, self.lam, self.clip, self.epochs, self.minibatches = float(gamma), float(lam), float(clip), int(epochs), \
            int(minibatches)
        self.vf_coef, self.ent_coef, self.max_grad_norm, self.norm_adv = float(vf_coef), float(ent_coef), max_grad_norm, norm_adv
        obs_dim, act_dim = env.info.obs_dim, env.info.action_dim
        self.actor_dims = (obs_dim, int(hidden[0]), int(hidden[1]), act_dim)
        self.critic_dims = (obs_dim, int(hidden[0]), int(hidden[1]), 1)
        self.actor = MLPPopulation(self.actor_dims, 1, dev)
        self.critic = MLPPopulation(self.critic_dims, 1, dev)
        self.noise = ActionNoise(act_dim, self.seed, dev)
        self.actor.attach_action_noise(self.noise)
        ta, tc = self.actor.init_theta(self.seed), self.critic.init_theta(self.seed + 1)
        ta[-(self.actor_dims[2] * act_dim + act_dim):] *= 0.01   # a near-zero mean at the start: the noise explores
        self.actor_theta = torch.nn.Parameter(ta)
        self.critic_theta = torch.nn.Parameter(tc)
        self.log_std = torch.nn.Parameter(torch.full((act_dim,), float(log_std), dtype=torch.float32, device=dev))
        # with optimizer="hip" this object is built and never stepped: the moments and the step count are self.adam's
        self.opt = torch.optim.Adam([self.actor_theta, self.critic_theta, self.log_std], lr=float(lr), eps=1e-5)
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(self.seed)
        self.iteration = 0
        self.obs_stats, self.obs_clip = None, float(obs_clip)
        if obs_norm:
            self.obs_stats = ObsStats(obs_dim, nb, group=nb // 2, device=dev)
            self._set_norm()  # the initial totals' normaliser
        T = self.steps
        kw = dict(dtype=torch.float32, device=dev)
        self._value = torch.zeros((T + 1, n), **kw)
        self._adv, self._ret = torch.zeros((T, n), **kw), torch.zeros((T, n), **kw)
        self._obs_all = torch.zeros(((T + 1) * n, obs_dim), **kw)
        self._std = torch.zeros(act_dim, **kw)
        # truncation="bootstrap": the critic's values of the terminal observations, written whole by every act_where
        self._term_value = torch.zeros((T, n), **kw) if truncation == "bootstrap" else None
        self.ret_stats, self.reward_clip = None, float(reward_clip)
        if reward_norm:
            if not self.reward_clip > 0.0:
                raise _native.PbgError(f"PPO: reward_clip must be > 0, got {reward_clip!r}")
            self.ret_stats = self._make_ret_stats(n, dev)
            # what gae reads in place of the rollout's rew_traj, written whole by every apply
            self._rew_scaled = torch.zeros((T, n), **kw)
        self.grad = None
        if backward == "hip":
            # the gradient tensors pbg_ppo_grad writes, bound once to the parameters' .grad
            self.grad = PPOGrad(self.actor_dims, (T * nb) // self.minibatches, dev, path=grad_path)
            for p in (self.actor_theta, self.critic_theta, self.log_std):
                p.grad = torch.zeros_like(p.data)
            self._grad_stats = torch.zeros(4, dtype=torch.float64, device=dev)
            # the storage both optimisers move in place: what every launch of the update reads and writes
            self._params = [self.actor_theta.data, self.critic_theta.data, self.log_std.data]
            self._grads = [self.actor_theta.grad, self.critic_theta.grad, self.log_std.grad]
        self.adam = self._graph = self.perm = self._it_dev = self._iter_graph = self.kl_gate = None
        self.permutation, self.lr_schedule, self.graph_iteration = permutation, lr_schedule, graph == "iteration"
        if optimizer == "hip":
            if norm_adv and (T * nb) // self.minibatches < 2:
                raise _native.PbgError("PPO: optimizer='hip' with norm_adv needs minibatches of at least 2 rows")
            self.adam = AdamClip([p.numel() for p in self._params], dev)
            self.lr, self.use_graph = float(lr), graph is True
            self._adv_norm = torch.zeros(2, **kw)
            self._opt_info = torch.zeros(2, dtype=torch.float64, device=dev)
            self._lr_now = self.lr   # what AdamClip.step gets: the float, or the schedule's device tensor
            if lr_schedule is not None or graph == "iteration":
                # the iteration count the schedule reads, advanced on the stream (inside a captured iteration)
                self._it_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            if lr_schedule is not None:
                self.schedule_iterations = int(schedule_iterations)
                self._lr_dev = torch.zeros(1, dtype=torch.float64, device=dev)
                self._lr_now = self._lr_dev
            if permutation == "device":
                self.perm = Permutation(self.seed, dev)
            # what the chain (and a replay of it) reads and every update refills in place
            self._perm = torch.zeros((self.epochs, self.minibatches, (T * nb) // self.minibatches), dtype=torch.int64, device=dev)
            self._logp_old = torch.zeros(T * nb, **kw)
            if self.target_kl is not None:
                self.kl_gate, self.kl_limit = KLGate(dev), 1.5 * self.target_kl
        env.reset()

    def _batch_envs(self, env) -> int:
        return env.num_envs

    def _make_ret_stats(self, n, dev):
        return RetStats(n, self.gamma, dev)

    def _scale_rewards(self, rew_traj, done_traj):
        """``reward_norm``'s three launches: the returns' walk, the totals and the scale, the scaled rewards."""
        self.ret_stats.update(rew_traj, done_traj)
        self.ret_stats.finalize()
        return self.ret_stats.apply(rew_traj, out=self._rew_scaled, clip=self.reward_clip)

    def _set_norm(self):
        mean, inv_std = self.obs_stats.finalize()
        self.actor.set_obs_norm(mean, inv_std, clip=self.obs_clip)
        self.critic.set_obs_norm(mean, inv_std, clip=self.obs_clip)

    def collect(self) -> Batch:
        """The collection half of an iteration: both networks take their weights, the env runs ``steps`` noisy
        steps, the critic values every visited observation and the last one, and ``gae`` turns them into
        advantages.  A function of the seed and the parameters alone: it repeats bit for bit."""
        env, T, n = self.env, self.steps, self.env.num_envs
        self.actor.set_all(self.actor_theta.data)
        self.critic.set_all(self.critic_theta.data)
        torch.exp(self.log_std.data, out=self._std)
        self.noise.set_std(self._std)
        if self.obs_stats is not None:
            self.actor.attach_obs_stats(self.obs_stats)
        boot = self.truncation == "bootstrap"
        res = env.rollout(self.actor, T, trajectory=True, truncation=boot)
        if self.obs_stats is not None:
            self.actor.attach_obs_stats(None)
        self._obs_all[:T * n].copy_(res.obs_traj.view(T * n, -1))
        self._obs_all[T * n:].copy_(env.obs)
        self.critic.act(self._obs_all, out=self._value.view((T + 1) * n, 1))
        rew = res.rew_traj if self.ret_stats is None else self._scale_rewards(res.rew_traj, res.done_traj)
        if boot:
            # one launch more: the truncated rows' terminal observations through the critic, zeros elsewhere
            self.critic.act_where(res.trunc_traj, res.term_obs_traj, out=self._term_value.view(T, n, 1))
            gae(rew, res.done_traj, self._value, self.gamma, self.lam, adv=self._adv, ret=self._ret,
                trunc_traj=res.trunc_traj, term_value=self._term_value)
        else:
            gae(rew, res.done_traj, self._value, self.gamma, self.lam, adv=self._adv, ret=self._ret)
        b = Batch(obs=res.obs_traj, act=res.act_traj, rew=res.rew_traj, done=res.done_traj, eps2=res.eps2_traj,
                  logp=res.logp_traj(self._std), value=self._value, adv=self._adv, ret=self._ret)
        if boot:
            b.trunc, b.term_value = res.trunc_traj, self._term_value
        if self.ret_stats is not None:
            b.rew_scaled = rew
        return b

    def update(self, b: Batch) -> dict:
        """``epochs`` passes of ``minibatches`` clipped-surrogate steps over the batch (Adam; the gradient by torch
        autograd, or by pbg_ppo_grad with ``backward="hip"``)."""
        if self.adam is not None:
            return self._update_opt(b)
        if self.grad is not None:
            return self._update_hip(b)
        T, n = self.steps, self.env.num_envs
        B, A = T * n, self.actor_dims[3]
        obs, act = b.obs.reshape(B, -1), b.act.reshape(B, A)
        logp_old, ret, adv = b.logp.reshape(B).float(), b.ret.reshape(B), b.adv.reshape(B)
        norm = self.actor.obs_norm
        stats = {}
        for _ in range(self.epochs):
            perm = torch.randperm(B, device=obs.device, generator=self._gen).view(self.minibatches, -1)
            for idx in perm:
                a_mb = adv[idx]
                if self.norm_adv:
                    a_mb = (a_mb - a_mb.mean()) / (a_mb.std() + 1e-8)
                mu = mlp_forward(self.actor_theta, self.actor_dims, obs[idx], norm)
                v = mlp_forward(self.critic_theta, self.critic_dims, obs[idx], norm).squeeze(1)
                z = (act[idx] - mu) * torch.exp(-self.log_std)
                logp = -0.5 * (z * z).sum(1) - self.log_std.sum() - 0.5 * A * math.log(2.0 * math.pi)
                ratio = torch.exp(logp - logp_old[idx])
                pg = -torch.min(ratio * a_mb, torch.clamp(ratio, 1.0 - self.clip, 1.0 + self.clip) * a_mb).mean()
                vf = 0.5 * ((v - ret[idx]) ** 2).mean()
                if self.vf_clip is not None:
                    vo = self._value_old()[idx]
                    vc = vo + torch.clamp(v - vo, -self.vf_clip, self.vf_clip)
                    vf = 0.5 * torch.maximum((v - ret[idx]) ** 2, (vc - ret[idx]) ** 2).mean()
                entropy = self.log_std.sum() + 0.5 * A * (1.0 + math.log(2.0 * math.pi))
                loss = pg + self.vf_coef * vf - self.ent_coef * entropy
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                if self.max_grad_norm:
                    torch.nn.utils.clip_grad_norm_([self.actor_theta, self.critic_theta, self.log_std], self.max_grad_norm)
                self.opt.step()
                stats = dict(pg=pg.detach(), vf=vf.detach())
        return stats

    def _grad_args(self, batch, idx, adv_norm):
        """What ``PPOGrad.run`` takes from the trainer, in the one place that knows it: ``(args, inputs, outputs)``.
        ``args``: the parameters' storage, read where it lies, then ``batch = (obs, act, logp_old, adv, ret)``;
        ``inputs``: the minibatch's rows, the two normalisers and the loss's coefficients; ``outputs``: the three
        ``.grad`` tensors and the stats, overwritten in place.  ``run`` and ``reduce`` take all three, ``run_part``
        the first two."""
        inputs = dict(idx=idx, adv_norm=adv_norm, obs_norm=self.actor.obs_norm, clip_eps=self.clip, vf_coef=self.vf_coef,
                      ent_coef=self.ent_coef)
        if self.vf_clip is not None:
            inputs.update(value_old=self._value_old(), vf_clip=self.vf_clip)
        if self.kl_gate is not None:
            inputs.update(gate=self.kl_gate.gate)
        outputs = dict(grad_actor=self._grads[0], grad_critic=self._grads[1], grad_log_std=self._grads[2], stats=self._grad_stats)
        return (*self._params, *batch), inputs, outputs

    def _value_old(self):
        """``vf_clip``'s ``value_old [B]``: ``Batch.value[:T]``, a view of the trainer's own buffer, in the batch's row
        order."""
        return self._value[:self.steps].reshape(-1)

    def _gradient(self, batch, idx, adv_norm):
        """The minibatch's gradient into the parameters' ``.grad``: pbg_ppo_grad_run, two launches."""
        args, inputs, outputs = self._grad_args(batch, idx, adv_norm)
        self.grad.run(*args, **inputs, **outputs)

    def _update_hip(self, b: Batch) -> dict:
        """``update`` with the gradient from ``PPOGrad.run``: the same permutation, clipping and optimiser step; the
        parameters' storage is read where it lies and the three ``.grad`` tensors are overwritten in place."""
        T, n = self.steps, self.env.num_envs
        B, A = T * n, self.actor_dims[3]
        adv = b.adv.reshape(B)
        batch = (b.obs.reshape(B, -1), b.act.reshape(B, A), b.logp.reshape(B).float(), adv, b.ret.reshape(B))
        params = [self.actor_theta, self.critic_theta, self.log_std]
        for _ in range(self.epochs):
            perm = torch.randperm(B, device=adv.device, generator=self._gen).view(self.minibatches, -1)
            for idx in perm:
                adv_norm = None
                if self.norm_adv:
                    a_mb = adv[idx]
                    adv_norm = torch.stack((a_mb.mean(), 1.0 / (a_mb.std() + 1e-8)))
                self._gradient(batch, idx, adv_norm)
                if self.max_grad_norm:
                    torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
                self.opt.step()
        st = self._grad_stats.clone()   # the last minibatch's
        return dict(pg=st[0], vf=st[1], clipfrac=st[2], kl=st[3])

    def _minibatch_opt(self, batch, idx):
        """One minibatch step as at most five launches of the library: pbg_adv_norm, pbg_ppo_grad_run (two),
        pbg_ppo_opt_step (two); with ``target_kl`` a sixth between the two pairs, pbg_ppo_gate, and the gate's array goes
        to both."""
        self._gradient(batch, idx, adv_norm(batch[3], idx, out=self._adv_norm) if self.norm_adv else None)
        if self.kl_gate is None:
            self.adam.step(self._params, self._grads, self._lr_now, (0.9, 0.999), 1e-5, self.max_grad_norm, info=self._opt_info)
            return
        self.kl_gate.check(self._grad_stats, self.kl_limit)
        self.adam.step(self._params, self._grads, self._lr_now, (0.9, 0.999), 1e-5, self.max_grad_norm, info=self._opt_info,
                       gate=self.kl_gate.gate)

    def _schedule(self):
        """The schedule's launch: this iteration's learning rate into ``_lr_dev``, from the device's iteration count."""
        if self.lr_schedule is not None:
            lr_linear(self._it_dev, self.schedule_iterations, self.lr, out=self._lr_dev)

    def _draw(self, B):
        """This update's ``epochs`` permutations into ``_perm`` (``permutation="device"``: one fill)."""
        self.perm.fill(B, self.epochs, out=self._perm.view(self.epochs, B))

    def _chain(self, batch, B):
        """The ``epochs x minibatches`` chain of ``optimizer="hip"``, launches of the library alone: with ``target_kl``
        the gate's reset, the schedule's, with ``permutation="device"`` the permutation fill, then every minibatch of
        ``_perm``."""
        if self.kl_gate is not None:
            self.kl_gate.reset()
        self._schedule()
        if self.perm is not None:
            self._draw(B)
        for e in range(self.epochs):
            for idx in self._perm[e]:
                self._minibatch_opt(batch, idx)

    def _update_opt(self, b: Batch) -> dict:
        """``update`` with ``optimizer="hip"``: ``logp_old`` and, with ``permutation="torch"``, the permutations
        (``_update_hip``'s: the same generator) are written into the buffers ``_chain`` reads, and the chain runs.
        With ``graph=True`` the chain is captured at the first call and replayed from then on, and every other pointer
        it baked (the rollout's trajectories, ``adv``, ``ret``, the normaliser)
        is checked to be the one it was captured with: they are allocated once, so the check fires only if something
        outside the trainer moves them, and it raises rather than replaying on stale addresses.  (``VecEnv.rollout``
        keeps one set of trajectory buffers per ``(steps, trajectory)``: a rollout of the trainer's env with another
        ``steps`` between iterations does not move the trainer's.)  ``lr`` is a launch argument: the graph keeps the value it
        was captured with, unless ``lr_schedule`` is set: then the chain starts with the schedule's launch and every step
        reads ``_lr_dev``.  With ``permutation="device"`` the chain's second item is the permutation fill (inside the
        graph with ``graph=True``) and ``torch.randperm`` is not called."""
        T, n = self.steps, self.env.num_envs
        B, A = T * n, self.actor_dims[3]
        obs, act = b.obs.reshape(B, -1), b.act.reshape(B, A)
        ret, adv = b.ret.reshape(B), b.adv.reshape(B)
        batch = (obs, act, self._logp_old, adv, ret)
        self._logp_old.copy_(b.logp.reshape(B))   # float64 -> float32, the rounding of ``.float()``
        if self.perm is None:
            for e in range(self.epochs):
                torch.randperm(B, device=obs.device, generator=self._gen, out=self._perm[e].view(B))
        if not self.use_graph:
            self._chain(batch, B)
            if self._capturing:   # graph="iteration": nothing may be read back inside the capture
                return {}
            return self._stats_now()
        norm = self.actor.obs_norm
        baked = tuple(t.data_ptr() for t in (obs, act, adv, ret) + (() if norm is None else norm[:2])) + \
            (None if norm is None else norm[2],)
        if self._graph is None:
            # once eagerly what writes only outputs the chain overwrites before it reads them (the normaliser pair,
            # the gradient, its stats): no kernel is launched for the first time inside the capture
            idx = self._perm[0, 0]
            self._schedule()   # it writes only the learning rate the chain's first launch writes again
            self._gradient(batch, idx, adv_norm(adv, idx, out=self._adv_norm) if self.norm_adv else None)
            with torch.cuda.device(obs.device):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self._chain(batch, B)
            self._graph, self._baked = graph, baked
        elif baked != self._baked:
            raise _native.PbgError("PPO.update: a buffer the captured update reads has moved since the capture")
        self._graph.replay()
        return self._stats_now()

    _capturing = False

    def _iterate_once(self) -> dict:
        """One iteration's launches in order, the device's iteration count included."""
        b = self.collect()
        stats = self.update(b)
        if self.obs_stats is not None:
            self._set_norm()
        if self._it_dev is not None:
            self._it_dev.add_(1)
        return stats

    def _stats_now(self) -> dict:
        st, info = self._grad_stats.clone(), self._opt_info.clone()   # the last minibatch's
        stats = dict(pg=st[0], vf=st[1], clipfrac=st[2], kl=st[3], grad_norm=info[0])
        if self.kl_gate is not None:
            g = self.kl_gate.state   # a stopped update: the tripping minibatch's stats, the last applied step's norm
            stats.update(updates=g[1], kl_stop=g[0])
        return stats

    def _baked_iteration(self):
        """The addresses an iteration's launches take that the trainer does not own alone: the env's observation and
        rollout buffers, and the normaliser's copies."""
        env, T = self.env, self.steps
        # truncation="bootstrap": its own key, whose trajectories include trunc_traj and term_obs_traj
        io, traj = env._ro_io[(T, True, True) if self.truncation == "bootstrap" else (T, True)]
        ts = [env.obs] + list(env._ro_work.values()) + list(env._ro_acc.values()) + [traj[k] for k in sorted(traj)]
        norm = self.actor.obs_norm
        return tuple(t.data_ptr() for t in ts + ([] if norm is None else list(norm[:2]))) + \
            (None if norm is None else norm[2],)

    def iterate(self) -> dict:
        stats = self._iterate()
        if self.ret_stats is not None:
            stats["rew_scale"] = self.ret_stats.scale   # a copy on the stream, after the iteration (or its replay)
        return stats

    def _iterate(self) -> dict:
        if not self.graph_iteration:
            stats = self._iterate_once()
            self.iteration += 1
            return stats
        if self._iter_graph is None:
            # iteration 0 runs eagerly: every kernel the graph will launch has then been launched once, every lazily
            # allocated buffer exists, and nothing has to be undone.  The capture itself executes nothing
            stats = self._iterate_once()
            with torch.cuda.device(self.env.device):
                graph = torch.cuda.CUDAGraph()
                self._capturing = True
                try:
                    with torch.cuda.graph(graph):
                        self._iterate_once()
                finally:
                    self._capturing = False
            self._iter_graph, self._iter_baked = graph, self._baked_iteration()
        else:
            if self._baked_iteration() != self._iter_baked:
                raise _native.PbgError("PPO.iterate: a buffer the captured iteration reads has moved since the capture")
            self._iter_graph.replay()
            stats = self._stats_now()
        self.iteration += 1
        return stats

    def evaluate(self, env, steps: int, init_q=None):
        """The noise-free mean policy on ``env`` (another ``VecEnv`` of the same robot, an even ``num_envs``):
        per-env ``(returns float64 [n], lengths int32 [n])`` of a fresh ``steps``-step rollout (of the first
        episode with ``autoreset=False``).  Moves neither the statistics nor the noise's counter."""
        self.actor.set_all(self.actor_theta.data)
        self.actor.attach_action_noise(None)
        env.reset(init_q=init_q)
        res = env.rollout(self.actor, steps, fresh=True)
        self.actor.attach_action_noise(self.noise)
        return res.done_return + res.cur_return, res.done_length + res.cur_length

    def save_npz(self, path):
        """The mean policy (and the normaliser in force, if any) under the reference's key names:
        ``MLPPolicy.from_npz`` and tools/enjoy.py load it."""
        self.actor.save_npz(path, self.actor_theta.data)

    def close(self):
        self.actor.attach_action_noise(None)
        self._graph = self._iter_graph = None
        for o in (self.actor, self.critic, self.noise, self.obs_stats, self.grad, self.adam, self.perm, self.ret_stats,
                  self.kl_gate):
            if o is not None:
                o.close()


def share_block_bytes(share: int, dtot: int) -> int:
    """The bytes of one rank's block of the partial all-gather: ``share`` rows of 4 float64 stats, then ``share`` rows of
    ``dtot`` float32 partials, rounded up to a multiple of 8 so that in the gathered ``[world, bytes]`` array every
    rank's doubles start 8-byte aligned whatever ``share`` and ``dtot`` are."""
    return 32 * share + 8 * ((share * dtot + 1) // 2)


def share_views(block, share: int, dtot: int):
    """A block of ``share_block_bytes`` uint8 as ``(stats float64 [share, 4], part float32 [share, dtot])``, views of
    its memory."""
    return block[:32 * share].view(torch.float64).view(share, 4), \
        block[32 * share:32 * share + 4 * share * dtot].view(torch.float32).view(share, dtot)


class ShardedPPO(PPO):
    """Data-parallel ``PPO`` over a ``ShardedVecEnv`` (one process per rank, ``torch.distributed`` initialised by the
    caller; ``group``: its process group, ``None`` the default one) that holds, on every rank, the bits of the
    one-process ``PPO(VecEnv(num_global), backward="hip", optimizer="hip", permutation="device")`` (DESIGN.md section
    18).  Each rank collects on its shard as ``PPO.collect`` does -- the reset noise, the action noise and the
    networks do not depend on the shard -- one ``distributed.gather_traj`` gives every rank the global batch in the
    global row order, every rank draws the same permutations and the same ``adv_norm``, runs the workgroups
    ``shard_range(G, rank, world)`` of each minibatch's gradient (``PPOGrad.run_part``), all-gathers the float32
    partials and the float64 stats, and runs the unchanged reduction and ``AdamClip.step`` on them.  With
    ``obs_norm=True`` the ranks' statistics slots are gathered in rank order into every rank's object before
    ``finalize``.  Needs ``backward="hip"``, ``optimizer="hip"``, ``permutation="device"`` and ``graph=False`` (the
    defaults here), equal shards of an even number of envs (a multiple of 32 with ``obs_norm`` or ``reward_norm``).
    With ``reward_norm=True`` each rank walks its shard's returns at the slots of its global envs, the ranks' slots are
    gathered in rank order before ``finalize``, and every rank holds the one-process trainer's totals and scale.
    With no process group initialised it runs as world 1: every workgroup as one part, no collective.  Under gloo the
    collectives are staged through the host."""

    _REQUIRED = dict(backward="hip", optimizer="hip", permutation="device", graph=False)

    def __init__(self, sharded_env, group=None, **ppo_kwargs):
        import torch.distributed as dist
        from .distributed import shard_range
        for name, want in self._REQUIRED.items():
            got = ppo_kwargs.setdefault(name, want)
            if got != want or type(got) is not type(want):
                raise _native.PbgError(f"ShardedPPO: {name} must be {want!r}, got {got!r}")
        self._group = group
        self._dist = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self._dist else 1
        self.rank = dist.get_rank(group) if self._dist else 0
        self.sharded_env, self.num_global = sharded_env, int(sharded_env.num_global)
        if (sharded_env.world, sharded_env.rank) != (self.world, self.rank):
            raise _native.PbgError(f"ShardedPPO: the env is shard {sharded_env.rank} of {sharded_env.world}, the process group "
                                   f"says rank {self.rank} of {self.world}")
        if self.num_global % self.world != 0:
            raise _native.PbgError(f"ShardedPPO: {self.num_global} global envs are no multiple of world = {self.world}: the "
                                   "shards must be equal")
        n_rank = self.num_global // self.world
        if n_rank % 2 != 0:
            raise _native.PbgError(f"ShardedPPO: {n_rank} envs per rank is odd (the actors are populations of one pair)")
        if ppo_kwargs.get("obs_norm", False) and n_rank % 32 != 0:
            raise _native.PbgError(f"ShardedPPO: obs_norm needs the {n_rank} envs per rank to be a multiple of 32, so that every "
                                   "rank's statistics tiles are tiles of the global trainer")
        if ppo_kwargs.get("reward_norm", False) and n_rank % 32 != 0:
            raise _native.PbgError(f"ShardedPPO: reward_norm needs the {n_rank} envs per rank to be a multiple of 32, so that "
                                   "every rank's return-statistics tiles are tiles of the global trainer")
        self._shard_range = shard_range
        super().__init__(sharded_env.env, **ppo_kwargs)
        dev, T = self.env.device, self.steps
        o, A = self.actor_dims[0], self.actor_dims[3]
        B = T * self.num_global
        self._mb_rows = B // self.minibatches
        self._G, self._dtot = self.grad.geometry(self._mb_rows)
        if self._G < 1:
            raise _native.PbgError(f"ShardedPPO: a minibatch of {self._mb_rows} rows has no workgroup")
        self._wg0, self._wgn = shard_range(self._G, self.rank, self.world)
        share = -(-self._G // self.world)
        # one rank's share as one block of bytes (share_block_bytes): what one all-gather moves
        self._send = torch.zeros(share_block_bytes(share, self._dtot), dtype=torch.uint8, device=dev)
        self._share = share
        self._part = torch.zeros((self._G, self._dtot), dtype=torch.float32, device=dev)
        self._part_stats = torch.zeros((self._G, 4), dtype=torch.float64, device=dev)
        kw = dict(dtype=torch.float32, device=dev)
        # vf_clip: one more column, the values the batch was collected under
        self._packed = torch.zeros((T, self.env.num_envs, o + A + 3 + (self.vf_clip is not None)), **kw)
        self._g_obs, self._g_act = torch.zeros((B, o), **kw), torch.zeros((B, A), **kw)
        self._g_adv, self._g_ret = torch.zeros(B, **kw), torch.zeros(B, **kw)
        self._g_value = torch.zeros(B, **kw) if self.vf_clip is not None else None

    def _batch_envs(self, env) -> int:
        return self.num_global

    def _make_ret_stats(self, n, dev):
        return RetStats(n, self.gamma, dev, n_slots=self.num_global // RetStats.TILE)

    def _value_old(self):
        return self._g_value

    def _gather_slots(self, stats, first, count):
        """The slots ``first .. first + count - 1`` of every rank's ``stats`` (an ``ObsStats`` or a ``RetStats``), one
        all-gather of ``counts | sums`` as 8-byte words (bits kept), in rank order into the slots ``0 .. world * count - 1``
        of this rank's: the global trainer's slots."""
        counts, sums = stats.get_slots(first, count)
        got = self._all_gather(torch.cat((counts.view(count, 1), sums.view(torch.int64)), dim=1)).view(self.world * count, -1)
        stats.set_slots(0, got[:, 0].contiguous(), got[:, 1:].contiguous().view(torch.float64))

    def _scale_rewards(self, rew_traj, done_traj):
        """``PPO._scale_rewards`` over the global envs: this rank's tiles at their global slots, the ranks' slots
        gathered, then the finalize over all of them."""
        rs, k = self.ret_stats, self.env.num_envs // RetStats.TILE
        rs.update(rew_traj, done_traj, slot_offset=self.rank * k)
        if self.world > 1:
            self._gather_slots(rs, self.rank * k, k)
        rs.finalize()
        return rs.apply(rew_traj, out=self._rew_scaled, clip=self.reward_clip)

    def _all_gather(self, send):
        from .distributed import all_gather_blocks
        return all_gather_blocks(send, self._group)

    def _share_views(self, block):
        return share_views(block, self._share, self._dtot)

    def _gradient(self, batch, idx, adv_norm):
        """``PPO._gradient`` as parts: this rank's workgroups, one all-gather, the reduction."""
        args, inputs, outputs = self._grad_args(batch, idx, adv_norm)
        # world 1: every workgroup (shard_range's 0, G) straight into the reduction's input, no collective
        st, pt = (self._part_stats, self._part) if self.world == 1 else (v[:self._wgn] for v in self._share_views(self._send))
        self.grad.run_part(*args, self._wg0, self._wgn, pt, st, **inputs)
        if self.world > 1:
            got = self._all_gather(self._send)
            for r in range(self.world):   # the pad rows of the narrower shares are dropped
                off, cnt = self._shard_range(self._G, r, self.world)
                st, pt = self._share_views(got[r])
                self._part_stats[off:off + cnt].copy_(st[:cnt])
                self._part[off:off + cnt].copy_(pt[:cnt])
        self.grad.reduce(*args, self._G, self._part, self._part_stats, **inputs, **outputs)

    def update(self, b: Batch) -> dict:
        """One gather of the shard's packed ``(obs | act | logp_old | adv | ret)`` columns, then ``PPO``'s chain of
        ``epochs x minibatches`` steps on the global batch in the global row order ``t * num_global + e``."""
        from .distributed import gather_traj
        T, o, A = self.steps, self.actor_dims[0], self.actor_dims[3]
        B, p = T * self.num_global, self._packed
        p[:, :, :o].copy_(b.obs)
        p[:, :, o:o + A].copy_(b.act)
        p[:, :, o + A].copy_(b.logp)   # float64 -> float32, the rounding of PPO's own copy
        p[:, :, o + A + 1].copy_(b.adv)
        p[:, :, o + A + 2].copy_(b.ret)
        if self.vf_clip is not None:
            p[:, :, o + A + 3].copy_(b.value[:T])
        g = (p if self.world == 1 else gather_traj(p, self.num_global, self._group)).view(B, p.shape[2])
        self._g_obs.copy_(g[:, :o])
        self._g_act.copy_(g[:, o:o + A])
        self._logp_old.copy_(g[:, o + A])
        self._g_adv.copy_(g[:, o + A + 1])
        self._g_ret.copy_(g[:, o + A + 2])
        if self.vf_clip is not None:
            self._g_value.copy_(g[:, o + A + 3])
        self._chain((self._g_obs, self._g_act, self._logp_old, self._g_adv, self._g_ret), B)
        return self._stats_now()

    def _merge_slots(self):
        """Every rank's used observation slots into this rank's object."""
        self._gather_slots(self.obs_stats, 0, self.env.num_envs // 16)

    def _iterate_once(self) -> dict:
        b = self.collect()
        stats = self.update(b)
        if self.obs_stats is not None:
            if self.world > 1:
                self._merge_slots()
            self._set_norm()
        if self._it_dev is not None:
            self._it_dev.add_(1)
        return stats
