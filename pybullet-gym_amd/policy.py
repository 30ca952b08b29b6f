"""The reference's pretrained-policy MLP as a native object (include/pbg.h pbg_policy_*).

``examples/roboschool-weights/enjoy_TF_*.py`` evaluate ``SmallReactivePolicy.act`` (:25-31 of each
file: relu(x w1 + b1) -> relu(. w2 + b2) -> . w3 + b3) once per env step on the host.  ``MLPPolicy``
holds the same weights in libpbg_amd.so: on a GPU ``act`` is one kernel launch for the whole batch,
and ``VecEnv.rollout`` runs the closed loop ``env.step(pi.act(obs))`` without leaving the device.
A host policy (``device=None``) evaluates the same floats on the CPU, bit for bit."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native

NPZ_KEYS = ("weights_dense1_w", "weights_dense1_b", "weights_dense2_w", "weights_dense2_b",
            "weights_final_w", "weights_final_b")  # the reference's names (enjoy_TF_*.py:21-24)
NORM_KEYS = ("obs_mean", "obs_inv_std", "obs_clip")  # this project's: a normaliser saved next to the weights


def _need(name):
    if not hasattr(_native.lib(), name):
        raise _native.PbgError(f"{_native.LIB_PATH} has no {name}: a build without observation normalisation")
    return getattr(_native.lib(), name)


def check_array(t, who, name, shape, dt, device):
    """The one check of an array whose pointer goes to the library as it is, and that pointer: ``t`` must already
    be a C-contiguous numpy array (``device`` None: the host) or a contiguous tensor on the GPU ``device``, of
    ``shape`` and of the numpy dtype ``dt``, so nothing is converted (or written past) silently.  ``who`` is the
    ``function`` the message starts with, or ``(object, method)`` for ``Class.method`` (put together only when the
    check fails: this runs for every pointer of every launch); ``name`` is the argument's."""
    shape = tuple(shape)
    if device is None:
        ok = isinstance(t, np.ndarray) and t.flags.c_contiguous and t.dtype == dt
    else:
        import torch
        ok = isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.is_contiguous() and \
            t.dtype == (_TORCH_DTYPES.get(dt) or _torch_dtype(dt))
    if not ok or tuple(t.shape) != shape:
        who = who if isinstance(who, str) else f"{type(who[0]).__name__}.{who[1]}"
        raise _native.PbgError(f"{who}: {name} must be a contiguous {np.dtype(dt).name} "
                               f"{'array' if device is None else f'tensor on the GPU {device}'} of shape {shape}")
    return t.ctypes.data if device is None else t.data_ptr()


_TORCH_DTYPES = {}


def _torch_dtype(dt):
    """The torch dtype of the numpy dtype ``dt``, looked up once."""
    if dt not in _TORCH_DTYPES:
        import torch
        _TORCH_DTYPES[dt] = getattr(torch, np.dtype(dt).name)
    return _TORCH_DTYPES[dt]


def new_array(shape, dt, device):
    """An uninitialised array that passes ``check_array(..., shape, dt, device)``."""
    if device is None:
        return np.empty(shape, dt)
    import torch
    return torch.empty(shape, dtype=_torch_dtype(dt), device=device)


def launch(device, fname, *args):
    """The library's ``fname(*args, stream)`` on the current stream of the GPU ``device``, checked; ``device`` None:
    ``fname(*args)``, a host entry point that takes no stream."""
    f = getattr(_native.lib(), fname)
    if device is None:
        _native.check(f(*args), fname)
        return
    import torch
    with torch.cuda.device(device):
        _native.check(f(*args, torch.cuda.current_stream(device).cuda_stream), fname)


class _NativeObject:
    """What the wrappers of a native object share: the handle ``_h`` and its destroy function, the guard
    against use after ``close``, the device as ``cuda:<index>`` (``None``: a host object, ``host`` is then true),
    the current stream, and the check (``_ptr``) and the allocator (``_new``) of an array whose pointer goes to
    the library as it is: a tensor on the object's GPU, a numpy array on the host.  A class whose host twin
    keeps its state in Python and owns no native object says so with ``_HOST_HANDLE = False``: the guard lets
    that twin through, and its ``close`` has nothing to destroy."""
    _DESTROY = None       # the library's destroy function
    _NOUN = "object"      # what the closed guard calls the object
    _HOST_HANDLE = True   # a host object owns a native object too
    _h = None
    device = None         # torch.device("cuda", index); None: a host object

    host = property(lambda self: self.device is None, doc="No GPU: numpy arrays in and out.")

    def _set_device(self, device, rule="a GPU", host=False) -> int:
        """Store ``device`` as ``torch.device("cuda", index)`` and return the index; with ``host``, ``None`` or
        ``"cpu"`` is the host: ``device`` None, index -1."""
        if host and (device is None or str(device) == "cpu"):
            self.device = None
            return -1
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _native.PbgError(f"{type(self).__name__}: device must be {rule}, got {device!r}")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        return idx

    def close(self):
        """Destroy the native object (an ``ObsStats``: detach it from every actor first)."""
        if self._h:
            getattr(_native.lib(), self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self, what):
        if not self._h and (self._HOST_HANDLE or self.device is not None):
            raise _native.PbgError(f"{type(self).__name__}.{what}: the {self._NOUN} is closed")
        return self._h

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _launch(self, fname, *args):
        """``launch`` on the object's side: ``fname(*args, stream)`` on its GPU, ``fname(*args)`` on the host."""
        launch(self.device, fname, *args)

    def _ptr(self, t, what, name, shape, dt=np.float32):
        """``check_array`` on the object's side: the pointer of ``t``, a contiguous tensor on the object's GPU
        (an array on the host) of ``shape`` and of the numpy dtype ``dt``."""
        return check_array(t, (self, what), name, shape, dt, self.device)

    def _vec(self, t, what, name, shape, dt=np.float32):
        """``_ptr`` for a caller that goes on with the array: ``t`` itself, checked."""
        self._ptr(t, what, name, shape, dt)
        return t

    def _new(self, shape, dt=np.float32):
        return new_array(shape, dt, self.device)


class ObsStats(_NativeObject):
    """Running per-component statistics of observations on one GPU (include/pbg.h pbg_obs_stats_*): float64
    totals ``count, sum[K], sumsq[K]`` (initially OpenAI ES's ``RunningStat(eps=1e-2)``) and one partial
    accumulator ("slot") per 16-row tile, so nothing is atomic and every sum has a stated order.

    ``n_envs`` and ``group`` size the slots for the launches the object will see: ``group=None`` for batches
    of up to ``n_envs`` rows tiled as ``MLPPolicy`` tiles them, ``group=G`` for ``n_envs / G`` groups of
    ``G`` consecutive rows tiled per group as ``MLPPopulation`` tiles its members' envs.  Attached to an
    actor (``attach_obs_stats``), every step of ``VecEnv.rollout`` with that actor adds the observations
    whose actions are booked; ``update`` adds a batch directly.  ``finalize`` folds the slots into the
    totals and returns ``(mean, inv_std)``.  Everything is asynchronous on the current stream."""
    _DESTROY = "pbg_obs_stats_destroy"

    def __init__(self, obs_dim: int, n_envs: int, group=None, device="cuda:0"):
        import torch
        self.obs_dim, self.n_envs = int(obs_dim), int(n_envs)
        self.group = None if group is None else int(group)
        if self.n_envs < 1 or (self.group is not None and (self.group < 1 or self.n_envs % self.group != 0)):
            raise _native.PbgError(f"ObsStats: n_envs {n_envs} must be >= 1 and a multiple of group {group}")
        G = self.n_envs if self.group is None else self.group
        self.n_slots = (self.n_envs // G) * ((G + 15) // 16)
        idx = self._set_device(device)
        h = ctypes.c_void_p()
        _native.check(_need("pbg_obs_stats_create")(idx, self.obs_dim, self.n_slots, ctypes.byref(h)),
                      "pbg_obs_stats_create")
        self._h = h
        self.mean = torch.zeros(self.obs_dim, dtype=torch.float32, device=self.device)
        self.inv_std = torch.ones(self.obs_dim, dtype=torch.float32, device=self.device)

    def update(self, obs, active=None):
        """Add ``obs`` (``[n, obs_dim]`` float32 on the device) to the slots: the rows whose ``active`` flag
        (``[n]`` uint8, None = all) is set and that hold no NaN or inf."""
        import torch
        s = self._open("update")
        n = obs.shape[0] if isinstance(obs, torch.Tensor) and obs.dim() == 2 else -1
        self._vec(obs, "update", "obs", (n, self.obs_dim))
        if active is not None:
            self._vec(active, "update", "active", (n,), np.uint8)
        _native.check(_native.lib().pbg_obs_stats_update(s, n, self.group or 0, obs.data_ptr(),
                                                         None if active is None else active.data_ptr(), self._stream()),
                      "pbg_obs_stats_update")

    def finalize(self):
        """Fold the slots into the totals (slot-ascending float64 adds), zero them and return ``(mean,
        inv_std)``: float32 ``[obs_dim]`` device tensors this object owns and overwrites, ``inv_std =
        1 / sqrt(max(var, 1e-2))``."""
        s = self._open("finalize")
        _native.check(_native.lib().pbg_obs_stats_finalize(s, self.mean.data_ptr(), self.inv_std.data_ptr(),
                                                           self._stream()), "pbg_obs_stats_finalize")
        return self.mean, self.inv_std

    def _slot_range(self, what, first, count):
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > self.n_slots:
            raise _native.PbgError(f"ObsStats.{what}: slots {first} .. {first} + {count} are outside the object's 0 .. "
                                   f"{self.n_slots}")
        return first, count

    def get_slots(self, first: int, count: int):
        """``(counts int64 [count], sums float64 [count, 2 obs_dim])`` of the slots ``first .. first + count - 1``,
        per slot ``sum | sumsq``: fresh device tensors, one launch (pbg_obs_stats_get_slots); the slots stay as
        they are."""
        import torch
        first, count = self._slot_range("get_slots", first, count)
        s = self._open("get_slots")
        counts = torch.empty(count, dtype=torch.int64, device=self.device)
        sums = torch.empty((count, 2 * self.obs_dim), dtype=torch.float64, device=self.device)
        _native.check(_need("pbg_obs_stats_get_slots")(s, first, count, counts.data_ptr(), sums.data_ptr(), self._stream()),
                      "pbg_obs_stats_get_slots")
        return counts, sums

    def set_slots(self, first: int, counts, sums):
        """Overwrite the slots ``first .. first + len(counts) - 1`` with ``counts`` (int64 ``[count]``) and ``sums``
        (float64 ``[count, 2 obs_dim]``), ``get_slots``' layout: one launch (pbg_obs_stats_set_slots).  Slots
        gathered from equal shards in shard order and finalized here give the unsharded object's bits."""
        import torch
        count = counts.shape[0] if isinstance(counts, torch.Tensor) and counts.dim() == 1 else -1
        first, count = self._slot_range("set_slots", first, count)
        s = self._open("set_slots")
        self._vec(counts, "set_slots", "counts", (count,), np.int64)
        self._vec(sums, "set_slots", "sums", (count, 2 * self.obs_dim), np.float64)
        _native.check(_need("pbg_obs_stats_set_slots")(s, first, count, counts.data_ptr(), sums.data_ptr(), self._stream()),
                      "pbg_obs_stats_set_slots")

    @property
    def totals(self):
        """``[1 + 2 obs_dim]`` float64 on the device: count, sum, sumsq (a fresh tensor; what the slots hold
        is not in it before ``finalize``).  Assignable, to resume a run or to merge shards by adding totals."""
        import torch
        s = self._open("totals")
        out = torch.empty(1 + 2 * self.obs_dim, dtype=torch.float64, device=self.device)
        _native.check(_native.lib().pbg_obs_stats_get_totals(s, out.data_ptr(), self._stream()),
                      "pbg_obs_stats_get_totals")
        return out

    @totals.setter
    def totals(self, value):
        import torch
        s = self._open("totals")
        t = torch.as_tensor(value).to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(t.shape) != (1 + 2 * self.obs_dim,):
            raise _native.PbgError(f"ObsStats.totals: shape {tuple(t.shape)}, expected ({1 + 2 * self.obs_dim},)")
        _native.check(_native.lib().pbg_obs_stats_set_totals(s, t.data_ptr(), self._stream()),
                      "pbg_obs_stats_set_totals")
        self._totals_src = t  # alive until the stream has copied it


class ActionNoise(_NativeObject):
    """Per-env Gaussian action noise on one GPU (include/pbg.h pbg_action_noise_*).  Attached to an actor
    (``attach_action_noise``), every step of ``VecEnv.rollout`` with that actor acts ``a = mu(obs) + std * eps``
    (float64 arithmetic, rounded once) inside the actor launch; ``act`` never samples.  ``eps`` is counter-based
    (Philox4x32-10 keyed by ``seed``, counter = block of 4 components, global env index, step count, 0xAC), so
    it depends on neither the batch, the shard nor the actor's kind, and ``fill`` regenerates the bits of any
    step.  ``std`` starts at zero, the step ``counter`` at zero; the counter lives on the device and every
    rollout call advances it by its steps, a graph replay included.  Everything is asynchronous on the current
    stream."""
    _DESTROY, _NOUN = "pbg_action_noise_destroy", "action noise"

    def __init__(self, act_dim: int, seed: int = 0, device="cuda:0"):
        self.act_dim, self.seed = int(act_dim), int(seed) & 0xFFFFFFFFFFFFFFFF
        idx = self._set_device(device)
        h = ctypes.c_void_p()
        _native.check(_need("pbg_action_noise_create")(idx, self.act_dim, self.seed, ctypes.byref(h)),
                      "pbg_action_noise_create")
        self._h = h
        self._eps2 = None  # the bound eps2_traj tensor (kept alive while bound)

    def set_std(self, std):
        """``std``: contiguous float32 ``[act_dim]`` on the device, copied on the current stream (not validated)."""
        z = self._open("set_std")
        std = self._vec(std, "set_std", "std", (self.act_dim,))
        _native.check(_native.lib().pbg_action_noise_set_std(z, std.data_ptr(), self._stream()), "pbg_action_noise_set_std")

    @property
    def counter(self) -> int:
        """Steps sampled so far (synchronises to read it); assignable, to resume a run."""
        import torch
        z = self._open("counter")
        out = torch.zeros(1, dtype=torch.int32, device=self.device)
        _native.check(_native.lib().pbg_action_noise_get_counter(z, out.data_ptr(), self._stream()),
                      "pbg_action_noise_get_counter")
        return int(out.item()) & 0xFFFFFFFF

    @counter.setter
    def counter(self, value):
        z = self._open("counter")
        _native.check(_native.lib().pbg_action_noise_set_counter(z, int(value) & 0xFFFFFFFF, self._stream()),
                      "pbg_action_noise_set_counter")

    def bind_eps2_traj(self, eps2_traj):
        """Where the next rollouts write each step's ``sum_j eps[e][j] ** 2``: a contiguous float64 ``[T, n]``
        device tensor for rollouts of T steps over n envs (None: nowhere).  ``VecEnv.rollout`` calls this."""
        import torch
        z = self._open("bind_eps2_traj")
        if eps2_traj is not None:
            shape = tuple(eps2_traj.shape) if isinstance(eps2_traj, torch.Tensor) and eps2_traj.dim() == 2 else (-1, -1)
            self._vec(eps2_traj, "bind_eps2_traj", "eps2_traj", shape, np.float64)
        _native.check(_native.lib().pbg_action_noise_set_eps2_traj(z, None if eps2_traj is None else eps2_traj.data_ptr()),
                      "pbg_action_noise_set_eps2_traj")
        self._eps2 = eps2_traj

    def fill(self, n: int, env_offset: int, step: int, out=None):
        """``[n, act_dim]`` float32: the eps of global envs ``env_offset .. env_offset + n`` at the absolute step
        count ``step`` (the counter before a rollout call plus the step inside it), the bits the actor adds."""
        import torch
        z = self._open("fill")
        shape = (int(n), self.act_dim)
        out = torch.empty(shape, dtype=torch.float32, device=self.device) if out is None else out
        out = self._vec(out, "fill", "out", shape)
        _native.check(_native.lib().pbg_action_noise_fill(z, int(n), int(env_offset), int(step) & 0xFFFFFFFF,
                                                          out.data_ptr(), self._stream()), "pbg_action_noise_fill")
        return out


def _attach_action_noise(actor, fname, noise):
    p = actor._open("attach_action_noise")
    _native.check(_need(fname)(p, None if noise is None else noise._open("attach")), fname)
    actor.action_noise = noise


class MLPPolicy(_NativeObject):
    """obs -> h1 -> h2 -> act, ReLU on the hidden layers, float32.

    ``w1 [obs_dim, h1]``, ``b1 [h1]``, ``w2 [h1, h2]``, ``b2 [h2]``, ``w3 [h2, act_dim]``,
    ``b3 [act_dim]``: numpy arrays (or anything ``np.asarray`` takes), the reference's layout.
    ``device``: None = a host policy (``act`` takes and returns numpy, no GPU needed); a torch device
    (``"cuda:0"``) = the weights live there and ``act`` takes and returns torch tensors on it.
    Dims: 1..256 for obs_dim / h1 / h2, 1..64 for act_dim, no multiple of anything required.
    ``obs_norm=(mean, inv_std, clip)``: a normaliser (``set_obs_norm``)."""
    _DESTROY, _NOUN = "pbg_policy_destroy", "policy"
    _ROLLOUT = "pbg_rollout"   # VecEnv.rollout's entry point for this actor
    n_members = 1              # one weight set for the whole batch
    action_noise = None        # the attached ActionNoise, or None

    def __init__(self, w1, b1, w2, b2, w3, b3, device=None, obs_norm=None):
        ws = [np.ascontiguousarray(np.asarray(a), dtype=np.float32) for a in (w1, b1, w2, b2, w3, b3)]
        w1, b1, w2, b2, w3, b3 = ws
        if w1.ndim != 2 or w2.ndim != 2 or w3.ndim != 2 or b1.ndim != 1 or b2.ndim != 1 or b3.ndim != 1:
            raise _native.PbgError("MLPPolicy: weights must be 2-d and biases 1-d")
        self.obs_dim, self.h1 = w1.shape
        self.h2, self.act_dim = w3.shape
        if w2.shape != (self.h1, self.h2) or b1.shape != (self.h1,) or b2.shape != (self.h2,) or \
                b3.shape != (self.act_dim,):
            raise _native.PbgError(f"MLPPolicy: inconsistent shapes {[a.shape for a in ws]}")
        idx = -1 if device is None else self._set_device(device, "None (host) or a GPU")
        if not hasattr(_native.lib(), "pbg_policy_create"):
            raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_policy_create: a build without the policy kernel")
        FP = ctypes.POINTER(ctypes.c_float)
        h = ctypes.c_void_p()
        _native.check(_native.lib().pbg_policy_create(idx, self.obs_dim, self.h1, self.h2, self.act_dim,
                                                      *[a.ctypes.data_as(FP) for a in ws], ctypes.byref(h)),
                      "pbg_policy_create")
        self._h = h
        self.obs_norm = None    # (mean, inv_std, clip) as numpy float32 / float, or None
        self.obs_stats = None   # the attached ObsStats, or None
        if obs_norm is not None:
            self.set_obs_norm(*obs_norm)

    @classmethod
    def from_npz(cls, path, device=None) -> "MLPPolicy":
        """Weights from an npz with the reference's names (``weights_dense1_w`` ... ``weights_final_b``), and
        the normaliser when the file holds one (``obs_mean``, ``obs_inv_std``, ``obs_clip``)."""
        with np.load(path) as z:
            norm = (z["obs_mean"], z["obs_inv_std"], float(z["obs_clip"])) if all(k in z for k in NORM_KEYS) else None
            return cls(*[z[k] for k in NPZ_KEYS], device=device, obs_norm=norm)

    def set_obs_norm(self, mean, inv_std=None, clip: float = 5.0):
        """Every later ``act`` / rollout feeds the MLP ``clip((obs - mean) * inv_std, -clip, clip)`` (float32,
        one rounding per operation); ``mean``, ``inv_std``: ``[obs_dim]`` arrays (or CPU / GPU tensors),
        copied.  ``set_obs_norm(None)`` switches the normaliser off.  Synchronises the device."""
        p = self._open("set_obs_norm")
        f = _need("pbg_policy_set_obs_norm")
        if mean is None and inv_std is None:
            _native.check(f(p, None, None, 0.0), "pbg_policy_set_obs_norm")
            self.obs_norm = None
            return
        arrs = []
        for a in (mean, inv_std):
            a = a.detach().cpu().numpy() if hasattr(a, "detach") else a
            a = np.ascontiguousarray(np.asarray(a), dtype=np.float32)
            if a.shape != (self.obs_dim,):
                raise _native.PbgError(f"MLPPolicy.set_obs_norm: mean and inv_std must have shape ({self.obs_dim},)")
            arrs.append(a.copy())
        _native.check(f(p, arrs[0].ctypes.data, arrs[1].ctypes.data, float(clip)), "pbg_policy_set_obs_norm")
        self.obs_norm = (arrs[0], arrs[1], float(clip))

    def attach_obs_stats(self, stats):
        """While an ``ObsStats`` is attached, every step of ``VecEnv.rollout`` with this policy adds its
        observations to it (``act`` never does); None detaches."""
        p = self._open("attach_obs_stats")
        _native.check(_need("pbg_policy_attach_obs_stats")(p, None if stats is None else stats._open("attach")),
                      "pbg_policy_attach_obs_stats")
        self.obs_stats = stats

    def attach_action_noise(self, noise):
        """While an ``ActionNoise`` is attached, every step of ``VecEnv.rollout`` with this policy acts
        ``mu + std * eps`` (``act`` never samples); None detaches."""
        _attach_action_noise(self, "pbg_policy_attach_action_noise", noise)

    def act(self, obs, out=None):
        """``[n, obs_dim]`` float32 observations -> ``[n, act_dim]`` actions.  Device policy: torch
        tensors on its device (``out``: an optional preallocated result, which keeps the call
        capturable).  Host policy: numpy in, numpy out."""
        p = self._open("act")
        if self.device is None:
            x = np.ascontiguousarray(obs, dtype=np.float32)
            if x.ndim != 2 or x.shape[1] != self.obs_dim:
                raise _native.PbgError(f"MLPPolicy.act: obs shape {x.shape}, expected [n, {self.obs_dim}]")
            y = np.empty((x.shape[0], self.act_dim), np.float32) if out is None else out
            if not isinstance(y, np.ndarray) or y.dtype != np.float32 or y.shape != (x.shape[0], self.act_dim) or \
                    not y.flags.c_contiguous or not y.flags.writeable:
                raise _native.PbgError(f"MLPPolicy.act: out must be a writable C-contiguous float32 array of shape "
                                       f"({x.shape[0]}, {self.act_dim})")
            _native.check(_native.lib().pbg_policy_act_host(p, x.shape[0], x.ctypes.data, y.ctypes.data),
                          "pbg_policy_act_host")
            return y
        import torch
        x = obs
        if x.dtype != torch.float32 or x.device != self.device or not x.is_contiguous():
            x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != self.obs_dim:
            raise _native.PbgError(f"MLPPolicy.act: obs shape {tuple(x.shape)}, expected [n, {self.obs_dim}]")
        y = torch.empty((x.shape[0], self.act_dim), dtype=torch.float32, device=self.device) if out is None else out
        y = self._vec(y, "act", "out", (x.shape[0], self.act_dim))
        _native.check(_native.lib().pbg_policy_act(p, x.shape[0], x.data_ptr(), y.data_ptr(), self._stream()),
                      "pbg_policy_act")
        return y


def param_count(dims) -> int:
    """D of the flat parameter vector of dims = (obs_dim, h1, h2, act_dim) (include/pbg.h)."""
    o, h1, h2, a = [int(d) for d in dims]
    return o * h1 + h1 + h1 * h2 + h2 + h2 * a + a


def pack_theta(ws) -> np.ndarray:
    """The six arrays w1, b1, w2, b2, w3, b3 -> the flat float32 ``[D]`` vector (their unpadded row-major
    concatenation, include/pbg.h "Flat parameter layout")."""
    return np.concatenate([np.ascontiguousarray(np.asarray(a), dtype=np.float32).ravel() for a in ws])


def unpack_theta(dims, theta):
    """The flat ``[D]`` vector -> the six arrays (copies) in ``MLPPolicy``'s order and shapes."""
    o, h1, h2, a = [int(d) for d in dims]
    t = np.ascontiguousarray(np.asarray(theta), dtype=np.float32)
    if t.shape != (param_count(dims),):
        raise _native.PbgError(f"unpack_theta: theta shape {t.shape}, expected ({param_count(dims)},)")
    out, at = [], 0
    for shape in ((o, h1), (h1,), (h1, h2), (h2,), (h2, a), (a,)):
        cnt = int(np.prod(shape))
        out.append(t[at:at + cnt].reshape(shape).copy())
        at += cnt
    return out


class MLPPopulation(_NativeObject):
    """``2 * n_pairs`` weight sets ("members") of one MLP shape on one GPU (include/pbg.h pbg_population_*):
    the population of an evolution strategy with mirrored sampling.  Members ``2 i`` and ``2 i + 1`` are the
    pair ``theta +- sigma eps_i``; ``pair0`` is the global index of the first pair when this object holds a
    slice of a larger population (the noise depends on the global index only).

    ``dims = (obs_dim, h1, h2, act_dim)``.  A parameter vector ("theta") is a contiguous float32 tensor of
    ``n_params`` elements on ``device``: w1, b1, w2, b2, w3, b3 concatenated (``pack_theta``).  ``act``
    and ``VecEnv.rollout`` split a batch of ``n = n_members * G`` envs into ``n_members`` consecutive
    groups of ``G``; group m runs member m.  Every method is asynchronous on the current stream and
    allocates only the results it is not handed (``out=``), so a generation captures into a HIP graph."""
    _DESTROY, _NOUN = "pbg_population_destroy", "population"
    _ROLLOUT = "pbg_rollout_population"   # VecEnv.rollout's entry point for this actor
    action_noise = None                   # the attached ActionNoise, or None

    def __init__(self, dims, n_pairs: int, device, pair0: int = 0):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 4:
            raise _native.PbgError(f"MLPPopulation: dims must be (obs_dim, h1, h2, act_dim), got {dims!r}")
        self.obs_dim, self.h1, self.h2, self.act_dim = self.dims
        self.n_pairs, self.pair0 = int(n_pairs), int(pair0)
        self.n_members = 2 * self.n_pairs
        self.n_params = param_count(self.dims)
        idx = self._set_device(device)
        if not hasattr(_native.lib(), "pbg_population_create"):
            raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_population_create: a build without populations")
        h = ctypes.c_void_p()
        _native.check(_native.lib().pbg_population_create(idx, *self.dims, self.n_pairs, self.pair0, ctypes.byref(h)),
                      "pbg_population_create")
        self._h = h
        self.obs_clip = None    # the normaliser's clip, None = no normaliser (set_obs_norm)
        self._norm = None       # this object's copies of its mean and inv_std, allocated by the first set_obs_norm
        self.obs_stats = None   # the attached ObsStats, or None

    # ------------------------------------------------------------------ normaliser
    def set_obs_norm(self, mean, inv_std=None, clip: float = 5.0):
        """Every member feeds its MLP ``clip((obs - mean) * inv_std, -clip, clip)`` from now on (stream
        order); ``mean``, ``inv_std``: contiguous float32 ``[obs_dim]`` tensors on the device, copied on the
        current stream (no host work after the first call, which allocates this object's copies for
        ``save_npz``).  ``set_obs_norm(None)`` switches the normaliser off."""
        import torch
        p = self._open("set_obs_norm")
        f = _need("pbg_population_set_obs_norm")
        if mean is None and inv_std is None:
            _native.check(f(p, None, None, 0.0, self._stream()), "pbg_population_set_obs_norm")
            self.obs_clip = None
            return
        mean = self._vec(mean, "set_obs_norm", "mean", (self.obs_dim,))
        inv_std = self._vec(inv_std, "set_obs_norm", "inv_std", (self.obs_dim,))
        _native.check(f(p, mean.data_ptr(), inv_std.data_ptr(), float(clip), self._stream()),
                      "pbg_population_set_obs_norm")
        if self._norm is None:
            self._norm = torch.empty((2, self.obs_dim), dtype=torch.float32, device=self.device)
        self._norm[0].copy_(mean)
        self._norm[1].copy_(inv_std)
        self.obs_clip = float(clip)

    @property
    def obs_norm(self):
        """``(mean, inv_std, clip)`` of the normaliser in force (device tensors, views of this object's
        copies), or None."""
        return None if self.obs_clip is None else (self._norm[0], self._norm[1], self.obs_clip)

    def attach_obs_stats(self, stats):
        """While an ``ObsStats`` (sized with ``group`` = the envs per member) is attached, every step of
        ``VecEnv.rollout`` with this population adds its observations to it; None detaches."""
        p = self._open("attach_obs_stats")
        _native.check(_need("pbg_population_attach_obs_stats")(p, None if stats is None else stats._open("attach")),
                      "pbg_population_attach_obs_stats")
        self.obs_stats = stats

    def attach_action_noise(self, noise):
        """While an ``ActionNoise`` is attached, every step of ``VecEnv.rollout`` with this population acts
        ``mu + std * eps``, the noise of an env depending on its global index only; None detaches."""
        _attach_action_noise(self, "pbg_population_attach_action_noise", noise)

    # ------------------------------------------------------------------ parameters
    def init_theta(self, seed: int = 0):
        """A fresh centre: weights N(0, 1 / fan-in), biases zero (numpy ``default_rng(seed)``), as a device
        float32 tensor ``[n_params]``."""
        import torch
        rng = np.random.default_rng(seed)
        ws = []
        for k, h in ((self.obs_dim, self.h1), (self.h1, self.h2), (self.h2, self.act_dim)):
            ws.append((rng.standard_normal((k, h)) / np.sqrt(k)).astype(np.float32))
            ws.append(np.zeros(h, np.float32))
        return torch.from_numpy(pack_theta(ws)).to(self.device)

    def perturb(self, theta, sigma: float, seed: int, generation: int):
        """members ``2 i``, ``2 i + 1`` = ``theta +- sigma * eps_i`` (float64 arithmetic, rounded once)."""
        p = self._open("perturb")
        theta = self._vec(theta, "perturb", "theta", (self.n_params,))
        _native.check(_native.lib().pbg_population_perturb(p, theta.data_ptr(), float(sigma), int(seed), int(generation),
                                                           self._stream()), "pbg_population_perturb")

    def noise(self, seed: int, generation: int, out=None):
        """``[n_pairs, n_params]`` float32: the eps of ``generation``, the bits ``perturb`` and ``grad`` use."""
        import torch
        p = self._open("noise")
        shape = (self.n_pairs, self.n_params)
        out = torch.empty(shape, dtype=torch.float32, device=self.device) if out is None else out
        out = self._vec(out, "noise", "out", shape)
        _native.check(_native.lib().pbg_population_noise(p, int(seed), int(generation), out.data_ptr(), self._stream()),
                      "pbg_population_noise")
        return out

    def grad(self, w, seed: int, generation: int, out=None):
        """``g[d] = sum_i w[i] * eps_i[d]`` (pair-ascending float64 sum, cast to float32); ``w``: float32
        ``[n_pairs]`` on the device."""
        import torch
        p = self._open("grad")
        w = self._vec(w, "grad", "w", (self.n_pairs,))
        out = torch.empty(self.n_params, dtype=torch.float32, device=self.device) if out is None else out
        out = self._vec(out, "grad", "out", (self.n_params,))
        _native.check(_native.lib().pbg_population_grad(p, w.data_ptr(), int(seed), int(generation), out.data_ptr(),
                                                        self._stream()), "pbg_population_grad")
        return out

    def fitness(self, rollout_result, out=None):
        """Per-member mean return per env, float64 ``[n_members]``: the mean over the member's envs of
        ``done_return + cur_return`` of a ``RolloutResult`` (env-ascending float64 sum / G)."""
        import torch
        p = self._open("fitness")
        cur, done = rollout_result.cur_return, rollout_result.done_return
        n = cur.shape[0] if isinstance(cur, torch.Tensor) and cur.dim() == 1 else -1
        if n < self.n_members or n % self.n_members != 0:
            raise _native.PbgError(f"MLPPopulation.fitness: {n} envs are not a positive multiple of the "
                                   f"{self.n_members} members")
        cur = self._vec(cur, "fitness", "cur_return", (n,), np.float64)
        done = self._vec(done, "fitness", "done_return", (n,), np.float64)
        out = torch.empty(self.n_members, dtype=torch.float64, device=self.device) if out is None else out
        out = self._vec(out, "fitness", "out", (self.n_members,), np.float64)
        _native.check(_native.lib().pbg_population_fitness(p, n, cur.data_ptr(), done.data_ptr(), out.data_ptr(),
                                                           self._stream()), "pbg_population_fitness")
        return out

    def set_all(self, theta):
        """Every member = ``theta`` (the centre's evaluation)."""
        self.set_member(-1, theta)

    def set_member(self, m: int, theta):
        p = self._open("set_member")
        theta = self._vec(theta, "set_member", "theta", (self.n_params,))
        _native.check(_native.lib().pbg_population_set_member(p, int(m), theta.data_ptr(), self._stream()),
                      "pbg_population_set_member")

    def get_member(self, m: int, out=None):
        """Member ``m``'s parameter vector as a device tensor."""
        import torch
        p = self._open("get_member")
        out = torch.empty(self.n_params, dtype=torch.float32, device=self.device) if out is None else out
        out = self._vec(out, "get_member", "out", (self.n_params,))
        _native.check(_native.lib().pbg_population_get_member(p, int(m), out.data_ptr(), self._stream()),
                      "pbg_population_get_member")
        return out

    def member_weights(self, m: int):
        """Member ``m`` as the six numpy arrays ``MLPPolicy`` takes (synchronises)."""
        return unpack_theta(self.dims, self.get_member(m).cpu().numpy())

    def save_npz(self, path, theta_or_member):
        """Write a parameter vector (a tensor or array ``[n_params]``) or member (an int) as an npz with the
        reference's key names: ``MLPPolicy.from_npz`` and tools/enjoy.py load it.  With a normaliser set the
        file also gets ``obs_mean``, ``obs_inv_std`` and ``obs_clip``."""
        if isinstance(theta_or_member, (int, np.integer)):
            ws = self.member_weights(int(theta_or_member))
        else:
            t = theta_or_member
            ws = unpack_theta(self.dims, t.detach().cpu().numpy() if hasattr(t, "detach") else t)
        extra = {}
        if self.obs_clip is not None:
            extra = dict(obs_mean=self._norm[0].cpu().numpy(), obs_inv_std=self._norm[1].cpu().numpy(),
                         obs_clip=np.float32(self.obs_clip))
        np.savez(path, **dict(zip(NPZ_KEYS, ws)), **extra)

    # ------------------------------------------------------------------ actor
    def act(self, obs, out=None):
        """``[n, obs_dim]`` float32 observations -> ``[n, act_dim]`` actions, ``n`` a multiple of
        ``n_members``: rows ``m G .. (m + 1) G`` (``G = n / n_members``) through member m, each row
        bit for bit what a host ``MLPPolicy`` of that member's weights computes."""
        import torch
        p = self._open("act")
        x = obs
        if not isinstance(x, torch.Tensor):
            raise _native.PbgError("MLPPopulation.act: obs must be a torch tensor")
        if x.dtype != torch.float32 or x.device != self.device or not x.is_contiguous():
            x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != self.obs_dim:
            raise _native.PbgError(f"MLPPopulation.act: obs shape {tuple(x.shape)}, expected [n, {self.obs_dim}]")
        n = x.shape[0]
        if n % self.n_members != 0:
            raise _native.PbgError(f"MLPPopulation.act: {n} rows are not a multiple of the {self.n_members} members")
        y = torch.empty((n, self.act_dim), dtype=torch.float32, device=self.device) if out is None else out
        y = self._vec(y, "act", "out", (n, self.act_dim))
        _native.check(_native.lib().pbg_population_act(p, n, x.data_ptr(), y.data_ptr(), self._stream()),
                      "pbg_population_act")
        return y

    def act_where(self, flags, obs, out=None):
        """``act`` for the flagged rows of a trajectory alone (pbg_population_act_where, one launch): ``flags`` uint8
        ``[T, n]``, ``obs`` float32 ``[T, n, obs_dim]`` -> ``out`` float32 ``[T, n, act_dim]``, contiguous tensors on
        the device, ``n`` a positive multiple of ``n_members`` (row ``(t, e)`` through member ``e // (n //
        n_members)``, the rollout's mapping).  Where the flag is set the row holds ``act``'s bits for it; elsewhere it
        is ``+0.0`` and the ``obs`` row is never read (it may be uninitialised memory, as the unwritten rows of
        ``RolloutResult.term_obs_traj`` are).  A 16-row tile without a flag returns before it touches the weights."""
        import torch
        p = self._open("act_where")
        if not hasattr(_native.lib(), "pbg_population_act_where"):
            raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_population_act_where: a build without truncation "
                                   "bootstrapping")
        if not isinstance(flags, torch.Tensor) or flags.dim() != 2:
            raise _native.PbgError("MLPPopulation.act_where: flags must be a uint8 [T, n] tensor")
        T, n = (int(d) for d in flags.shape)
        if T < 1 or n < 1 or n % self.n_members != 0:
            raise _native.PbgError(f"MLPPopulation.act_where: T = {T} must be >= 1 and n = {n} a positive multiple of the "
                                   f"{self.n_members} members")
        flags = self._vec(flags, "act_where", "flags", (T, n), np.uint8)
        obs = self._vec(obs, "act_where", "obs", (T, n, self.obs_dim))
        out = torch.empty((T, n, self.act_dim), dtype=torch.float32, device=self.device) if out is None else out
        out = self._vec(out, "act_where", "out", (T, n, self.act_dim))
        _native.check(_native.lib().pbg_population_act_where(p, T, n, flags.data_ptr(), obs.data_ptr(), out.data_ptr(),
                                                             self._stream()), "pbg_population_act_where")
        return out
