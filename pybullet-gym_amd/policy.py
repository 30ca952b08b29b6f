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


class MLPPolicy:
    """obs -> h1 -> h2 -> act, ReLU on the hidden layers, float32.

    ``w1 [obs_dim, h1]``, ``b1 [h1]``, ``w2 [h1, h2]``, ``b2 [h2]``, ``w3 [h2, act_dim]``,
    ``b3 [act_dim]``: numpy arrays (or anything ``np.asarray`` takes), the reference's layout.
    ``device``: None = a host policy (``act`` takes and returns numpy, no GPU needed); a torch device
    (``"cuda:0"``) = the weights live there and ``act`` takes and returns torch tensors on it.
    Dims: 1..256 for obs_dim / h1 / h2, 1..64 for act_dim, no multiple of anything required."""

    def __init__(self, w1, b1, w2, b2, w3, b3, device=None):
        ws = [np.ascontiguousarray(np.asarray(a), dtype=np.float32) for a in (w1, b1, w2, b2, w3, b3)]
        w1, b1, w2, b2, w3, b3 = ws
        if w1.ndim != 2 or w2.ndim != 2 or w3.ndim != 2 or b1.ndim != 1 or b2.ndim != 1 or b3.ndim != 1:
            raise _native.PbgError("MLPPolicy: weights must be 2-d and biases 1-d")
        self.obs_dim, self.h1 = w1.shape
        self.h2, self.act_dim = w3.shape
        if w2.shape != (self.h1, self.h2) or b1.shape != (self.h1,) or b2.shape != (self.h2,) or \
                b3.shape != (self.act_dim,):
            raise _native.PbgError(f"MLPPolicy: inconsistent shapes {[a.shape for a in ws]}")
        self.device = None
        idx = -1
        if device is not None:
            import torch
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise _native.PbgError(f"MLPPolicy: device must be None (host) or a GPU, got {device!r}")
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.device = torch.device("cuda", idx)
        if not hasattr(_native.lib(), "pbg_policy_create"):
            raise _native.PbgError(f"{_native.LIB_PATH} has no pbg_policy_create: a build without the policy kernel")
        FP = ctypes.POINTER(ctypes.c_float)
        h = ctypes.c_void_p()
        _native.check(_native.lib().pbg_policy_create(idx, self.obs_dim, self.h1, self.h2, self.act_dim,
                                                      *[a.ctypes.data_as(FP) for a in ws], ctypes.byref(h)),
                      "pbg_policy_create")
        self._p = h

    @classmethod
    def from_npz(cls, path, device=None) -> "MLPPolicy":
        """Weights from an npz with the reference's names (``weights_dense1_w`` ... ``weights_final_b``)."""
        with np.load(path) as z:
            return cls(*[z[k] for k in NPZ_KEYS], device=device)

    def close(self):
        if getattr(self, "_p", None):
            _native.lib().pbg_policy_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def act(self, obs, out=None):
        """``[n, obs_dim]`` float32 observations -> ``[n, act_dim]`` actions.  Device policy: torch
        tensors on its device (``out``: an optional preallocated result, which keeps the call
        capturable).  Host policy: numpy in, numpy out."""
        if not self._p:
            raise _native.PbgError("MLPPolicy.act: the policy is closed")
        if self.device is None:
            x = np.ascontiguousarray(obs, dtype=np.float32)
            if x.ndim != 2 or x.shape[1] != self.obs_dim:
                raise _native.PbgError(f"MLPPolicy.act: obs shape {x.shape}, expected [n, {self.obs_dim}]")
            y = np.empty((x.shape[0], self.act_dim), np.float32) if out is None else out
            if not isinstance(y, np.ndarray) or y.dtype != np.float32 or y.shape != (x.shape[0], self.act_dim) or \
                    not y.flags.c_contiguous or not y.flags.writeable:
                raise _native.PbgError(f"MLPPolicy.act: out must be a writable C-contiguous float32 array of shape "
                                       f"({x.shape[0]}, {self.act_dim})")
            _native.check(_native.lib().pbg_policy_act_host(self._p, x.shape[0], x.ctypes.data, y.ctypes.data),
                          "pbg_policy_act_host")
            return y
        import torch
        x = obs
        if x.dtype != torch.float32 or x.device != self.device or not x.is_contiguous():
            x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != self.obs_dim:
            raise _native.PbgError(f"MLPPolicy.act: obs shape {tuple(x.shape)}, expected [n, {self.obs_dim}]")
        y = torch.empty((x.shape[0], self.act_dim), dtype=torch.float32, device=self.device) if out is None else out
        if not isinstance(y, torch.Tensor) or y.dtype != torch.float32 or y.device != self.device or \
                not y.is_contiguous() or tuple(y.shape) != (x.shape[0], self.act_dim):
            raise _native.PbgError(f"MLPPolicy.act: out must be a contiguous float32 tensor of shape "
                                   f"({x.shape[0]}, {self.act_dim}) on {self.device}")
        _native.check(_native.lib().pbg_policy_act(self._p, x.shape[0], x.data_ptr(), y.data_ptr(),
                                                   torch.cuda.current_stream(self.device).cuda_stream),
                      "pbg_policy_act")
        return y
