"""Shared by the uninitialised-memory invariance tests: the three poison patterns of
tests/test_gpu.py's test_uninitialised_memory_invariance, the poison itself (every CU's LDS, an env handle's
workspace, every SIMD's register file), the witness that reads back what a workgroup finds in its LDS, and the
bitwise comparison.

A kernel that reads a word it did not write in that launch computes from the pattern: its result then differs
between the patterns, while two plain runs (or a run on a side stream, or a replayed graph) see the same stale
state twice and agree."""
import ctypes
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGPR_LIB = os.path.join(REPO, "tools", "libvgpr_poison.so")

# (LDS and workspace pattern, register-file base): a float NaN (a double NaN too when paired) with a NaN high
# word in the registers, zero, and 0x5A5A5A5A (a finite float, 1.5e16) with 1.0's high word.  Register i of every
# SIMD holds base | i (VGPRs) or base | 0x100 | i (AGPRs), tools/vgpr_poison.hip
PATTERNS = ((0x7FC00000, 0x7FF80000), (0x00000000, 0x00000000), (0x5A5A5A5A, 0x3FF00000))
RUNS = (None,) + PATTERNS   # an invariance case: once unpoisoned, once under each pattern


@functools.lru_cache(maxsize=None)
def _vgpr_lib():
    assert os.path.exists(VGPR_LIB), "tools/libvgpr_poison.so: run __graft_entry__.build()"
    L = ctypes.CDLL(VGPR_LIB)
    L.vgpr_poison.argtypes = [ctypes.c_uint32, ctypes.c_int]
    return L


def poison(handle, pat, reg, device="cuda:0"):
    """pbg_debug_poison (``handle``: an env's ``_h``, whose workspace is filled too; None: the LDS alone), a
    synchronize, then the register-file poison: what test_uninitialised_memory_invariance does before each step."""
    import torch
    from pybulletgym_amd import _native
    from pybulletgym_amd.vec_env import _stream
    dev = torch.device(device)
    with torch.cuda.device(dev):
        _native.check(_native.lib().pbg_debug_poison(handle, pat, _stream(dev)), "pbg_debug_poison")
        torch.cuda.synchronize()
        assert _vgpr_lib().vgpr_poison(reg, 8192) == 0


def poison_run(run, handle=None, device="cuda:0"):
    """``poison`` for an element of RUNS: nothing for the unpoisoned run."""
    if run is not None:
        poison(handle, run[0], run[1], device)


def surrounded(a, run, device="cuda:0", pad=64, shift=0):
    """The array ``a`` (numpy) on the device inside a larger buffer: at least ``pad`` elements, and for an array
    of rows at least one whole row, before and after it, every byte of them from the run's pattern word repeated
    (the unpoisoned run takes the NaN pattern).  ``shift``: further elements in front (1 breaks the 16-byte
    alignment).  Returns the contiguous view of ``a``'s shape and dtype."""
    import torch
    a = np.ascontiguousarray(a)
    word = PATTERNS[0][0] if run is None else run[0]
    row = int(np.prod(a.shape[1:])) if a.ndim > 1 else 1
    # whole rows, in bytes; a multiple of 16 rows, so that the array is as aligned as at the head of an allocation
    pad = -(-max(pad, row) // (16 * row)) * 16 * row * a.itemsize
    lo = pad + shift * a.itemsize
    raw = np.resize(np.frombuffer(np.uint32(word).tobytes(), np.uint8), lo + a.nbytes + pad)
    raw[lo:lo + a.nbytes] = a.reshape(-1).view(np.uint8)
    buf = torch.from_numpy(raw).to(device)
    view = buf[lo:lo + a.nbytes].view(torch.from_numpy(a[:0].copy()).dtype).view(a.shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + lo
    return view


class Guarded:
    """An output of ``shape`` on the device between ``GUARD`` guard elements on either side: NaN for the float types,
    -7 for the integer ones."""
    GUARD = 64

    def __init__(self, shape, dtype, device="cuda:0", shift=0, init=None):
        """``shift``: further guard elements in front (1 breaks the 16-byte alignment); ``init``: a numpy array
        the output starts as (an array updated in place), default the guards' value."""
        import torch
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape))
        self.mark = float("nan") if dtype.is_floating_point else -7
        self.lo = self.GUARD + shift
        self.full = torch.full((self.lo + n + self.GUARD,), self.mark, dtype=dtype, device=device)
        self.view = self.full[self.lo:self.lo + n].view(shape)
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(device))

    def numpy(self, what=""):
        """The output as numpy after checking that the guards are as they were."""
        import torch
        g = torch.cat((self.full[:self.lo], self.full[self.full.shape[0] - self.GUARD:]))
        ok = torch.isnan(g).all() if self.full.dtype.is_floating_point else (g == self.mark).all()
        assert bool(ok), f"{what}: a guard element was written"
        return self.view.cpu().numpy()


def bits(a):
    """A numpy array (or a tensor) as unsigned words: float32 as uint32, float64 as uint64, the rest as it is."""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view({np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}.get(a.dtype, a.dtype))


def assert_same_bits(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if not np.array_equal(g, w):
        at = np.argwhere(g != w)
        i = tuple(int(k) for k in at[0])
        raise AssertionError(f"{what}: {at.shape[0]} of {g.size} words differ, the first at {i}: "
                             f"{int(g[i]):#x} against {int(w[i]):#x}")


def assert_runs_agree(runs, what=""):
    """``runs``: per element of RUNS a dict of arrays; every array of every poisoned run must be the unpoisoned
    run's bits."""
    assert len(runs) == len(RUNS)
    for run, other in zip(RUNS[1:], runs[1:]):
        assert set(other) == set(runs[0])
        for k in runs[0]:
            assert_same_bits(other[k], runs[0][k], f"{what} {k} under pattern {run[0]:#010x}")


def lds_peek(words_per_wg, n_wg, device="cuda:0"):
    """The first ``words_per_wg`` words of LDS that each of ``n_wg`` workgroups finds (pbgdt_lds_peek_dev of the
    test-only library), uint32 ``[n_wg, words_per_wg]``."""
    import torch
    import devmath
    out = torch.zeros((n_wg, words_per_wg), dtype=torch.int32, device=device)
    with torch.cuda.device(torch.device(device)):
        rc = devmath.lib().pbgdt_lds_peek_dev(ctypes.c_void_p(out.data_ptr()), ctypes.c_int(words_per_wg), ctypes.c_int(n_wg),
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)
