"""The array boundary of the raster functions: NumPy or tensor in, a contiguous device tensor for the kernels, the same
kind of array back out.

The general helpers (``_torch``, ``_stream``, ``_ptr``, ``_to_device``, ``_suffix``) serve every module of the package;
:class:`Raster` is what the raster families (surface, focal, terrain, morphometry, nearest and the disk filters of
``api``) build from their first argument.  torch is imported on first use, not with the package.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._device import is_tensor as _is_tensor
from ._xfer import to_device as _h2d, to_host as _d2h


def _torch():
    import torch
    return torch


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _to_device(a, dtype=None):
    """NumPy / tensor -> contiguous CUDA tensor (float32 and float64 kept, others -> float64)."""
    torch = _torch()
    _lib.require_gpu()
    if _is_tensor(a):
        t = a
    else:
        arr = np.asarray(a)
        if dtype is None and arr.dtype not in (np.float32, np.float64):
            arr = arr.astype(np.float64)
        t = _h2d(arr)                                      # pinned staging for large arrays
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if not t.is_cuda:
        t = t.cuda()
    return t.contiguous()


def _suffix(t):
    return "f32" if t.dtype == _torch().float32 else "f64"


def _pyfloat(v):
    """a parameter as a Python float (NumPy scalars included: they would otherwise promote float32 rasters)"""
    return float(v)


def _need_2d(X):
    """the one 2-D rule, made on the argument's shape before the device is touched"""
    if (X.dim() if _is_tensor(X) else len(np.shape(X))) != 2:
        raise ValueError("expected a 2-D raster")


class Raster:
    """A function's raster argument on the device: ``t`` (contiguous CUDA, float32 or float64 unless ``dtype`` is
    given), its ``rows`` and ``cols``, and whether the caller passed a tensor."""

    __slots__ = ("was_tensor", "t", "rows", "cols")

    def __init__(self, X, dtype=None):
        self.was_tensor = _is_tensor(X)
        if (X.dim() if self.was_tensor else len(np.shape(X))) != 2:     # _need_2d, with the one look at X's kind
            raise ValueError("expected a 2-D raster")
        self.t = _to_device(X, dtype)
        self.rows, self.cols = self.t.shape

    def empty(self, dtype=None):
        """an uninitialised plane of the raster's shape, in the raster's dtype unless one is given"""
        return _torch().empty((self.rows, self.cols), dtype=dtype or self.t.dtype, device=self.t.device)

    def out(self, t):
        """a result as the caller's kind of array: the tensor itself, or its NumPy copy"""
        return t if self.was_tensor else _d2h(t)

    def call(self, stem, *args):
        """``smrf_<stem>_<f32|f64>(*args, stream)`` with the status checked; nothing is launched on an empty raster"""
        if self.rows == 0 or self.cols == 0:
            return
        fn = getattr(_lib.load(), "smrf_" + stem + "_" + _suffix(self.t))
        _lib.check(fn(*args, _stream()))
