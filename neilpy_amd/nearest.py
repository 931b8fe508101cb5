"""Nearest-cell infill of a raster and the feature transform behind it (MI355X only).

``inpaint_nearest`` mirrors the reference function of that name (neilpy/neilpy.py:1277 of the reference checkout): every
cell that is not finite takes the value of the nearest finite cell, in place.  ``nearest_source`` returns what the kernels
compute on the way, the exact Euclidean distance to that cell and its (row, column), in the argument layout of
``scipy.ndimage.distance_transform_edt``.

Both run the separable integer feature transform of ``csrc/nearest.hip`` (``smrf_nearest_*``); the contract - holes,
squared distances as exact integers, the tie rule (lowest row, then lowest column) - is DESIGN.md section 11.  NumPy in
-> the same NumPy array filled; a CUDA tensor in -> the same tensor filled on its device.  float32 and float64 are
native.  There is no CPU fallback: without the library or a GPU both raise :class:`neilpy_amd.SmrfHipError`.

Deviations from the reference: any ``rows x cols`` shape is accepted (the reference's meshgrid
only fits square rasters); ties between equally near cells are decided by the rule above (the reference's KD-tree
leaves them to its traversal order).
"""
import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._raster import Raster, _need_2d, _ptr, _stream, _torch

__all__ = ["inpaint_nearest", "nearest_source"]


def _transform(R, out, want_index, want_dist):
    """one run of the kernels over the raster ``R``: values into ``out`` (``R.t`` itself for an in-place fill, or
    None); returns the flat int64 index plane and the uint32 squared distances asked for"""
    torch = _torch()
    index = R.empty(torch.int64) if want_index else None
    dist2 = R.empty(torch.int32) if want_dist else None   # unsigned bits
    nbytes = _lib.load().smrf_nearest_workspace_bytes(R.rows, R.cols, R.t.element_size())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=R.t.device)
    R.call("nearest", _ptr(R.t), _ptr(out), _ptr(index), _ptr(dist2), R.rows, R.cols, _ptr(ws), nbytes)
    return index, dist2


@_device_scoped
def inpaint_nearest(X):
    """Fill every non-finite cell (NaN, +-inf) of ``X`` with the value of the nearest finite cell, in place, and return
    ``X``.  Same argument and result as neilpy.inpaint_nearest; equally near cells are decided by lowest row, then
    lowest column.  A raster without a finite cell, and a dtype that cannot hold a hole, come back unchanged."""
    torch = _torch()
    if _is_tensor(X) or isinstance(X, np.ndarray):
        _need_2d(X)
    _lib.require_gpu()
    if _is_tensor(X):
        if X.dtype not in (torch.float32, torch.float64):
            if X.dtype.is_floating_point:
                raise TypeError("inpaint_nearest fills float32 and float64 tensors")
            return X                                          # no holes in an integer or bool raster
        R = Raster(X)
        in_place = X.is_cuda and X.is_contiguous()            # R.t is X's own memory
        if not in_place and R.t.data_ptr() == X.data_ptr():   # contiguous() of a contiguous view
            R.t = R.t.clone()
        _transform(R, R.t, False, False)
        if not in_place:
            X.copy_(R.t)
        return X
    if not isinstance(X, np.ndarray):
        raise TypeError("inpaint_nearest writes into its argument: pass a NumPy array or a tensor")
    if X.dtype.kind != 'f':
        return X                                              # as the reference: np.isfinite is true everywhere
    if X.dtype not in (np.float32, np.float64) and X.dtype != np.float16:
        raise TypeError("inpaint_nearest fills float16, float32 and float64 arrays")
    R = Raster(X)                                             # float16 is widened to float64: exact both ways
    _transform(R, R.t, False, False)
    X[...] = R.out(R.t)
    return X


@_device_scoped
def nearest_source(X, return_distances=True, return_indices=True):
    """For every cell of ``X`` the nearest finite cell (a finite cell is its own): the Euclidean distance in cells
    (float64, the square root of the exact integer) and / or the index array ``(2, rows, cols)`` of its row and column
    (int64), returned as ``scipy.ndimage.distance_transform_edt(~np.isfinite(X), ...)`` returns them - a tuple when
    both are asked for.  Equally near cells: lowest row, then lowest column.  Without any finite cell the distance is
    inf and the indices are -1.  ``X`` is not modified.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensors out."""
    if not return_distances and not return_indices:
        raise ValueError("at least one of return_distances / return_indices must be True")
    torch = _torch()
    R = Raster(X)
    rows, cols = R.rows, R.cols
    index, dist2 = _transform(R, None, bool(return_indices), bool(return_distances))
    dist = R.empty(torch.float64) if return_distances else None
    rc = torch.empty((2, rows, cols), dtype=torch.int64, device=R.t.device) if return_indices else None
    if rows and cols:
        _lib.check(_lib.load().smrf_nearest_planes(_ptr(index), _ptr(dist2), rows * cols, cols, _ptr(dist),
                                                   _ptr(rc[0]) if return_indices else None,
                                                   _ptr(rc[1]) if return_indices else None, _stream()))
    res = tuple(R.out(t) for t in (dist, rc) if t is not None)
    return res if len(res) == 2 else res[0]
