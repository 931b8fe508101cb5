"""A point cloud as a boolean voxel model (MI355X only).

``voxelize`` mirrors the reference function of that name (neilpy/neilpy.py:195 of the reference checkout): the cloud is
moved to its minimum corner, binned with ``np.histogramdd`` over ``resolution`` cells along the longer of x and y (z cells
``ve`` times finer), a voxel is set where at least ``threshold`` points fell, every column is filled below its lowest set
voxel, and ``pad`` solid layers go under the model.  Here the minima and maxima are one device reduction, the bin edges
are formed on the host by the reference's own expressions, and the points are scattered into a bit set (or, for
``threshold > 1``, into integer counts) and expanded to bytes by the kernels of ``csrc/voxel.hip`` (``smrf_voxel_*``).
The result equals the reference's bit for bit; the contract is DESIGN.md section 15.

NumPy in -> NumPy ``bool`` out; CUDA tensors in -> a ``torch.bool`` CUDA tensor on their device, with no host copy of the
cloud.  There is no CPU fallback: without the library or a GPU it raises :class:`neilpy_amd.SmrfHipError`.

Deviations from the reference: ``filename`` must be ``None`` (the mesh export goes through
``voxelfuse``, which is no part of this package) and ``material`` is accepted and unused; x, y and z of different float
dtypes are widened to float64 first; and these are ``ValueError``: ``resolution``, ``threshold`` < 1 or ``pad`` < 0 or
not integers, ``ve`` <= 0 or not finite, arrays that are not 1-D or differ in length, an empty cloud, more than
2**31 - 1 points (all raised before the device is touched), a NaN or infinite coordinate, and a cloud whose x and y
extents are both 0 (both found by the reduction that finds the extents).
"""
import ctypes as C
import math
import operator

import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._xfer import to_device as _h2d, to_host as _d2h
from ._raster import _ptr, _stream, _suffix, _to_device, _torch

__all__ = ["voxelize"]

MAX_POINTS = 2 ** 31 - 1
BOUNDS_BYTES = 57344          # SMRF_VOXEL_BOUNDS_BYTES of include/smrf_hip.h


def _integer(value, name, least):
    try:
        v = operator.index(value)
    except TypeError:
        raise ValueError("%s must be an integer, got %r" % (name, value)) from None
    if v < least:
        raise ValueError("%s must be at least %d, got %d" % (name, least, v))
    return v


def _parameters(resolution, threshold, ve, pad):
    """the scalar arguments as Python numbers (a NumPy scalar would change the promotion of a float32 cloud's edges)"""
    resolution = _integer(resolution, "resolution", 1)
    threshold = _integer(threshold, "threshold", 1)
    pad = _integer(pad, "pad", 0)
    try:
        ve = float(ve)
    except (TypeError, ValueError):
        raise ValueError("ve must be a number, got %r" % (ve,)) from None
    if not (math.isfinite(ve) and ve > 0):
        raise ValueError("ve must be positive and finite, got %r" % (ve,))
    return resolution, threshold, ve, pad


def _length(x, y, z):
    """the common length of the three coordinate arrays, from their shapes alone"""
    shapes = [tuple(a.shape) if _is_tensor(a) else np.shape(a) for a in (x, y, z)]
    for name, s in zip("xyz", shapes):
        if len(s) != 1:
            raise ValueError("%s: expected a 1-D array of coordinates, got shape %s" % (name, (s,)))
    if not shapes[0] == shapes[1] == shapes[2]:
        raise ValueError("x, y and z differ in length: %d, %d, %d" % (shapes[0][0], shapes[1][0], shapes[2][0]))
    n = shapes[0][0]
    if n == 0:
        raise ValueError("empty cloud")
    if n > MAX_POINTS:
        raise ValueError("%d points are more than one call takes (2**31 - 1)" % n)
    return n


def _is_float32(a):
    if _is_tensor(a):
        return a.dtype == _torch().float32
    return getattr(a, "dtype", None) == np.float32 or np.asarray(a).dtype == np.float32


def bin_edges(box, dtype, resolution, ve):
    """``((xbins, ybins, zbins), (min_x, min_y, min_z))`` from the cloud's box ``(min_x, max_x, min_y, max_y, min_z,
    max_z)``: the reference's expressions on NumPy scalars of ``dtype``.  ``max(v - min)`` is ``max(v) - min`` rounded once
    (rounding is monotone), so the box of the raw values is enough."""
    T = np.dtype(dtype).type
    mins = tuple(T(box[2 * a]) for a in range(3))
    max_x, max_y, max_z = (T(box[2 * a + 1]) - mins[a] for a in range(3))
    if not (max_x > 0 or max_y > 0):
        raise ValueError("the cloud has no extent in x and y: the voxel size would be 0")
    if max_x > max_y:
        interval = np.ceil(max_x) / resolution
    else:
        interval = np.ceil(max_y) / resolution
    xbins = np.arange(0, np.ceil(max_x) + interval, interval)
    ybins = np.arange(0, np.ceil(max_y) + interval, interval)
    zbins = np.arange(0, np.ceil(max_z) + interval / ve, interval / ve)
    return tuple(np.asarray(b, dtype=np.float64) for b in (xbins, ybins, zbins)), mins


@_device_scoped
def voxelize(filename, x, y, z, resolution, bottom_fill=True, threshold=1, material=0, ve=1, pad=0, *,
             return_edges=False):
    """Boolean voxel model of the cloud ``x``, ``y``, ``z`` (1-D, equal length); same arguments and result as
    neilpy.voxelize with ``filename=None``: a ``bool`` array of shape ``(nx, ny, nz + pad)``, C order.  ``resolution``:
    voxels along the longer of x and y; ``bottom_fill``: fill every column below its lowest occupied voxel;
    ``threshold``: points a voxel needs; ``ve``: vertical exaggeration, the z cells are ``1 / ve`` of the x and y cells;
    ``pad``: solid layers put under the model.  ``return_edges=True`` returns ``(H, (xbins, ybins, zbins), (min_x, min_y,
    min_z))``: the float64 bin edges that were used and the offsets that were subtracted first, so that voxel
    ``H[i, j, pad + k]`` spans ``min_x + xbins[i] .. min_x + xbins[i + 1]`` and so on."""
    if filename is not None:
        raise NotImplementedError("voxelize(filename=%r): the mesh export is no part of neilpy_amd; pass None and export "
                                  "the returned array" % (filename,))
    resolution, threshold, ve, pad = _parameters(resolution, threshold, ve, pad)
    n = _length(x, y, z)
    torch = _torch()
    was_tensor = _is_tensor(x)
    dtype = torch.float32 if all(_is_float32(a) for a in (x, y, z)) else torch.float64
    tx, ty, tz = (_to_device(a, dtype) for a in (x, y, z))
    lib = _lib.load()
    sfx = _suffix(tx)
    dev = tx.device

    small = torch.empty(BOUNDS_BYTES, dtype=torch.uint8, device=dev)
    box = (C.c_double * 6)()
    bad = C.c_int64(0)
    _lib.check(getattr(lib, "smrf_voxel_bounds_" + sfx)(_ptr(tx), _ptr(ty), _ptr(tz), n, box, C.byref(bad), _ptr(small),
                                                        BOUNDS_BYTES, _stream()))
    if bad.value:
        raise ValueError("%d coordinates are NaN or infinite" % bad.value)
    edges, mins = bin_edges(list(box), np.float32 if dtype == torch.float32 else np.float64, resolution, ve)
    nx, ny, nz = (len(e) - 1 for e in edges)
    nbytes = lib.smrf_voxel_workspace_bytes(nx, ny, nz, threshold)
    if nbytes == 0 or nz + pad > 2 ** 31 - 1 or nx * ny * (nz + pad) > 2 ** 42:
        raise ValueError("a volume of %d x %d x %d voxels is more than one call takes" % (nx, ny, nz + pad))

    H = torch.empty((nx, ny, nz + pad), dtype=torch.bool, device=dev)
    if H.numel():
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d_edges = [_h2d(e, dev) for e in edges]
        offsets = (C.c_double * 3)(*[float(m) for m in mins])
        _lib.check(getattr(lib, "smrf_voxel_mark_" + sfx)(_ptr(tx), _ptr(ty), _ptr(tz), n, offsets, _ptr(d_edges[0]),
                                                          _ptr(d_edges[1]), _ptr(d_edges[2]), nx, ny, nz, threshold,
                                                          _ptr(ws), nbytes, _stream()))
        _lib.check(lib.smrf_voxel_expand(_ptr(ws), nbytes, nx, ny, nz, threshold, 1 if bottom_fill else 0, pad, _ptr(H),
                                         _stream()))
    out = H if was_tensor else _d2h(H)
    if return_edges:
        return out, edges, mins
    return out
