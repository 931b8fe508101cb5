"""Multi-scale terrain tools built on ``ashift(surface, direction, n)`` (MI355X only).

Mirrors the reference functions (paths relative to the reference checkout): ``scaled_morphometry``
(neilpy/neilpy.py:2472), ``vip_score`` (:1832), ``ashift`` (:1290) and the host helper ``triangle_height`` (:1818).

Every raster function is one launch of the strided stencil kernels of ``csrc/morphometry.hip`` (``smrf_morphometry_*``,
``smrf_vip_*``, ``smrf_ashift_*``).  One sampling rule, ashift's: a neighbour whose row or column is off the raster is
the cell itself.  The arithmetic contract is DESIGN.md section 13.  NumPy in -> NumPy out; a CUDA tensor in -> a CUDA
tensor out on the same device.  float32 and float64 rasters keep their dtype (``vip_score`` is float64, as NumPy 2
promotes it); other dtypes are widened to float64.  There is no CPU fallback: without the library or a GPU every raster
function raises :class:`neilpy_amd.SmrfHipError`.

Deviations from the reference (each in DESIGN.md section 13): ``lookup_pixels`` and ``n`` must be integers >= 1
(``ValueError`` otherwise, before the device is touched); a NumPy-scalar ``cellsize`` is taken as a Python float; the
process's ``np.seterr`` state is left alone.
"""
import numpy as np

from ._device import device_scoped as _device_scoped
from ._raster import Raster, _ptr, _pyfloat, _torch

__all__ = ["scaled_morphometry", "vip_score", "ashift", "triangle_height"]

KEYS = ("A", "S", "K", "K_profile", "K_cross", "K_long", "K_tan", "K_plan")
_INT_MAX = 2 ** 31 - 1


def _stride(n, name):
    """an integer >= 1 (the reference fails on 0 and on floats, and scrambles the raster on negatives)"""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("%s must be an integer >= 1, got %r" % (name, n))
    return min(int(n), _INT_MAX)    # a stride beyond the raster is "every sample is the cell", whatever its value


# ------------------------------------------------------------------------------------------
# host helper
# ------------------------------------------------------------------------------------------
def triangle_height(h0, h1, x_dist=1):
    """Height above its base of the triangle (-x_dist, h0), (0, 0), (x_dist, h1), for 1-D arrays of heights relative
    to the centre: twice the area (the 2-D cross product, written out: np.cross of 2-vectors is deprecated) over the
    base.  Same arguments and bits as neilpy.triangle_height."""
    n = np.shape(h0)
    a = np.column_stack((-x_dist * np.ones(n), h0))
    b = np.column_stack((x_dist * np.ones(n), h1))
    cp = np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])
    base = np.sqrt((2 * x_dist) ** 2 + (b[:, 1] - a[:, 1]) ** 2)
    return cp / base


# ------------------------------------------------------------------------------------------
# raster functions
# ------------------------------------------------------------------------------------------
@_device_scoped
def scaled_morphometry(X, cellsize=1, lookup_pixels=1, *, outputs=None):
    """Wood's (1991) quadratic through the nine samples ``lookup_pixels`` cells apart: a dict of aspect ``A`` and slope
    ``S`` (degrees) and the curvatures ``K``, ``K_profile``, ``K_cross``, ``K_long``, ``K_tan``, ``K_plan``, in that
    order.  ``outputs`` (an iterable of those keys) limits what is computed and returned.  No NaN repair: flats give
    NaN in the five ratio curvatures.  Same arguments and results as neilpy.scaled_morphometry."""
    n = _stride(lookup_pixels, "lookup_pixels")
    if outputs is None:
        want = KEYS
    else:
        asked = [outputs] if isinstance(outputs, str) else list(outputs)
        for k in asked:
            if k not in KEYS:
                raise ValueError("unknown output %r (one of %s)" % (k, list(KEYS)))
        want = tuple(k for k in KEYS if k in asked)
    L = _pyfloat(cellsize) * int(lookup_pixels)
    div = (6 * L ** 2, 3 * L ** 2, 4 * L ** 2, 6 * L)
    R = Raster(X)
    planes = {k: R.empty() for k in want}
    if want:
        R.call("morphometry", _ptr(R.t), R.rows, R.cols, n, *div, *[_ptr(planes.get(k)) for k in KEYS])
    return {k: R.out(planes[k]) for k in want}


@_device_scoped
def vip_score(Z, cellsize=1):
    """"Very important points" score: the mean over the four lines through a cell (two axes, two diagonals) of the
    cell's height above the line joining its two neighbours (``triangle_height``).  float64, of Z's shape.  Same
    arguments and results as neilpy.vip_score."""
    cs = _pyfloat(cellsize)
    dlist = np.array([np.sqrt(2), 1])
    x = [dlist[k] * cs for k in (0, 1)]
    b2 = [(2 * v) ** 2 for v in x]          # a NumPy float64 scalar power: C pow, as the reference's
    R = Raster(Z)
    H = R.empty(_torch().float64)
    R.call("vip", _ptr(R.t), R.rows, R.cols, float(x[0]), float(x[1]), float(b2[0]), float(b2[1]), _ptr(H))
    return R.out(H)


@_device_scoped
def ashift(surface, direction, n=1):
    """A copy of the raster in which every cell holds its neighbour ``n`` cells away in ``direction`` (0 upper left,
    clockwise to 7 left), or itself where that neighbour is off the raster; any other direction is a plain copy.  Same
    arguments and results as neilpy.ashift."""
    n = _stride(n, "n")
    d = next((k for k in range(8) if direction == k), -1)
    R = Raster(surface)
    out = R.empty()
    R.call("ashift", _ptr(R.t), R.rows, R.cols, d, n, _ptr(out))
    return R.out(out)
