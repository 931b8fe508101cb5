"""Weighted focal statistics of a raster: a convolution primitive, std, TPI and reduce_peaks (MI355X only).

Mirrors, argument for argument, the reference functions (paths relative to the reference checkout): ``std``
(neilpy/neilpy.py:2039), ``reduce_peaks`` (:2056), ``topographic_position_index`` (:2098) and the host helper
``distance_kernel`` (:2450).  ``focal_convolve`` is this package's own name for what they all rest on,
``scipy.ndimage.convolve(X, weights, mode='nearest')``.

Every raster function is a launch or a few of the tap kernel family of ``csrc/focal.hip`` (``smrf_focal_*``), which
accumulates the non-zero weights in ndimage's order, one fp64 multiply and one fp64 add per tap, and so gives ndimage's
bits; the arithmetic contract is DESIGN.md section 12.  NumPy in -> NumPy out; a CUDA tensor in -> a CUDA tensor out on
the same device.  float32 and float64 rasters keep the dtype the reference gives them (``std`` and ``reduce_peaks``
return float64, as NumPy 2 promotes them); other dtypes are widened to float64.  There is no CPU fallback: without the
library or a GPU every raster function raises :class:`neilpy_amd.SmrfHipError`.

Deviations from the reference (each in DESIGN.md section 12): integer rasters are widened to float64 where ndimage
keeps them integer; weights are taken as float64 whatever their dtype; ``topographic_position_index`` raises
``ValueError`` for a radius below 1 or not an integer; its standardising sd comes from fixed-order float64 sums where
NumPy sums pairwise in the raster's dtype.
"""
import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped
from ._raster import Raster, _ptr, _stream, _torch
from .api import disk

__all__ = ["focal_convolve", "std", "topographic_position_index", "reduce_peaks", "distance_kernel"]

TAP_DTYPE = np.dtype([("drow", "<i4"), ("dcol", "<i4"), ("w", "<f8")])


# ------------------------------------------------------------------------------------------
# host helpers
# ------------------------------------------------------------------------------------------
def distance_kernel(radius, cellsize=1, method='binary', idw_power=2):
    """Square window of odd width ``round(2 * radius / cellsize)`` (made odd by adding 1) holding each cell's distance
    D from the centre in cells ('distance', or any unknown method), ``D < radius / cellsize`` ('binary') or
    ``1 / D**idw_power`` ('idw').  Same arguments and results as neilpy.distance_kernel."""
    radius_in_pixels = radius / cellsize
    window = (np.round(2 * radius_in_pixels)).astype(int)
    if window % 2 == 0:
        window = window + 1
    offs = np.arange(window) - np.floor(window / 2)
    xi, yi = np.meshgrid(offs, offs)
    D = (xi ** 2 + yi ** 2) ** .5
    if method == 'idw':
        return 1 / D ** idw_power
    if method == 'binary':
        return D < radius / cellsize
    return D


def _weights(w):
    w = np.asarray(w)
    if w.ndim != 2 or w.size == 0:
        raise ValueError("expected a 2-D kernel of at least 1 x 1")
    return np.ascontiguousarray(w, dtype=np.float64)


def _taps(weights):
    """The non-zero weights of a KH x KW kernel as (drow, dcol, w) records in ndimage's order: s = KH-1 .. 0 outer,
    t = KW-1 .. 0 inner, the tap reading X[i + KH//2 - s, j + KW//2 - t]."""
    w = _weights(weights)
    kh, kw = w.shape
    s, t = np.nonzero(w[::-1, ::-1] != 0)           # row-major order of the flipped kernel
    s, t = kh - 1 - s, kw - 1 - t
    taps = np.empty(len(s), dtype=TAP_DTYPE)
    taps["drow"] = kh // 2 - s
    taps["dcol"] = kw // 2 - t
    taps["w"] = w[s, t]
    return taps


# ------------------------------------------------------------------------------------------
# the launch
# ------------------------------------------------------------------------------------------
def _workspace(R):
    n = _lib.load().smrf_focal_workspace_bytes(R.rows, R.cols)
    return _torch().empty(max(n // 8, 4), dtype=_torch().float64, device=R.t.device)


def _launch(R, mode, weights, outs, S=0.0, sub=None, ws=None, impl=_lib.FOCAL_IMPL_AUTO):
    """one launch of smrf_focal_* over ``R``, a Raster or (for callers that hold only the plane) a CUDA tensor"""
    if not isinstance(R, Raster):
        R = Raster(R)
    w = _weights(weights)
    taps = _taps(w)
    tab = _torch().from_numpy(taps.view(np.uint8)).to(R.t.device) if len(taps) else None
    o = list(outs) + [None] * (2 - len(outs))
    R.call("focal", _ptr(R.t), _ptr(sub), R.rows, R.cols, mode, _ptr(tab), len(taps), w.shape[0], w.shape[1], float(S),
           _ptr(o[0]), _ptr(o[1]), _ptr(ws), 0 if ws is None else ws.numel() * 8, int(impl))
    # the tap table is freed by the caching allocator on this stream only after the launch has read it


# ------------------------------------------------------------------------------------------
# public raster functions
# ------------------------------------------------------------------------------------------
@_device_scoped
def focal_convolve(X, weights, *, impl=_lib.FOCAL_IMPL_AUTO):
    """``scipy.ndimage.convolve(X, weights, mode='nearest')`` for a 2-D raster and a kernel of any size from 1 x 1,
    bit for bit: the non-zero weights are accumulated in float64 in ndimage's order and the sum is rounded to the
    raster's dtype.  ``impl`` forces the tiled or the direct kernel path (same bits)."""
    w = _weights(weights)
    R = Raster(X)
    out = R.empty()
    _launch(R, _lib.FOCAL_SUM, w, [out], impl=impl)
    return R.out(out)


def _std(R, strel, sub=None, impl=_lib.FOCAL_IMPL_AUTO):
    out = R.empty(_torch().float64)
    _launch(R, _lib.FOCAL_STD, strel, [out], S=float(np.sum(strel)), sub=sub, impl=impl)
    return out


@_device_scoped
def std(X, strel, *, impl=_lib.FOCAL_IMPL_AUTO):
    """Weighted focal standard deviation from the convolutions of X and X**2 with ``strel``, negatives clamped to 0
    before the root; float64.  One launch: both sums come from one read and no intermediate raster is written.  Same
    arguments and results as neilpy.std."""
    strel = np.asarray(strel)
    _weights(strel)
    R = Raster(X)
    return R.out(_std(R, strel, impl=impl))


@_device_scoped
def topographic_position_index(X, radius=1, standardize=True, *, impl=_lib.FOCAL_IMPL_AUTO):
    """The cell minus the mean of its neighbourhood (a 3 x 3 square for radius 1, otherwise ``disk(radius)``, centre
    excluded), divided by ``sqrt(mean(conv(X**2)) - mean(result)**2)`` when ``standardize``.  Same arguments and
    results as neilpy.topographic_position_index; a radius below 1 or not an integer raises ``ValueError``."""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or radius < 1:
        raise ValueError("radius must be an integer of at least 1, got %r" % (radius,))
    radius = int(radius)
    strel = np.ones((3, 3), dtype=np.uint8) if radius == 1 else disk(radius)
    strel[radius, radius] = 0
    strel = strel / np.sum(strel)
    R = Raster(X)
    out = R.empty()
    if R.t.numel():
        ws = _workspace(R)
        _launch(R, _lib.FOCAL_TPI, strel, [out], ws=ws, impl=impl)
        if standardize:
            R.call("focal_divide", _ptr(out), out.numel(), _ptr(ws[2:]))
    return R.out(out)


@_device_scoped
def reduce_peaks(Z, radius, blend_rate=2, kernel_rate='auto', *, impl=_lib.FOCAL_IMPL_AUTO):
    """Blend Z with its distance-weighted focal mean M, drawing more from Z where the focal standard deviation of
    Z - M is low: ``(1 - V)*M + V*Z`` with ``V = (1 - normalize(STD))**blend_rate``; float64.  Same arguments and
    results as neilpy.reduce_peaks."""
    if isinstance(kernel_rate, str) and kernel_rate == 'auto':
        kernel_rate = 1 / blend_rate
    strel = distance_kernel(radius, method='distance')
    strel = 1 - (strel / np.max(strel))
    strel = strel ** kernel_rate
    R = Raster(Z)
    out = R.empty(_torch().float64)
    if R.t.numel():
        M = R.empty()
        _launch(R, _lib.FOCAL_SUM, strel / np.sum(strel), [M], impl=impl)
        STD = _std(R, strel, sub=M, impl=impl)
        ws = _workspace(R)
        _lib.check(_lib.load().smrf_focal_minmax_f64(_ptr(STD), STD.numel(), _ptr(ws), ws.numel() * 8, _stream()))
        R.call("focal_mix", _ptr(R.t), _ptr(M), _ptr(STD), _ptr(ws), float(blend_rate), _ptr(out), out.numel())
    return R.out(out)
