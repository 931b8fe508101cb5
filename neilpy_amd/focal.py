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
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._xfer import to_host as _d2h
from .api import _ptr, _stream, _suffix, _to_device, _torch, disk

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
def _raster(X):
    Xd = _to_device(X)
    if Xd.dim() != 2:
        raise ValueError("expected a 2-D raster")
    return Xd


def _out(t, was_tensor):
    return t if was_tensor else _d2h(t)


def _workspace(Xd):
    rows, cols = Xd.shape
    n = _lib.load().smrf_focal_workspace_bytes(rows, cols)
    return _torch().empty(max(n // 8, 4), dtype=_torch().float64, device=Xd.device)


def _launch(Xd, mode, weights, outs, S=0.0, sub=None, ws=None, impl=_lib.FOCAL_IMPL_AUTO):
    lib = _lib.load()
    rows, cols = Xd.shape
    if rows == 0 or cols == 0:
        return
    w = _weights(weights)
    taps = _taps(w)
    tab = _torch().from_numpy(taps.view(np.uint8)).to(Xd.device) if len(taps) else None
    o = list(outs) + [None] * (2 - len(outs))
    fn = getattr(lib, "smrf_focal_" + _suffix(Xd))
    _lib.check(fn(_ptr(Xd), _ptr(sub), rows, cols, mode, _ptr(tab), len(taps), w.shape[0], w.shape[1], float(S),
                  _ptr(o[0]), _ptr(o[1]), _ptr(ws), 0 if ws is None else ws.numel() * 8, int(impl), _stream()))
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
    was_tensor = _is_tensor(X)
    Xd = _raster(X)
    out = _torch().empty_like(Xd)
    _launch(Xd, _lib.FOCAL_SUM, w, [out], impl=impl)
    return _out(out, was_tensor)


def _std(Xd, strel, sub=None, impl=_lib.FOCAL_IMPL_AUTO):
    out = _torch().empty(Xd.shape, dtype=_torch().float64, device=Xd.device)
    _launch(Xd, _lib.FOCAL_STD, strel, [out], S=float(np.sum(strel)), sub=sub, impl=impl)
    return out


@_device_scoped
def std(X, strel, *, impl=_lib.FOCAL_IMPL_AUTO):
    """Weighted focal standard deviation from the convolutions of X and X**2 with ``strel``, negatives clamped to 0
    before the root; float64.  One launch: both sums come from one read and no intermediate raster is written.  Same
    arguments and results as neilpy.std."""
    strel = np.asarray(strel)
    _weights(strel)
    was_tensor = _is_tensor(X)
    Xd = _raster(X)
    return _out(_std(Xd, strel, impl=impl), was_tensor)


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
    was_tensor = _is_tensor(X)
    Xd = _raster(X)
    out = _torch().empty_like(Xd)
    if Xd.numel():
        ws = _workspace(Xd)
        _launch(Xd, _lib.FOCAL_TPI, strel, [out], ws=ws, impl=impl)
        if standardize:
            fn = getattr(_lib.load(), "smrf_focal_divide_" + _suffix(Xd))
            _lib.check(fn(_ptr(out), out.numel(), _ptr(ws[2:]), _stream()))
    return _out(out, was_tensor)


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
    was_tensor = _is_tensor(Z)
    Zd = _raster(Z)
    torch = _torch()
    out = torch.empty(Zd.shape, dtype=torch.float64, device=Zd.device)
    if Zd.numel():
        lib = _lib.load()
        M = torch.empty_like(Zd)
        _launch(Zd, _lib.FOCAL_SUM, strel / np.sum(strel), [M], impl=impl)
        STD = _std(Zd, strel, sub=M, impl=impl)
        ws = _workspace(Zd)
        _lib.check(lib.smrf_focal_minmax_f64(_ptr(STD), STD.numel(), _ptr(ws), ws.numel() * 8, _stream()))
        fn = getattr(lib, "smrf_focal_mix_" + _suffix(Zd))
        _lib.check(fn(_ptr(Zd), _ptr(M), _ptr(STD), _ptr(ws), float(blend_rate), _ptr(out), out.numel(), _stream()))
    return _out(out, was_tensor)
