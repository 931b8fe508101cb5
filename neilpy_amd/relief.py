"""Relief colouring and raster statistics (MI355X only): the last step from a DTM to the coloured relief image.

Mirrors, argument for argument, the reference functions (paths relative to the reference checkout) ``swiss_shading``
(neilpy/neilpy.py:1848), ``colortable_shade`` (:1870), ``rmse`` (:1918), ``cutter`` (:1932), ``normalize`` (:1961) and
``brassel_atmospheric_perspective`` (:1993), and adds :func:`raster_stats`, the NaN-ignoring reduction under them:
count, min, max, mean, sum of squares and an exact median (a radix select, ``csrc/select_plan.h``).

Every raster function runs in the kernels of ``csrc/relief.hip`` (``smrf_raster_stats_*``, ``smrf_normalize_*``,
``smrf_colortable_*``, ``smrf_brassel_*``); the arithmetic contract is DESIGN.md section 16.  NumPy in -> NumPy out; a
CUDA tensor in -> a CUDA tensor out on the same device.  There is no CPU fallback: without the library or a GPU every
raster function raises :class:`neilpy_amd.SmrfHipError`.  ``cutter`` is host code: it only makes views.

Deviations from the reference (each in DESIGN.md section 16): ``colortable_shade`` takes its table as an array only (a
string raises ``NotImplementedError``: the reference's PNG tables are not shipped, and its named colour specs fail in
the reference itself) and ``swiss_shading`` takes it as the keyword ``lut``; a ``'mean'`` knot of ``normalize`` is the
float64 sum in the device's order divided by the count, not ``np.nanmean``'s pairwise sum in the raster's dtype;
``rmse`` sums in float64; ``brassel_atmospheric_perspective`` raises ``ValueError`` for ``k < 1`` (the reference's
``raise('...')`` is a ``TypeError``) and divides a float32 shade above 1 by 255 in float64; rasters below 2 cells per
axis raise np.gradient's ``ValueError`` in the two shading functions.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._raster import Raster, _ptr, _pyfloat as _f, _stream, _suffix, _torch
from ._xfer import to_host as _d2h
from .surface import _angle_row, _need_gradient

__all__ = ["raster_stats", "normalize", "rmse", "colortable_shade", "swiss_shading",
           "brassel_atmospheric_perspective", "cutter"]

STATS = ('count', 'min', 'max', 'mean', 'median', 'sum_sq')
_ROW = {'count': _lib.STATS_COUNT, 'min': _lib.STATS_MIN, 'max': _lib.STATS_MAX, 'mean': _lib.STATS_MEAN,
        'median': _lib.STATS_MEDIAN_AT, 'sum_sq': _lib.STATS_SUM_SQ}


# ------------------------------------------------------------------------------------------
# the statistics row
# ------------------------------------------------------------------------------------------
def _stats_row(t, what):
    """smrf_raster_stats_* on a contiguous device tensor (float32, float64 or, moments only, uint8): the host row"""
    torch = _torch()
    lib = _lib.load()
    stem = "u8" if t.dtype == torch.uint8 else _suffix(t)
    ws = torch.empty(int(lib.smrf_raster_stats_workspace_bytes(t.element_size(), what)), dtype=torch.uint8,
                     device=t.device)
    row = (C.c_double * _lib.STATS_ROW)()
    _lib.check(getattr(lib, "smrf_raster_stats_" + stem)(_ptr(t), t.numel(), what, row, _ptr(ws), ws.numel(),
                                                         _stream()))
    return list(row)


def _want(names):
    what = 0
    for n in names:
        if n not in _ROW:
            raise ValueError("unknown statistic %r (one of %s)" % (n, list(STATS)))
        what |= _lib.STATS_MEDIAN if n == 'median' else _lib.STATS_MOMENTS
    return what


@_device_scoped
def raster_stats(X, what=STATS):
    """NaN-ignoring statistics of a raster as a dict: the entries of ``what`` ('count', 'min', 'max', 'mean', 'median',
    'sum_sq') and always 'has_nan'.  +-inf are values; an empty or all-NaN raster gives count 0 and NaN.  'min', 'max'
    and 'median' come in the raster's dtype ('median' is np.nanmedian's value exactly), 'mean' and 'sum_sq' (cells
    squared in the raster's dtype) are float64 sums in the fixed order of DESIGN.md section 16: the same input gives
    the same bits on every call.  One device-to-host copy per call."""
    what = (what,) if isinstance(what, str) else tuple(what)
    bits = _want(what) | _lib.STATS_MOMENTS                 # has_nan and count come with the moments
    R = Raster(X)
    dt = np.float32 if _suffix(R.t) == "f32" else np.float64
    row = _stats_row(R.t, bits) if R.t.numel() else [0.0, 0.0] + [np.nan] * 6
    out = {}
    for n in what:
        v = row[_ROW[n]]
        out[n] = int(v) if n == 'count' else dt(v) if n in ('min', 'max', 'median') else np.float64(v)
    out['has_nan'] = row[_lib.STATS_NAN] > 0
    return out


# ------------------------------------------------------------------------------------------
# normalize, rmse
# ------------------------------------------------------------------------------------------
@_device_scoped
def normalize(X, xrange=['min', 'max'], yrange=[0, 1], *, return_knots=False):
    """``np.interp(X, knots, yrange)`` in float64, cell for cell, with the knots 'min', 'max', 'mean', 'median' taken
    from :func:`raster_stats` (numbers pass through).  Same arguments and results as neilpy.normalize, except that a
    'mean' knot is the device's float64 mean.  ``return_knots=True`` also returns the float64 knots used."""
    xr, yr = list(xrange), [_f(v) for v in yrange]
    if len(xr) < 2 or len(xr) != len(yr):
        raise ValueError("xrange and yrange need the same number of knots, at least 2")
    names = [k for k in xr if isinstance(k, str)]
    for k in names:
        if k not in ('min', 'max', 'mean', 'median'):
            raise ValueError("unknown knot %r (one of 'min', 'max', 'mean', 'median', or a number)" % k)
    bits = _want(names)
    R = Raster(X)
    row = _stats_row(R.t, bits) if (bits and R.t.numel()) else [np.nan] * _lib.STATS_ROW
    knots = np.array([row[_ROW[k]] if isinstance(k, str) else _f(k) for k in xr], dtype=np.float64)
    out = R.empty(_torch().float64)
    tab = _torch().from_numpy(np.concatenate([knots, np.array(yr, dtype=np.float64)])).to(R.t.device)
    R.call("normalize", _ptr(R.t), R.t.numel(), _ptr(tab), len(xr), _ptr(out))
    res = R.out(out)
    return (res, knots) if return_knots else res


@_device_scoped
def rmse(X):
    """``sqrt(nansum(X ** 2) / X.size)`` (the size counts NaN cells), rounded to the raster's dtype: a NumPy scalar, or
    a 0-dim tensor for a tensor.  Same argument as neilpy.rmse; the squares are summed in float64."""
    R = Raster(X)
    n = R.t.numel()
    row = _stats_row(R.t, _lib.STATS_MOMENTS) if n else None
    ss = np.float64(0.0) if (row is None or row[_lib.STATS_COUNT] == 0) else np.float64(row[_lib.STATS_SUM_SQ])
    with np.errstate(divide='ignore', invalid='ignore'):
        v = np.sqrt(ss / np.float64(n))
    if R.was_tensor:
        return _torch().tensor(float(v), dtype=R.t.dtype, device=R.t.device)
    return (np.float32 if _suffix(R.t) == "f32" else np.float64)(v)


# ------------------------------------------------------------------------------------------
# colour tables
# ------------------------------------------------------------------------------------------
def _check_table(lut):
    shape = tuple(lut.shape) if _is_tensor(lut) else np.shape(lut)
    if not (shape[:2] == (256, 256) and (len(shape) == 2 or (len(shape) == 3 and shape[2] >= 3))):
        raise ValueError("a colour table is 256 x 256 or 256 x 256 x C with C >= 3, not %s" % (shape,))


def _packed_table(lut, device):
    """the table as 256 x 256 device words R | G << 8 | B << 16, cast to uint8 as NumPy assignment casts"""
    torch = _torch()
    if _is_tensor(lut) and lut.dtype == torch.uint8:
        t = lut.to(device)
    else:
        a = lut.detach().cpu().numpy() if _is_tensor(lut) else np.asarray(lut)
        with np.errstate(invalid='ignore'):
            t = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8))).to(device)
    if t.dim() == 2:
        t = t[:, :, None].expand(256, 256, 3)
    w = t[:, :, :3].to(torch.int32)
    return (w[:, :, 0] | (w[:, :, 1] << 8) | (w[:, :, 2] << 16)).contiguous()


def _shade(Z, lut, cellsize):
    _check_table(lut)
    _need_gradient(Z)
    R = Raster(Z)
    torch = _torch()
    rgb = torch.empty((R.rows, R.cols, 3), dtype=torch.uint8, device=R.t.device)
    if R.t.numel():
        # np.min / np.max: a NaN anywhere makes both NaN, and every cell indexes row 0
        row = _stats_row(R.t, _lib.STATS_MOMENTS)
        poison = row[_lib.STATS_NAN] > 0
        zmin = np.nan if poison else row[_lib.STATS_MIN]
        zmax = np.nan if poison else row[_lib.STATS_MAX]
        angle = (C.c_double * 3)(*_angle_row(45, 315))
        R.call("colortable", _ptr(R.t), R.rows, R.cols, zmin, zmax, _f(cellsize), angle,
               _ptr(_packed_table(lut, R.t.device)), _ptr(rgb))
    return R.out(rgb)


@_device_scoped
def colortable_shade(Z, name='swiss', cellsize=1):
    """uint8 ``(rows, cols, 3)``: ``table[zi, H]`` with H = ``hillshade(Z, cellsize)`` and zi = the elevation scaled to
    0..255 between the raster's min and max.  ``name`` is the table as an array, 256 x 256 (grey) or 256 x 256 x C with
    C >= 3; a string raises ``NotImplementedError``.  One reduction and one fused launch that reads the raster once."""
    if isinstance(name, str):
        raise NotImplementedError("colortable_shade(name=%r): named tables are not shipped with neilpy_amd; pass the "
                                  "256 x 256 (x C) table as an array" % name)
    return _shade(Z, name, cellsize)


@_device_scoped
def swiss_shading(Z, cellsize=1, *, lut):
    """:func:`colortable_shade` with the first three channels of ``lut`` (the reference reads its own PNG table; this
    package takes the table from the caller)."""
    if isinstance(lut, str):
        raise NotImplementedError("swiss_shading(lut=%r): pass the 256 x 256 x C table as an array" % lut)
    return _shade(Z, lut, cellsize)


# ------------------------------------------------------------------------------------------
# Brassel
# ------------------------------------------------------------------------------------------
def _shade_tensor(H):
    """the shade on the device, contiguous, as uint8, float32 or float64 (anything else widened to float64)"""
    torch = _torch()
    _lib.require_gpu()
    t = H if _is_tensor(H) else torch.from_numpy(np.ascontiguousarray(H))
    if t.dtype not in (torch.uint8, torch.float32, torch.float64):
        t = t.to(torch.float64)
    return (t if t.is_cuda else t.cuda()).contiguous()


@_device_scoped
def brassel_atmospheric_perspective(H, Z, k, flat=180, Zmid=None, reverse=False, C2=0):
    """Brassel's (1974) atmospheric perspective of a shaded relief ``H`` (uint8, or float in 0..1) over elevations
    ``Z``: ``(H - flat) * e ** (Zstar * log(k)) + flat`` clipped to 0..1, plus the tonal term ``C2 * (Zstar - 1) / 2``.
    A shade with a value above 1 is taken as 0..255 and comes back as uint8, otherwise the result is float64.  Same
    arguments and results as neilpy.brassel_atmospheric_perspective; the result is a tensor if ``H`` is one."""
    if k < 1:
        raise ValueError('k must be equal to or greater than one.')
    hshape = tuple(H.shape) if _is_tensor(H) else np.shape(H)
    zshape = tuple(Z.shape) if _is_tensor(Z) else np.shape(Z)
    if hshape != zshape:
        raise ValueError("H %s and Z %s differ in shape" % (hshape, zshape))
    torch = _torch()
    R = Raster(Z)
    Ht = _shade_tensor(H).to(R.t.device)
    n = R.t.numel()
    was_int = bool(n) and _stats_row(Ht, _lib.STATS_MOMENTS)[_lib.STATS_MAX] > 1
    flat = _f(flat)
    if flat > 1:
        flat = flat / 255
    out = torch.empty((R.rows, R.cols), dtype=torch.uint8 if was_int else torch.float64, device=R.t.device)
    if n:
        zrow = _stats_row(R.t, _lib.STATS_MOMENTS)
        opts = (_lib.BRASSEL_WAS_INT if was_int else 0) | (_lib.BRASSEL_ZMID if Zmid is not None else 0) | \
            (_lib.BRASSEL_REVERSE if reverse else 0)
        htype = {torch.uint8: _lib.SHADE_U8, torch.float32: _lib.SHADE_F32, torch.float64: _lib.SHADE_F64}[Ht.dtype]
        R.call("brassel", _ptr(Ht), htype, _ptr(R.t), n, opts, flat, zrow[_lib.STATS_MIN], zrow[_lib.STATS_MAX],
               0.0 if Zmid is None else _f(Zmid), float(np.log(k)), _f(C2), _ptr(out))
    return out if _is_tensor(H) else _d2h(out)


# ------------------------------------------------------------------------------------------
# cutter (host only: views)
# ------------------------------------------------------------------------------------------
def _tensor_split(t, sections, dim):
    if isinstance(sections, (int, np.integer)):
        if t.shape[dim] % sections:
            raise ValueError('array split does not result in an equal division')
        return list(_torch().tensor_split(t, int(sections), dim=dim))
    return list(_torch().tensor_split(t, [int(i) for i in sections], dim=dim))


def cutter(x, r, c):
    """Split a raster into ``r`` x ``c`` pieces: a list of ``r`` lists of ``c`` views, ``[np.hsplit(i, c) for i in
    np.vsplit(x, r)]`` (for a tensor, the same views of the tensor).  A shape that does not divide raises NumPy's
    ``ValueError``.  Same arguments and results as neilpy.cutter."""
    if not _is_tensor(x):
        return [np.hsplit(i, c) for i in np.vsplit(x, r)]
    if x.dim() < 2:
        raise ValueError('vsplit only works on arrays of 2 or more dimensions')
    return [_tensor_split(i, c, 1) for i in _tensor_split(x, r, 0)]
