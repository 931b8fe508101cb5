"""Median, rank, percentile, minimum and maximum filters of a raster with any flat footprint, under scipy.ndimage's names
(MI355X only).

``median_filter``, ``rank_filter``, ``percentile_filter``, ``minimum_filter`` and ``maximum_filter`` take
``scipy.ndimage``'s parameters, same names, order and defaults, and give its values for a 2-D raster, a flat footprint
(``size=`` or ``footprint=``: odd, even, non-square, larger than the raster) and the border modes ``'reflect'`` and
``'nearest'``: the member (s, t) of a KH x KW footprint samples ``X[idx(i + s - KH // 2), idx(j + t - KW // 2)]`` -
:func:`neilpy_amd.morphology.plan`'s erosion offsets, for ``maximum_filter`` too (``grey_dilation`` reads the mirrored
footprint) - and the result is ``np.sort(samples)[rank]`` with the rank :func:`resolve` gives, SciPy's.  The contract is
DESIGN.md section 20.

Every call is one launch of ``csrc/rank.hip`` (``smrf_rank_filter_*``, include/smrf_rank.h), which selects by comparison
of order-preserving integer keys: by counting positions (COUNT) for small footprints, by a radix select (BISECT) for
large ones, on samples staged in LDS (TILE) while the tile fits and read from global memory (GLOBAL) otherwise.  Every
path gives the same bits; ``impl=`` forces one.  Rank 0 and rank n - 1 of a raster without NaN under ``impl=0`` go to
the grey-morphology kernel (``smrf_footprint_filter_*``) with the same offsets; its minimum and maximum do not order
-0.0 against +0.0, so there the sign of a zero result is either.

NumPy in -> NumPy out; a CUDA tensor in -> a CUDA tensor out on the same device; float32 and float64 kept, other dtypes
widened to float64.  There is no CPU fallback: argument errors come from the host before the device is touched, and a
valid call without the library or a GPU raises :class:`neilpy_amd.SmrfHipError`.

Deviations from SciPy (each in DESIGN.md section 20): ``output=``, a non-zero ``origin``, ``axes=``, other modes,
rasters that are not 2-D and footprints beyond ``morphology.MAX_EXTENT`` are refused with ``NotImplementedError``;
``cval`` is accepted and unused; integer and boolean rasters are widened to float64.  NaN sorts after +inf, as in
``np.sort``: a cell is NaN iff fewer than ``rank + 1`` of its samples are not NaN.  SciPy's selection compares with
``<`` and its result with a NaN among the samples depends on the visiting order; this also makes ``minimum_filter``
and ``maximum_filter`` differ, with NaN present, from ``grey_erosion`` / ``grey_dilation``'s first-visited rule.
"""
import ctypes as C
import operator

import numpy as np

from . import _lib, morphology
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._raster import Raster, _ptr, _stream, _suffix, _torch
from .api import _has_nan

__all__ = ["median_filter", "rank_filter", "percentile_filter", "minimum_filter", "maximum_filter", "resolve"]

# include/smrf_rank.h: the selection methods and sample sources ``impl=`` forces (FORCE_NAN_AWARE is this module's own
# flag on top: the NaN-aware launch whatever the raster holds), what smrf_rank_path reports, the LDS cap of the tile,
# the candidates COUNT holds per sweep and the largest member count the automatic choice gives to COUNT
IMPL_AUTO, IMPL_COUNT, IMPL_BISECT, FORCE_NAN_AWARE, IMPL_GLOBAL, IMPL_TILE = 0, 1, 2, 4, 8, 16
PATH_COUNT, PATH_BISECT, PATH_TILE, PATH_GLOBAL = 0, 1, 0, 2
TILE_BYTES = 53248
COUNT_BLOCK = 8
COUNT_MAX_TAPS = {4: 25, 8: 81}

# name -> (result, arguments).  Attached to the library on first use.
_i, _p = C.c_int, C.c_void_p
SIGNATURES = {
    "smrf_rank_tile_bytes": (_i, []),
    "smrf_rank_count_max_taps": (_i, [_i]),
    "smrf_rank_path": (_i, [_p, _i, _i]),
    "smrf_rank_filter_f32": (_i, [_p, _p, _i, _i, _p, _p, _i, _i, _i, _i, _p]),
    "smrf_rank_filter_f64": (_i, [_p, _p, _i, _i, _p, _p, _i, _i, _i, _i, _p]),
}
_bound = None


def _library():
    """the loaded library with this family's prototypes attached; a library without them is an error"""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib


# ------------------------------------------------------------------------------------------
# the rank, on the host
# ------------------------------------------------------------------------------------------
def resolve(kind, n, value=None):
    """The position in the sorted samples that ``kind`` ('median', 'rank', 'percentile', 'minimum', 'maximum') asks of a
    footprint of ``n`` members, as scipy.ndimage resolves it: the median is ``n // 2``; a negative percentile counts
    from 100, 100 is the last member, any other is ``int(float(n) * p / 100.0)``; a negative rank counts from ``n``."""
    n = operator.index(n)
    if kind == "median":
        rank = n // 2
    elif kind == "minimum":
        rank = 0
    elif kind == "maximum":
        rank = n - 1
    elif kind == "percentile":
        p = value
        if p < 0.0:
            p += 100.0
        if p < 0 or p > 100:
            raise RuntimeError('invalid percentile')
        rank = n - 1 if p == 100.0 else int(float(n) * p / 100.0)
    elif kind == "rank":
        rank = operator.index(value)
    else:
        raise ValueError("unknown kind %r" % (kind,))
    if rank < 0:
        rank += n
    if rank < 0 or rank >= n:
        raise RuntimeError('rank not within filter footprint size')
    return rank


# ------------------------------------------------------------------------------------------
# arguments and the launch
# ------------------------------------------------------------------------------------------
def _filter(kind, value, input, size, footprint, output, mode, origin, axes, impl):
    """one public call: the argument rules and the rank on the host, then the raster on the device and one launch"""
    if axes is not None:
        raise NotImplementedError("axes= is not supported: the raster's two axes are filtered")
    if size is None and footprint is None:
        raise RuntimeError("no footprint or filter size provided")
    impl = operator.index(impl)
    force_nan, impl = bool(impl & FORCE_NAN_AWARE), impl & ~FORCE_NAN_AWARE
    if impl < 0 or (impl & ~(IMPL_GLOBAL | IMPL_TILE)) > IMPL_BISECT or impl & IMPL_GLOBAL and impl & IMPL_TILE:
        raise ValueError("unknown impl %r" % (impl,))
    fp, mode, _, _ = morphology._arguments(size, footprint, None, output, mode, origin, morphology.IMPL_AUTO)
    rank = resolve(kind, int(np.count_nonzero(fp)), value)
    if (input.dim() if _is_tensor(input) else len(np.shape(input))) != 2:
        raise NotImplementedError("only 2-D rasters are supported on the device")
    R = Raster(input)
    out = R.empty()
    if not R.t.numel():
        return R.out(out)
    nan_aware = force_nan or _has_nan(R.t)
    P = morphology.plan(fp, False, itemsize=R.t.element_size())
    n = len(P.offsets)
    table = _torch().from_numpy(P.table).to(R.t.device)
    head = P.head.ctypes.data_as(C.c_void_p)
    if impl == IMPL_AUTO and not nan_aware and rank in (0, n - 1):
        # the extremes of a raster without NaN: the grey-morphology kernel over the same (unmirrored) samples
        R.call("footprint_filter", _ptr(R.t), _ptr(None), _ptr(out), R.rows, R.cols, _ptr(table), head,
               int(n > 1 and rank == n - 1), mode, 0, morphology.IMPL_AUTO, morphology.STORE)
    else:
        fn = getattr(_library(), "smrf_rank_filter_" + _suffix(R.t))
        _lib.check(fn(_ptr(R.t), _ptr(out), R.rows, R.cols, _ptr(table), head, rank, mode, int(nan_aware), impl, _stream()))
    # the table is freed by the caching allocator on this stream only after the launch has read it
    return R.out(out)


@_device_scoped
def median_filter(input, size=None, footprint=None, output=None, mode='reflect', cval=0.0, origin=0, *, axes=None,
                  impl=IMPL_AUTO):
    """``scipy.ndimage.median_filter`` of a 2-D raster by a flat footprint: the sample at position ``n // 2`` of the
    footprint's ``n`` samples sorted ascending.  ``impl`` forces a kernel path (same bits)."""
    return _filter("median", None, input, size, footprint, output, mode, origin, axes, impl)


@_device_scoped
def rank_filter(input, rank, size=None, footprint=None, output=None, mode='reflect', cval=0.0, origin=0, *, axes=None,
                impl=IMPL_AUTO):
    """``scipy.ndimage.rank_filter``: the sample at position ``rank`` (a negative one counts from the end)."""
    return _filter("rank", rank, input, size, footprint, output, mode, origin, axes, impl)


@_device_scoped
def percentile_filter(input, percentile, size=None, footprint=None, output=None, mode='reflect', cval=0.0, origin=0, *,
                      axes=None, impl=IMPL_AUTO):
    """``scipy.ndimage.percentile_filter``: the sample at position ``int(n * percentile / 100)``, the last one at 100 (a
    negative percentile counts from 100)."""
    return _filter("percentile", percentile, input, size, footprint, output, mode, origin, axes, impl)


@_device_scoped
def minimum_filter(input, size=None, footprint=None, output=None, mode='reflect', cval=0.0, origin=0, *, axes=None,
                   impl=IMPL_AUTO):
    """``scipy.ndimage.minimum_filter``: rank 0.  NaN iff every sample is NaN (``grey_erosion``: iff the first is)."""
    return _filter("minimum", None, input, size, footprint, output, mode, origin, axes, impl)


@_device_scoped
def maximum_filter(input, size=None, footprint=None, output=None, mode='reflect', cval=0.0, origin=0, *, axes=None,
                   impl=IMPL_AUTO):
    """``scipy.ndimage.maximum_filter``: rank ``n - 1`` over the footprint as it stands (``grey_dilation`` mirrors
    it).  NaN iff any sample is NaN."""
    return _filter("maximum", None, input, size, footprint, output, mode, origin, axes, impl)
