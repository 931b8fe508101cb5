"""Grey morphology of a raster with any flat footprint, under scipy.ndimage's names (MI355X only).

``grey_erosion``, ``grey_dilation``, ``grey_opening``, ``grey_closing``, ``white_tophat``, ``black_tophat`` and
``morphological_gradient`` take ``scipy.ndimage``'s parameters, same names, order and defaults, and give its values
bit for bit for a 2-D raster, a flat footprint (``size=`` or ``footprint=``: odd, even, non-square, larger than the
raster) and the border modes ``'reflect'`` and ``'nearest'``.  ``rectangle``, ``square`` and ``diamond`` are host
helpers next to ``disk``.  The disk-only ``erosion`` / ``dilation`` / ``opening`` of ``neilpy_amd.api`` are untouched.

Every function is one or two launches of ``csrc/footprint.hip`` (``smrf_footprint_filter_*``): erosion and dilation
one; opening, closing and the top-hats two, a top-hat's subtraction riding in its second launch; the gradient one
launch that takes the minimum and the maximum from the same samples when the footprint is its own mirror image, two
otherwise.  The host turns the footprint into a :func:`plan` - offsets in ndimage's visiting order, runs of consecutive
members, the LDS planes of the runs path - and uploads it with the call.  The contract is DESIGN.md section 19.

NumPy in -> NumPy out; a CUDA tensor in -> a CUDA tensor out on the same device; float32 and float64 kept, other dtypes
widened to float64.  There is no CPU fallback: argument errors come from the host before the device is touched, and a
valid call without the library or a GPU raises :class:`neilpy_amd.SmrfHipError`.

Deviations from SciPy (each in DESIGN.md section 19): ``structure=`` (non-flat), ``output=``, a non-zero ``origin``,
other modes and rasters that are not 2-D are refused; integer and boolean rasters are widened to float64; the NaN rule
of ndimage's footprint filter (NaN iff the first visited member's sample is NaN) holds for every footprint, also the
all-ones ones that SciPy sends through its separable filters.
"""
import ctypes as C
import operator
from collections import namedtuple

import numpy as np

from ._device import device_scoped as _device_scoped
from ._raster import Raster, _ptr, _torch
from .api import _has_nan

__all__ = ["grey_erosion", "grey_dilation", "grey_opening", "grey_closing", "white_tophat", "black_tophat",
           "morphological_gradient", "rectangle", "square", "diamond", "plan"]

# include/smrf_hip.h, the family's part of the C ABI: border modes, the paths ``impl=`` forces (FORCE_NAN_AWARE is
# this module's own flag on top: the NaN-aware launch whatever the raster holds), store epilogues, the LDS cap of the
# runs path and the least member count of an automatic runs launch
REFLECT, NEAREST = 0, 1
IMPL_AUTO, IMPL_RUNS, IMPL_TAPS, FORCE_NAN_AWARE = 0, 1, 2, 4
STORE, SUB_MINUS, MINUS_SUB, GRADIENT = range(4)
TILE_BYTES = 53248
RUNS_MIN_TAPS = 9

TX, TY = 64, 8                 # the workgroup's cells (csrc/footprint.hip)
MAX_LEVELS = 16                # slots of the plan's head
MAX_EXTENT = 1 << 20           # footprint rows / columns the library accepts
MODES = {"reflect": REFLECT, "nearest": NEAREST}

Plan = namedtuple("Plan", "dilate offsets runs levels slots nplanes box tile halo lds_bytes path head table")


# ------------------------------------------------------------------------------------------
# host helpers
# ------------------------------------------------------------------------------------------
def rectangle(nrows, ncols, dtype=np.uint8):
    """skimage.morphology.rectangle: ``nrows`` x ``ncols`` ones."""
    return np.ones((operator.index(nrows), operator.index(ncols)), dtype=dtype)


def square(width, dtype=np.uint8):
    """skimage.morphology.square: ``width`` x ``width`` ones."""
    return rectangle(width, width, dtype)


def diamond(radius, dtype=np.uint8):
    """skimage.morphology.diamond: ``|dy| + |dx| <= radius`` on a (2r+1)^2 grid."""
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return np.array(np.abs(X) + np.abs(Y) <= radius, dtype=dtype)


# ------------------------------------------------------------------------------------------
# the host plan
# ------------------------------------------------------------------------------------------
def _slots(levels):
    """an LDS plane for every level 0 .. max(levels): a level is built from the one below, so never into its plane, and
    never into the plane of a level a run still reads; a plane nothing reads any more is taken again"""
    slots, pinned, nplanes = [0], set(), 1
    for k in range(1, max(levels) + 1):
        if k - 1 in levels:
            pinned.add(slots[k - 1])
        free = [p for p in range(nplanes) if p not in pinned and p != slots[k - 1]]
        if not free:
            free = [nplanes]
            nplanes += 1
        slots.append(free[0])
    return tuple(slots), nplanes


def plan(footprint, dilate=False, mode="reflect", itemsize=4, gradient=False, impl=IMPL_AUTO,
         cap=TILE_BYTES):
    """What one launch of ``smrf_footprint_filter_*`` needs of a footprint, as a pure function of its arguments.

    With ``ch, cw = KH // 2, KW // 2`` the member (s, t) samples ``X[idx(i + s - ch), idx(j + t - cw)]`` for an
    erosion and ``X[idx(i - (s - ch)), idx(j - (t - cw))]`` for a dilation; ``mode`` decides ``idx`` on the device and
    nothing here.  The fields:

    ``offsets``    (n, 2) int32 (drow, dcol) in ndimage's visiting order, the first visited member first: row-major
                   for an erosion, the reverse of row-major (at the mirrored offsets) for a dilation;
    ``runs``       per row of samples the maximal runs of consecutive members, ``(drow, dcol0, length)``;
    ``levels``     the ``floor(log2(length))`` that occur, ascending;
    ``slots``, ``nplanes``   the LDS plane of every level up to the largest, and how many planes that takes;
    ``box``        ``(r_lo, c_lo, bh, bw)``: the least offsets and the extent of the members' bounding box;
    ``tile``, ``halo``       rows and columns of an LDS plane, and of them the cells beyond the workgroup's own;
    ``lds_bytes``  what the planes take (twice for ``gradient``, which keeps a min and a max set);
    ``path``       ``'runs'`` or ``'taps'`` as the library will choose under ``impl``, ``'refused'`` where RUNS is
                   forced past ``cap``;
    ``head``, ``table``      the int32 arrays the entry point takes (include/smrf_hip.h).
    """
    if mode not in MODES:
        raise NotImplementedError("mode %r: only 'reflect' and 'nearest' are supported on the device" % (mode,))
    fp = np.asarray(footprint)
    if fp.ndim != 2:
        raise ValueError("expected a 2-D footprint")
    fp = fp != 0
    if not fp.any():
        raise ValueError("the footprint has no member")
    kh, kw = fp.shape
    if kh > MAX_EXTENT or kw > MAX_EXTENT:
        raise NotImplementedError("footprints beyond %d rows or columns are not supported" % MAX_EXTENT)
    s, t = np.nonzero(fp)                                   # row-major
    drow, dcol = s - kh // 2, t - kw // 2
    if dilate:
        drow, dcol = -drow[::-1], -dcol[::-1]
    offsets = np.stack([drow, dcol], axis=1).astype(np.int32)

    order = np.lexsort((dcol, drow))
    dr, dc = drow[order], dcol[order]
    cut = np.flatnonzero((np.diff(dr) != 0) | (np.diff(dc) != 1)) + 1
    first, last = np.r_[0, cut], np.r_[cut, len(dr)]
    runs = tuple((int(dr[a]), int(dc[a]), int(b - a)) for a, b in zip(first, last))
    levels = tuple(sorted({L.bit_length() - 1 for _, _, L in runs}))
    slots, nplanes = _slots(levels)

    r_lo, c_lo = int(drow.min()), int(dcol.min())
    bh, bw = int(drow.max()) - r_lo + 1, int(dcol.max()) - c_lo + 1
    tile = (TY + bh - 1, TX + bw - 1)
    lds_bytes = (2 if gradient else 1) * nplanes * tile[0] * tile[1] * int(itemsize)
    fits = lds_bytes <= cap
    if impl == IMPL_AUTO:
        path = "runs" if fits and len(offsets) >= RUNS_MIN_TAPS else "taps"
    elif impl == IMPL_RUNS:
        path = "runs" if fits else "refused"
    elif impl == IMPL_TAPS:
        path = "taps"
    else:
        raise ValueError("unknown impl %r" % (impl,))

    head = np.zeros(8 + MAX_LEVELS, dtype=np.int32)
    head[:8] = (len(offsets), len(runs), r_lo, c_lo, bh, bw, levels[-1], nplanes)
    head[8:8 + len(slots)] = slots
    recs = np.empty((len(runs), 4), dtype=np.int32)
    for i, (d, c0, L) in enumerate(runs):
        k = L.bit_length() - 1
        recs[i] = (d - r_lo, c0 - c_lo, c0 - c_lo + L - (1 << k), slots[k])
    table = np.concatenate([offsets.ravel(), recs.ravel()])
    return Plan(bool(dilate), offsets, runs, levels, slots, nplanes, (r_lo, c_lo, bh, bw), tile, (bh - 1, bw - 1),
                lds_bytes, path, head, table)


# ------------------------------------------------------------------------------------------
# arguments and the launch
# ------------------------------------------------------------------------------------------
def _arguments(size, footprint, structure, output, mode, origin, impl):
    """the argument rules, all on the host: the footprint as a boolean array, and the library's impl and NaN flag"""
    if structure is not None:
        raise NotImplementedError("structure= (a non-flat structuring element) is not supported on the device")
    if output is not None:
        raise NotImplementedError("output= is not supported: the result is a new array")
    if np.any(np.asarray(origin) != 0):
        raise NotImplementedError("only origin=0 is supported on the device")
    if mode not in MODES:
        raise NotImplementedError("mode %r: only 'reflect' and 'nearest' are supported on the device" % (mode,))
    if footprint is not None:                                # as in SciPy, a footprint wins over size
        fp = np.asarray(footprint)
        if fp.ndim != 2:
            raise ValueError("expected a 2-D footprint")
        fp = fp != 0
    elif size is not None:
        sz = np.asarray(size)
        if sz.ndim > 1 or (sz.ndim == 1 and sz.size != 2):
            raise ValueError("size is an integer or a pair of integers")
        sz = tuple(operator.index(v) for v in (sz.tolist() if sz.ndim else [sz.item()] * 2))
        if min(sz) < 1:
            raise ValueError("size must be at least 1 along every axis")
        if max(sz) > MAX_EXTENT:
            raise NotImplementedError("footprints beyond %d rows or columns are not supported" % MAX_EXTENT)
        fp = np.ones(sz, dtype=bool)
    else:
        raise ValueError("size, footprint, or structure must be specified")
    if not fp.any():
        raise ValueError("the footprint has no member")
    if max(fp.shape) > MAX_EXTENT:
        raise NotImplementedError("footprints beyond %d rows or columns are not supported" % MAX_EXTENT)
    impl = operator.index(impl)
    force_nan, impl = bool(impl & FORCE_NAN_AWARE), impl & ~FORCE_NAN_AWARE
    if impl not in (IMPL_AUTO, IMPL_RUNS, IMPL_TAPS):
        raise ValueError("unknown impl %r" % (impl,))
    return fp, MODES[mode], impl, force_nan


class _Filter:
    """one public call: the raster on the device, the footprint, and the launches over them"""

    def __init__(self, input, size, footprint, structure, output, mode, origin, impl):
        self.fp, self.mode, self.impl, force_nan = _arguments(size, footprint, structure, output, mode, origin, impl)
        self.R = R = Raster(input)
        self.nan_aware = force_nan or (_has_nan(R.t) if R.t.numel() else False)

    def symmetric(self):
        """the footprint is its own mirror image about (KH // 2, KW // 2): erosion and dilation read the same samples"""
        kh, kw = self.fp.shape
        return kh % 2 == 1 and kw % 2 == 1 and np.array_equal(self.fp, self.fp[::-1, ::-1])

    def run(self, src, dilate, sub=None, epilogue=STORE):
        """one launch over the plane ``src``: its erosion or dilation, through ``epilogue``"""
        R = self.R
        out = R.empty()
        if R.t.numel():
            P = plan(self.fp, dilate, itemsize=R.t.element_size(), gradient=epilogue == GRADIENT)
            table = _torch().from_numpy(P.table).to(R.t.device)
            R.call("footprint_filter", _ptr(src), _ptr(sub), _ptr(out), R.rows, R.cols, _ptr(table),
                   P.head.ctypes.data_as(C.c_void_p), int(dilate), self.mode, int(self.nan_aware), self.impl, epilogue)
            # the table is freed by the caching allocator on this stream only after the launch has read it
        return out


@_device_scoped
def grey_erosion(input, size=None, footprint=None, structure=None, output=None, mode='reflect', cval=0.0, origin=0, *,
                 impl=IMPL_AUTO):
    """``scipy.ndimage.grey_erosion`` of a 2-D raster by a flat footprint: the minimum over the footprint's members,
    NaN iff the first member's sample (row-major) is NaN.  ``impl`` forces the runs or the taps kernel path (same
    values)."""
    f = _Filter(input, size, footprint, structure, output, mode, origin, impl)
    return f.R.out(f.run(f.R.t, False))


@_device_scoped
def grey_dilation(input, size=None, footprint=None, structure=None, output=None, mode='reflect', cval=0.0, origin=0, *,
                  impl=IMPL_AUTO):
    """``scipy.ndimage.grey_dilation``: the maximum over the footprint mirrored about its centre (KH // 2, KW // 2),
    NaN iff the last member's sample is NaN."""
    f = _Filter(input, size, footprint, structure, output, mode, origin, impl)
    return f.R.out(f.run(f.R.t, True))


@_device_scoped
def grey_opening(input, size=None, footprint=None, structure=None, output=None, mode='reflect', cval=0.0, origin=0, *,
                 impl=IMPL_AUTO):
    """``scipy.ndimage.grey_opening``: the dilation of the erosion."""
    f = _Filter(input, size, footprint, structure, output, mode, origin, impl)
    return f.R.out(f.run(f.run(f.R.t, False), True))


@_device_scoped
def grey_closing(input, size=None, footprint=None, structure=None, output=None, mode='reflect', cval=0.0, origin=0, *,
                 impl=IMPL_AUTO):
    """``scipy.ndimage.grey_closing``: the erosion of the dilation."""
    f = _Filter(input, size, footprint, structure, output, mode, origin, impl)
    return f.R.out(f.run(f.run(f.R.t, True), False))


@_device_scoped
def white_tophat(input, size=None, footprint=None, structure=None, output=None, mode='reflect', cval=0.0, origin=0, *,
                 impl=IMPL_AUTO):
    """``scipy.ndimage.white_tophat``: the raster minus its opening, the subtraction made by the second launch."""
    f = _Filter(input, size, footprint, structure, output, mode, origin, impl)
    return f.R.out(f.run(f.run(f.R.t, False), True, sub=f.R.t, epilogue=SUB_MINUS))


@_device_scoped
def black_tophat(input, size=None, footprint=None, structure=None, output=None, mode='reflect', cval=0.0, origin=0, *,
                 impl=IMPL_AUTO):
    """``scipy.ndimage.black_tophat``: the closing minus the raster, the subtraction made by the second launch."""
    f = _Filter(input, size, footprint, structure, output, mode, origin, impl)
    return f.R.out(f.run(f.run(f.R.t, True), False, sub=f.R.t, epilogue=MINUS_SUB))


@_device_scoped
def morphological_gradient(input, size=None, footprint=None, structure=None, output=None, mode='reflect', cval=0.0,
                           origin=0, *, impl=IMPL_AUTO):
    """``scipy.ndimage.morphological_gradient``: the dilation minus the erosion.  One launch that reads each sample
    once when the footprint is its own mirror image; otherwise the two read different samples and the erosion's launch
    subtracts itself from the dilation."""
    f = _Filter(input, size, footprint, structure, output, mode, origin, impl)
    if f.symmetric():
        return f.R.out(f.run(f.R.t, False, epilogue=GRADIENT))
    return f.R.out(f.run(f.R.t, False, sub=f.run(f.R.t, True), epilogue=SUB_MINUS))
