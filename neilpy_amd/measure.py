"""Measurements of the objects of a label raster on the device, under scipy.ndimage's names (MI355X only).

``sum_labels``, ``mean``, ``variance``, ``standard_deviation``, ``minimum``, ``maximum``, ``extrema``, ``minimum_position``
and ``maximum_position`` take ``scipy.ndimage``'s parameters, same names, order and defaults, on a 2-D raster;
``region_stats`` is their device-resident form, a table per label as ``neilpy_amd.label.region_sizes`` gives the sizes.
The contract is DESIGN.md section 22.

Every value is the same on every run.  Extrema and positions are exact.  A sum is not the sequential fp64 sum SciPy makes
(no parallel kernel reproduces that): each value is cut into fixed-point integers relative to its label's largest
magnitude, the integers are added with 64-bit integer atomics and the total is rounded once, which depends on no order
and lies closer to the exact sum than SciPy's (``csrc/measure.hip``, ``csrc/measure_fixed.h``).  ``tests/measure_numpy.py``
restates all of it in plain Python.

NumPy in -> NumPy out; a CUDA tensor in -> CUDA tensors out on the same device (positions are host tuples either way).
There is no CPU fallback: argument errors come from the host before the device is touched, and a valid call without the
library or a GPU raises :class:`neilpy_amd.SmrfHipError`.

Deviations from SciPy (each in DESIGN.md section 22): ``labels`` must have ``input``'s shape (no broadcasting); ``index``
must be of integers; position ties go to the lowest C index; a scalar ``index`` that does not occur gives what an array
``index`` gives for it (SciPy raises for the extrema); rasters that are not 2-D, rasters of ``2**31`` cells or more and
64-bit integer input are refused with ``NotImplementedError``.
"""
import ctypes as C
import operator

import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._raster import _ptr, _stream, _torch
from ._xfer import to_host as _d2h
from .label import _Cells, _count, _integer_labels, _labels_int32, _max_label, _shape_2d

__all__ = ["sum_labels", "mean", "variance", "standard_deviation", "minimum", "maximum", "extrema", "minimum_position",
           "maximum_position", "region_stats"]

# include/smrf_measure.h: the measurement mask, a label's flag word, how the labels plane is read
WHAT = {"count": 1, "sum": 2, "mean": 4, "variance": 8, "min": 16, "max": 32, "min_index": 64, "max_index": 128, "flags": 256}
WHAT_ALL = 511
HAS_NAN, HAS_POS_INF, HAS_NEG_INF = 1, 2, 4
LABELS_AS_GIVEN, LABELS_POSITIVE = 0, 1
MAX_LABEL = 2 ** 31 - 2
STATS = ("count", "sum", "mean", "variance", "min", "max", "min_index", "max_index")
# what NumPy says of the least or largest of no value at all, which is what SciPy raises for an empty raster
EMPTY_ERROR = "zero-size array to reduction operation %s which has no identity"


class Out(C.Structure):
    """``smrf_measure_out``: one pointer per measurement, in the order of the mask's bits"""
    _fields_ = [(name, C.c_void_p) for name in WHAT]


_i, _p, _ll = C.c_int, C.c_void_p, C.c_longlong
SIGNATURES = {
    "smrf_measure_workspace_bytes": (_ll, [_ll, _i]),
    "smrf_measure_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _ll, _p]),
    "smrf_measure_f64": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _ll, _p]),
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


def mask_of(what):
    """the measurement mask of an iterable of names"""
    if isinstance(what, str):
        what = (what,)
    what = tuple(what)
    for name in what:
        if name not in WHAT:
            raise ValueError("unknown measurement %r: one of %s" % (name, ", ".join(STATS)))
    if not what:
        raise ValueError("no measurement asked for")
    m = 0
    for name in what:
        m |= WHAT[name]
    return m


def workspace_bytes(n, what):
    """the documented size of ``smrf_measure_*``'s workspace for labels ``0 .. n`` and a measurement mask"""
    L = n + 1
    up = lambda b: (b + 255) & ~255                                   # noqa: E731
    size = 4 * up(8 * L) + up(4 * L)
    if what & (WHAT["sum"] | WHAT["mean"] | WHAT["variance"]):
        size += up(24 * L) + up(8 * L)
    if what & (WHAT["min_index"] | WHAT["max_index"]):
        size += up(16 * L)
    if what & WHAT["variance"]:
        size += up(24 * L)
    return size


def passes_of(what):
    """how many of the three passes over the raster a measurement mask needs"""
    if what & WHAT["variance"]:
        return 3
    return 2 if what & (WHAT["sum"] | WHAT["mean"] | WHAT["min_index"] | WHAT["max_index"]) else 1


# ------------------------------------------------------------------------------------------
# arguments, on the host
# ------------------------------------------------------------------------------------------
def _values(input):
    """``input`` as an array, its shape, and the dtype results come back in (a NumPy dtype for an array, a torch dtype for
    a tensor); a dtype the kernels cannot be given exactly is refused"""
    input, shape = _shape_2d(input)
    dt = input.dtype
    if _is_tensor(input):
        if not dt.is_floating_point and dt != _torch().bool and input.element_size() > 4:
            raise NotImplementedError("64-bit integer input is not supported: float64 does not hold it")
        return input, shape, dt
    if dt.kind not in "biuf":
        raise TypeError("input must be of a real numeric dtype, got %s" % (dt,))
    if dt.kind in "iu" and dt.itemsize > 4:
        raise NotImplementedError("64-bit integer input is not supported: float64 does not hold it")
    if dt.kind == "f" and dt.itemsize > 8:
        raise NotImplementedError("input wider than float64 is not supported")
    return input, shape, dt


def _label_plane(labels, shape):
    if labels is None:
        return None
    labels, lshape = _integer_labels(labels)
    if lshape != shape:
        raise ValueError("labels of shape %s for an input of shape %s" % (lshape, shape))
    return labels


def _index(index):
    """``(scalar?, int64 array)`` of an ``index`` argument"""
    if _is_tensor(index):
        index = index.detach().cpu().numpy()
    if np.ndim(index) == 0:
        return True, np.array([operator.index(index)], dtype=np.int64)
    arr = np.asarray(index)
    if arr.size and arr.dtype.kind not in "iub":
        raise TypeError("index must be of integers, got %s" % (arr.dtype,))
    return False, arr.astype(np.int64)


# ------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------
def _empty_table(n, what, device, float_dtype):
    """the table of a raster without cells: every label is one that does not occur"""
    torch = _torch()
    fill = {"count": (0, torch.int64), "sum": (0.0, torch.float64), "mean": (float("nan"), torch.float64),
            "variance": (float("nan"), torch.float64), "min": (0, float_dtype), "max": (0, float_dtype),
            "min_index": (-1, torch.int64), "max_index": (-1, torch.int64), "flags": (0, torch.int32)}
    return {name: torch.full((n + 1,), fill[name][0], dtype=fill[name][1], device=device)
            for name, bit in WHAT.items() if what & bit}


def _measure_device(X, L, n, mode, what):
    """``{name: tensor of n + 1}`` for a contiguous float32 / float64 plane and an int32 plane or None"""
    torch = _torch()
    lib = _library()
    dtypes = {"count": torch.int64, "sum": torch.float64, "mean": torch.float64, "variance": torch.float64, "min": X.dtype,
              "max": X.dtype, "min_index": torch.int64, "max_index": torch.int64, "flags": torch.int32}
    res = {name: torch.empty(n + 1, dtype=dtypes[name], device=X.device) for name, bit in WHAT.items() if what & bit}
    out = Out(**{name: t.data_ptr() for name, t in res.items()})
    nbytes = int(lib.smrf_measure_workspace_bytes(n, what))
    if nbytes < 0:
        _lib.check(nbytes)
    work = torch.empty(nbytes, dtype=torch.uint8, device=X.device)
    fn = lib.smrf_measure_f32 if X.dtype == torch.float32 else lib.smrf_measure_f64
    _lib.check(fn(_ptr(X), _ptr(L), X.shape[0], X.shape[1], n, mode, what, C.cast(C.pointer(out), C.c_void_p), _ptr(work),
                  C.c_longlong(nbytes), _stream()))
    # the workspace is freed by the caching allocator on this stream only after the launches have used it
    return res


class _Table:
    """The table of one call: ``t[name]`` are device tensors of ``n + 1`` entries in the kernels' dtypes; ``out`` gives
    one back as the caller's kind of array, min and max in the input's dtype."""

    def __init__(self, input, labels, n, mode, what):
        input, shape, self.dtype = _values(input)
        labels = _label_plane(labels, shape)
        self.cols = shape[1]
        self.was_tensor = _is_tensor(input)
        torch = _torch()
        if shape[0] * shape[1] == 0:
            device = input.device if self.was_tensor else "cpu"
            self.n = n or 0
            self.t = _empty_table(self.n, what, device, torch.float64)
            return
        if not self.was_tensor and ((self.dtype.kind == "u" and self.dtype.itemsize > 1) or self.dtype.itemsize < 4 and self.dtype.kind == "f"):
            input = input.astype(np.float64 if self.dtype.kind == "u" else np.float32)      # no torch dtype for these: exact
        X = _Cells(input).t
        if X.dtype not in (torch.float32, torch.float64):
            X = X.to(torch.float32 if X.dtype.is_floating_point else torch.float64)      # exact
        L = None
        if labels is not None:
            L = _labels_int32(_Cells(labels, labels=True))
            if L.device != X.device:
                L = L.to(X.device)
        if n is None:
            n = _max_label(L) if L is not None else 1
        self.n = n
        self.t = _measure_device(X, L, n, mode, what)

    def out(self, name, t=None):
        t = self.t[name] if t is None else t
        if name in ("min", "max"):
            if self.was_tensor:
                return t.to(self.dtype)
            return _d2h(t).astype(self.dtype)
        return t if self.was_tensor else _d2h(t)


# ------------------------------------------------------------------------------------------
# the device-resident form
# ------------------------------------------------------------------------------------------
@_device_scoped
def region_stats(input, labels, num_features=None, what=STATS):
    """The measurements ``what`` of every label of ``labels`` over ``input``: a dict of arrays of length ``n + 1``, entry
    ``k`` for label ``k``, index 0 the background - :func:`neilpy_amd.label.region_sizes`' numbering.  ``n`` is
    ``num_features``, or with ``None`` the raster's maximum; cells below 0 or above ``n`` are ignored.

    ``count`` int64; ``sum``, ``mean``, ``variance`` float64; ``min``, ``max`` in ``input``'s dtype (0 for a label that
    does not occur); ``min_index``, ``max_index`` int64 linear C indices, ties to the lowest, -1 for a label that does
    not occur.  Only what ``what`` names is computed, in the fewest of the three passes over the raster that serve it:
    one for counts and extrema, two with sums, means or positions, three with the variance."""
    mask = mask_of(what)
    if mask & WHAT["flags"]:
        raise ValueError("unknown measurement 'flags': one of %s" % ", ".join(STATS))
    if labels is None:
        raise TypeError("region_stats needs a label raster")
    n = _count(num_features, "num_features")
    if n is not None and n > MAX_LABEL:
        raise ValueError("num_features exceeds what a raster of fewer than 2**31 cells can hold")
    T = _Table(input, labels, n, LABELS_AS_GIVEN, mask)
    return {name: T.out(name) for name in WHAT if mask & WHAT[name]}


# ------------------------------------------------------------------------------------------
# scipy.ndimage's forms of labels and index
# ------------------------------------------------------------------------------------------
MISSING = {"sum": 0.0, "mean": float("nan"), "variance": float("nan"), "min": 0, "max": 0, "min_index": -1, "max_index": -1}


def _select(input, labels, index, names):
    """``[result per name]`` under SciPy's rules: ``labels=None`` the whole raster, ``index=None`` the cells with a
    positive label, a scalar ``index`` a scalar, an array ``index`` an array in its order"""
    what = mask_of(names)
    single = labels is None or index is None
    if single:
        scalar, idx, n, mode = True, np.array([1], dtype=np.int64), 1, LABELS_POSITIVE
    else:
        scalar, idx = _index(index)
        n, mode = int(min(max(int(idx.max()) if idx.size else 0, 0), MAX_LABEL)), LABELS_AS_GIVEN
    if scalar and what & (WHAT["min"] | WHAT["max"]):
        what |= WHAT["flags"]                    # np.min and np.max of one selection: NaN where a NaN is present
    T = _Table(input, labels, n, mode, what)
    # the gather: plumbing by torch, where the table lies (the host for a NumPy raster without cells)
    torch = _torch()
    found = (idx >= 0) & (idx <= T.n)
    results = []
    for name in names:
        t = T.t[name]
        at = torch.as_tensor(np.where(found, idx, 0), device=t.device)
        g = t[at]
        if not found.all():
            g = torch.where(torch.as_tensor(found, device=t.device), g, torch.full_like(g, MISSING[name]))
        if scalar and name in ("min", "max"):
            nan = (T.t["flags"][at] & HAS_NAN) != 0
            g = torch.where(nan, torch.full_like(g, float("nan")), g)
        g = T.out(name, g)
        results.append(g[0] if scalar else g)
    return results, T


def _no_cells(input):
    shape = tuple(input.shape) if _is_tensor(input) else np.shape(input)
    return len(shape) == 2 and shape[0] * shape[1] == 0


def _empty_refusal(input, labels, index, extremum=None):
    """An empty raster raises what SciPy raises for it: the extrema have no identity, and with an array ``index`` SciPy
    asks the labels for their least and largest first, whatever is measured"""
    if not _no_cells(input):
        return
    if extremum is not None and not (labels is not None and index is not None and np.ndim(index) != 0):
        raise ValueError(EMPTY_ERROR % extremum)
    if labels is not None and index is not None and np.ndim(index) != 0:
        raise ValueError(EMPTY_ERROR % ("minimum" if extremum is None else "maximum"))


def _check(input, labels, index, extremum=None):
    """the argument rules, then what an empty raster raises: all on the host, before the device is touched"""
    _, shape, _ = _values(input)
    _label_plane(labels, shape)
    _empty_refusal(input, labels, index, extremum)


def _position(T, linear):
    """a linear C index, or an array of them, as SciPy's tuple of Python ints, or list of tuples; (0, 0) where there is
    none"""
    arr = linear.cpu().numpy() if _is_tensor(linear) else np.asarray(linear)
    cols = max(T.cols, 1)
    if arr.ndim == 0:
        v = max(int(arr), 0)
        return (v // cols, v % cols)
    return [(max(int(v), 0) // cols, max(int(v), 0) % cols) for v in arr]


@_device_scoped
def sum_labels(input, labels=None, index=None):
    """``scipy.ndimage.sum_labels`` of a 2-D raster: the fixed-point sum of DESIGN.md section 22 of each selection, float64;
    0.0 for a label that does not occur"""
    _check(input, labels, index)
    return _select(input, labels, index, ("sum",))[0][0]


@_device_scoped
def mean(input, labels=None, index=None):
    """``scipy.ndimage.mean``: the sum over the count, one fp64 division; NaN for a label that does not occur"""
    _check(input, labels, index)
    return _select(input, labels, index, ("mean",))[0][0]


@_device_scoped
def variance(input, labels=None, index=None):
    """``scipy.ndimage.variance``: the fixed-point sum of the squared differences from the mean, over the count (the
    two-pass form, as SciPy's); NaN for a label that does not occur"""
    _check(input, labels, index)
    return _select(input, labels, index, ("variance",))[0][0]


@_device_scoped
def standard_deviation(input, labels=None, index=None):
    """``scipy.ndimage.standard_deviation``: the square root of :func:`variance`"""
    v = variance(input, labels, index)
    return v.sqrt() if _is_tensor(v) else np.sqrt(v)


@_device_scoped
def minimum(input, labels=None, index=None):
    """``scipy.ndimage.minimum``, in ``input``'s dtype: with an array ``index`` the first of ``np.sort`` of each label's
    values (NaN only where every value is NaN) and 0 for a label that does not occur; otherwise ``np.min`` of the
    selection (NaN where a NaN is present)"""
    _check(input, labels, index, "minimum")
    return _select(input, labels, index, ("min",))[0][0]


@_device_scoped
def maximum(input, labels=None, index=None):
    """``scipy.ndimage.maximum``, in ``input``'s dtype: the last of ``np.sort`` of each label's values (NaN where a NaN is
    present); 0 for a label that does not occur"""
    _check(input, labels, index, "maximum")
    return _select(input, labels, index, ("max",))[0][0]


@_device_scoped
def minimum_position(input, labels=None, index=None):
    """``scipy.ndimage.minimum_position``: a tuple of Python ints, or a list of them for an array ``index``; ties go to the
    lowest C index, ``(0, 0)`` for a label that does not occur.  The result is read to the host."""
    _check(input, labels, index, "minimum")
    (pos,), T = _select(input, labels, index, ("min_index",))
    return _position(T, pos)


@_device_scoped
def maximum_position(input, labels=None, index=None):
    """``scipy.ndimage.maximum_position``: as :func:`minimum_position`; ties go to the lowest C index here too"""
    _check(input, labels, index, "maximum")
    (pos,), T = _select(input, labels, index, ("max_index",))
    return _position(T, pos)


@_device_scoped
def extrema(input, labels=None, index=None):
    """``scipy.ndimage.extrema``: ``(minimums, maximums, min_positions, max_positions)`` from one call of the kernels"""
    _check(input, labels, index, "minimum")
    (lo, hi, lo_at, hi_at), T = _select(input, labels, index, ("min", "max", "min_index", "max_index"))
    return lo, hi, _position(T, lo_at), _position(T, hi_at)
