"""Connected components of a raster on the device, under scipy.ndimage's names (MI355X only).

``label`` and ``find_objects`` take ``scipy.ndimage``'s parameters, same names, order and defaults, and give its values
for a 2-D raster; ``region_sizes``, ``bounding_boxes`` and ``remove_small_objects`` are what usually follows them, kept on
the device.  The contract is DESIGN.md section 21.

``label`` numbers the objects from 1 in the C order of their first cells: object ``k`` is the one whose first cell comes
``k``-th among all objects' first cells.  That is SciPy's numbering for every structure it accepts, so the result equals
SciPy's bit for bit, and it is the same on every run: ``csrc/label.hip`` unites cells by an atomic minimum on linear
indices, which makes every object's root its first cell whatever order the atomics land in, and numbers the roots by a
scan.  A structure is a 3 x 3 array; SciPy accepts exactly the centrally symmetric ones and ignores the centre, which
leaves four links (E, S, SE, SW) and 16 structures, all served by one kernel through a 4-bit link mask
(``smrf_label_links``, include/smrf_label.h).

NumPy in -> NumPy out; a CUDA tensor in -> CUDA tensors out on the same device.  There is no CPU fallback: argument
errors come from the host before the device is touched, and a valid call without the library or a GPU raises
:class:`neilpy_amd.SmrfHipError`.

Deviations from SciPy (each in DESIGN.md section 21): ``output=`` other than ``None`` or ``int32``, rasters that are not
2-D and rasters of ``2**31`` cells or more are refused with ``NotImplementedError``; complex input is refused with
``TypeError`` as in SciPy.
"""
import ctypes as C
import operator

import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._raster import Raster, _ptr, _stream, _torch
from ._xfer import to_device as _h2d

__all__ = ["label", "region_sizes", "bounding_boxes", "find_objects", "remove_small_objects"]

# include/smrf_label.h: the four links of a structure, the tile and the cells per block of the numbering scan
LINK_E, LINK_S, LINK_SE, LINK_SW = 1, 2, 4, 8
TILE_ROWS, TILE_COLS, SCAN_BLOCK = 64, 64, 2048
MAX_CELLS = 2 ** 31
# what scipy.ndimage.label raises for a structure that is not centrally symmetric
ASYMMETRIC_ERROR = AssertionError

# name -> (result, arguments).  Attached to the library on first use.
_i, _p, _ll = C.c_int, C.c_void_p, C.c_longlong
SIGNATURES = {
    "smrf_label_links": (_i, [_p]),
    "smrf_label_workspace_bytes": (_ll, [_i, _i]),
    "smrf_label_u8": (_i, [_p, _p, _i, _i, _i, _p, _ll, _p, _p]),
    "smrf_label_regions": (_i, [_p, _i, _i, _i, _p, _p, _p]),
    "smrf_label_keep": (_i, [_p, _p, _ll, _ll, _p, _p]),
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


def workspace_bytes(rows, cols):
    """the documented size of ``smrf_label_u8``'s workspace: one int32 plane and one uint32 per SCAN_BLOCK cells, each
    rounded up to 256 bytes"""
    cells = rows * cols
    up = lambda b: (b + 255) & ~255                                   # noqa: E731
    return up(4 * cells) + up(4 * ((cells + SCAN_BLOCK - 1) // SCAN_BLOCK)) if cells else 0


# ------------------------------------------------------------------------------------------
# arguments, on the host
# ------------------------------------------------------------------------------------------
def _shape_2d(X):
    """an array-like argument as an array, and its shape: 2-D with fewer than 2**31 cells, or it is refused before the device
    is touched"""
    if not _is_tensor(X):
        X = np.asarray(X)
    shape = tuple(X.shape)
    if len(shape) != 2:
        raise NotImplementedError("only 2-D rasters are supported on the device")
    if shape[0] * shape[1] >= MAX_CELLS:
        raise NotImplementedError("rasters of 2**31 cells or more are not supported: cell indices are int32")
    if X.dtype.is_complex if _is_tensor(X) else np.iscomplexobj(X):
        raise TypeError('Complex type not supported')
    return X, shape


def links_of(structure):
    """The 4-bit link mask of ``structure`` for a 2-D raster (``None``: SciPy's default, the 4-neighbourhood), with
    SciPy's refusals: ``RuntimeError`` for another rank, ``ValueError`` for another shape, and for a structure that is
    not centrally symmetric what :data:`ASYMMETRIC_ERROR` names."""
    if structure is None:
        return LINK_E | LINK_S
    if _is_tensor(structure):
        structure = structure.detach().cpu().numpy()
    s = np.asarray(structure, dtype=bool)
    if s.ndim != 2:
        raise RuntimeError('structure and input must have equal rank')
    if s.shape != (3, 3):
        raise ValueError('structure dimensions must be equal to 3')
    flat = np.ascontiguousarray(s, dtype=np.uint8).reshape(9)
    links = _library().smrf_label_links(flat.ctypes.data_as(C.c_void_p))
    if links < 0:
        raise ASYMMETRIC_ERROR('Structuring element is not symmetric')
    return links


class _Cells(Raster):
    """:class:`Raster`'s boundary for a raster whose cells keep the caller's dtype (Raster widens to float): ``t`` is
    the contiguous device tensor of any 2-D view, NumPy or tensor"""

    __slots__ = ()

    def __init__(self, X, labels=False):
        self.was_tensor = _is_tensor(X)
        _lib.require_gpu()
        if self.was_tensor:
            t = X
        else:
            arr = np.asarray(X)
            if (arr.dtype.kind not in "bif" and arr.dtype != np.uint8) or arr.dtype.itemsize > 8:
                # a dtype torch does not take or compare on the device (the wider unsigned integers, long double): labels
                # are clamped into int32 here as _labels_int32 clamps the others there, of a mask only `!= 0` is asked
                arr = np.minimum(arr, 2 ** 31 - 1).astype(np.int32) if labels else arr != 0
            t = _h2d(arr)
        if not t.is_cuda:
            t = t.cuda()
        self.t = t.contiguous()
        self.rows, self.cols = self.t.shape


def _byte_mask(t):
    """``t != 0`` as a contiguous byte plane: bool and uint8 are read as they are, anything else is compared by torch on
    the device (NaN is non-zero, -0.0 is zero)"""
    torch = _torch()
    if t.dtype == torch.uint8:
        return t
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return (t != 0).view(torch.uint8)


def _labels_int32(R):
    """a raster of labels as int32 on the device; integers beyond int32 are clamped into it first (they lie above every
    label count a raster can hold, or below zero: ignored either way)"""
    torch = _torch()
    t = R.t
    if t.dtype == torch.int32:
        return t
    if t.element_size() >= 4:
        t = t.clamp(min=-1, max=2 ** 31 - 1) if t.dtype.is_signed else t.clamp(max=2 ** 31 - 1)
    return t.to(torch.int32)


def _integer_labels(input):
    """find_objects' and the region functions' first argument: 2-D, of an integer (or bool) dtype"""
    input, shape = _shape_2d(input)
    dt = input.dtype
    integral = not (dt.is_floating_point or dt.is_complex) if _is_tensor(input) else dt.kind in "iub"
    if not integral:
        raise TypeError("labels must be of an integer dtype, got %s" % (dt,))
    return input, shape


def _count(value, name):
    if value is None:
        return None
    n = operator.index(value)
    if n < 0:
        raise ValueError("%s must not be negative" % name)
    if n >= MAX_CELLS:
        raise ValueError("%s exceeds what a raster of fewer than 2**31 cells can hold" % name)
    return n


# ------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------
def _label_device(mask, links):
    """``(labels int32 tensor, count int32 tensor of one element)`` of a contiguous byte plane, all on the device"""
    torch = _torch()
    lib = _library()
    rows, cols = mask.shape
    labels = torch.empty((rows, cols), dtype=torch.int32, device=mask.device)
    count = torch.empty(1, dtype=torch.int32, device=mask.device)
    nbytes = int(lib.smrf_label_workspace_bytes(rows, cols))
    if nbytes < 0:
        _lib.check(nbytes)
    work = torch.empty(nbytes, dtype=torch.uint8, device=mask.device) if nbytes else None
    _lib.check(lib.smrf_label_u8(_ptr(mask), _ptr(labels), rows, cols, links, _ptr(work), C.c_longlong(nbytes), _ptr(count),
                                 _stream()))
    # the workspace is freed by the caching allocator on this stream only after the launches have used it
    return labels, count


def _regions_device(L, n, want_size, want_box):
    """``(sizes int64 (n + 1) | None, boxes int32 (n, 4) | None)`` of a contiguous int32 plane"""
    torch = _torch()
    size = torch.empty(n + 1, dtype=torch.int64, device=L.device) if want_size else None
    box = torch.empty((n, 4), dtype=torch.int32, device=L.device) if want_box else None
    if n == 0 and not want_size:
        return None, box                                   # no label: an empty table, nothing to launch
    _lib.check(_library().smrf_label_regions(_ptr(L), L.shape[0], L.shape[1], n, _ptr(size), _ptr(box), _stream()))
    return size, box


def _max_label(L):
    """the raster's largest label, at least 0: one reduction by torch and one 4-byte read"""
    return max(int(L.max().item()), 0) if L.numel() else 0


# ------------------------------------------------------------------------------------------
# the public functions
# ------------------------------------------------------------------------------------------
@_device_scoped
def label(input, structure=None, output=None):
    """``scipy.ndimage.label`` of a 2-D raster: ``(labels, num_features)``, ``labels`` an int32 ``rows x cols`` array with
    0 for background and the objects numbered from 1 in the C order of their first cells, bit for bit SciPy's.

    A cell is foreground iff its value is ``!= 0`` (NaN is foreground).  ``bool`` and ``uint8`` rasters are read as they
    are; any other dtype is turned into a byte mask by torch on the device first.  ``structure``: ``None`` (the
    4-neighbourhood) or any 3 x 3 structure SciPy accepts.  ``output``: ``None`` or ``np.int32``.  ``num_features`` is a
    Python ``int``: bringing it to the host costs one 4-byte read, which also waits for the launches."""
    input, shape = _shape_2d(input)
    links = links_of(structure)
    if output is not None:
        if isinstance(output, np.ndarray) or _is_tensor(output):
            raise NotImplementedError("output= as an array to fill is not supported")
        try:
            same = np.dtype(output) == np.int32
        except TypeError:
            same = False
        if not same:
            raise NotImplementedError("output= other than int32 is not supported")
    if shape[0] * shape[1] == 0:
        if _is_tensor(input):
            return _torch().empty(shape, dtype=_torch().int32, device=input.device), 0
        return np.empty(shape, np.int32), 0
    R = _Cells(input)
    labels, count = _label_device(_byte_mask(R.t), links)
    return R.out(labels), int(count.item())


@_device_scoped
def region_sizes(labels, num_features=None):
    """The cell count of every label: an int64 array of length ``n + 1`` equal to
    ``np.bincount(labels.ravel(), minlength=n + 1)`` for labels in ``0 .. n``; index 0 is the background.  ``n`` is
    ``num_features``, or with ``None`` the raster's maximum (a reduction by torch and one 4-byte read).  Cells below 0 or
    above ``n`` are ignored."""
    labels, shape = _integer_labels(labels)
    n = _count(num_features, "num_features")
    torch = _torch()
    if shape[0] * shape[1] == 0:
        n = n or 0
        if _is_tensor(labels):
            return torch.zeros(n + 1, dtype=torch.int64, device=labels.device)
        return np.zeros(n + 1, np.int64)
    R = _Cells(labels, labels=True)
    L = _labels_int32(R)
    size, _ = _regions_device(L, _max_label(L) if n is None else n, True, False)
    return R.out(size)


@_device_scoped
def bounding_boxes(labels, num_features=None):
    """The bounding box of every label ``1 .. n``: an ``(n, 4)`` int32 array of ``r0, r1, c0, c1``, half-open, so
    that ``labels[r0:r1, c0:c1]`` is label ``k + 1``'s box for row ``k``; ``(0, 0, 0, 0)`` for a label that does not occur.
    This is :func:`find_objects`' device-resident form.  ``n`` as in :func:`region_sizes`."""
    labels, shape = _integer_labels(labels)
    n = _count(num_features, "num_features")
    torch = _torch()
    if shape[0] * shape[1] == 0:
        n = n or 0
        if _is_tensor(labels):
            return torch.zeros((n, 4), dtype=torch.int32, device=labels.device)
        return np.zeros((n, 4), np.int32)
    R = _Cells(labels, labels=True)
    L = _labels_int32(R)
    _, box = _regions_device(L, _max_label(L) if n is None else n, False, True)
    return R.out(box)


@_device_scoped
def find_objects(input, max_label=0):
    """``scipy.ndimage.find_objects`` of a 2-D raster of integer labels: a host list of ``(slice, slice)`` tuples, entry
    ``k`` the bounding box of label ``k + 1``, ``None`` for a label that does not occur.  Cells ``<= 0`` or above
    ``max_label`` are ignored; ``max_label`` below 1 means the raster's maximum (taken with torch), and an all-zero
    raster gives ``[]``.  Built from :func:`bounding_boxes`: one launch and one copy of ``4 * max_label`` integers."""
    input, shape = _integer_labels(input)
    max_label = operator.index(max_label)
    if max_label >= MAX_CELLS:
        raise ValueError("max_label exceeds what a raster of fewer than 2**31 cells can hold")
    if shape[0] * shape[1] == 0:
        if max_label < 1:
            raise ValueError("zero-size array to reduction operation maximum which has no identity")
        return [None] * max_label
    R = _Cells(input, labels=True)
    L = _labels_int32(R)
    n = _max_label(L) if max_label < 1 else max_label
    if n == 0:
        return []
    _, box = _regions_device(L, n, False, True)
    rows = box.cpu().numpy().tolist()
    return [(slice(r0, r1, None), slice(c0, c1, None)) if r1 else None for r0, r1, c0, c1 in rows]


@_device_scoped
def remove_small_objects(mask, min_size=64, connectivity=1):
    """The cells of ``mask`` that belong to objects of at least ``min_size`` cells, as a ``bool`` raster.
    ``connectivity`` 1 is the 4-neighbourhood, 2 the 8-neighbourhood.  Label, sizes and the keep pass all run on the
    device; the object count is the only value read in between.

    Any input is taken as the mask ``mask != 0`` and labelled here.  This is the project's own rule, not scikit-image's,
    which treats an integer array as a label image and keeps its labels."""
    mask, shape = _shape_2d(mask)
    min_size = operator.index(min_size)
    if min_size < 0:
        raise ValueError("min_size must not be negative")
    if connectivity not in (1, 2):
        raise ValueError("connectivity must be 1 or 2 for a 2-D raster, got %r" % (connectivity,))
    links = LINK_E | LINK_S | (LINK_SE | LINK_SW if connectivity == 2 else 0)
    torch = _torch()
    if shape[0] * shape[1] == 0:
        if _is_tensor(mask):
            return torch.empty(shape, dtype=torch.bool, device=mask.device)
        return np.empty(shape, bool)
    R = _Cells(mask)
    labels, count = _label_device(_byte_mask(R.t), links)
    size, _ = _regions_device(labels, int(count.item()), True, False)
    out = torch.empty((R.rows, R.cols), dtype=torch.uint8, device=labels.device)
    _lib.check(_library().smrf_label_keep(_ptr(labels), _ptr(size), C.c_longlong(labels.numel()),
                                          C.c_longlong(min(min_size, 2 ** 62)), _ptr(out), _stream()))
    return R.out(out.view(torch.bool))
