"""Binary morphology of a raster on the device, under scipy.ndimage's names (MI355X only).

``binary_erosion``, ``binary_dilation``, ``binary_opening``, ``binary_closing``, ``binary_hit_or_miss``,
``binary_propagation`` and ``binary_fill_holes`` take ``scipy.ndimage``'s parameters, same names, order and defaults, and
give its bits for a 2-D raster.  The contract is DESIGN.md section 23.

A raster travels as a bit plane, 64 cells of a row to a word (``csrc/binary.hip``, ``csrc/binary_bits.h``): one lane makes
64 cells of a step from shifted words, for a structure of any size and origin.  ``iterations < 1`` launches steps in
batches of :data:`CHECK_EVERY` and reads one flag per batch.  ``binary_propagation`` and ``binary_fill_holes`` under a
centrally symmetric 3 x 3 structure with its centre set do not iterate at all: the converged result is read off the
components of the mask, which ``smrf_label_u8`` gives in six launches whatever the paths (``impl='labels'``, the default
where it applies; ``impl='iterate'`` forces the steps).

NumPy in -> NumPy out; a CUDA tensor in -> a CUDA tensor out on the same device.  There is no CPU fallback: argument
errors come from the host before the device is touched, and a valid call without the library or a GPU raises
:class:`neilpy_amd.SmrfHipError`.

Deviations from SciPy (each in DESIGN.md section 23): an origin outside ``-(n // 2) <= origin <= (n - 1) // 2`` for a
structure axis of length ``n`` raises ``ValueError`` (SciPy 1.15 reads out of bounds there); ``iterations < 1`` with a
structure whose centre is not a member raises ``NotImplementedError`` (the steps need not converge); ``output=`` other than
``None`` or ``bool``, ``axes`` other than ``None`` or both axes, rasters that are not 2-D and rasters of ``2**31`` cells or
more are refused with ``NotImplementedError``.
"""
import ctypes as C
import operator

import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._raster import _ptr, _stream, _torch
from .label import LINK_E, LINK_S, LINK_SE, LINK_SW, MAX_CELLS, _Cells, _byte_mask

__all__ = ["binary_erosion", "binary_dilation", "binary_opening", "binary_closing", "binary_hit_or_miss",
           "binary_propagation", "binary_fill_holes"]

# include/smrf_binary.h: the op of a step
ERODE, DILATE = 0, 1
# steps launched between two reads of the "changed" flags where iterations < 1 (profiles/binary_bench.md)
CHECK_EVERY = 16
IMPLS = (None, "labels", "iterate")

# name -> (result, arguments).  Attached to the library on first use.
_i, _p, _ll = C.c_int, C.c_void_p, C.c_longlong
SIGNATURES = {
    "smrf_binary_offsets": (_i, [_p, _i, _i, _i, _i, _i, _p]),
    "smrf_binary_plane_bytes": (_ll, [_i, _i]),
    "smrf_binary_pack": (_i, [_p, _p, _i, _i, _i, _p]),
    "smrf_binary_unpack": (_i, [_p, _p, _i, _i, _i, _p]),
    "smrf_binary_step": (_i, [_p, _p, _i, _i, _p, _p, _i, _i, _i, _p, _p]),
    "smrf_binary_hit_or_miss": (_i, [_p, _p, _i, _i, _p, _i, _p, _i, _p]),
    "smrf_binary_propagate_workspace_bytes": (_ll, [_i, _i]),
    "smrf_binary_propagate": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _ll, _p]),
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


def plane_bytes(rows, cols):
    """the size of a bit plane: one 64-bit word per 64 cells of a row"""
    return 8 * rows * ((cols + 63) // 64)


def propagate_workspace_bytes(rows, cols):
    """the documented size of ``smrf_binary_propagate``'s workspace: the labels plane, label's own workspace, the flag
    plane of ``cells + 1`` bytes, three bit planes and 256 bytes for the object count, each rounded up to 256 bytes"""
    from .label import workspace_bytes
    cells = rows * cols
    up = lambda b: (b + 255) & ~255                                   # noqa: E731
    if not cells:
        return 0
    return up(4 * cells) + workspace_bytes(rows, cols) + up(cells + 1) + 3 * up(plane_bytes(rows, cols)) + 256


# ------------------------------------------------------------------------------------------
# arguments, on the host
# ------------------------------------------------------------------------------------------
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)


def _raster_2d(X):
    """the raster argument and its shape: 2-D, fewer than 2**31 cells, not complex, or refused before the device is touched"""
    if not _is_tensor(X):
        X = np.asarray(X)
    if X.dtype.is_complex if _is_tensor(X) else np.iscomplexobj(X):
        raise TypeError('Complex type not supported')
    shape = tuple(X.shape)
    if len(shape) != 2:
        raise NotImplementedError("only 2-D rasters are supported on the device")
    if shape[0] * shape[1] >= MAX_CELLS:
        raise NotImplementedError("rasters of 2**31 cells or more are not supported: cell indices are int32")
    return X, shape


def _structure(structure, dilates=False):
    """a structure argument as a 2-D bool array (``None``: the 4-neighbourhood), with SciPy's refusals.  ``dilates``: the
    function dilates first; SciPy's dilation walks the input's axes over the structure's shape before it compares the
    ranks, so a structure of a lower rank is an ``IndexError`` there"""
    if structure is None:
        return CROSS
    if _is_tensor(structure):
        structure = structure.detach().cpu().numpy()
    s = np.asarray(structure).astype(bool)
    if s.ndim != 2:
        if dilates and s.ndim < 2:
            raise IndexError('tuple index out of range')
        raise RuntimeError('structure and input must have same dimensionality')
    if s.size < 1:
        raise RuntimeError('structure must not be empty')
    return np.ascontiguousarray(s)


def _origin(origin):
    """``origin`` as two integers: a scalar for both axes or a sequence of two"""
    if hasattr(origin, "__iter__") and not isinstance(origin, str):
        o = list(origin)
        if len(o) != 2:
            raise RuntimeError("sequence argument must have length equal to input rank")
    else:
        o = [origin, origin]
    return operator.index(o[0]), operator.index(o[1])


def _table(s, origin, reflect):
    """the member table of a structure about its origin as ``smrf_binary_offsets`` writes it, an int32 array of (dr, dc)
    rows; ``ValueError`` for an origin outside the structure's accepted range"""
    for n, o in zip(s.shape, origin):
        if not -(n // 2) <= o <= (n - 1) // 2:
            raise ValueError("origin %r lies outside -(n // 2) <= origin <= (n - 1) // 2 for a structure of shape %r" % (
                tuple(origin), s.shape))
    flat = np.ascontiguousarray(s, dtype=np.uint8)
    out = np.zeros((max(int(flat.sum()), 1), 2), dtype=np.int32)
    n = _library().smrf_binary_offsets(flat.ctypes.data_as(C.c_void_p), s.shape[0], s.shape[1], origin[0], origin[1],
                                       int(reflect), out.ctypes.data_as(C.c_void_p))
    if n < 0:
        raise ValueError("origin %r is not accepted for a structure of shape %r" % (tuple(origin), s.shape))
    return out[:n]


def _centre_is_member(s, origin):
    r, c = s.shape[0] // 2 + origin[0], s.shape[1] // 2 + origin[1]
    return bool(s[r, c])


def _check_common(output, axes):
    if output is not None:
        if isinstance(output, np.ndarray) or _is_tensor(output):
            raise NotImplementedError("output= as an array to fill is not supported")
        try:
            same = np.dtype(output) == np.bool_
        except TypeError:
            same = False
        if not same:
            raise NotImplementedError("output= other than bool is not supported")
    if axes is not None:
        try:
            ax = tuple(operator.index(a) for a in axes)
        except TypeError:
            ax = None
        if ax not in ((0, 1), (-2, -1), (0, -1), (-2, 1)):
            raise NotImplementedError("axes= other than None or both axes in order is not supported")


def _mask_arg(mask, shape):
    if mask is None:
        return None
    if not _is_tensor(mask):
        mask = np.asarray(mask)
    if tuple(mask.shape) != shape:
        raise RuntimeError('mask and input must have equal sizes')
    return mask


def _empty_like(input, shape):
    if _is_tensor(input):
        return _torch().empty(shape, dtype=_torch().bool, device=input.device)
    return np.empty(shape, bool)


class _Spec:
    """one run of steps, decided on the host: the table, the op, the border value and the number of steps"""

    __slots__ = ("table", "op", "border", "iterations")

    def __init__(self, s, origin, op, border_value, iterations):
        self.table = _table(s, origin, reflect=op == DILATE)
        self.op = op
        self.border = int(bool(border_value))
        self.iterations = iterations
        if iterations < 1 and not _centre_is_member(s, origin):
            raise NotImplementedError("iterations < 1 needs the structure's centre (at its origin) to be a member: "
                                      "otherwise the steps need not converge")


# ------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------
class _Planes:
    """the bit planes of one call on the device: pack, the steps in ping-pong, unpack"""

    def __init__(self, R):
        self.torch = _torch()
        self.lib = _library()
        self.rows, self.cols = R.rows, R.cols
        self.device = R.t.device
        self.words = self.rows * ((self.cols + 63) // 64)

    def plane(self):
        return self.torch.empty(self.words, dtype=self.torch.int64, device=self.device)

    def pack(self, bytes_, complement=False):
        bits = self.plane()
        _lib.check(self.lib.smrf_binary_pack(_ptr(bytes_), _ptr(bits), self.rows, self.cols, int(complement), _stream()))
        return bits

    def unpack(self, bits, complement=False):
        out = self.torch.empty((self.rows, self.cols), dtype=self.torch.uint8, device=self.device)
        _lib.check(self.lib.smrf_binary_unpack(_ptr(bits), _ptr(out), self.rows, self.cols, int(complement), _stream()))
        return out.view(self.torch.bool)

    def table(self, table):
        """a member table on the device; None for a structure without members"""
        if not len(table):
            return None
        return self.torch.from_numpy(np.ascontiguousarray(table)).to(self.device, non_blocking=False)

    def run(self, cur, spec, mask_bits):
        """``spec.iterations`` steps from the plane ``cur`` (which the steps may overwrite), or with ``iterations < 1``
        steps until one changes nothing; returns the plane that holds the result.  Steps go out in batches of
        CHECK_EVERY with one flag each and the flags are read once per batch, and only where more steps would follow: a
        step that changed nothing ends the run, for the steps after it would change nothing either."""
        torch = self.torch
        table = self.table(spec.table)
        n = len(spec.table)
        left = spec.iterations if spec.iterations >= 1 else None
        nxt = self.plane()
        stream = _stream()
        while left is None or left > 0:
            batch = CHECK_EVERY if left is None else min(CHECK_EVERY, left)
            more = left is None or left > batch
            flags = torch.zeros(batch, dtype=torch.int32, device=self.device) if more else None
            for k in range(batch):
                flag = C.c_void_p(flags.data_ptr() + 4 * k) if more else C.c_void_p(0)
                _lib.check(self.lib.smrf_binary_step(_ptr(cur), _ptr(nxt), self.rows, self.cols, _ptr(mask_bits), _ptr(table), n,
                                                     spec.op, spec.border, flag, stream))
                cur, nxt = nxt, cur
            if left is not None:
                left -= batch
            if more and int(flags[batch - 1].item()) == 0:
                break
        return cur

    def hit_or_miss(self, cur, hit, miss):
        out = self.plane()
        th, tm = self.table(hit), self.table(miss)
        _lib.check(self.lib.smrf_binary_hit_or_miss(_ptr(cur), _ptr(out), self.rows, self.cols, _ptr(th), len(hit), _ptr(tm),
                                                    len(miss), _stream()))
        return out


def _morph(input, specs_of, mask, output, axes):
    """the common path of erosion, dilation, opening and closing: ``specs_of()`` makes the runs of steps (and refuses bad
    arguments) before the device is touched"""
    input, shape = _raster_2d(input)
    specs = specs_of()
    mask = _mask_arg(mask, shape)
    _check_common(output, axes)
    if shape[0] * shape[1] == 0:
        return _empty_like(input, shape)
    R = _Cells(input)
    P = _Planes(R)
    mask_bits = None
    if mask is not None:
        mask_bits = P.pack(_byte_mask(_Cells(mask).t.to(R.t.device)))
    cur = P.pack(_byte_mask(R.t))
    for spec in specs:
        cur = P.run(cur, spec, mask_bits)
    return R.out(P.unpack(cur))


def _label_links(s, origin):
    """the link mask of a structure the label route serves - 3 x 3, centrally symmetric, centre set, origin 0 - or None"""
    if s.shape != (3, 3) or tuple(origin) != (0, 0) or not s[1, 1] or not np.array_equal(s, s[::-1, ::-1]):
        return None
    return LINK_E * bool(s[1, 2]) | LINK_S * bool(s[2, 1]) | LINK_SE * bool(s[2, 2]) | LINK_SW * bool(s[2, 0])


def _propagate(R, input_bytes, mask_bytes, s, origin, border_value, impl, complement):
    """binary_propagation of byte planes on the device (``input_bytes`` None: all zeros), complemented for fill_holes:
    through the components of the mask where the structure allows it, by steps otherwise"""
    torch = _torch()
    lib = _library()
    links = _label_links(s, origin)
    if impl == "labels" and links is None:
        raise ValueError("impl='labels' needs a centrally symmetric 3 x 3 structure with its centre set and origin 0")
    if impl != "iterate" and links is not None:
        nbytes = int(lib.smrf_binary_propagate_workspace_bytes(R.rows, R.cols))
        if nbytes < 0:
            _lib.check(nbytes)
        work = torch.empty(nbytes, dtype=torch.uint8, device=R.t.device)
        out = torch.empty((R.rows, R.cols), dtype=torch.uint8, device=R.t.device)
        _lib.check(lib.smrf_binary_propagate(_ptr(input_bytes), _ptr(mask_bytes), _ptr(out), R.rows, R.cols, links,
                                             int(bool(border_value)), int(complement), _ptr(work), C.c_longlong(nbytes),
                                             _stream()))
        return out.view(torch.bool)
    spec = _Spec(s, origin, DILATE, border_value, -1)
    P = _Planes(R)
    mask_bits = P.pack(mask_bytes)
    if input_bytes is None:
        cur = P.plane().zero_()
    else:
        cur = P.pack(input_bytes)
    return P.unpack(P.run(cur, spec, mask_bits), complement)


def _check_impl(impl):
    if impl not in IMPLS:
        raise ValueError("impl must be None, 'labels' or 'iterate', got %r" % (impl,))


# ------------------------------------------------------------------------------------------
# the public functions
# ------------------------------------------------------------------------------------------
@_device_scoped
def binary_erosion(input, structure=None, iterations=1, mask=None, output=None, border_value=0, origin=0, brute_force=False,
                   *, axes=None):
    """``scipy.ndimage.binary_erosion`` of a 2-D raster, bit for bit, as a ``bool`` raster.

    A cell is foreground iff its value is ``!= 0`` (NaN is foreground).  ``structure``: any 2-D array, ``None`` for the
    4-neighbourhood; its centre is ``size // 2 + origin`` per axis.  ``iterations < 1`` repeats until a step changes
    nothing and needs the centre to be a member.  ``mask``: cells where it is clear keep their value at every step.
    ``brute_force`` is accepted and changes nothing."""
    iterations = operator.index(iterations)
    return _morph(input, lambda: [_Spec(_structure(structure), _origin(origin), ERODE, border_value, iterations)], mask,
                  output, axes)


@_device_scoped
def binary_dilation(input, structure=None, iterations=1, mask=None, output=None, border_value=0, origin=0, brute_force=False,
                    *, axes=None):
    """``scipy.ndimage.binary_dilation`` of a 2-D raster, bit for bit: ``out[p]`` is the OR over the structure's members
    ``d`` of ``in[p - d]``.  Arguments as :func:`binary_erosion`."""
    iterations = operator.index(iterations)
    return _morph(input, lambda: [_Spec(_structure(structure, True), _origin(origin), DILATE, border_value, iterations)], mask,
                  output, axes)


def _two(first, second, structure, iterations, mask, border_value, origin):
    iterations = operator.index(iterations)

    def specs():
        s, o = _structure(structure, first == DILATE), _origin(origin)
        return [_Spec(s, o, first, border_value, iterations), _Spec(s, o, second, border_value, iterations)]
    return specs


@_device_scoped
def binary_opening(input, structure=None, iterations=1, output=None, origin=0, mask=None, border_value=0, brute_force=False,
                   *, axes=None):
    """``scipy.ndimage.binary_opening``: erosion, then dilation, each with the same ``iterations``, ``mask``,
    ``border_value`` and ``origin``; the raster stays a bit plane between the two."""
    return _morph(input, _two(ERODE, DILATE, structure, iterations, mask, border_value, origin), mask, output, axes)


@_device_scoped
def binary_closing(input, structure=None, iterations=1, output=None, origin=0, mask=None, border_value=0, brute_force=False,
                   *, axes=None):
    """``scipy.ndimage.binary_closing``: dilation, then erosion, as :func:`binary_opening`."""
    return _morph(input, _two(DILATE, ERODE, structure, iterations, mask, border_value, origin), mask, output, axes)


@_device_scoped
def binary_hit_or_miss(input, structure1=None, structure2=None, output=None, origin1=0, origin2=None, *, axes=None):
    """``scipy.ndimage.binary_hit_or_miss``: the cells where ``structure1`` fits the foreground and ``structure2`` (default:
    the complement of ``structure1``) fits the background, about ``origin1`` and ``origin2`` (default: ``origin1``).  The
    outside of the raster is background.  Both halves are one launch."""
    input, shape = _raster_2d(input)
    s1 = _structure(structure1)
    s2 = np.logical_not(s1) if structure2 is None else _structure(structure2)
    o1 = _origin(origin1)
    o2 = o1 if origin2 is None else _origin(origin2)
    hit, miss = _table(s1, o1, False), _table(s2, o2, False)
    _check_common(output, axes)
    if shape[0] * shape[1] == 0:
        return _empty_like(input, shape)
    R = _Cells(input)
    P = _Planes(R)
    return R.out(P.unpack(P.hit_or_miss(P.pack(_byte_mask(R.t)), hit, miss)))


@_device_scoped
def binary_propagation(input, structure=None, mask=None, output=None, border_value=0, origin=0, *, axes=None, impl=None):
    """``scipy.ndimage.binary_propagation``: ``binary_dilation(input, structure, -1, mask, None, border_value, origin)``,
    the cells of ``mask`` that the seeds of ``input`` reach through it.

    ``impl``: ``None`` takes the components of the mask (no iteration, six launches of ``label`` and a handful more) where
    the structure is 3 x 3, centrally symmetric with its centre set and ``origin`` is 0, and steps in batches otherwise;
    ``'labels'`` and ``'iterate'`` force one or the other.  Both give the same bits."""
    _check_impl(impl)
    input, shape = _raster_2d(input)
    s, o = _structure(structure, True), _origin(origin)
    _table(s, o, True)
    if _label_links(s, o) is None or impl == "iterate":
        if impl == "labels":
            raise ValueError("impl='labels' needs a centrally symmetric 3 x 3 structure with its centre set and origin 0")
        _Spec(s, o, DILATE, border_value, -1)
    mask = _mask_arg(mask, shape)
    _check_common(output, axes)
    if shape[0] * shape[1] == 0:
        return _empty_like(input, shape)
    R = _Cells(input)
    torch = _torch()
    if mask is None:
        mask_bytes = torch.ones((R.rows, R.cols), dtype=torch.uint8, device=R.t.device)
    else:
        mask_bytes = _byte_mask(_Cells(mask).t.to(R.t.device))
    return R.out(_propagate(R, _byte_mask(R.t), mask_bytes, s, o, border_value, impl, False))


@_device_scoped
def binary_fill_holes(input, structure=None, output=None, origin=0, *, axes=None, impl=None):
    """``scipy.ndimage.binary_fill_holes``: the raster with its holes filled, a hole being background that the structure
    does not join to the raster's outside - ``~binary_dilation(zeros, structure, -1, ~input, None, 1, origin)``.  ``impl``
    as in :func:`binary_propagation`."""
    _check_impl(impl)
    if not _is_tensor(input):
        input = np.asarray(input)
    if input.dtype.is_complex if _is_tensor(input) else np.iscomplexobj(input):
        input = input != 0                                      # SciPy takes a complex raster here, and here only
    input, shape = _raster_2d(input)
    s, o = _structure(structure, True), _origin(origin)
    _table(s, o, True)
    if _label_links(s, o) is None or impl == "iterate":
        if impl == "labels":
            raise ValueError("impl='labels' needs a centrally symmetric 3 x 3 structure with its centre set and origin 0")
        _Spec(s, o, DILATE, 1, -1)
    _check_common(output, axes)
    if shape[0] * shape[1] == 0:
        return _empty_like(input, shape)
    R = _Cells(input)
    background = (R.t == 0).view(_torch().uint8)                # the mask of the propagation: NaN is foreground
    return R.out(_propagate(R, None, background, s, o, 1, impl, True))
