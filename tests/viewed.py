"""Inputs as offset, strided and host-order views (a plain helper module, no test in it; its proof is in
tests/test_viewed_host.py, the families run under it in tests/test_gpu_views.py).

``run_viewed(fn, inputs, kw, name=, reference=, known=, ctx=)`` takes ``run_guarded``'s keywords, so a case dict of
tests/family_cases.py is passed as it is (``after`` and ``stream`` mean nothing here).  It calls ``fn`` once on ordinary
contiguous device tensors - the *plain* call, whose result ``reference`` checks - and then once per layout and per poison
of tests/guarded.py with every ``np.ndarray`` input rebuilt as a view inside a buffer of its own that is filled with the
poison byte.  Four assertions per run, each with an error class of its own:

Identity      every leaf of the result has the plain call's dtype, shape and bits (:class:`IdentityError`);
Surroundings  every buffer byte outside the view is still the poison (:class:`SurroundingsError`);
Inputs        the view's cells hold what the plain call left in its contiguous input, bit for bit: the input's own bits
              where ``known(i, a)`` says so (default: everywhere), the plain call's filled values in the other cells - the
              fill went through the view (:class:`InputsError`);
Results       returned tensors are contiguous, on the inputs' device and share no storage with an input's buffer, unless
              the function returns its argument; a host call returns no tensor (:class:`ResultsError`).

A run is judged in the order Surroundings, Inputs, Identity, Results - what became of the caller's memory before what
came back - so a fill that went into a copy is an Inputs failure also where the function returns its argument.

Device layouts (a tensor goes in), by ``carve``:

``offset``      contiguous, ``k`` elements into a 1-D buffer with ``k`` the smallest odd number with ``k * itemsize >= 64``
                and a tail pad of the same size: the data pointer is aligned to its element and to nothing wider
                (``data_ptr % (2 * itemsize) == itemsize`` is asserted);
``strided``     a raster is ``buf[1:1+rows, 2:2+cols]`` of ``(rows + 2, cols + 3)``, a vector ``buf[1:1+2n:2]`` of
                ``(2n + 1,)``, an ``(n, d)`` cloud (d <= 3) ``buf[1:1+n, 1:1+d]`` of ``(n + 2, d + 2)``, a
                ``(256, 256, C)`` table ``buf[..., :C]`` of ``(256, 256, C + 1)``;
``transposed``  ``.t()`` of the transposed copy, for the 2-D inputs.

Host layouts (a NumPy array goes in, NumPy comes out and is compared with the plain result as NumPy):

``fortran``     what ``np.asfortranarray`` gives: the transpose of the C-ordered array of the reversed shape;
``reversed``    ``a[::-1, ::-1]`` (``a[::-1]``) of the flipped copy, negative strides; the flipped copy is the first half of
                a buffer twice its size;
``readonly``    a contiguous view ``k`` elements into a 1-D buffer with ``setflags(write=False)``; not run for a case
                that fills its argument.

An input a layout has no form for (a vector in a ``transposed`` or ``fortran`` run, a one-row raster whose strided view
is contiguous anyway) goes as the offset view of its side.  A layout that no input of a case has a form for is not run.

Every layout keeps one property, asserted from the sizes: as many cells as the view has, counted from the view's first
element, end before the buffer does.  Code that wrongly takes a view for contiguous from its data pointer therefore reads
and writes the harness's own buffer, where Identity or Surroundings sees it, and nothing else.
"""
import functools

import numpy as np

from family_cases import DEVICE, leaves, rebuild, to_numpy
from family_checks import same_bits
from guarded import POISONS

DEVICE_LAYOUTS = ("offset", "strided", "transposed")
HOST_LAYOUTS = ("fortran", "reversed", "readonly")
LAYOUTS = DEVICE_LAYOUTS + HOST_LAYOUTS


class IdentityError(AssertionError):
    """a result differs from the plain call's"""


class SurroundingsError(AssertionError):
    """a byte of an input's buffer outside the view was written"""


class InputsError(AssertionError):
    """the view's cells are not what the plain call left in its input"""


class ResultsError(AssertionError):
    """a result is not contiguous, is on another device, or aliases an input's buffer"""


# ------------------------------------------------------------------------------------------
# the layouts
# ------------------------------------------------------------------------------------------
def pad_elements(itemsize):
    """the smallest odd k with k * itemsize >= 64"""
    k = -(-64 // int(itemsize))
    return k if k % 2 else k + 1


def _count(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def carve(shape, itemsize, layout):
    """``(buffer shape, cut, form)``: ``cut(buf)`` is the view of ``shape`` inside a C-ordered buffer (a tensor or a NumPy
    array, the same expression serves both), ``form`` the layout it really has - ``layout``, or ``offset`` where ``layout``
    has no form for this shape"""
    shape = tuple(int(v) for v in shape)
    n, nd = _count(shape), len(shape)
    if layout == "strided" and n > 1:
        if nd == 1:
            return (2 * n + 1,), (lambda b: b[1:1 + 2 * n:2]), layout
        if nd == 2 and shape[1] <= 3 and shape[0] > 1:
            return (shape[0] + 2, shape[1] + 2), (lambda b: b[1:1 + shape[0], 1:1 + shape[1]]), layout
        if nd == 2 and shape[0] > 1:
            return (shape[0] + 2, shape[1] + 3), (lambda b: b[1:1 + shape[0], 2:2 + shape[1]]), layout
        if nd == 3:
            return shape[:2] + (shape[2] + 1,), (lambda b: b[..., :shape[2]]), layout
    if layout == "transposed" and nd == 2 and shape[0] > 1 and shape[1] > 1:
        return (shape[1], shape[0]), (lambda b: b.transpose(0, 1) if hasattr(b, "is_contiguous") else b.T), layout
    if layout == "fortran" and nd >= 2 and sum(v > 1 for v in shape) > 1:
        return shape[::-1], (lambda b: b.permute(*range(nd - 1, -1, -1)) if hasattr(b, "is_contiguous") else b.T), layout
    if layout == "reversed" and n > 1:
        if nd == 1:
            return (2 * n,), (lambda b: b[:n][::-1]), layout
        return (2 * shape[0],) + shape[1:], (lambda b: b[:shape[0]][::-1, ::-1]), layout
    k = pad_elements(itemsize)
    return (n + 2 * k,), (lambda b: b[k:k + n].reshape(shape)), ("readonly" if layout == "readonly" else "offset")


@functools.lru_cache(maxsize=None)
def cells_of(shape, itemsize, layout):
    """the flat positions of the view's cells in its buffer, in the view's shape (int64, NumPy), and the buffer's cell
    count - with the bound every layout keeps asserted: ``n`` cells from the view's first element end inside the buffer"""
    bshape, cut, form = carve(shape, itemsize, layout)
    total = _count(bshape)
    idx = np.ascontiguousarray(cut(np.arange(total, dtype=np.int64).reshape(bshape)))
    assert idx.shape == tuple(shape) and np.unique(idx).size == idx.size, (shape, layout)
    first, n = int(idx.reshape(-1)[0]), idx.size
    assert 0 <= first and first + n <= total, (shape, layout, first, n, total)
    return idx, total, form


class View:
    """one input in one layout: ``buf`` (the whole poisoned buffer), ``arg`` (what the function gets), ``idx`` (the flat
    buffer positions of the view's cells) and the checks on them"""

    def __init__(self, a, layout, poison, device):
        import torch
        self.host = layout in HOST_LAYOUTS
        self.poison, self.shape, self.itemsize = int(poison), tuple(a.shape), a.dtype.itemsize
        bshape, cut, self.form = carve(a.shape, a.dtype.itemsize, layout)
        self.idx, self.total, _ = cells_of(tuple(a.shape), a.dtype.itemsize, layout)
        nbytes = self.total * self.itemsize
        if self.host:
            self.buf = np.full(nbytes, self.poison, dtype=np.uint8).view(a.dtype).reshape(bshape)
            self.arg = cut(self.buf)
            self.arg[...] = a
            if layout == "readonly":
                self.arg.setflags(write=False)
            if self.form == "fortran":
                assert self.arg.flags.f_contiguous and not self.arg.flags.c_contiguous, (self.shape, layout)
            if self.form == "reversed":
                assert all(s < 0 for s, v in zip(self.arg.strides[:2], self.shape[:2]) if v > 1), (self.shape, self.arg.strides)
        else:
            src = torch.from_numpy(np.ascontiguousarray(a))
            self.buf = torch.full((nbytes,), self.poison, dtype=torch.uint8, device=device).view(src.dtype).view(bshape)
            self.arg = cut(self.buf)
            self.arg.copy_(src)
            if self.form == "offset":
                odd = self.arg.data_ptr() % (2 * self.itemsize) == self.itemsize
                assert odd and self.arg.is_contiguous(), (self.shape, layout, self.arg.data_ptr())
            else:
                assert not self.arg.is_contiguous(), (self.shape, layout, self.arg.stride())
        assert tuple(self.arg.shape) == self.shape

    def cells(self):
        """the view's cells read back through the buffer, as a contiguous NumPy array"""
        flat = self.buf.reshape(-1)
        if self.host:
            return flat[self.idx]
        import torch
        return flat[torch.from_numpy(self.idx).to(flat.device)].cpu().numpy()

    def damaged(self):
        """how many bytes of the buffer outside the view are not the poison"""
        outside = np.ones(self.total, dtype=bool)
        outside[self.idx.reshape(-1)] = False
        if not outside.any():
            return 0
        if self.host:
            raw = self.buf.reshape(-1).view(np.uint8).reshape(self.total, self.itemsize)
            return int(np.count_nonzero(raw[outside] != self.poison))
        import torch
        raw = self.buf.reshape(-1).view(torch.uint8).view(self.total, self.itemsize)
        return int(torch.count_nonzero(raw[torch.from_numpy(outside).to(raw.device)] != self.poison))

    def aliases(self, v):
        """whether the result leaf ``v`` lives in this input's buffer"""
        if self.host:
            return isinstance(v, np.ndarray) and np.may_share_memory(v, self.buf)
        import torch
        return isinstance(v, torch.Tensor) and v.device == self.buf.device and \
            v.untyped_storage().data_ptr() == self.buf.untyped_storage().data_ptr()


def layouts_for(inputs, layouts=LAYOUTS, fills=False):
    """the layouts of ``layouts`` that some ``np.ndarray`` input has a form for; ``readonly`` only for a case that does
    not fill its argument"""
    arrays = [a for a in inputs if isinstance(a, np.ndarray)]
    out = []
    for layout in layouts:
        if layout == "readonly":
            if arrays and not fills:
                out.append(layout)
        elif any(carve(a.shape, a.dtype.itemsize, layout)[2] == layout for a in arrays):
            out.append(layout)
    return out


# ------------------------------------------------------------------------------------------
# run_viewed
# ------------------------------------------------------------------------------------------
def same_leaf(u, v):
    """dtype, shape and bits: family_checks.same_bits for the float planes, the bytes for every other"""
    if u is None or v is None:
        return u is None and v is None
    u, v = np.asarray(u), np.asarray(v)
    if u.dtype != v.dtype or u.shape != v.shape:
        return False
    if u.dtype.kind == "f":
        return bool(same_bits(u, v))
    return np.ascontiguousarray(u).tobytes() == np.ascontiguousarray(v).tobytes()


def _same_bytes(u, v):
    return u.dtype == v.dtype and u.shape == v.shape and np.ascontiguousarray(u).tobytes() == np.ascontiguousarray(v).tobytes()


def _sync(device):
    import torch
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _check_results(res, views, args, device, host, tag):
    import torch
    for path, v in leaves(res):
        if any(v is a for a in args):
            continue                                           # the function returns its argument
        if host:
            if isinstance(v, torch.Tensor):
                raise ResultsError("%r: %s is a tensor, NumPy went in" % (tag, path or "result"))
        elif isinstance(v, torch.Tensor):
            if not v.is_contiguous():
                raise ResultsError("%r: %s is not contiguous, strides %r" % (tag, path or "result", tuple(v.stride())))
            if v.device != torch.device(device):
                raise ResultsError("%r: %s is on %s, the inputs on %s" % (tag, path or "result", v.device, device))
        for i, w in views:
            if w.aliases(v):
                raise ResultsError("%r: %s shares the buffer of input %d" % (tag, path or "result", i))


def run_viewed(fn, inputs, kw=None, *, name, reference=None, known=None, ctx=None, after=None, stream=None,
               layouts=LAYOUTS, device=DEVICE, stats=None):
    """``fn(*inputs, **kw)`` on plain contiguous tensors of ``device``, checked by ``reference``, then under every layout
    of ``layouts`` that applies and both poisons with the four assertions of the module docstring.  ``stats``: a dict that
    gets ``runs`` (calls under a layout) added.  Returns ``(the plain result as NumPy, the layouts that ran)``."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    kw = kw or {}
    arrays = [(i, a) for i, a in enumerate(inputs) if isinstance(a, np.ndarray)]
    # the plain call
    tens = [torch.from_numpy(np.ascontiguousarray(a)).to(device).clone() if isinstance(a, np.ndarray) else a for a in inputs]
    res = fn(*tens, **kw)
    _sync(device)
    _check_results(res, [], tens, device, False, (name, ctx, "plain"))
    plain = rebuild(res, to_numpy)
    left = {i: tens[i].cpu().numpy() for i, _ in arrays}       # what the plain call left in its inputs
    for i, a in arrays:
        keep = known(i, a) if known else None
        keep = np.ones(a.shape, bool) if keep is None else np.asarray(keep, bool)
        if not _same_bytes(left[i][keep], np.ascontiguousarray(a)[keep]):
            raise InputsError("%r: the plain call changed known cells of input %d" % ((name, ctx), i))
    fills = any(not _same_bytes(left[i], np.ascontiguousarray(a)) for i, a in arrays)
    del res, tens
    if reference is not None:
        reference(plain)
    want = list(leaves(plain))
    ran = layouts_for(inputs, layouts, fills)
    for layout in ran:
        host = layout in HOST_LAYOUTS
        for poison in POISONS:
            tag = (name, ctx, layout, "poison 0x%02X" % poison)
            views = [(i, View(a, layout, poison, device)) for i, a in arrays]
            args = list(inputs)
            for i, w in views:
                args[i] = w.arg
            res = fn(*args, **kw)
            _sync(device)
            for i, w in views:                                                               # Surroundings
                n = w.damaged()
                if n:
                    raise SurroundingsError("%r: %d bytes of input %d's buffer outside the view were written" % (tag, n, i))
            for i, w in views:                                                               # Inputs
                if not _same_bytes(w.cells(), left[i]):
                    raise InputsError("%r: input %d does not hold what the plain call left in its input%s" % (
                        tag, i, " (the fill did not arrive in the view)" if fills else ""))
            got = list(leaves(rebuild(res, to_numpy)))
            if [p for p, _ in got] != [p for p, _ in want]:                                  # Identity
                raise IdentityError("%r: the result has leaves %r, the plain call's %r" % (
                    tag, [p for p, _ in got], [p for p, _ in want]))
            for (path, u), (_, v) in zip(got, want):
                if not same_leaf(u, v):
                    how = "%s%s for %s%s" % (getattr(u, "dtype", None), getattr(u, "shape", None), getattr(v, "dtype", None),
                                             getattr(v, "shape", None))
                    if u is not None and v is not None and u.dtype == v.dtype and u.shape == v.shape:
                        raw = [np.ascontiguousarray(w).reshape(-1).view(np.uint8) for w in (u, v)]
                        how = "%d of %d bytes differ" % (int(np.sum(raw[0] != raw[1])), v.nbytes)
                    raise IdentityError("%r: %s differs from the plain call's: %s" % (tag, path or "result", how))
            _check_results(res, views, args, device, host, tag)                              # Results
            if stats is not None:
                stats["runs"] = stats.get("runs", 0) + 1
            del res, args, views
    return plain, ran
