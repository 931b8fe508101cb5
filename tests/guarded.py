"""Poisoned, guard-banded memory for the package's allocations (a plain helper module, no test in it).

``with guarded(device, poison) as g:`` redirects the allocation calls the package makes through the ``torch`` module
(``torch.empty`` / ``empty_like`` / ``zeros`` / ``zeros_like`` / ``ones`` / ``ones_like`` / ``full`` / ``full_like``:
the package looks them up at call time, a grep of ``neilpy_amd/*.py`` shows no ``new_empty`` / ``new_zeros``) for as long
as it is active and restores them on exit, also when the body raises.  A request for another device, for pinned memory,
for zero elements, with ``out=`` or with a layout other than strided passes through untouched.

Every redirected request is carved out of an arena of its own::

    [ front guard, GUARD bytes | interior, exactly the requested bytes | tail guard, GUARD bytes ]

filled with the byte ``poison``.  GUARD is a multiple of 512, so the interior keeps the alignment torch's caching
allocator would have given; the tail guard starts at the interior's exact last byte, not at a rounded size.  ``empty``
and ``empty_like`` hand the interior out still poisoned, ``zeros`` / ``ones`` / ``full`` fill the interior only.  The
arenas stay alive until the harness is dropped, so no later request can be served from an earlier one's memory.

What a test then asks of the harness:

``g.tensor(array)``   an input in such an arena (poisoned surroundings), with a snapshot of its bytes taken;
``g.check()``         every guard byte of every arena served so far still equals ``poison`` (one reduction per arena, on
                      the device); the failure names the allocation's dtype, shape and call site, front or behind, and
                      the byte offset of the first damaged byte;
``g.owns(t)``         ``t``'s storage is one of the arenas;
``g.unchanged(t)``    ``t`` has the bytes of its snapshot (NaN payloads and zero signs included); ``where=`` restricts
                      the comparison to the elements of a boolean mask (entry points that fill a raster in place);
``before_fill=``      (optional, also settable as ``g.before_fill``) a callable run on the current stream before each
                      arena's poison fill; tests/streamed.py enqueues a delay there.  Absent, nothing changes.
``same_bits(a, b)``   two NumPy results agree byte for byte - the comparison of a run under poison 0xFF (NaN in every
                      float type, 255 in uint8) with a run under 0x5A (an ordinary finite number in every float type):
                      a cell nobody wrote, or one computed from memory nobody wrote, differs between the two.
"""
import contextlib
import os
import sys

import numpy as np
import torch

GUARD = 4096
POISONS = (0xFF, 0x5A)
PATCHED = ("empty", "empty_like", "zeros", "zeros_like", "ones", "ones_like", "full", "full_like")
_THIS = os.path.abspath(__file__).rstrip("c")
_ORIG = {name: getattr(torch, name) for name in PATCHED}      # the real ones, whatever is patched when they are needed
_active = []


class GuardError(AssertionError):
    pass


class _Arena:
    __slots__ = ("buf", "nbytes", "dtype", "shape", "site", "snap")

    def describe(self):
        return "%s%s allocated at %s" % (str(self.dtype).replace("torch.", ""), tuple(self.shape), self.site)


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename).rstrip("c") == _THIS:
        f = f.f_back
    return "%s:%d" % (os.path.relpath(f.f_code.co_filename), f.f_lineno) if f is not None else "?"


def _shape_of(args):
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(int(v) for v in args[0])
    return tuple(int(v) for v in args)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


class Guarded:
    def __init__(self, device, poison, before_fill=None):
        self.device = self._resolve(device)
        self.poison = int(poison)
        assert 0 <= self.poison <= 255
        self.before_fill = before_fill                # tests/streamed.py: called on the current stream ahead of every poison fill
        self.arenas = []

    # ------------------------------------------------------------------ allocation
    @staticmethod
    def _resolve(device):
        d = torch.device(device) if device is not None else torch.device("cpu")
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        return d

    def _mine(self, device, kw):
        """whether a request is redirected: this device, pageable strided memory, no out="""
        if kw.get("pin_memory") or kw.get("out") is not None:
            return False
        if kw.get("layout", torch.strided) is not torch.strided or kw.get("requires_grad"):
            return False
        if kw.get("memory_format", torch.contiguous_format) not in (torch.contiguous_format, torch.preserve_format):
            return False
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        return self._resolve(device) == self.device

    def alloc(self, shape, dtype, fill=None):
        """the interior of a new arena as a contiguous ``dtype`` tensor of ``shape``, poisoned or filled"""
        shape = tuple(int(v) for v in shape)
        n = 1
        for v in shape:
            n *= v
        a = _Arena()
        a.nbytes = n * _ORIG["empty"](0, dtype=dtype).element_size()
        if self.before_fill is not None:
            self.before_fill()
        a.buf = _ORIG["full"]((GUARD + a.nbytes + GUARD,), self.poison, dtype=torch.uint8, device=self.device)
        a.dtype, a.shape, a.site, a.snap = dtype, shape, _call_site(), None
        self.arenas.append(a)
        t = a.buf[GUARD:GUARD + a.nbytes].view(dtype).view(shape)
        if fill is not None:
            t.fill_(fill)
        return t

    def _like(self, t, kw):
        return tuple(t.shape), kw.get("dtype") or t.dtype, kw.get("device") if kw.get("device") is not None else t.device

    def _make(self, name):
        orig = _ORIG[name]
        like = name.endswith("_like")
        fill = {"empty": None, "zeros": 0, "ones": 1}.get(name.split("_")[0], "arg")

        def patched(*args, **kw):
            try:
                if like:
                    shape, dtype, device = self._like(args[0], kw)
                    value = (args[1] if len(args) > 1 else kw["fill_value"]) if fill == "arg" else fill
                else:
                    if fill == "arg":
                        size = args[0] if args else kw["size"]
                        value = args[1] if len(args) > 1 else kw["fill_value"]
                        shape = _shape_of((size,))
                    else:
                        shape, value = _shape_of(args if args else (kw["size"],)), fill
                    dtype, device = kw.get("dtype"), kw.get("device")
                    if dtype is None:
                        dtype = torch.tensor(value).dtype if fill == "arg" else torch.get_default_dtype()
                numel = 1
                for v in shape:
                    numel *= v
                redirect = numel > 0 and self._mine(device, kw)
            except Exception:                         # an argument form not understood here: torch's own call decides
                redirect = False
            if not redirect:
                return orig(*args, **kw)
            return self.alloc(shape, dtype, value)
        patched.__name__ = name
        return patched

    def __enter__(self):
        assert not _active, "guarded() does not nest"
        _active.append(self)
        for name in PATCHED:
            setattr(torch, name, self._make(name))
        return self

    def __exit__(self, *exc):
        for name in PATCHED:
            setattr(torch, name, _ORIG[name])
        _active.remove(self)
        return False

    # ------------------------------------------------------------------ what the tests ask
    def tensor(self, array):
        """``array`` (NumPy or tensor) in an arena of its own, with a snapshot for :meth:`unchanged`"""
        src = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        t = self.alloc(src.shape, src.dtype)
        t.copy_(src)
        self.snapshot(t)
        return t

    def bytes_of(self, nbytes):
        """a poisoned ``uint8`` workspace of exactly ``nbytes`` bytes: the tail guard sits on the first byte past it"""
        return self.alloc((int(nbytes),), torch.uint8)

    def _arena_of(self, t):
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            return None
        p = t.untyped_storage().data_ptr()
        for a in self.arenas:
            if a.buf.untyped_storage().data_ptr() == p:
                return a
        return None

    def owns(self, t):
        return self._arena_of(t) is not None

    def raw(self, t):
        """``(cells, first)``: ``t``'s whole arena as a flat tensor of ``t``'s dtype, guards included, and the index of
        ``t``'s first element in it - the address space a stand-in kernel of the harness's own tests writes through"""
        a = self._arena_of(t)
        assert a is not None
        return a.buf.view(a.dtype), GUARD // t.element_size()

    def _interior(self, a):
        return a.buf[GUARD:GUARD + a.nbytes]

    def snapshot(self, t):
        a = self._arena_of(t)
        assert a is not None, "snapshot() is for tensors of the harness"
        a.snap = self._interior(a).clone()

    def unchanged(self, t, where=None):
        a = self._arena_of(t)
        assert a is not None and a.snap is not None, "unchanged() needs a tensor made by tensor() or given to snapshot()"
        now, then = self._interior(a), a.snap
        if where is not None:
            keep = torch.as_tensor(where, device=self.device).reshape(-1).bool()
            now, then = now.view(keep.numel(), -1)[keep], then.view(keep.numel(), -1)[keep]
        return bool(torch.equal(now, then))

    def check(self):
        """raises GuardError unless every guard byte of every arena still holds the poison"""
        if not self.arenas:
            return
        bad = torch.stack([torch.count_nonzero(torch.cat((a.buf[:GUARD], a.buf[GUARD + a.nbytes:])) != self.poison)
                           for a in self.arenas]).cpu().tolist()
        msgs = []
        for a, n in zip(self.arenas, bad):
            if not n:
                continue
            for side, g in (("in front of", a.buf[:GUARD]), ("behind", a.buf[GUARD + a.nbytes:])):
                hit = torch.nonzero(g != self.poison).reshape(-1)
                if hit.numel():
                    first, last = int(hit[0]), int(hit[-1])
                    # in front: bytes before the interior's first byte; behind: bytes past its last byte
                    off = first - GUARD if side == "in front of" else first
                    msgs.append("%d guard byte(s) damaged %s %s: first at byte offset %+d from the interior's %s, last at %+d"
                                % (int(hit.numel()), side, a.describe(), off,
                                   "start" if side == "in front of" else "end",
                                   last - GUARD if side == "in front of" else last))
        if msgs:
            raise GuardError("; ".join(msgs))


@contextlib.contextmanager
def guarded(device, poison, before_fill=None):
    g = Guarded(device, poison, before_fill)
    with g:
        yield g
