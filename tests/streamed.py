"""The side-stream harness (a plain helper module, no test in it; its proof is in tests/test_streamed_host.py and at the
head of tests/test_gpu_streams.py).

The cases it is run on are those tests/family_cases.py marks ``stream=True``; result trees are read with that module's
``rebuild`` and ``to_numpy``.

``run_streamed(fn, inputs, kw, name=, reference=, ctx=)`` calls a public function with a fresh non-default
``torch.cuda.Stream()`` as the current stream and combines three checks:

Handles   while the call runs, the object ``neilpy_amd._lib.load()`` returns is a recording proxy: every ``smrf_*`` call is
          forwarded unchanged and the value in its ``stream`` slot is kept.  The slot's position is read from
          include/smrf_hip.h (it is not always last).  At least one call must carry a stream, and every one must carry
          the side stream's handle, never 0 (:class:`HandleError`).
Data      every ``np.ndarray`` input sits on the device in an arena of tests/guarded.py that holds a *decoy* (the same
          values in another order) when the device is synchronised.  Then, all on the side stream: two delays, the copy of the
          real input into that arena, the call - under ``guarded(DEVICE, 0xFF)`` with a delay enqueued ahead of every
          arena's poison fill - and the read-back of the result, which ``reference`` compares with the family's own
          restatement under the family's own margins.  A launch, memset, copy or torch op that lands on another stream
          runs while the side stream still sleeps: it reads the decoy, or writes an output that the queued poison fill
          then overwrites with NaN / 255.  Both fail ``reference``.
Guards    ``g.check()`` as in tests/test_gpu_guarded.py.

A wrong-stream launch that follows a host synchronisation inside the call leaves no race for Data; Handles is exact for
the Python layer there.

The delay is ``torch.cuda._sleep(cycles)``, calibrated once per process with events.  ``D_MS`` is a sensitivity setting,
never a tolerance: correct code passes at any length.  Whether a new stream shares a hardware queue with the default
stream is not known here (a process has few queues); on a shared queue an offender would queue behind the delay and
escape.  ``side_stream()`` therefore takes the first of at most ``CANDIDATES`` freshly created streams on which the
offending stand-ins (a) and (b) below are caught, and raises :class:`StreamHarnessError` if none is.
"""
import contextlib
import ctypes as C
import os
import re

import numpy as np

from family_cases import rebuild, to_numpy
from guarded import guarded

DEVICE = "cuda:0"
D_MS = 1.0                       # the delay ahead of every fill, milliseconds: 16 x the measured detection threshold
                                 # (tests/test_gpu_streams.py's docstring)
CANDIDATES = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HandleError(AssertionError):
    """a library call carried a stream handle other than the current stream's"""


class StreamHarnessError(AssertionError):
    """the harness itself cannot detect an offender here"""


# ------------------------------------------------------------------------------------------
# where the stream goes: include/smrf_hip.h
# ------------------------------------------------------------------------------------------
def declarations(text=None):
    """{name: [parameter names]} of every SMRF_API declaration (the regular expression of tests/test_abi.py, with the
    parameter list)"""
    if text is None:
        text = open(os.path.join(ROOT, "include", "smrf_hip.h")).read()
    out = {}
    for name, params in re.findall(r"^SMRF_API [\w \*]*?\b(smrf_\w+)\(([^;{]*?)\);", text, flags=re.M | re.S):
        params = re.sub(r"/\*.*?\*/", " ", params, flags=re.S)
        names = []
        for p in params.split(","):
            p = p.strip()
            if p and p != "void":
                names.append(re.findall(r"\w+", p)[-1])
        out[name] = names
    return out


def stream_slots(text=None):
    """{name: position of the ``stream`` parameter, or None}"""
    return {n: (p.index("stream") if "stream" in p else None) for n, p in declarations(text).items()}


# ------------------------------------------------------------------------------------------
# the recording proxy
# ------------------------------------------------------------------------------------------
def handle_of(v):
    if isinstance(v, C.c_void_p):
        v = v.value
    return int(v) if v is not None else 0


class Recorder:
    """stands in for the CDLL object: ``smrf_*`` calls are forwarded with their arguments and return values untouched,
    ``calls`` keeps (name, stream handle) of every one that has a stream slot"""

    def __init__(self, real, slots):
        self._real, self._slots, self.calls = real, slots, []

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if not name.startswith("smrf_"):
            return attr
        slot = self._slots.get(name)

        def call(*args):
            if slot is not None:
                self.calls.append((name, handle_of(args[slot])))
            return attr(*args)
        call.__name__ = name
        return call


@contextlib.contextmanager
def recording(real=None, slots=None):
    """``neilpy_amd._lib.load()`` returns a :class:`Recorder` of ``real`` (default: the loaded library) inside the block"""
    from neilpy_amd import _lib
    before = _lib._lib
    rec = Recorder(real if real is not None else _lib.load(), slots if slots is not None else stream_slots())
    _lib._lib = rec
    try:
        yield rec
    finally:
        _lib._lib = before


def check_handles(calls, allowed, tag):
    if not calls:
        raise HandleError("%r: no library call carrying a stream was recorded" % (tag,))
    bad = sorted({(n, h) for n, h in calls if h == 0 or h not in allowed})
    if bad:
        raise HandleError("%r: calls on another stream than the current one (%s): %s" % (
            tag, ", ".join("0x%x" % h for h in sorted(allowed)), ", ".join("%s got 0x%x" % b for b in bad)))


# ------------------------------------------------------------------------------------------
# the delay
# ------------------------------------------------------------------------------------------
_cycles_per_ms = None


def cycles_per_ms():
    """``torch.cuda._sleep`` cycles per millisecond, measured once with events"""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        torch.cuda._sleep(1000000)                       # first launch: module load
        torch.cuda.synchronize()
        probe = 20000000
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, ("torch.cuda._sleep(%d) took %.4f ms: it is no delay here" % (probe, ms))
        _cycles_per_ms = probe / ms
    return _cycles_per_ms


def delay(ms=None):
    """a callable that enqueues ``ms`` (default D_MS) of sleep on the current stream"""
    import torch
    cycles = max(1, int((D_MS if ms is None else ms) * cycles_per_ms()))
    return lambda: torch.cuda._sleep(cycles)


# ------------------------------------------------------------------------------------------
# run_streamed
# ------------------------------------------------------------------------------------------
def decoy_of(a, k=0):
    """another draw of the shape and dtype of ``a``, input ``k`` of a call: its own values in another order (so whatever
    reads the decoy reads values of the kind the real input holds), from a generator seeded by ``k`` and the shape"""
    rng = np.random.default_rng([20261201, k] + list(a.shape))
    d = rng.permutation(a.reshape(-1)).reshape(a.shape)
    if d.tobytes() == a.tobytes():
        d = np.ascontiguousarray(a.reshape(-1)[::-1]).reshape(a.shape)
    return np.ascontiguousarray(d)


@contextlib.contextmanager
def _streams_made(into):
    """the streams the call creates for itself (neilpy_amd/sharded.py's overlap stream) are collected in ``into``"""
    import torch
    real = torch.cuda.Stream

    def make(*a, **k):
        s = real(*a, **k)
        into.append(s)
        return s
    torch.cuda.Stream = make
    try:
        yield
    finally:
        torch.cuda.Stream = real


def run_streamed(fn, inputs, kw=None, *, name, reference=None, ctx=None, stream=None, delay_ms=None, own_streams=False,
                 lib=None, slots=None, stats=None):
    """``fn(*inputs, **kw)`` with a side stream current, under the three checks of the module docstring.  ``np.ndarray``
    inputs become device tensors that hold a decoy until the side stream, after a delay, copies the real values in; other
    inputs (host arrays a NumPy-in case wants passed as they are come wrapped in :class:`Host`) pass through.
    ``own_streams``: handles of streams the call itself creates are accepted too (the band driver's overlap stream).
    ``lib`` / ``slots``: another object behind the proxy (the stand-ins' fake library).  ``stats``: a dict that gets
    ``allocations`` added.  Returns the result as NumPy arrays."""
    import torch
    side = stream if stream is not None else side_stream()
    assert side.cuda_stream != 0 and side != torch.cuda.default_stream()
    sleep = delay(delay_ms)
    tag = (name, ctx)
    made = []
    with guarded(DEVICE, 0xFF) as g:
        args, real = [], []
        for k, a in enumerate(inputs):
            if isinstance(a, np.ndarray):
                args.append(g.tensor(decoy_of(a, k)))
                real.append(torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE))
            else:
                args.append(a.array if isinstance(a, Host) else a)
                real.append(None)
        torch.cuda.synchronize()
        g.before_fill = sleep
        try:
            with recording(lib, slots) as rec, torch.cuda.stream(side), _streams_made(made):
                sleep()
                sleep()                                  # twice: an offender's own first allocation sleeps once, on its stream
                for t, r in zip(args, real):
                    if r is not None:
                        t.copy_(r, non_blocking=True)
                res = fn(*args, **(kw or {}))
                g.before_fill = None
                got = rebuild(res, to_numpy)             # .cpu() on the side stream: waits for it, and for nothing else
                g.check()
        finally:
            g.before_fill = None
            torch.cuda.synchronize()
    if stats is not None:
        stats["allocations"] = stats.get("allocations", 0) + len(g.arenas)
    allowed = {side.cuda_stream} | ({s.cuda_stream for s in made} if own_streams else set())
    check_handles(rec.calls, allowed, tag)
    if reference is not None:
        reference(got)
    return got


class Host:
    """an input that stays the host array it is (the NumPy-in, NumPy-out cases)"""

    def __init__(self, array):
        self.array = array


# ------------------------------------------------------------------------------------------
# stand-ins: torch ops on the harness's memory, no kernel of the package
# ------------------------------------------------------------------------------------------
class FakeLib:
    """what the stand-ins call through the proxy: takes a pointer, a count and a stream, launches nothing"""

    def __init__(self):
        self.seen = []

    def smrf_fake(self, ptr, n, stream):
        self.seen.append((ptr, n, stream))
        return 0


FAKE_SLOTS = {"smrf_fake": 2}
STANDINS = ("ok", "a", "b", "c")


def standin(kind):
    """``ok``: out = 2 * Z + 1 into torch.empty_like on the current stream.  ``a``: all of it under the default stream.
    ``b``: the last copy into ``out`` on the default stream.  ``c``: the fake library call carries stream 0."""
    import torch
    from neilpy_amd import _lib

    def fn(Zt):
        here = torch.cuda.current_stream().cuda_stream
        if kind == "a":
            with torch.cuda.stream(torch.cuda.default_stream()):
                out = torch.empty_like(Zt)
                out.copy_(2 * Zt + 1)
        else:
            out = torch.empty_like(Zt)
            tmp = 2 * Zt + 1
            if kind == "b":
                with torch.cuda.stream(torch.cuda.default_stream()):
                    out.copy_(tmp)
            else:
                out.copy_(tmp)
        assert _lib.load().smrf_fake(C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(0 if kind == "c" else here)) == 0
        return out
    return fn


def standin_input():
    return np.random.default_rng(20261202).normal(100.0, 5.0, (67, 131)).astype(np.float32)


def standin_verdict(kind, stream, delay_ms=None):
    """how the harness judges a stand-in on ``stream``: "passes", "handle" (the handle check failed), "decoy" (the result is
    2 * decoy + 1), "poison" (the result is NaN throughout) or "wrong" (any other wrong result)"""
    Z = standin_input()
    seen = []

    def reference(got):
        seen.append(got)
        assert got.dtype == Z.dtype and np.array_equal(got, 2 * Z + 1)
    try:
        run_streamed(standin(kind), [Z], name="stand-in " + kind, reference=reference, stream=stream, delay_ms=delay_ms,
                     lib=FakeLib(), slots=FAKE_SLOTS)
    except HandleError:
        return "handle"
    except AssertionError:
        if not seen:
            raise
        got = seen[0]
        if np.array_equal(got, 2 * decoy_of(Z) + 1):
            return "decoy"
        return "poison" if np.isnan(got).all() else "wrong"
    return "passes"


EXPECTED = {"ok": "passes", "a": "decoy", "b": "poison", "c": "handle"}
_side = None
SIDE_INDEX = None
_tried = []


def side_stream():
    """the stream every case runs on: the first of CANDIDATES fresh ones on which (a) and (b) are caught"""
    global _side, SIDE_INDEX
    if _side is None:
        import torch
        report = []
        for k in range(CANDIDATES):
            s = torch.cuda.Stream()
            _tried.append(s)                             # kept alive: the next candidate is another stream
            warm = standin_verdict("ok", s)                # the first launch of each torch kernel loads it: not while racing
            if warm != "passes":
                raise StreamHarnessError("the correct stand-in is judged %r on fresh stream %d" % (warm, k))
            verdicts = {kind: standin_verdict(kind, s) for kind in ("a", "b")}
            report.append((k, verdicts))
            if all(verdicts[kind] == EXPECTED[kind] for kind in verdicts):
                _side, SIDE_INDEX = s, k
                break
        else:
            raise StreamHarnessError("no offending stand-in is caught on any of %d fresh streams at D = %g ms: %r - an "
                                     "offender on the default stream queues behind the delay here" % (CANDIDATES, D_MS, report))
    return _side
