"""The library called from four host threads at once, each on a stream of its own (no global state but a
thread-local error string, atomically filled launch caches and the switch snapshot; per-thread host rows and taken lists).

The reference is the serial result of the same call on the main thread, bit for bit - the functions themselves are
checked against NumPy elsewhere.  The workloads are chosen for the state they would share if it were not per thread:

W1  run_pf (tests/pf_run.py) on (203, 331) float32, windows 1..20: route and the thread's smrf_pf_ero_inc_windows list
    against smrf_pf_plan, inside run_pf;
W2  run_pf on (70, 300), float32 and float64, windows 16, 17, 18, 40: another taken list than W1's;
W3  raster_stats with the median, colortable_shade, chamfer_distance, voxelize: the host rows[] of the reductions and
    the synchronising readbacks;
W4  inpaint_nans_by_springs, the spline solve and evaluation, nearest_source, topographic_position_index: workspaces and
    the LSQR scalar readback.

Rounds 0..2: thread t runs W((t + r) mod 4).  Round 3: all four run W3 on four different rasters and clouds.  Round 4: all
four run the progressive filter with four different window lists.  A barrier stands in front of every round; exceptions
are collected per thread and raised on the main thread; every join has a timeout.  ``api.last_stats`` is a module-level
dict that reports the process's latest call and is not looked at here.  The rasters, the spline pair and the reading
of result trees are tests/family_cases.py's, shared with the guarded and the stream module.
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, golden
from family_cases import holes, leaves, pf_raster, raster, spline_case, to_numpy
from pf_run import run_pf

pytestmark = pytest.mark.gpu

NTHREADS = 4
WAIT = 120.0                     # a barrier or join that takes longer has hung: the test fails instead of waiting on
F32, F64 = np.float32, np.float64
PF_LISTS = (((203, 331), F32, list(range(1, 21))), ((70, 300), F32, [16, 17, 18, 40]),
            ((203, 331), F32, [15, 16, 17, 18, 19]), ((70, 300), F64, [1, 2, 3, 30]))


def digest(parts):
    h = hashlib.sha1()
    for p in parts:
        a = np.ascontiguousarray(p)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def host(v):
    """tensors, dicts, tuples and scalars of a result as a flat list of NumPy arrays (read on the current stream)"""
    return [np.asarray(to_numpy(x)) for _, x in leaves(v) if x is not None]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def pf_work(shape, dtype, windows):
    Zd = dev(pf_raster(shape, dtype, False))

    def work():
        mask, when, _planes, route, taken = run_pf(Zd, windows)
        return host((mask, when)) + [np.asarray(route), np.asarray(taken)]
    return work


def w1():
    return [pf_work(*PF_LISTS[0])]


def w2():
    return [pf_work((70, 300), F32, [16, 17, 18, 40]), pf_work((70, 300), F64, [16, 17, 18, 40])]


def w3(k=0):
    import neilpy_amd as na
    from test_gpu_voxel import cloud
    rng = np.random.default_rng(500 + k)
    X = (rng.normal(size=(211 + k, 307)) * 30 + 400).astype(F32 if k % 2 == 0 else F64)
    X[rng.random(X.shape) < 0.02] = np.nan
    Xd = dev(X)
    Zd = dev(raster((67 + k, 131), F64, seed=k))
    lut = dev(golden("relief.npz")["lut_ghc"])
    q, p = dev(rng.uniform(-1, 11, (257, 2 + k % 2))), dev(rng.uniform(0, 10, (3000 + 10 * k, 2 + k % 2)))
    x, y, z = (dev(c) for c in cloud(4000 + k, 77 + k, F64))
    return [lambda: host(na.raster_stats(Xd)), lambda: host(na.colortable_shade(Zd, lut, 2)),
            lambda: host(na.chamfer_distance(q, p)),
            lambda: host(na.voxelize(None, x, y, z, 32, ve=33 / 8.0, bottom_fill=True, pad=3, threshold=2))]


def w4():
    import neilpy_amd as na
    from test_gpu_springs import raster as springs_raster
    A = dev(np.array(springs_raster((37, 53), 1, .5)))
    X = dev(holes((67, 131), F32, .6, 2))
    Zd = dev(raster((67, 131), F64, seed=3))
    case = spline_case((9, 300))
    sp = [dev(a) for a in case["inputs"]]

    def springs():
        B = A.clone()
        assert na.inpaint_nans_by_springs(B, inplace=True) is None
        return host(B)

    def spline():
        return host(case["fn"](sp[0].clone(), *sp[1:]))
    return [springs, spline, lambda: host(na.nearest_source(X)),
            lambda: host(na.topographic_position_index(Zd, radius=4, standardize=True))]


def run_threads(jobs):
    """``jobs[r][t]``: the list of calls thread t makes in round r.  Returns ``got[r][t]``, the digests of their results."""
    import torch
    rounds = len(jobs)
    barrier = threading.Barrier(NTHREADS)
    got = [[None] * NTHREADS for _ in range(rounds)]
    errors = []

    def body(t):
        try:
            stream = torch.cuda.Stream()
            assert stream.cuda_stream != 0
            for r in range(rounds):
                barrier.wait(WAIT)
                with torch.cuda.stream(stream):
                    got[r][t] = [digest(f()) for f in jobs[r][t]]
        except BaseException as e:  # noqa: BLE001
            errors.append((t, e))
            barrier.abort()
    threads = [threading.Thread(target=body, args=(t,), name="caller-%d" % t) for t in range(NTHREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(WAIT)
    assert not any(th.is_alive() for th in threads), "a thread did not finish within %g s" % WAIT
    real = [(t, e) for t, e in errors if not isinstance(e, threading.BrokenBarrierError)]
    if real:
        raise real[0][1]
    assert not errors, errors
    return got


def serial(calls):
    import torch
    out = [digest(f()) for f in calls]
    torch.cuda.synchronize()
    return out


def test_four_threads_five_rounds(gpu_device):
    W = [w1(), w2(), w3(), w4()]
    W3 = [w3(k) for k in range(NTHREADS)]
    W3[0] = W[2]
    PF = [[pf_work(*spec)] for spec in PF_LISTS]
    jobs = [[W[(t + r) % 4] for t in range(NTHREADS)] for r in range(3)] + [W3, PF]
    want = {id(calls): serial(calls) for calls in W + W3 + PF}
    again = {id(calls): serial(calls) for calls in W}
    assert all(again[k] == want[k] for k in again)           # the serial reference is itself reproducible
    assert len({tuple(want[id(c)]) for c in W3}) == NTHREADS and len({tuple(want[id(c)]) for c in PF}) == NTHREADS
    got = run_threads(jobs)
    for r, row in enumerate(jobs):
        for t, calls in enumerate(row):
            assert got[r][t] == want[id(calls)], ("round %d, thread %d: call(s) %s differ from the serial run" % (
                r, t, [i for i, (a, b) in enumerate(zip(got[r][t], want[id(calls)])) if a != b]))


def test_error_text_is_per_thread(gpu_device):
    """after a barrier every thread makes a call that fails before anything is launched (a window of -(100 + t)); after a
    second barrier each reads smrf_last_error(): it names the thread's own window"""
    import torch
    from neilpy_amd import _lib
    lib = _lib.load()
    Zd = dev(pf_raster((70, 300), F32, False))
    mask = torch.zeros((70, 300), dtype=torch.uint8, device=Zd.device)
    nbytes = int(lib.smrf_progressive_filter_workspace_bytes(70, 300, 4))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=Zd.device)
    torch.cuda.synchronize()
    barrier = threading.Barrier(NTHREADS)
    texts, errors = [None] * NTHREADS, []

    def body(t):
        try:
            stream = torch.cuda.Stream()
            win = np.array([-(100 + t)], dtype=np.int32)
            thr = np.array([.15])
            barrier.wait(WAIT)
            rc = lib.smrf_progressive_filter_f32(C.c_void_p(Zd.data_ptr()), 70, 300, win.ctypes.data_as(C.c_void_p),
                                                 thr.ctypes.data_as(C.c_void_p), 1, C.c_void_p(mask.data_ptr()), None,
                                                 C.c_void_p(ws.data_ptr()), nbytes, 0, 0, C.c_void_p(stream.cuda_stream))
            assert rc != 0
            barrier.wait(WAIT)
            texts[t] = lib.smrf_last_error().decode()
        except BaseException as e:  # noqa: BLE001
            errors.append((t, e))
            barrier.abort()
    threads = [threading.Thread(target=body, args=(t,)) for t in range(NTHREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(WAIT)
    assert not any(th.is_alive() for th in threads) and not errors, errors
    for t, text in enumerate(texts):
        assert "negative window -%d" % (100 + t) in text, (t, texts)
    assert not mask.any()                                    # nothing was launched


def test_first_use_from_four_threads(gpu_device):
    """a fresh interpreter whose very first library calls come from four threads behind a barrier, all with the same ring
    radius (the launch-attribute caches are filled once per process), then a springs solve from one of them: the digests
    the child prints equal the ones computed serially here"""
    import neilpy_amd as na
    import threads_child as child
    Z, A = child.inputs()
    want_e = digest(host(na.erosion(dev(Z), radius=child.RADIUS)))
    B = dev(A)
    assert na.inpaint_nans_by_springs(B, inplace=True) is None
    want_s = digest(host(B))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "threads_child.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(("erosion ", "springs "))]
    assert sorted(lines) == sorted([["erosion", str(t), want_e] for t in range(NTHREADS)] + [["springs", want_s]]), (lines, want_e,
                                                                                                                   want_s)
