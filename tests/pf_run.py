"""progressive_filter through the C ABI with everything the routing tests look at, the rule of csrc/pf_route.h for which
windows take the incremental erosion, restated, and the comparisons of a call against the independent reference
(tests/morph_numpy.py) that tests/test_gpu_incero_edges.py and tests/test_gpu_dil_cross.py share; their cases are in
tests/window_cases.py."""
import ctypes as C

import numpy as np

import morph_numpy as mn


def run_pf(Zd, windows, nan_aware=-1, impl=0):
    """(mask, when, the workspace's three planes, route per window, took the incremental erosion per window)"""
    import torch
    from neilpy_amd import _lib
    lib = _lib.load()
    rows, cols = Zd.shape
    win = np.ascontiguousarray(np.asarray(windows, dtype=np.int32))
    thr = np.ascontiguousarray(.15 * (win * 1.0))
    sfx = "f32" if Zd.dtype == torch.float32 else "f64"
    nbytes = lib.smrf_progressive_filter_workspace_bytes(rows, cols, Zd.element_size())
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=Zd.device)
    mask = torch.empty((rows, cols), dtype=torch.uint8, device=Zd.device)
    when = torch.empty((rows, cols), dtype=torch.uint8, device=Zd.device)
    ms = np.zeros(win.size, dtype=np.float32)
    route = np.zeros(win.size, dtype=np.int32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = getattr(lib, "smrf_progressive_filter_timed_" + sfx)
    _lib.check(fn(C.c_void_p(Zd.data_ptr()), rows, cols, win.ctypes.data_as(C.c_void_p), thr.ctypes.data_as(C.c_void_p),
                  int(win.size), C.c_void_p(mask.data_ptr()), C.c_void_p(when.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes,
                  int(nan_aware), int(impl), st, ms.ctypes.data_as(C.c_void_p), route.ctypes.data_as(C.c_void_p)))
    taken = np.zeros(win.size, dtype=np.uint8)
    assert lib.smrf_pf_ero_inc_windows(taken.ctypes.data_as(C.c_void_p), int(win.size)) == win.size
    # what ran is what the plan says (csrc/pf_route.h through smrf_pf_plan, same arguments; a call with nan_aware < 0 follows the
    # plan for what the raster holds)
    has_nan = bool(torch.isnan(Zd).any()) if nan_aware < 0 else nan_aware != 0
    p_route = np.full(win.size, -1, dtype=np.int32)
    p_taken = np.full(win.size, 9, dtype=np.uint8)
    _lib.check(lib.smrf_pf_plan(Zd.element_size(), win.ctypes.data_as(C.c_void_p), int(win.size), rows, rows * cols, int(has_nan),
                                int(impl), 0, p_route.ctypes.data_as(C.c_void_p), p_taken.ctypes.data_as(C.c_void_p)))
    assert [int(v) for v in route] == [int(v) for v in p_route], (route, p_route)
    assert [int(v) for v in taken] == [int(v) for v in p_taken], (taken, p_taken)
    planes = ws.view(Zd.dtype).view(3, rows, cols)
    return mask, when, planes, [int(v) for v in route], [int(v) for v in taken]


def adopted_radii():
    """kEroIncAdoptF32 of csrc/ero_inc_adopt.inc: what SMRF_ERO_INC=1 (the default) takes"""
    from pf_host import table
    return table("kEroIncAdoptF32", "ero_inc_adopt.inc")


def inc_rule(windows, route, mode, fp32=True):
    """pf_route.h, restated independently: window i takes the incremental erosion when it runs as two ring passes, the previous window did too,
    its radius is the previous one's + 1, an instance exists (fp32, 16..64) and, under mode 1, the table adopts the radius"""
    from neilpy_amd import _lib
    adopt = adopted_radii()
    win = [int(v) for v in windows]
    return [int(mode != 0 and fp32 and i > 0 and route[i] == _lib.ROUTE_TWO_PASS and route[i - 1] == _lib.ROUTE_TWO_PASS and
                win[i] == win[i - 1] + 1 and 16 <= win[i] <= 64 and (mode == 2 or bool(adopt[win[i]]))) for i in range(len(win))]


def rotation_plan(windows):
    """which windows of a list take the incremental erosion under SMRF_ERO_INC=2, judged on the radii alone: every radius
    15..64 runs as two ring passes on a small raster (test_plane_rotation_across_routes asserts the routes of the call)"""
    from neilpy_amd import _lib
    return inc_rule(windows, [_lib.ROUTE_TWO_PASS if 15 <= r <= 64 else _lib.ROUTE_DIRECT for r in windows], 2)


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def bits(a):
    """the bit patterns of a float array: -0.0 is not +0.0"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(t, a):
    return np.array_equal(t.cpu().numpy().astype(a.dtype), a)


def holds(planes, want):
    """one of the workspace's three planes is `want`, bit for bit"""
    got, want = bits(planes.cpu().numpy()), bits(want)
    return any(np.array_equal(got[k], want) for k in range(3))


_references = {}


def reference(case, Zh, windows):
    """(mask, when, eroded surfaces, opened surfaces) of the reference, once per case id and window list.  Of a long list
    only the last two windows' surfaces are kept (what a workspace can hold); the others are None."""
    key = (case, tuple(int(r) for r in windows))
    if key not in _references:
        m, w, er, op = mn.progressive_filter(Zh, windows, 1, .15, return_when_dropped=True, return_surfaces=True)
        early = [None] * max(0, len(er) - 2)
        _references[key] = (m, w, early + er[-2:], early + op[-2:])
    return _references[key]


def pair_failures(r, mask, when, planes, ref, e_restated=None):
    """windows [r - 1, r] against ref = (mask, when, eroded surfaces, opened surfaces): e_R, opened_R and opened_{R-1} in
    the workspace's three planes, mask and when_dropped.  Returns the failing (r, what)."""
    rm, rw, er, op = ref
    checks = [("e_R", holds(planes, er[1])), ("opened_R", holds(planes, op[1])), ("opened_R-1", holds(planes, op[0])),
              ("mask", same(mask, rm)), ("when", same(when, rw))]
    if e_restated is not None:
        checks.append(("e_R restated", holds(planes, e_restated)))
    return [(r, what) for what, ok in checks if not ok]


def check_pairs(Zh, device, radii=range(16, 65), restated=False):
    """every R of radii alone: windows [R-1, R], the second one incremental, against the reference (pair_failures); with
    restated also e_R against the erosion of the opening written out.  Returns the failing (R, what)."""
    import torch
    Zd = torch.from_numpy(Zh).to(device)
    bad = []
    for r in radii:
        m, w, planes, route, taken = run_pf(Zd, [r - 1, r])
        assert taken == [0, 1], (r, taken, route)
        ref = mn.progressive_filter(Zh, [r - 1, r], 1, .15, return_when_dropped=True, return_surfaces=True)
        e = mn.erosion(mn.dilation(mn.erosion(Zh, r - 1, "rows"), r - 1, "rows"), r, "rows") if restated else None
        bad += pair_failures(r, m, w, planes.cpu(), ref, e)
    return bad
