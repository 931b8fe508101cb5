"""The incremental erosion route of progressive_filter (csrc/morph_incero.h) and the large-disk ring
kernels beside it on the GPU, at the shapes, values, launch grids and window lists where such kernels go wrong
(tests/window_cases.py), against an INDEPENDENT reference (tests/morph_numpy.py, pinned to SciPy and the goldens by
tests/test_morph_numpy.py): per radius the eroded and opened surfaces in the workspace, mask and when_dropped, bit for bit
(tests/pf_run.py).  Radii beyond 4 min(rows, cols) are in scope: the reference is the period-2n reflect the kernels claim
(DESIGN.md 2).  Then every radius against the ring erosion it replaces (SMRF_ERO_INC=2 against 0), and which windows are
eligible.  The premises these tests rest on are held without a GPU by tests/test_window_cases_host.py."""
import numpy as np
import pytest

import morph_numpy as mn
import window_cases as wc
from conftest import switch
from pf_run import adopted_radii, check_pairs, holds, inc_rule, reference, rotation_plan, run_pf, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nz(gpu_device):
    import neilpy_amd
    neilpy_amd.load_library()
    return neilpy_amd


# ---- a. every radius in isolation: one table, one run.  The rows of the shapes and of the value classes keep the test names
# and ids they have always had; every other row, and every new one, is a case of test_every_radius_alone ----
def alone_rows(prefix):
    return [pytest.param(c, id=c.id[len(prefix):]) for c in wc.ALONE if c.id.startswith(prefix)]


def run_alone(case, gpu_device, monkeypatch):
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    for name, value in case.switches.items():
        switch(monkeypatch, name, value)
    bad = check_pairs(case.make(), gpu_device, wc.RADII, restated=case.restated)
    assert not bad, bad


@pytest.mark.parametrize("case", alone_rows("shape_"))
def test_every_radius_alone_against_the_reference(nz, gpu_device, monkeypatch, case):
    run_alone(case, gpu_device, monkeypatch)


@pytest.mark.parametrize("case", alone_rows("value_"))
def test_every_radius_alone_awkward_values(nz, gpu_device, monkeypatch, case):
    run_alone(case, gpu_device, monkeypatch)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in wc.ALONE if not c.id.startswith(("shape_", "value_"))])
def test_every_radius_alone(nz, gpu_device, monkeypatch, case):
    run_alone(case, gpu_device, monkeypatch)


# ---- b. windows 15..64 in one call: many strips, several segments, streaming stores ------------------------------------
def check_15_64(Zh, case, gpu_device):
    import torch
    m, w, planes, route, taken = run_pf(torch.from_numpy(Zh).to(gpu_device), wc.W15_64)
    assert taken == [0] + [1] * 49, taken
    rm, rw, er, op = reference(case, Zh, wc.W15_64)
    assert same(m, rm) and same(w, rw)
    assert holds(planes, er[-1]), "eroded surface of window 64"
    assert holds(planes, op[-1]), "opened surface of window 64"


@pytest.mark.parametrize("remap", [None, "0"], ids=["xcd", "plain"])
@pytest.mark.parametrize("rows,cols,seg,grid,branch", wc.GRIDS, ids=["%dx%d" % (g[0], g[1]) for g in wc.GRIDS])
def test_many_strips_and_segments(nz, gpu_device, monkeypatch, rows, cols, seg, grid, branch, remap):
    wc.assert_grid(rows, cols, seg, grid, branch)
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    switch(monkeypatch, "SMRF_RING_SEG", seg)
    switch(monkeypatch, "SMRF_XCD_REMAP", remap)
    check_15_64(wc.grid_raster(rows, cols), "grid_%dx%d" % (rows, cols), gpu_device)


@pytest.mark.parametrize("name,value", wc.SEGMENT_SWITCHES)
@pytest.mark.parametrize("shape", wc.SEGMENT_SHAPES, ids=["%dx%d" % s for s in wc.SEGMENT_SHAPES])
def test_stores_and_segments(nz, gpu_device, monkeypatch, shape, name, value):
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    switch(monkeypatch, name, value)
    check_15_64(wc.segment_raster(shape), "segments_%dx%d" % shape, gpu_device)


# ---- c. plane rotation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [None, "0", "2"], ids=["fused_default", "fused0", "fused2"])
@pytest.mark.parametrize("k", range(30))
def test_plane_rotation_across_routes(nz, gpu_device, monkeypatch, k, fused):
    import torch
    from neilpy_amd import _lib
    win = wc.LISTS[k]
    # the premise: under mode 2 some window takes the route and a later one leaves it
    plan = rotation_plan(win)
    assert any(plan[i] and not plan[i + 1] for i in range(len(win) - 1)), win
    Zh = wc.rotation_raster()
    rm, rw, _, op = reference("rotation", Zh, win)
    Zd = torch.from_numpy(Zh).to(gpu_device)
    switch(monkeypatch, "SMRF_FUSED", fused)
    for mode in (0, 1, 2):
        switch(monkeypatch, "SMRF_ERO_INC", mode)
        m, w, planes, route, taken = run_pf(Zd, win)
        for r, rt in zip(win, route):
            if r == 0:
                assert rt == _lib.ROUTE_COPY
            elif r > 64:
                assert rt == _lib.ROUTE_DIRECT
            elif r >= 15 or fused == "0":
                assert rt == _lib.ROUTE_TWO_PASS, (r, rt)
            else:
                assert rt != _lib.ROUTE_TWO_PASS and rt not in (_lib.ROUTE_COPY, _lib.ROUTE_DIRECT), (r, rt)
        assert taken == inc_rule(win, route, mode), (mode, win, route, taken)
        if mode == 2:
            assert taken == plan
        assert same(m, rm) and same(w, rw), (mode, win)
        assert holds(planes, op[-1]), (mode, win)


def test_public_entry_point_numpy_and_tensor(nz, gpu_device, monkeypatch):
    import torch
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    win = np.array(wc.LISTS[3])
    Zh = wc.rough((120, 400), 78)
    rm, rw = mn.progressive_filter(Zh, win, 1, .15, return_when_dropped=True)
    m, w = nz.progressive_filter(Zh, win, 1, .15, return_when_dropped=True)
    assert isinstance(m, np.ndarray) and np.array_equal(m, rm) and np.array_equal(w, rw)
    mt, wt = nz.progressive_filter(torch.from_numpy(Zh).to(gpu_device), win, 1, .15, return_when_dropped=True)
    assert isinstance(mt, torch.Tensor) and mt.is_cuda
    assert np.array_equal(mt.cpu().numpy().astype(bool), rm) and np.array_equal(wt.cpu().numpy(), rw)


@pytest.mark.parametrize("lo,hi", [(15, 40), (30, 50)])
def test_whole_calls(nz, gpu_device, monkeypatch, lo, hi):
    """windows 15..40 and 30..50 on three strips give the reference's mask and when_dropped"""
    import torch
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    Z = wc.random_raster((150, 600), 33)
    windows = list(range(lo, hi + 1))
    m, w, planes, route, taken = run_pf(torch.from_numpy(Z).to(gpu_device), windows)
    assert taken == [0] + [1] * (len(windows) - 1), (taken, route)
    rm, rw = mn.progressive_filter(Z, windows, 1, .15, return_when_dropped=True)
    assert same(m, rm) and same(w, rw)


# ---- d. against the ring erosion it replaces, and eligibility -----------------------------------------------------------
@pytest.mark.parametrize("rows,cols,seg", [(150, 600, None), (1100, 520, None), (1100, 520, "136"), (40, 300, None)])
def test_every_radius_equals_the_ring_erosion(nz, gpu_device, monkeypatch, rows, cols, seg):
    """windows 1..64: a raster smaller than the large disks (150 x 600), one cut into several row segments per strip with a
    ragged last strip and last segment (1100 x 520; also with forced 136-row segments: warm-up rows of one segment inside
    another's outputs), and one shorter than most disks (40 rows: rows reflected several times over)"""
    import torch
    from neilpy_amd import _lib
    switch(monkeypatch, "SMRF_RING_SEG", seg)
    Zh = wc.synth_raster(rows, cols, 11)
    Zd = torch.from_numpy(Zh).to(gpu_device)
    win = np.arange(1, 65)
    switch(monkeypatch, "SMRF_ERO_INC", "0")
    m0, w0, p0, r0, t0 = run_pf(Zd, win)
    assert t0 == [0] * 64
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    m2, w2, p2, r2, t2 = run_pf(Zd, win)
    assert r2 == r0                                           # still two passes
    first_two_pass = r0.index(_lib.ROUTE_TWO_PASS)
    want = [int(i > first_two_pass and r0[i] == _lib.ROUTE_TWO_PASS and r0[i - 1] == _lib.ROUTE_TWO_PASS and win[i] >= 16)
            for i in range(64)]
    assert t2 == want and sum(t2) >= 49
    assert torch.equal(m0, m2) and torch.equal(w0, w2)
    # the last opened surface and the last eroded surface are in the workspace, in planes whose roles rotate
    last = torch.from_numpy(Zh).to(gpu_device)
    for r in win:
        e = nz.erosion(last, radius=int(r))
        last = nz.dilation(e, radius=int(r))
    for p in (p0, p2):
        assert any(torch.equal(p[k], last) for k in range(3))
        assert any(torch.equal(p[k], e) for k in range(3))


def test_eligibility(nz, gpu_device, monkeypatch):
    """the incremental erosion is taken for a two-pass window whose radius is the previous window's + 1 and whose previous
    window ran as two ring passes - not after a gap, not for the first two-pass window, not on a raster with NaNs, not with
    impl = direct, not in fp64, and with SMRF_ERO_INC=1 only where the table adopts the radius; the same bits every time"""
    import torch
    from neilpy_amd import _lib
    Zh = wc.synth_raster(300, 700, 5)
    Zd = torch.from_numpy(Zh).to(gpu_device)
    win = [15, 16, 18, 19, 30, 31, 31, 32, 20, 21]
    switch(monkeypatch, "SMRF_ERO_INC", "0")
    m0, w0, _, r0, t0 = run_pf(Zd, win)
    assert t0 == [0] * len(win) and r0 == [_lib.ROUTE_TWO_PASS] * len(win)
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    m2, w2, _, r2, t2 = run_pf(Zd, win)
    assert r2 == r0
    assert t2 == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert torch.equal(m0, m2) and torch.equal(w0, w2)
    # a fused window in between: 14 runs as one launch under SMRF_FUSED=2, so 15 has no eroded plane to start from
    switch(monkeypatch, "SMRF_FUSED", "2")
    _, _, _, rf, tf = run_pf(Zd, [13, 14, 15, 16])
    assert rf[1] == _lib.ROUTE_FUSED and rf[2:] == [_lib.ROUTE_TWO_PASS] * 2 and tf == [0, 0, 0, 1]
    switch(monkeypatch, "SMRF_FUSED", None)
    # impl = direct: the footprint-gather kernels, never
    md, wd, _, rd, td = run_pf(Zd, [15, 16, 17], impl=_lib.IMPL_DIRECT)
    assert rd == [_lib.ROUTE_DIRECT] * 3 and td == [0, 0, 0]
    mr, wr, _, rr, tr = run_pf(Zd, [15, 16, 17], impl=_lib.IMPL_RING)
    assert tr == [0, 1, 1] and torch.equal(md, mr) and torch.equal(wd, wr)
    # NaNs: scipy's NaN rule stays on the ring kernels (found by the library's own scan, or told by the caller)
    Zn = Zh.copy()
    Zn[17, 33] = np.nan
    Zn[200:203, 650:] = np.nan
    Znd = torch.from_numpy(Zn).to(gpu_device)
    mn_, wn, _, _, tn = run_pf(Znd, np.arange(1, 41))
    assert tn == [0] * 40
    switch(monkeypatch, "SMRF_ERO_INC", "0")
    mn0, wn0, _, _, _ = run_pf(Znd, np.arange(1, 41))
    assert torch.equal(mn_, mn0) and torch.equal(wn, wn0)
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    _, _, _, _, tn1 = run_pf(Znd, [15, 16, 17], nan_aware=1)
    assert tn1 == [0, 0, 0]
    # fp64 keeps the ring erosion
    _, _, _, r64, t64 = run_pf(Zd.double(), [15, 16, 17])
    assert r64 == [_lib.ROUTE_TWO_PASS] * 3 and t64 == [0, 0, 0]
    # the default (SMRF_ERO_INC unset = 1): the per-radius table of csrc/ero_inc_adopt.inc
    switch(monkeypatch, "SMRF_ERO_INC", None)
    adopt = adopted_radii()
    m1, w1, _, r1, t1 = run_pf(Zd, np.arange(1, 65))
    assert t1 == [int(r >= 16 and adopt[r]) for r in range(1, 65)]
    switch(monkeypatch, "SMRF_ERO_INC", "0")
    m00, w00, _, _, _ = run_pf(Zd, np.arange(1, 65))
    assert torch.equal(m1, m00) and torch.equal(w1, w00)
