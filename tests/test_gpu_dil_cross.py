"""The cross on load (csrc/morph_ring.h ring_cross_kernel, routed by smrf_pf_fold of csrc/pf_route.h): a rim-free window
(R = 16, 21, 36: P_R empty, e_R = erode(e_{R-1}, 5-point cross)) launches no erosion, its dilation pass takes the cross while it
loads e_{R-1}.  Mask and when_dropped against the independent reference tests/morph_numpy.py, bit for bit, and against the same
call under SMRF_DIL_CROSS=0, at the shapes where a strip kernel goes wrong: rows far below 2R, strip seams, a one-column last
strip, a raster narrower than a strip, forced short segments; and on the value classes of the incremental erosion's tests.
Window lists, shapes and rasters are in tests/window_cases.py, the comparisons in tests/pf_run.py.

Whether a window was folded shows in the workspace: a folded LAST window leaves e_{R-1} there and no e_R (the planes hold e_{R-1},
opened_{R-1}, opened_R); a window on its own erosion leaves e_R and has written it over e_{R-1}."""
import numpy as np
import pytest

import pf_host
from conftest import switch
from pf_run import holds, reference, run_pf, same
from window_cases import (NOT_TAKEN, PLANE_LISTS, SHAPES, TABLE_LISTS, TAKEN, VALUE_KINDS, VALUE_LISTS, cross_raster, rough,
                          table_raster, value_raster)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nz(gpu_device):
    import neilpy_amd
    neilpy_amd.load_library()
    return neilpy_amd


def check(Zh, case, win, gpu_device, monkeypatch, folds_last):
    """the call under SMRF_DIL_CROSS=2 and =0: both equal the reference, and the workspace shows which of them folded"""
    import torch
    Zd = torch.from_numpy(Zh).to(gpu_device)
    rm, rw, er, op = reference(case, Zh, win)
    for mode in ("2", "0"):
        switch(monkeypatch, "SMRF_DIL_CROSS", mode)
        m, w, planes, route, taken = run_pf(Zd, win)
        assert same(m, rm), (mode, win, "mask")
        assert same(w, rw), (mode, win, "when")
        assert holds(planes, op[-1]), (mode, win, "opened surface of the last window")
        if folds_last and mode == "2":
            assert holds(planes, er[-2]) and holds(planes, op[-2]), (win, "a folded last window leaves e_{R-1} and opened_{R-1}")
            if not any(np.array_equal(er[-1], other) for other in (er[-2], op[-2], op[-1])):
                assert not holds(planes, er[-1]), (win, "e_R was written: the window ran an erosion pass")
        else:
            assert holds(planes, er[-1]), (mode, win, "eroded surface of the last window")


@pytest.mark.parametrize("win", TAKEN + NOT_TAKEN, ids=lambda w: "w" + "_".join(str(r) for r in w))
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes(nz, gpu_device, monkeypatch, shape, win):
    check(cross_raster(shape), "cross_%dx%d" % shape, win, gpu_device, monkeypatch, folds_last=win in TAKEN[:2])


@pytest.mark.parametrize("win", TAKEN, ids=lambda w: "w" + "_".join(str(r) for r in w))
@pytest.mark.parametrize("seg", [8, 24])
def test_segment_seams_inside_the_raster(nz, gpu_device, monkeypatch, seg, win):
    """SMRF_RING_SEG forces segments of 8 and 24 rows: 19 and 7 of them down the 150 rows, each starting 2R + 1 rows early"""
    switch(monkeypatch, "SMRF_RING_SEG", seg)
    check(cross_raster((150, 513)), "cross_150x513", win, gpu_device, monkeypatch, folds_last=win in TAKEN[:2])


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_value_classes(nz, gpu_device, monkeypatch, kind):
    Zh = value_raster(kind)
    for win in VALUE_LISTS:
        check(Zh, "value_" + kind, win, gpu_device, monkeypatch, folds_last=len(win) == 2)


def test_the_table_is_the_default_and_keeps_the_last_window(nz, gpu_device, monkeypatch):
    """default switches: a rim-free LAST window keeps its erosion pass (e_R is in the workspace); in the middle of a call the radii
    of dil_cross_adopt.inc fold and the results are the reference's"""
    import torch
    switch(monkeypatch, "SMRF_DIL_CROSS", None)
    Zh = table_raster()
    Zd = torch.from_numpy(Zh).to(gpu_device)
    for win in TABLE_LISTS:
        rm, rw, er, op = reference("cross_table", Zh, win)
        m, w, planes, route, taken = run_pf(Zd, win)
        assert same(m, rm) and same(w, rw), win
        assert holds(planes, er[-1]) and holds(planes, op[-1]), win


@pytest.mark.parametrize("win", PLANE_LISTS, ids=lambda w: "w" + "_".join(str(r) for r in w))
def test_the_workspace_plane_by_plane(nz, gpu_device, monkeypatch, win):
    """The plan against the execution, at plane level: the call's route and incremental-erosion report, the fold restated
    (pf_host.restated) and the driver's plane rotation restated (pf_host.parent_steps) say which surface EACH of the three planes
    holds after the call; each is the reference's, bit for bit.  SMRF_DIL_CROSS 0 / 1 / 2 x SMRF_ERO_INC 0 / 2."""
    import torch
    Zh = table_raster()
    Zd = torch.from_numpy(Zh).to(gpu_device)
    rm, rw, er, op = reference("cross_table", Zh, win)
    surfaces = {"e": er, "o": op}                           # (the windows before the last two: None, and never what a plane holds)
    for cross in (0, 1, 2):
        for inc_mode in (0, 2):
            switch(monkeypatch, "SMRF_DIL_CROSS", cross)
            switch(monkeypatch, "SMRF_ERO_INC", inc_mode)
            m, w, planes, route, taken = run_pf(Zd, win)
            fold, _ = pf_host.restated(dict(windows=win, dil_cross=cross), route, taken)
            labels = pf_host.replay(win, route, fold, pf_host.parent_steps(win, route, taken, fold))
            assert sum(lab != "junk" for lab in labels) == (3 if len(win) > 1 else 2), (cross, inc_mode, win, labels)
            for k, lab in enumerate(labels):
                if lab != "junk":
                    want = torch.from_numpy(surfaces[lab[0]][lab[1]]).to(gpu_device)
                    assert torch.equal(planes[k], want), (cross, inc_mode, win, k, labels)
            assert same(m, rm) and same(w, rw), (cross, inc_mode, win)


def test_a_raster_with_one_nan_is_not_taken(nz, gpu_device, monkeypatch):
    """scipy's NaN rule lives in the plain two-pass kernels: the same bytes in mask, when and all three planes with the switch at 2 and at 0"""
    import torch
    Zh = rough((97, 257), 655)
    Zh[40, 130] = np.nan
    Zd = torch.from_numpy(Zh).to(gpu_device)
    got = {}
    for mode in ("2", "0"):
        switch(monkeypatch, "SMRF_DIL_CROSS", mode)
        m, w, planes, route, taken = run_pf(Zd, [15, 16])
        got[mode] = [t.cpu().numpy().copy() for t in (m, w, planes)]
    for a, b in zip(got["2"], got["0"]):
        assert a.tobytes() == b.tobytes()
    assert np.isnan(got["2"][2]).any()
