"""The incremental erosion route of progressive_filter (csrc/morph_incero.h) on the GPU: every radius
16..64 against the ring erosion it replaces (SMRF_ERO_INC=2 against 0) - mask, when_dropped, and the last opened and
eroded surfaces in the workspace, bit for bit - and which windows are eligible."""
import numpy as np
import pytest

from conftest import switch
from pf_run import run_pf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nz(gpu_device):
    import neilpy_amd
    neilpy_amd.load_library()
    return neilpy_amd


def raster(nz, rows, cols, seed):
    rng = np.random.default_rng(seed)
    Z = nz.synth_dem(cols, seed=seed, dtype=np.float32, rows=rows)
    return (Z + (rng.random((rows, cols)) < 0.03) * rng.uniform(1, 25, (rows, cols))).astype(np.float32)


@pytest.mark.parametrize("rows,cols,seg", [(150, 600, None), (1100, 520, None), (1100, 520, "136"), (40, 300, None)])
def test_every_radius_equals_the_ring_erosion(nz, gpu_device, monkeypatch, rows, cols, seg):
    """windows 1..64: a raster smaller than the large disks (150 x 600), one cut into several row segments per strip with a
    ragged last strip and last segment (1100 x 520; also with forced 136-row segments: warm-up rows of one segment inside
    another's outputs), and one shorter than most disks (40 rows: rows reflected several times over)"""
    import torch
    from neilpy_amd import _lib
    switch(monkeypatch, "SMRF_RING_SEG", seg)
    Zh = raster(nz, rows, cols, 11)
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
    Zh = raster(nz, 300, 700, 5)
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
    mn, wn, _, _, tn = run_pf(Znd, np.arange(1, 41))
    assert tn == [0] * 40
    switch(monkeypatch, "SMRF_ERO_INC", "0")
    mn0, wn0, _, _, _ = run_pf(Znd, np.arange(1, 41))
    assert torch.equal(mn, mn0) and torch.equal(wn, wn0)
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    _, _, _, _, tn1 = run_pf(Znd, [15, 16, 17], nan_aware=1)
    assert tn1 == [0, 0, 0]
    # fp64 keeps the ring erosion
    _, _, _, r64, t64 = run_pf(Zd.double(), [15, 16, 17])
    assert r64 == [_lib.ROUTE_TWO_PASS] * 3 and t64 == [0, 0, 0]
    # the default (SMRF_ERO_INC unset = 1): the per-radius table of csrc/ero_inc_adopt.inc
    switch(monkeypatch, "SMRF_ERO_INC", None)
    import re, os
    inc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neilpy_amd", "csrc", "ero_inc_adopt.inc")).read()
    adopt = [int(v) for v in re.search(r"kEroIncAdoptF32\[65\] = \{(.*?)\}", inc, re.S).group(1).replace("\n", " ").split(",")]
    assert len(adopt) == 65
    m1, w1, _, r1, t1 = run_pf(Zd, np.arange(1, 65))
    assert t1 == [int(r >= 16 and adopt[r]) for r in range(1, 65)]
    switch(monkeypatch, "SMRF_ERO_INC", "0")
    m00, w00, _, _, _ = run_pf(Zd, np.arange(1, 65))
    assert torch.equal(m1, m00) and torch.equal(w1, w00)
