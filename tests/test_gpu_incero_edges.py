"""The incremental erosion (csrc/morph_incero.h) and the large-disk ring kernels beside it at the shapes, values and
launch grids where such kernels go wrong, against an INDEPENDENT reference (tests/morph_numpy.py, pinned to SciPy and the
goldens by tests/test_morph_numpy.py): per radius the eroded and opened surfaces, mask and when_dropped, bit for bit.
Radii beyond 4 min(rows, cols) are in scope: the reference is the period-2n reflect the kernels claim.
SMRF_ERO_INC=2 unless said otherwise.  No raster mixes -0.0 with +0.0; NaN rasters never take the route (test_eligibility)."""
import numpy as np
import pytest

import morph_numpy as mn
from conftest import switch
from pf_run import inc_rule, run_pf

pytestmark = pytest.mark.gpu

RADII = list(range(16, 65))
W15_64 = list(range(15, 65))


@pytest.fixture(scope="module")
def nz(gpu_device):
    import neilpy_amd
    neilpy_amd.load_library()
    return neilpy_amd


def rough(shape, seed):
    """finite, positive, rough at every scale, with isolated objects"""
    rng = np.random.default_rng(seed)
    Z = rng.normal(0, 1, shape).cumsum(0).cumsum(1) * .05 + 200 + rng.random(shape) * 2
    return (Z + (rng.random(shape) < .05) * rng.uniform(1, 25, shape)).astype(np.float32)


def holds(planes, want):
    import torch
    w = torch.from_numpy(want).to(planes.device)
    return any(torch.equal(planes[k], w) for k in range(3))


def same(t, a):
    return np.array_equal(t.cpu().numpy().astype(a.dtype), a)


def check_pairs(Zh, gpu_device):
    """every R in 16..64 alone: windows [R-1, R], the second one incremental; e_R, opened_R and opened_{R-1} in the
    workspace's three planes, mask and when_dropped - all against the reference.  Returns the failing (R, what)."""
    import torch
    Zd = torch.from_numpy(Zh).to(gpu_device)
    bad = []
    for r in RADII:
        m, w, planes, route, taken = run_pf(Zd, [r - 1, r])
        assert taken == [0, 1], (r, taken, route)
        rm, rw, er, op = mn.progressive_filter(Zh, [r - 1, r], 1, .15, return_when_dropped=True, return_surfaces=True)
        for what, ok in (("e_R", holds(planes, er[1])), ("opened_R", holds(planes, op[1])), ("opened_R-1", holds(planes, op[0])),
                         ("mask", same(m, rm)), ("when", same(w, rw))):
            if not ok:
                bad.append((r, what))
    return bad


# ---- a. every radius in isolation, awkward shapes -------------------------------------------------------------------
SHAPES = [(151, 300),                                     # odd, not a multiple of 8
          (1, 300), (3, 257), (7, 520),                   # fewer than 8 rows: one batch, DELTA rows early, rows folded many times
          (90, 5), (33, 1), (64, 2),                      # narrower than the reach: the column fold wraps several periods
          (24, 255), (24, 256), (24, 257)]                # strip edges


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_every_radius_alone_against_the_reference(nz, gpu_device, monkeypatch, shape):
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    bad = check_pairs(rough(shape, 100 + shape[0] + shape[1]), gpu_device)
    assert not bad, bad


# ---- b. many strips, several segments: the three placement branches ------------------------------------------------
def incero_grid(rows, cols, seg):
    """inc_erode_launch's grid under a forced SMRF_RING_SEG: seg rounded up to a multiple of 8"""
    seg = (seg + 7) // 8 * 8
    return (cols + 255) // 256, (rows + seg - 1) // seg


GRIDS = [  # rows, cols, SMRF_RING_SEG, grid, remap branch
    (40, 2048, 16, (8, 3), "mult8"),
    (48, 4096, 20, (16, 2), "mult8"),                     # 20 -> 24
    (40, 2100, 16, (9, 3), "ragged"),                     # 27 workgroups
    (56, 4200, 20, (17, 3), "ragged"),                    # 20 -> 24: segments of 24, 24, 8 rows; 51 workgroups
]
_ref_cache = {}


def reference_15_64(key, Zh):
    if key not in _ref_cache:
        m, w, er, op = mn.progressive_filter(Zh, W15_64, 1, .15, return_when_dropped=True, return_surfaces=True)
        _ref_cache[key] = (m, w, er[-1], op[-1])
    return _ref_cache[key]


def check_15_64(Zh, key, gpu_device):
    import torch
    m, w, planes, route, taken = run_pf(torch.from_numpy(Zh).to(gpu_device), W15_64)
    assert taken == [0] + [1] * 49, taken
    rm, rw, e_last, o_last = reference_15_64(key, Zh)
    assert same(m, rm) and same(w, rw)
    assert holds(planes, e_last), "eroded surface of window 64"
    assert holds(planes, o_last), "opened surface of window 64"


@pytest.mark.parametrize("remap", [None, "0"], ids=["xcd", "plain"])
@pytest.mark.parametrize("rows,cols,seg,grid,branch", GRIDS, ids=["%dx%d" % (g[0], g[1]) for g in GRIDS])
def test_many_strips_and_segments(nz, gpu_device, monkeypatch, rows, cols, seg, grid, branch, remap):
    gx, gy = incero_grid(rows, cols, seg)
    assert (gx, gy) == grid and gy > 1
    if branch == "mult8":
        assert gx % 8 == 0
    else:
        assert gx > 8 and gx % 8 != 0 and (gx * gy) % 8 != 0
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    switch(monkeypatch, "SMRF_RING_SEG", seg)
    switch(monkeypatch, "SMRF_XCD_REMAP", remap)
    check_15_64(rough((rows, cols), 7 + cols), ("grid", rows, cols), gpu_device)


# ---- c. values ------------------------------------------------------------------------------------------------------
def value_raster(kind):
    shape = (151, 300)
    rng = np.random.default_rng(31)
    Z = rough(shape, 32)
    if kind == "inf":
        Z[rng.random(shape) < .01] = np.inf
        Z[rng.random(shape) < .01] = -np.inf
    elif kind == "inf_block":                             # whole disks of +inf: the erosion's own identity element as a VALUE
        Z[:, :150] = np.inf
        Z[100:, :] = np.inf
    elif kind == "constant":
        Z[...] = np.float32(123.456)
    elif kind == "four_levels":
        Z = np.floor(rng.random(shape) * 4).astype(np.float32) * np.float32(2.5) + 1
    elif kind == "subnormal":
        Z = (rng.integers(1, 1 << 22, shape) * np.float32(1e-45)).astype(np.float32)
        assert (Z > 0).all() and (Z < np.finfo(np.float32).tiny).all()
    elif kind == "near_max":
        Z = rng.uniform(-3e38, 3e38, shape).astype(np.float32)
    elif kind == "negative_zero":
        Z = -np.abs(Z - 205)
        Z[rng.random(shape) < .1] = -0.0
        assert np.signbit(Z).all() and (Z == 0).any()
    return Z


@pytest.mark.parametrize("kind", ["inf", "inf_block", "constant", "four_levels", "subnormal", "near_max", "negative_zero"])
def test_every_radius_alone_awkward_values(nz, gpu_device, monkeypatch, kind):
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    bad = check_pairs(value_raster(kind), gpu_device)
    assert not bad, bad


# ---- d. streaming stores and forced segment lengths -----------------------------------------------------------------
@pytest.mark.parametrize("name,value", [("SMRF_NT", "1"), ("SMRF_RING_SEG", "8"), ("SMRF_RING_SEG", "50"), ("SMRF_RING_SEG", "136")])
@pytest.mark.parametrize("shape", [(1100, 520), (151, 300)], ids=["1100x520", "151x300"])
def test_stores_and_segments(nz, gpu_device, monkeypatch, shape, name, value):
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    switch(monkeypatch, name, value)
    check_15_64(rough(shape, 55), ("seg",) + shape, gpu_device)


# ---- e. plane rotation ----------------------------------------------------------------------------------------------
JOINS = ["repeat", "descent", "chain", "fused", "zero", "r65", "r70"]


def window_list(k):
    """three consecutive runs inside 15..64 joined by two of JOINS (every kind comes up 8-9 times over the 30 lists)"""
    rng = np.random.default_rng(9000 + k)
    out = []
    for j in range(3):
        n = int(rng.integers(2, 6))
        a = int(rng.integers(15, 65 - n + 1))
        run = list(range(a, a + n))
        out += run
        if j == 2:
            break
        kind = JOINS[(2 * k + j) % len(JOINS)]
        if kind == "repeat":
            out += [run[-1]]
        elif kind == "descent":
            out += [run[-1] - int(rng.integers(1, 4))]
        elif kind == "chain":
            out += [1, 2, 3]
        elif kind == "fused":
            out += [int(rng.choice([5, 8]))]
        elif kind == "zero":
            out += [0]
        else:
            out += [65 if kind == "r65" else 70]
    return out


LISTS = [window_list(k) for k in range(30)]
_rot_cache = {}


@pytest.mark.parametrize("fused", [None, "0", "2"], ids=["fused_default", "fused0", "fused2"])
@pytest.mark.parametrize("k", range(30))
def test_plane_rotation_across_routes(nz, gpu_device, monkeypatch, k, fused):
    import torch
    from neilpy_amd import _lib
    win = LISTS[k]
    # the premise: under mode 2 some window takes the route and a later one leaves it (judged on the radii alone: every
    # radius 15..64 runs as two ring passes on a raster this small, asserted below)
    two_pass = [int(15 <= r <= 64) for r in win]
    plan = inc_rule(win, [_lib.ROUTE_TWO_PASS if t else _lib.ROUTE_DIRECT for t in two_pass], 2)
    assert any(plan[i] and not plan[i + 1] for i in range(len(win) - 1)), win
    Zh = rough((120, 400), 77)
    if k not in _rot_cache:
        m, w, _, op = mn.progressive_filter(Zh, win, 1, .15, return_when_dropped=True, return_surfaces=True)
        _rot_cache[k] = (m, w, op[-1])
    rm, rw, o_last = _rot_cache[k]
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
        assert holds(planes, o_last), (mode, win)


def test_public_entry_point_numpy_and_tensor(nz, gpu_device, monkeypatch):
    import torch
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    win = np.array(LISTS[3])
    Zh = rough((120, 400), 78)
    rm, rw = mn.progressive_filter(Zh, win, 1, .15, return_when_dropped=True)
    m, w = nz.progressive_filter(Zh, win, 1, .15, return_when_dropped=True)
    assert isinstance(m, np.ndarray) and np.array_equal(m, rm) and np.array_equal(w, rw)
    mt, wt = nz.progressive_filter(torch.from_numpy(Zh).to(gpu_device), win, 1, .15, return_when_dropped=True)
    assert isinstance(mt, torch.Tensor) and mt.is_cuda
    assert np.array_equal(mt.cpu().numpy().astype(bool), rm) and np.array_equal(wt.cpu().numpy(), rw)
