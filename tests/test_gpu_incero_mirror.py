"""The incremental erosion under its mirror plan (csrc/morph_incero.h): one pair of LDS reads serves the low and the high ring
slot of a rim pair, so a wrong plan - a contribution applied twice or never, a first update that reads a slot already turned -
changes e_R.  Windows [R-1, R] for every R in 16..64 (the second one incremental, SMRF_ERO_INC=2) against
tests/morph_numpy.py's erosion, BIT FOR BIT, at the smallest shapes that reach each way the plan can go wrong:

  150 x 600           three strips: halo columns come from neighbouring strips
  7 x 300             fewer rows than the reach: the row fold wraps several times inside one batch
  40 x 257            one column in the second strip: the re-read lane of the last staging position
  130 x 256, seg 8/50 batches straddle segment starts, DELTA differs per radius (SMRF_RING_SEG)

on a seeded random raster and on one with +inf, -inf and -0.0 cells (no +0.0: min(-0.0, +0.0) has no agreed sign).  Whole
calls (windows 15..40 and 30..50 on 150 x 600) must give morph_numpy's mask and when_dropped."""
import numpy as np
import pytest

import morph_numpy as mn
from conftest import switch
from pf_run import run_pf

RADII = list(range(16, 65))


@pytest.fixture(scope="module")
def nz(gpu_device):
    import neilpy_amd
    neilpy_amd.load_library()
    return neilpy_amd


def random_raster(shape, seed):
    """rough at every scale, positive, with isolated low and high cells"""
    rng = np.random.default_rng(seed)
    Z = rng.normal(0, 1, shape).cumsum(0).cumsum(1) * .05 + 200 + rng.random(shape) * 2
    Z -= (rng.random(shape) < .02) * rng.uniform(1, 25, shape)
    return (Z + (rng.random(shape) < .05) * rng.uniform(1, 25, shape)).astype(np.float32)


def special_raster(shape, seed):
    """positive values with +inf cells (never a minimum), -0.0 cells (below every other finite value) and two -inf cells"""
    rng = np.random.default_rng(seed)
    Z = (rng.random(shape) * 3 + 1).astype(np.float32)
    Z[rng.random(shape) < .10] = np.inf
    Z[rng.random(shape) < .003] = -0.0
    for _ in range(2):
        Z[int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1]))] = -np.inf
    assert not np.any((Z == 0) & ~np.signbit(Z))
    return Z


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def failing_radii(Zh, gpu_device):
    """every R alone: e_R of windows [R-1, R] is one of the workspace's planes, bit for bit"""
    import torch
    Zd = torch.from_numpy(Zh).to(gpu_device)
    bad = []
    for r in RADII:
        m, w, planes, route, taken = run_pf(Zd, [r - 1, r])
        assert taken == [0, 1], (r, taken, route)
        last = mn.dilation(mn.erosion(Zh, r - 1, "rows"), r - 1, "rows")      # opened_{R-1}: what window R erodes
        want = bits(mn.erosion(last, r, "rows"))
        got = planes.cpu().numpy()
        if not any(np.array_equal(bits(got[k]), want) for k in range(3)):
            bad.append(r)
    return bad


SHAPES = [  # id, shape, SMRF_RING_SEG
    ("150x600", (150, 600), None),
    ("7x300", (7, 300), None),
    ("40x257", (40, 257), None),
    ("130x256_seg8", (130, 256), 8),
    ("130x256_seg50", (130, 256), 50),
]


@pytest.mark.gpu
@pytest.mark.parametrize("values", ["random", "inf_and_negative_zero"])
@pytest.mark.parametrize("shape,seg", [c[1:] for c in SHAPES], ids=[c[0] for c in SHAPES])
def test_every_radius_alone_bit_for_bit(nz, gpu_device, monkeypatch, shape, seg, values):
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    switch(monkeypatch, "SMRF_RING_SEG", seg)
    Z = random_raster(shape, 31) if values == "random" else special_raster(shape, 32)
    bad = failing_radii(Z, gpu_device)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", [(15, 40), (30, 50)])
def test_whole_calls(nz, gpu_device, monkeypatch, lo, hi):
    import torch
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    Z = random_raster((150, 600), 33)
    windows = list(range(lo, hi + 1))
    m, w, planes, route, taken = run_pf(torch.from_numpy(Z).to(gpu_device), windows)
    assert taken == [0] + [1] * (len(windows) - 1), (taken, route)
    rm, rw = mn.progressive_filter(Z, windows, 1, .15, return_when_dropped=True)
    assert np.array_equal(m.cpu().numpy().astype(bool), rm)
    assert np.array_equal(w.cpu().numpy(), rw)
