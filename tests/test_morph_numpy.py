"""tests/morph_numpy.py (the fast NumPy reference of the GPU tests) against the oracle's SciPy erosion / dilation /
progressive_filter and the reference's own goldens, bit for bit.  No raster mixes -0.0 with +0.0 (min / max do not order
them, in NumPy or in SciPy); comparisons are by value."""
import numpy as np
import pytest

import morph_numpy as mn
from conftest import golden, unpack
from oracle import smrf_oracle as orc


def raster(shape, dtype, seed, inf=False):
    rng = np.random.default_rng(seed)
    Z = (rng.normal(0, 1, shape).cumsum(0).cumsum(1) * .05 + 200 + (rng.random(shape) < .06) * rng.uniform(1, 25, shape)).astype(dtype)
    if inf:
        Z[rng.random(shape) < .01] = np.inf
        Z[rng.random(shape) < .01] = -np.inf
    return Z


def test_fold_is_the_period_2n_reflect():
    for n in (1, 2, 3, 7, 40):
        ext = np.concatenate([np.arange(n), np.arange(n)[::-1]])          # one period: 0 .. n-1, n-1 .. 0
        i = np.arange(-5 * n - 3, 5 * n + 4)
        assert np.array_equal(mn.fold(i, n), ext[np.mod(i, 2 * n)])
        assert np.array_equal(mn.fold(i, n), mn.fold(-1 - i, n))          # symmetric about the edge between -1 and 0
    Z = np.arange(12.).reshape(3, 4)
    assert np.array_equal(Z[mn.fold(np.arange(-3, 6), 3)], np.pad(Z, ((3, 3), (0, 0)), mode="symmetric"))


def test_disk_offsets_are_the_oracles_disk():
    for r in range(0, 71):
        d = orc.disk(r)
        want = sorted((int(y) - r, int(x) - r) for y, x in np.argwhere(d))
        assert sorted(mn.disk_offsets(r)) == want, r


FORMS = ["cells", "rows"]


@pytest.mark.parametrize("r", [1, 7, 16, 33, 50])
def test_erosion_and_dilation_equal_scipy_150x600(r):
    Z = raster((150, 600), np.float32, 3)
    fp = orc.disk(r)
    want_e = orc.erosion(Z, fp)
    want_d = orc.dilation(want_e, fp)
    for form in FORMS:
        e = mn.erosion(Z, r, form)
        assert e.dtype == Z.dtype and np.array_equal(e, want_e), form
        d = mn.dilation(e, r, form)
        assert d.dtype == Z.dtype and np.array_equal(d, want_d), form


@pytest.mark.parametrize("shape,radii,inf", [((37, 41), (0, 1, 2, 5, 12, 36, 40), False),       # odd sides, radius up to the sides
                                             ((37, 41), (3, 19, 50), True),
                                             ((9, 300), (1, 8, 9, 10, 20, 35), True),            # fewer rows than the radius
                                             ((300, 9), (4, 17, 35), False),
                                             ((1, 48), (1, 2, 3), False), ((64, 1), (1, 2, 3), True)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_erosion_and_dilation_equal_scipy_awkward_shapes(shape, radii, inf, dtype):
    """radii stay below 4 min(rows, cols), where SciPy's reflect table is valid"""
    Z = raster(shape, dtype, 11, inf=inf)
    for r in radii:
        assert r < 4 * min(shape)
        fp = orc.disk(r)
        want_e, want_d = orc.erosion(Z, fp), orc.dilation(Z, fp)
        for form in FORMS:
            e, d = mn.erosion(Z, r, form), mn.dilation(Z, r, form)
            assert e.dtype == d.dtype == dtype
            assert np.array_equal(e, want_e), (shape, r, form)
            assert np.array_equal(d, want_d), (shape, r, form)


@pytest.mark.parametrize("shape", [(151, 300), (1, 300), (3, 257), (90, 5), (33, 1), (64, 2), (1, 1), (24, 256)])
def test_both_forms_give_the_same_bits_at_every_radius(shape):
    """r = 0..70 on the shapes of the GPU tests, radii far beyond the raster's sides included, with +-inf cells, ties
    everywhere (4 levels), values near FLT_MAX and subnormals"""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    base = raster(shape, np.float32, 17, inf=True)
    rasters = [base, np.floor(rng.random(shape) * 4).astype(np.float32), (rng.uniform(-3e38, 3e38, shape)).astype(np.float32),
               (rng.integers(1, 1 << 20, shape) * np.float32(1e-45)).astype(np.float32), base.astype(np.float64)]
    for r in range(0, 71):
        for Z in rasters[:1] if r % 7 else rasters:
            for fn in (mn.erosion, mn.dilation):
                a, b = fn(Z, r, "cells"), fn(Z, r, "rows")
                assert a.dtype == b.dtype == Z.dtype and np.array_equal(a, b), (shape, r, fn.__name__)


def test_negative_zero_alone_and_a_constant_raster():
    Z = -np.abs(raster((20, 33), np.float32, 5)) + 200
    Z[Z > -1] = -0.0
    assert np.signbit(Z).all()
    for r in (1, 6, 21):
        for form in FORMS:
            assert np.array_equal(mn.erosion(Z, r, form), orc.erosion(Z, orc.disk(r)))
            assert np.array_equal(mn.dilation(Z, r, form), orc.dilation(Z, orc.disk(r)))
    C = np.full((13, 17), 7.25, dtype=np.float64)
    for form in FORMS:
        assert np.array_equal(mn.erosion(C, 9, form), C) and np.array_equal(mn.dilation(C, 9, form), C)


def test_radius_beyond_scipys_reflect_table():
    """r >= 4 min(rows, cols): no SciPy answer to compare with, so the definition itself, cell by cell"""
    Z = raster((3, 5), np.float64, 9)
    r = 23
    rows, cols = Z.shape
    e = mn.erosion(Z, r)
    assert np.array_equal(e, mn.erosion(Z, r, "rows"))
    for y in range(rows):
        for x in range(cols):
            want = min(Z[mn.fold(y + dy, rows), mn.fold(x + dx, cols)] for dy, dx in mn.disk_offsets(r))
            assert e[y, x] == want
    assert np.array_equal(mn.dilation(Z, r), -mn.erosion(-Z, r))


@pytest.mark.parametrize("shape,dtype,windows,cellsize,slope,inf", [
    ((150, 600), np.float32, [1, 7, 16, 33, 50], 1, .15, False),
    ((37, 41), np.float64, [0, 3, 4, 4, 12, 2], .5, .2, True),
    ((9, 300), np.float32, [2, 8, 20, 21, 35], 2, .1, True),
    ((41, 37), np.float32, [5], 1, .15, False),                           # one window: `last` stays the input
    ((41, 37), np.float64, [], 1, .15, False),
])
def test_progressive_filter_equals_the_oracle(shape, dtype, windows, cellsize, slope, inf):
    Z = raster(shape, dtype, 21, inf=inf)
    win = np.asarray(windows, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        m2, w2 = orc.progressive_filter(Z, win, cellsize, slope, return_when_dropped=True)
    for form in FORMS:
        m, w, er, op = mn.progressive_filter(Z, win, cellsize, slope, return_when_dropped=True, return_surfaces=True, form=form)
        assert np.array_equal(m, m2) and np.array_equal(w, w2), form
    assert m.dtype == bool and w.dtype == np.uint8 and len(er) == len(op) == len(win)
    assert np.array_equal(m, m2) and np.array_equal(w, w2)
    assert np.array_equal(mn.progressive_filter(Z, win, cellsize, slope), m2)
    last = Z
    for i, r in enumerate(win):                                            # the surfaces are the oracle's, window by window
        assert er[i].dtype == op[i].dtype == dtype
        assert np.array_equal(er[i], orc.erosion(last, orc.disk(r)))
        assert np.array_equal(op[i], orc.dilation(er[i], orc.disk(r)))
        if len(win) > 1:
            last = op[i]


PF = golden("progressive_filter.npz")


@pytest.mark.parametrize("tag", [str(c) for c in PF["cases"] if not str(c).startswith("nan_")])
def test_progressive_filter_goldens(tag):
    """every golden of the reference without NaNs, thin_*_rbig (R = 30 on 12 rows) included"""
    Z = PF[tag + "_Z"]
    cellsize, slope = PF[tag + "_params"]
    if cellsize == int(cellsize):
        cellsize = int(cellsize)
    mask, wd = mn.progressive_filter(Z, PF[tag + "_windows"], cellsize, slope, return_when_dropped=True)
    assert np.array_equal(mask, unpack(PF[tag + "_mask_bits"], Z.shape))
    assert np.array_equal(wd, PF[tag + "_when_dropped"])


def test_progressive_filter_w50_golden():
    """the benchmark's window list 1..50 on 768 x 1024 fp32 (the oracle needs 280 s for it): mask, when_dropped and the last
    opened surface as the reference computed them"""
    from neilpy_amd.synth import synth_dem
    mid = golden("progressive_filter_w50_mid.npz")
    rows, cols = (int(v) for v in mid["shape"])
    Z = synth_dem(cols, seed=int(mid["seed"]), dtype=np.float32, rows=rows)
    m, w, _, op = mn.progressive_filter(Z, mid["windows"], 1, .15, return_when_dropped=True, return_surfaces=True)
    assert np.array_equal(m, unpack(mid["mask_bits"], Z.shape))
    assert np.array_equal(w, mid["when_dropped"])
    assert np.array_equal(op[-1], mid["opened_last"])
