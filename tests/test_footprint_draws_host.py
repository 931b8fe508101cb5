"""The drawn footprint table (tests/footprint_draws.py), everything that needs no GPU: a NumPy model of the runs kernel
working from the plan that morphology.plan packs (footprint_numpy.runs_from_plan) against the restatement, so that a
failure on the device can be told from a failure of the plan; what the table covers, asserted, so that a redraw cannot
lose it; and the table's two oracles against each other (DESIGN.md sections 19 and 20)."""
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi

import footprint_draws as fd
import footprint_numpy as fpn
import rank_numpy as rkn
from test_gpu_footprint import _symmetric, assert_same
from test_gpu_rank import ranks_of

RUNS = 1


def _mo():
    from neilpy_amd import morphology
    return morphology


@functools.lru_cache(maxsize=None)
def plans(cid):
    """the erosion's plan of a case's footprint for float32 and float64, forced to the runs path"""
    mo = _mo()
    fp = fd.build(fd.CASES[fd.IDS.index(str(cid))][4])
    return {item: mo.plan(fp, itemsize=item, impl=RUNS) for item in (4, 8)}


# ------------------------------------------------------------------------------------------
# the model of the runs kernel
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fd.CASES, ids=fd.IDS)
def test_runs_model_equals_the_restatement(case):
    """erosion, dilation and the one-launch gradient (the maximum and the minimum of the erosion's samples: the
    gradient itself where the footprint is its own mirror image) in both modes, wherever the planes fit the cap; a
    float64 case whose planes fit for float32 only is modelled on the raster rounded to float32"""
    mo = _mo()
    X, fp = fd.inputs(case)
    if plans(case[0])[X.dtype.itemsize].path == "refused" and plans(case[0])[4].path == "runs":
        X = X.astype(np.float32)
    item = X.dtype.itemsize
    ran = 0
    for mode in ("reflect", "nearest"):
        low = None
        for op, dilate, gradient in (("min", False, False), ("max", True, False), ("both", False, True)):
            P = mo.plan(fp, dilate, itemsize=item, gradient=gradient, impl=RUNS)
            if P.path == "refused":
                continue
            got = fpn.runs_from_plan(X, P.head, P.table, mode, op)
            if op == "min":
                want = low = fpn.grey_erosion(X, fp, mode)
            elif op == "max":
                want = fpn.grey_dilation(X, fp, mode)
            else:
                low = fpn.grey_erosion(X, fp, mode) if low is None else low
                want = fpn._minus(-fpn.grey_erosion(-X, fp, mode), low)
                if _symmetric(fp):
                    assert_same(want, fpn.morphological_gradient(X, fp, mode), (case[0], mode, "symmetric"))
            assert_same(got, want, (case[0], mode, op, P.levels, P.slots))
            ran += 1
    assert ran or plans(case[0])[item].path == "refused"


# ------------------------------------------------------------------------------------------
# what the table covers
# ------------------------------------------------------------------------------------------
def test_the_table_is_well_formed():
    assert len(fd.CASES) >= 55 and len(set(fd.IDS)) == len(fd.CASES)
    for cid, shape, dtype, mode, spec, nan in fd.CASES:
        assert shape[0] in fd.ROWS and shape[1] in fd.COLS and dtype in fd.DTYPES and mode in ("reflect", "nearest"), cid
        kind, kh, kw = spec[:3]
        fp = fd.build(spec)
        assert fp.shape == (kh, kw) and kind in fd.KINDS, cid
        assert shape[0] * shape[1] * int(fp.sum()) <= fd.MAX_WORK <= 2e7, cid     # the rank bound, within morphology's
        if kind == "runs":
            assert 1 <= len(spec[3]) <= 6 and all(L in fd.RUN_LENGTHS for _, runs in spec[3] for _, L in runs), cid
            assert sorted(_mo().plan(fp).runs) == sorted((r - kh // 2, c - kw // 2, L) for r, runs in spec[3] for c, L in runs)
        elif kind == "bernoulli":
            assert 1 <= kh <= 40 and 1 <= kw <= 90 and spec[3] in fd.DENSITIES, cid
        elif kind == "thin":
            assert (min(kh, kw) in (1, 2, 3) and max(kh, kw) in fd.THIN_LONG and spec[3] in (1.0, 0.7)), cid
        elif kind == "margin":
            s, t = np.nonzero(fp)
            sides = (s.min() > 0) + (t.min() > 0) + (s.max() < kh - 1) + (t.max() < kw - 1)
            assert 1 <= sides <= 4, cid
            assert (s.min() + s.max(), t.min() + t.max()) != (2 * (kh // 2), 2 * (kw // 2)), (cid, "off-centre")
        else:
            assert (kh, kw) in fd.FAR_EXTENTS and shape in fd.FAR_RASTERS and 2 <= fp.sum() <= 5, cid
            assert not fpn.scipy_comparable(fp, shape), cid                          # the oracle is the restatement
    nans = sum(case[5] for case in fd.CASES)
    assert abs(nans - len(fd.CASES) / 5) <= 1
    thin = [c[4] for c in fd.CASES if c[4][0] == "thin"]
    assert {max(s[1], s[2]) for s in thin} == set(fd.THIN_LONG) and {s[3] for s in thin} == {1.0, 0.7}
    assert {min(s[1], s[2]) for s in thin} == {1, 2, 3}
    assert any(s[1] > s[2] for s in thin) and any(s[1] < s[2] for s in thin)
    margins = [fd.build(c[4]) for c in fd.CASES if c[4][0] == "margin"]
    assert sum(fp.sum() == 1 for fp in margins) >= 1 and sum(fp.sum() == 2 for fp in margins) >= 1
    far = {(c[4][1:3], c[1], c[3]) for c in fd.CASES if c[4][0] == "far"}
    assert far == {(e, s, m) for e in fd.FAR_EXTENTS for s in fd.FAR_RASTERS for m in ("reflect", "nearest")}
    ends = [np.nonzero(fd.build(c[4])) for c in fd.CASES if c[4][0] == "far"]
    assert max(max(s.max() - s.min(), t.max() - t.min()) for s, t in ends) == (1 << 20) - 1


def test_kinds_modes_and_dtypes():
    seen = {(c[4][0], c[3], c[2]) for c in fd.CASES}
    for kind in fd.KINDS:
        assert {m for k, m, _ in seen if k == kind} == {"reflect", "nearest"}, kind
        assert {d for k, _, d in seen if k == kind} == {"f32", "f64"}, kind
    even = [fd.build(c[4]).shape for c in fd.CASES if c[4][0] == "runs"]
    assert any(kh % 2 == 0 for kh, _ in even) and any(kw % 2 == 0 for _, kw in even)


def test_rasters_smaller_than_the_box():
    """at least eight cases with a raster smaller than the members' box in one axis and four in both, the far
    footprints - which are all of that kind - not counted"""
    one = both = 0
    for cid, shape, dtype, mode, spec, nan in fd.CASES:
        if spec[0] == "far":
            continue
        bh, bw = fd.box(fd.build(spec))
        under = (shape[0] < bh) + (shape[1] < bw)
        one += under == 1
        both += under == 2
    assert one >= 8 and both >= 4, (one, both)


def test_levels_slots_and_the_cap():
    tops, gapped, three, f64_only = set(), set(), 0, 0
    for case in fd.CASES:
        P = plans(case[0])
        levels = P[4].levels
        tops.add(levels[-1])
        if set(range(levels[0], levels[-1])) - set(levels):
            gapped.add(levels)
        three += P[4].nplanes >= 3
        f64_only += P[4].path == "runs" and P[8].path == "refused"
    assert tops >= set(range(8)), tops                      # every top level 0 .. 7
    assert len(gapped) >= 6, gapped                         # level sets with a gap between two used levels
    assert three >= 3 and f64_only >= 3, (three, f64_only)


# ------------------------------------------------------------------------------------------
# the table's references agree
# ------------------------------------------------------------------------------------------
COMPARABLE = [c for c in fd.CASES if not c[5] and c[4][0] != "far" and fpn.scipy_comparable(fd.build(c[4]), c[1])]


def test_most_cases_are_within_scipys_reach():
    assert len(COMPARABLE) >= 20, len(COMPARABLE)


@pytest.mark.parametrize("case", COMPARABLE, ids=lambda c: str(c[0]))
def test_scipy_equals_the_restatement(case):
    """the cases without NaN whose footprint SciPy's reflect table reaches: erosion, dilation and the rank filter"""
    X, fp = fd.inputs(case)
    mode = case[3]
    assert_same(fpn.grey_erosion(X, fp, mode), ndi.grey_erosion(X, footprint=fp, mode=mode), (case[0], "erosion"))
    assert_same(fpn.grey_dilation(X, fp, mode), ndi.grey_dilation(X, footprint=fp, mode=mode), (case[0], "dilation"))
    ordered = np.sort(rkn.samples(X, fp, mode), axis=-1)
    for rank in ranks_of(int(fp.sum())):
        assert_same(rkn.rank_filter(X, rank, fp, mode) if rank == 0 else ordered[..., rank],
                    ndi.rank_filter(X, rank, footprint=fp, mode=mode), (case[0], "rank", rank))
