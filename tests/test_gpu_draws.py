"""The drawn footprint table (tests/footprint_draws.py) on the MI355X: grey morphology and the rank
filters (section 20) at run lengths, level sets, tall and thin boxes, empty margins and members up to MAX_EXTENT apart
that the hand-made footprints of the sibling modules do not reach; the LDS caps of the runs path and of the rank tile at
rectangular boxes, computed from the library's own figures; three of the kinds on poisoned guard-banded memory.  Every
comparison is exact: by value against the oracle the siblings' reference() choose, bit for bit between paths.
tests/test_footprint_draws_host.py runs the same table through a NumPy model of the runs kernel, so a failure here
with that module green is the device's."""
import ctypes as C

import numpy as np
import pytest

import footprint_draws as fd
import footprint_numpy as fpn
import rank_numpy as rkn
from test_gpu_footprint import AUTO, RUNS, TAPS, NAMES, assert_same, check_paths, raster, reference, runs_refused
from test_gpu_rank import BISECT, TILE, impls, on_every_path, ranks_of
from test_gpu_rank import reference as rank_reference

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
GRADIENT = 3                                     # the store epilogue of the one-launch gradient (include/smrf_hip.h)
EDGE_HEIGHTS = (1, 3, 17, 40)
EDGE_SHAPE = (70, 129)


def _na():
    import neilpy_amd
    return neilpy_amd


def _mo():
    from neilpy_amd import morphology
    return morphology


def _rk():
    from neilpy_amd import rank
    return rank


# ------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fd.CASES, ids=fd.IDS)
def test_morphology_draws(gpu_device, case):
    """erosion and dilation (every fourth case: the seven functions) under AUTO, RUNS and TAPS, a forced runs launch
    refused exactly where the plan says so; a single member is a pure shift and is compared with the gather written
    directly; a float64 case whose planes fit for float32 only is run once more as float32, so that its level set
    is launched"""
    cid, shape, dtype, mode, spec, nan = case
    X, fp = fd.inputs(case)
    names = NAMES if fd.CASES.index(case) % 4 == 0 else ("grey_erosion", "grey_dilation")
    for name in names:
        check_paths(name, X, fp, mode, reference(name, X, fp, mode), (cid, name, mode))
    if fp.sum() == 1:
        mo = _mo()
        (dr,), (dc,) = fpn.members(fp)
        i, j = np.arange(shape[0]), np.arange(shape[1])
        for name, sign in (("grey_erosion", 1), ("grey_dilation", -1)):
            want = X[fpn.index(i + sign * dr, shape[0], mode)][:, fpn.index(j + sign * dc, shape[1], mode)]
            for impl in (AUTO, RUNS, TAPS):
                assert_same(getattr(mo, name)(X, footprint=fp, mode=mode, impl=impl), want, (cid, name, "shift", impl))
    if X.dtype == np.float64 and runs_refused("grey_erosion", fp, np.float64) and not runs_refused("grey_erosion", fp, np.float32):
        X32 = X.astype(np.float32)
        for name in ("grey_erosion", "grey_dilation"):
            check_paths(name, X32, fp, mode, reference(name, X32, fp, mode), (cid, name, mode, "as float32"), impls=(RUNS,))


@pytest.mark.parametrize("case", fd.CASES, ids=fd.IDS)
def test_rank_draws(gpu_device, case):
    """ranks {0, 1, n // 2, n - 2, n - 1} on every path; far footprints and those of more than 1000 members under AUTO
    and BISECT only"""
    cid, shape, dtype, mode, spec, nan = case
    X, fp = fd.inputs(case)
    n = int(fp.sum())
    paths = (AUTO, BISECT) if spec[0] == "far" or n > 1000 else impls(n)
    for rank in ranks_of(n):
        on_every_path(X, rank, fp, mode, rank_reference(X, rank, fp, mode), (cid, mode, rank), paths=paths)


# ------------------------------------------------------------------------------------------
# the LDS caps at rectangular boxes
# ------------------------------------------------------------------------------------------
def widest(fits):
    """the width w with fits(1 .. w) and not fits(w + 1)"""
    assert fits(1)
    w = 1
    while fits(w + 1):
        w += 1
    return w


@pytest.mark.parametrize("bh", EDGE_HEIGHTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_runs_cap_at_rectangles(gpu_device, dtype, bh):
    """bh x bw ones at the widest bw whose planes fit the cap the library reports and one wider, for the plain store and
    for the one-launch gradient (twice the planes): the path flips, both widths equal the reference, the forced runs
    launch past the cap is refused.  The public gradient takes one launch only for a footprint that is its own mirror
    image, so under an odd bh the odd widths on either side of that cap are run as well"""
    na, mo = _na(), _mo()
    lib = na.load_library()
    cap, item = lib.smrf_footprint_tile_bytes(), np.dtype(dtype).itemsize
    X = raster(np.random.default_rng([20270203, bh]), EDGE_SHAPE, dtype)
    path = lambda w, epilogue, impl: lib.smrf_footprint_path(                                           # noqa: E731
        mo.plan(np.ones((bh, w)), itemsize=item).head.ctypes.data_as(C.c_void_p), item, epilogue, impl)
    for gradient, epilogue, names in ((False, mo.STORE, ("grey_erosion", "grey_dilation")), (True, GRADIENT, ("morphological_gradient",))):
        w = widest(lambda bw: mo.plan(np.ones((bh, bw)), itemsize=item, gradient=gradient, cap=cap).lds_bytes <= cap)
        assert path(w, epilogue, RUNS) == 1 and path(w + 1, epilogue, RUNS) < 0, (bh, w, gradient)
        if bh * w >= mo.RUNS_MIN_TAPS:
            assert path(w, epilogue, AUTO) == 1 and path(w + 1, epilogue, AUTO) == 0, (bh, w, gradient)
        widths = [w, w + 1]
        if gradient and bh % 2:
            odd = w if w % 2 else w - 1
            widths += [v for v in (odd, odd + 2) if v >= 1 and v not in widths]
        for width in widths:
            fp = np.ones((bh, width), np.uint8)
            for name in names:
                check_paths(name, X, fp, "reflect", reference(name, X, fp, "reflect"), (name, bh, width))
            if gradient and bh % 2 and width % 2:                 # one launch: refused exactly past the gradient's cap
                assert runs_refused("morphological_gradient", fp, dtype) == (width > w), (bh, width)
            if not gradient and width > w:
                with pytest.raises(na.SmrfHipError, match="LDS"):
                    mo.grey_erosion(X, footprint=fp, impl=RUNS)


@pytest.mark.parametrize("density", [1.0, 0.1])
@pytest.mark.parametrize("bh", EDGE_HEIGHTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_tile_cap_at_rectangles(gpu_device, dtype, bh, density):
    """the tile of a bh x bw box takes (TY + bh - 1)(TX + bw - 1) keys and 4 bytes per member: for all-ones boxes and
    for boxes a tenth full (the box, not the members, fills the LDS) the widest bw under the cap the library reports and
    one wider: staged at the first, read from global memory at the second and a forced tile refused there, both equal
    to the reference"""
    na, mo, rk = _na(), _mo(), _rk()
    lib = rk._library()
    cap, item = lib.smrf_rank_tile_bytes(), np.dtype(dtype).itemsize
    cells = np.random.default_rng([20270204, bh]).random((bh, cap // (mo.TY * item) + 2)) < density

    def footprint(bw):
        fp = cells[:, :bw].astype(np.uint8)
        fp[0, 0] = fp[-1, -1] = 1                                  # the members span the box
        return fp
    w = widest(lambda bw: (mo.TY + bh - 1) * (mo.TX + bw - 1) * item + 4 * int(footprint(bw).sum()) <= cap)
    path = lambda bw: lib.smrf_rank_path(mo.plan(footprint(bw)).head.ctypes.data_as(C.c_void_p), item, AUTO)   # noqa: E731
    assert path(w) & rk.PATH_GLOBAL == 0 and path(w + 1) & rk.PATH_GLOBAL, (bh, w)
    X = raster(np.random.default_rng([20270205, bh]), EDGE_SHAPE, dtype)
    for width in (w, w + 1):
        fp = footprint(width)
        assert fd.box(fp) == (bh, width)
        want = rank_reference(X, int(fp.sum()) // 2, fp, "reflect")
        assert_same(rk.median_filter(X, footprint=fp), want, (bh, width, density, "auto"))
        if width == w:
            assert_same(rk.median_filter(X, footprint=fp, impl=TILE), want, (bh, width, density, "tile"))
        else:
            with pytest.raises(na.SmrfHipError, match="LDS"):
                rk.median_filter(X, footprint=fp, impl=TILE)


# ------------------------------------------------------------------------------------------
# guarded memory
# ------------------------------------------------------------------------------------------
GUARDED = (534, 547, 556)                         # a thin, a margin and a far case


def harness_cases():
    """erosion and median of one thin, one margin and one far case, as the harness_cases() of the sibling modules"""
    mo, rk = _mo(), _rk()
    for cid in GUARDED:
        case = fd.CASES[fd.IDS.index(str(cid))]
        mode, kind = case[3], case[4][0]
        X, fp = fd.inputs(case)
        yield dict(name="grey_erosion", fn=lambda Zt, fp=fp, mode=mode: mo.grey_erosion(Zt, footprint=fp, mode=mode), inputs=[X],
                   ctx=(cid, kind, "erosion"),
                   reference=lambda got, X=X, fp=fp, mode=mode: assert_same(got, reference("grey_erosion", X, fp, mode), "erosion"))
        yield dict(name="median_filter", fn=lambda Zt, fp=fp, mode=mode: rk.median_filter(Zt, footprint=fp, mode=mode), inputs=[X],
                   ctx=(cid, kind, "median"),
                   reference=lambda got, X=X, fp=fp, mode=mode: assert_same(got, rkn.median_filter(X, fp, mode), "median"))


def test_on_guarded_memory(gpu_device):
    from test_gpu_guarded import run_guarded
    assert [fd.CASES[fd.IDS.index(str(cid))][4][0] for cid in GUARDED] == ["thin", "margin", "far"]
    for case in harness_cases():
        run_guarded(**case)
