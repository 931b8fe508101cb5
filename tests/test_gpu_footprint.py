"""Grey morphology with arbitrary flat footprints on the MI355X (neilpy_amd/morphology.py, csrc/footprint.hip; DESIGN.md
section 19): float32 and float64, the runs and the taps kernel path forced and the automatic choice, equality by value
with scipy.ndimage - or, where SciPy cannot serve (a NaN raster under an all-ones footprint, a footprint whose
half-extent reaches 2 * min(rows, cols)), with the NumPy restatement tests/footprint_numpy.py, which
tests/test_footprint_host.py pins to SciPy.  Rasters hold one sign of zero."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import footprint_numpy as fpn
from guarded import same_bits

pytestmark = pytest.mark.gpu

AUTO, RUNS, TAPS, FORCE_NAN = 0, 1, 2, 4
DTYPES = [np.float32, np.float64]
MODES = ["reflect", "nearest"]
NAMES = tuple(fpn.FUNCTIONS)


def _na():
    import neilpy_amd
    return neilpy_amd


def _mo():
    from neilpy_amd import morphology
    return morphology


def assert_same(got, want, ctx):
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), \
        (ctx, int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want))))))


def footprints():
    na, mo = _na(), _mo()
    rng = np.random.default_rng(20261110)
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 0, 0]], dtype=np.uint8)            # the lower arm missing
    rand47 = (rng.random((4, 7)) < 0.6).astype(np.uint8)
    rand47[0, 0], rand47[3, 6], rand47[1, 2] = 1, 1, 0                              # spans its box, holds a zero
    L = np.zeros((7, 4), dtype=np.uint8)
    L[:, 0] = 1
    L[6, :] = 1
    return {"1x1": np.ones((1, 1), np.uint8), "1x2": np.ones((1, 2), np.uint8), "2x1": np.ones((2, 1), np.uint8),
            "3x3": np.ones((3, 3), np.uint8), "cross": cross, "rand4x7": rand47, "L7x4": L,
            "row65": np.ones((1, 65), np.uint8), "diamond5": mo.diamond(5), "square31": mo.square(31)}


SHAPES = ((1, 1), (1, 130), (130, 1), (7, 5), (9, 65), (70, 129), (150, 300))


def raster(rng, shape, dtype, nan=0.0):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    Z = np.sin(x / 7.0) * 9 + np.cos(y / 5.0) * 6 + rng.normal(size=shape) * 2 + 50
    Z = Z.astype(dtype)
    if nan:
        Z[rng.random(shape) < nan] = np.nan
    return Z


def reference(name, X, fp, mode):
    """SciPy where it is the oracle of the contract, the restatement elsewhere"""
    if fpn.scipy_comparable(fp, X.shape) and not (np.isnan(X).any() and np.all(fp != 0)):
        with np.errstate(invalid="ignore"):
            return getattr(ndi, name)(X, footprint=fp, mode=mode)
    return fpn.FUNCTIONS[name](X, fp, mode)


def refused(fp, dilate, dtype, gradient=False):
    mo = _mo()
    return mo.plan(fp, dilate, itemsize=np.dtype(dtype).itemsize, gradient=gradient, impl=RUNS).path == "refused"


def runs_refused(name, fp, dtype):
    """whether a forced runs launch of this function is refused: one of its launches' planes do not fit the LDS cap"""
    launches = {"grey_erosion": [(0, 0)], "grey_dilation": [(1, 0)],
                "morphological_gradient": [(0, 1)] if _symmetric(fp) else [(0, 0), (1, 0)]}.get(name, [(0, 0), (1, 0)])
    return any(refused(fp, d, dtype, g) for d, g in launches)


def check_paths(name, X, fp, mode, want, ctx, impls=(AUTO, RUNS, TAPS)):
    """one function under every impl: the forced runs path is refused exactly where the plan says so"""
    na, mo = _na(), _mo()
    f = getattr(mo, name)
    for impl in impls:
        if impl == RUNS and runs_refused(name, fp, X.dtype):
            with pytest.raises(na.SmrfHipError, match="LDS"):
                f(X, footprint=fp, mode=mode, impl=impl)
            continue
        assert_same(f(X, footprint=fp, mode=mode, impl=impl), want, ctx + (impl,))


def _symmetric(fp):
    fp = np.asarray(fp) != 0
    return fp.shape[0] % 2 == 1 and fp.shape[1] % 2 == 1 and np.array_equal(fp, fp[::-1, ::-1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_erosion_and_dilation_against_scipy(gpu_device, dtype, mode):
    rng = np.random.default_rng(20261111)
    for shape in SHAPES:
        X = raster(rng, shape, dtype)
        for tag, fp in footprints().items():
            for name in ("grey_erosion", "grey_dilation"):
                check_paths(name, X, fp, mode, reference(name, X, fp, mode), (name, shape, tag, mode))


@pytest.mark.parametrize("dtype", DTYPES)
def test_size_is_an_all_ones_footprint(gpu_device, dtype):
    na, mo = _na(), _mo()
    X = raster(np.random.default_rng(3), (70, 129), dtype)
    for size in (3, (2, 5), (6, 1)):
        for name in NAMES:
            assert_same(getattr(mo, name)(X, size), getattr(ndi, name)(X, size=size), (name, size))
    assert_same(mo.grey_erosion(X, 5, np.ones((1, 2))), ndi.grey_erosion(X, footprint=np.ones((1, 2))), "footprint wins")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_seven_functions_against_scipy(gpu_device, dtype, mode):
    """with the fused epilogues: the top-hats and the gradient equal the planes computed launch by launch"""
    na, mo = _na(), _mo()
    rng = np.random.default_rng(20261112)
    X = raster(rng, (70, 129), dtype)
    fps = footprints()
    for tag in ("rand4x7", "diamond5"):             # the gradient of the first takes two launches, of the second one
        fp = fps[tag]
        for name in NAMES:
            check_paths(name, X, fp, mode, reference(name, X, fp, mode), (name, tag, mode))
        for impl in (RUNS, TAPS):
            kw = dict(footprint=fp, mode=mode, impl=impl)
            assert_same(mo.white_tophat(X, **kw), X - mo.grey_opening(X, **kw), ("white", tag, impl))
            assert_same(mo.black_tophat(X, **kw), mo.grey_closing(X, **kw) - X, ("black", tag, impl))
            if not (impl == RUNS and runs_refused("morphological_gradient", fp, dtype)):
                assert_same(mo.morphological_gradient(X, **kw), mo.grey_dilation(X, **kw) - mo.grey_erosion(X, **kw),
                            ("gradient", tag, impl))


@pytest.mark.parametrize("dtype", DTYPES)
def test_disks_equal_the_disk_kernels(gpu_device, dtype):
    na, mo = _na(), _mo()
    X = raster(np.random.default_rng(20261113), (70, 129), dtype)
    for r in (0, 1, 8, 30):
        fp = na.disk(r)
        for name, old in (("grey_erosion", na.erosion), ("grey_dilation", na.dilation), ("grey_opening", na.opening)):
            check_paths(name, X, fp, "reflect", old(X, radius=r), (name, "disk", r))


@pytest.mark.parametrize("dtype", DTYPES)
def test_runs_path_at_the_lds_cap_and_past_it(gpu_device, dtype):
    """the largest square whose planes fit the cap the library reports: runs = taps = SciPy; one wider: the automatic
    choice is the taps path and a forced runs launch is refused"""
    na, mo = _na(), _mo()
    cap = na.load_library().smrf_footprint_tile_bytes()
    item = np.dtype(dtype).itemsize
    w = 1
    while mo.plan(mo.square(w + 1), itemsize=item, cap=cap).lds_bytes <= cap:
        w += 1
    assert mo.plan(mo.square(w), itemsize=item, cap=cap).path == "runs"
    assert mo.plan(mo.square(w + 1), itemsize=item, cap=cap).path == "taps"
    X = raster(np.random.default_rng(20261114), (70, 129), dtype)
    for width in (w, w + 1):
        for name in ("grey_erosion", "grey_dilation"):
            want = getattr(ndi, name)(X, size=width)
            assert_same(getattr(mo, name)(X, size=width), want, (name, width, "auto"))
            assert_same(getattr(mo, name)(X, size=width, impl=TAPS), want, (name, width, "taps"))
            if width == w:
                assert_same(getattr(mo, name)(X, size=width, impl=RUNS), want, (name, width, "runs"))
            else:
                with pytest.raises(na.SmrfHipError, match="LDS"):
                    getattr(mo, name)(X, size=width, impl=RUNS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan(gpu_device, dtype):
    na, mo = _na(), _mo()
    rng = np.random.default_rng(20261115)
    fps = footprints()
    holed = ("cross", "rand4x7", "L7x4", "diamond5")                # SciPy's footprint filter is the oracle
    ones = ("1x2", "2x1", "3x3", "row65", "square31")               # the restatement is (deviations)
    assert all(not fps[t].all() for t in holed) and all(fps[t].all() for t in ones)
    for X in (raster(rng, (70, 129), dtype, nan=0.2), np.full((9, 65), np.nan, dtype=dtype)):
        for tag in holed + ones:
            for mode in MODES:
                for name in ("grey_erosion", "grey_dilation", "white_tophat", "morphological_gradient"):
                    if name in ("white_tophat", "morphological_gradient") and (mode == "nearest" or tag == "square31"):
                        continue
                    check_paths(name, X, fps[tag], mode, reference(name, X, fps[tag], mode), (name, tag, mode, X.shape))
    # the NaN-aware launch on a raster without NaN: the same bits as the plain one
    X = raster(rng, (70, 129), dtype)
    for tag in ("rand4x7", "diamond5", "3x3"):
        for name in NAMES:
            for impl in (RUNS, TAPS):
                if impl == RUNS and runs_refused(name, fps[tag], dtype):
                    continue
                assert same_bits(getattr(mo, name)(X, footprint=fps[tag], impl=impl | FORCE_NAN),
                                 getattr(mo, name)(X, footprint=fps[tag], impl=impl)), (name, tag, impl)


def test_tensors_and_views(gpu_device):
    """tensor in, tensor out; the dtypes; integer and empty rasters (views of the input: tests/test_gpu_views.py)"""
    import torch
    na, mo = _na(), _mo()
    rng = np.random.default_rng(20261116)
    Z = raster(rng, (90, 140), np.float64)
    Z[5, 7] = np.nan
    Zt = torch.from_numpy(Z).to(gpu_device)
    keep = Zt.clone()
    fp = footprints()["rand4x7"]
    for name in NAMES:
        f = lambda A: getattr(mo, name)(A, footprint=fp, mode="nearest")
        t, n = f(Zt), f(Z)
        assert isinstance(t, torch.Tensor) and t.device == Zt.device and t.dtype == Zt.dtype and isinstance(n, np.ndarray)
        assert_same(t.cpu().numpy(), n, name)
        assert f(Zt.float()).dtype == torch.float32
    assert torch.equal(Zt.view(torch.int64), keep.view(torch.int64))           # the input is unchanged
    # integer rasters are widened to float64; an empty raster comes back empty
    Zi = np.round(Z[:, 10:] * 3).astype(np.int32)
    assert_same(mo.grey_opening(Zi, footprint=fp), ndi.grey_opening(Zi.astype(np.float64), footprint=fp), "int raster")
    for name in NAMES:
        e = getattr(mo, name)(np.zeros((0, 5), np.float32), size=3)
        assert e.shape == (0, 5) and e.dtype == np.float32
