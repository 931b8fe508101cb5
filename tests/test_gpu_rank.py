"""Median, rank, percentile, minimum and maximum filters with arbitrary flat footprints on the MI355X (neilpy_amd/rank.py,
csrc/rank.hip): float32 and float64, both selection methods and both sample sources forced and the
automatic choice, equality by value with scipy.ndimage - or, where SciPy cannot serve (a NaN raster, a footprint whose
half-extent reaches 2 * min(rows, cols)), with the NumPy restatement tests/rank_numpy.py, which tests/test_rank_host.py
pins to SciPy - and equality bit for bit between the paths.  No tolerance anywhere.  Rasters hold one sign of zero."""
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

import footprint_numpy as fpn
import rank_numpy as rkn
from conftest import ROOT
from guarded import same_bits
from test_gpu_footprint import SHAPES, assert_same, footprints, raster

pytestmark = pytest.mark.gpu

AUTO, COUNT, BISECT, FORCE_NAN, GLOBAL, TILE = 0, 1, 2, 4, 8, 16
DTYPES = [np.float32, np.float64]
MODES = ["reflect", "nearest"]
PERCENTILES = (0, 10, 33.3, 50, 75, 99.9, 100, -20)
COUNT_LIMIT = 65                      # COUNT is forced on footprints of at most this many members
BIG = "square31"                      # 961 members: on 70 x 129 only, under AUTO and BISECT only


def _rk():
    from neilpy_amd import rank
    return rank


def impls(n):
    """every path that is run for a footprint of n members: (method, method with GLOBAL forced)"""
    methods = (AUTO, BISECT) + ((COUNT,) if n <= COUNT_LIMIT else ())
    return [m | g for m in methods for g in (0, GLOBAL)]


def ranks_of(n):
    return sorted({r for r in (0, 1, n // 2, n - 2, n - 1) if 0 <= r < n})


def reference(X, rank, fp, mode):
    """SciPy where it is the oracle of the contract, the restatement elsewhere"""
    if fpn.scipy_comparable(fp, X.shape) and not np.isnan(X).any():
        return ndi.rank_filter(X, rank, footprint=fp, mode=mode)
    return rkn.rank_filter(X, rank, fp, mode)


def on_every_path(X, rank, fp, mode, want, ctx, paths=None):
    """rank_filter under every path: the first against the reference by value, the others against the first bit for bit"""
    import torch
    rk = _rk()
    Xt = torch.from_numpy(X).cuda()
    first = None
    for impl in paths or impls(int(np.count_nonzero(fp))):
        got = rk.rank_filter(Xt, rank, footprint=fp, mode=mode, impl=impl).cpu().numpy()
        if first is None:
            first = got
            assert_same(got, want, ctx + (impl,))
        else:
            assert same_bits(got, first), ctx + (impl, int(np.sum(got.view(np.uint8) != first.view(np.uint8))))
    return first


# ------------------------------------------------------------------------------------------
# ranks and paths
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_ranks_on_every_path_against_scipy(gpu_device, dtype, mode):
    """every shape x footprint at ranks {0, 1, n // 2, n - 2, n - 1}: AUTO against SciPy (the restatement where the
    footprint outgrows SciPy's reflect table), then COUNT, BISECT and each with GLOBAL forced against AUTO's bits - the
    forced methods take rank 0 and n - 1 through the rank kernel, AUTO through the grey-morphology kernel"""
    rng = np.random.default_rng(20261211)
    for shape in SHAPES:
        X = raster(rng, shape, dtype)
        for tag, fp in footprints().items():
            if tag == BIG and shape != (70, 129):
                continue
            for rank in ranks_of(int(fp.sum())):
                on_every_path(X, rank, fp, mode, reference(X, rank, fp, mode), (shape, tag, mode, rank))


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_edges_of_count(gpu_device, dtype):
    """all-ones rows of block - 1, block, block + 1 and 2 block + 1 members: the last block of candidates full, one short
    and holding one member"""
    rk = _rk()
    B = rk.COUNT_BLOCK
    X = np.round(raster(np.random.default_rng(20261212), (9, 65), dtype))          # ties across the block's edge
    for n in (B - 1, B, B + 1, 2 * B, 2 * B + 1):
        fp = np.ones((1, n), np.uint8)
        for rank in range(n):
            on_every_path(X, rank, fp, "reflect", reference(X, rank, fp, "reflect"), ("row", n, rank),
                          paths=(COUNT, COUNT | GLOBAL, BISECT))


@pytest.mark.parametrize("dtype", DTYPES)
def test_prefix_skip_of_bisect(gpu_device, dtype):
    """a constant raster (all members equal: no pass), two values that differ in the lowest mantissa bit (one pass), values
    of both signs (no common prefix), a quantised raster (ties) and one with +-inf"""
    rng = np.random.default_rng(20261213)
    shape = (70, 129)
    one = dtype(37.25)
    two = np.where(rng.random(shape) < 0.5, one, np.nextafter(one, dtype(100))).astype(dtype)
    signs = (rng.normal(size=shape) * 1e3).astype(dtype)
    signs[rng.random(shape) < 0.1] = 0.0
    inf = raster(rng, shape, dtype)
    inf[rng.random(shape) < 0.1] = np.inf
    inf[rng.random(shape) < 0.1] = -np.inf
    rasters = {"constant": np.full(shape, one, dtype), "lowest bit": two, "both signs": signs,
               "quantised": np.round(raster(rng, shape, dtype)), "inf": inf}
    fps = footprints()
    for name, X in rasters.items():
        for tag in ("rand4x7", "diamond5", "1x2"):
            fp = fps[tag]
            for rank in ranks_of(int(fp.sum())):
                on_every_path(X, rank, fp, "reflect", reference(X, rank, fp, "reflect"), (name, tag, rank))


# ------------------------------------------------------------------------------------------
# the public functions
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_public_functions_against_scipy(gpu_device, dtype):
    rk = _rk()
    X = raster(np.random.default_rng(20261214), (70, 129), dtype)
    fps = footprints()
    for mode in MODES:
        for size in (3, (2, 5), (6, 1)):
            kw = dict(size=size, mode=mode)
            assert_same(rk.median_filter(X, **kw), ndi.median_filter(X, **kw), ("median", size, mode))
            assert_same(rk.minimum_filter(X, **kw), ndi.minimum_filter(X, **kw), ("minimum", size, mode))
            assert_same(rk.maximum_filter(X, **kw), ndi.maximum_filter(X, **kw), ("maximum", size, mode))
            assert_same(rk.rank_filter(X, -2, **kw), ndi.rank_filter(X, -2, **kw), ("rank -2", size, mode))
        for tag in ("rand4x7", "diamond5", "cross"):
            kw = dict(footprint=fps[tag], mode=mode)
            assert_same(rk.median_filter(X, **kw), ndi.median_filter(X, **kw), ("median", tag, mode))
            assert_same(rk.minimum_filter(X, **kw), ndi.minimum_filter(X, **kw), ("minimum", tag, mode))
            assert_same(rk.maximum_filter(X, **kw), ndi.maximum_filter(X, **kw), ("maximum", tag, mode))
            for p in PERCENTILES:
                assert_same(rk.percentile_filter(X, p, **kw), ndi.percentile_filter(X, p, **kw), ("percentile", p, tag, mode))
    # positional as in SciPy; a footprint wins over size
    assert_same(rk.median_filter(X, 5, np.ones((1, 2))), ndi.median_filter(X, footprint=np.ones((1, 2))), "footprint wins")
    assert_same(rk.rank_filter(X, 3, (2, 3)), ndi.rank_filter(X, 3, (2, 3)), "positional rank")
    assert_same(rk.percentile_filter(X, 40, 3), ndi.percentile_filter(X, 40, 3), "positional percentile")


@pytest.mark.parametrize("dtype", DTYPES)
def test_maximum_reads_the_footprint_unmirrored(gpu_device, dtype):
    """on the even, asymmetric rand4x7 maximum_filter is ndimage's and is not grey_dilation, on every path"""
    from neilpy_amd import morphology as mo
    rk = _rk()
    X = raster(np.random.default_rng(20261215), (70, 129), dtype)
    fp = footprints()["rand4x7"]
    want = ndi.maximum_filter(X, footprint=fp)
    assert not np.array_equal(want, ndi.grey_dilation(X, footprint=fp))
    assert not np.array_equal(rk.maximum_filter(X, footprint=fp), mo.grey_dilation(X, footprint=fp))
    for impl in impls(int(fp.sum())):
        assert_same(rk.maximum_filter(X, footprint=fp, impl=impl), want, ("maximum", impl))
        assert_same(rk.minimum_filter(X, footprint=fp, impl=impl), ndi.minimum_filter(X, footprint=fp), ("minimum", impl))


# ------------------------------------------------------------------------------------------
# NaN
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan(gpu_device, dtype):
    """20 % NaN (a tenth of them of negative sign) and all NaN: np.sort's order on every path; with NaN present rank 0 and
    n - 1 go through the rank kernel too"""
    rk = _rk()
    rng = np.random.default_rng(20261216)
    fps = footprints()
    Z = raster(rng, (70, 129), dtype, nan=0.2)
    neg = np.isnan(Z) & (rng.random(Z.shape) < 0.1)
    Z[neg] = np.copysign(np.nan, -1)
    assert np.signbit(Z[neg]).all() and neg.any()
    for X in (Z, np.full((9, 65), np.nan, dtype=dtype)):
        for tag in ("1x1", "1x2", "2x1", "3x3", "cross", "rand4x7", "L7x4", "diamond5"):
            fp = fps[tag]
            for mode in MODES:
                for rank in ranks_of(int(fp.sum())):
                    want = rkn.rank_filter(X, rank, fp, mode)
                    on_every_path(X, rank, fp, mode, want, ("nan", X.shape, tag, mode, rank))
    fp = fps["rand4x7"]
    lo, hi = rk.minimum_filter(Z, footprint=fp), rk.maximum_filter(Z, footprint=fp)
    assert_same(lo, rkn.minimum_filter(Z, fp), "minimum with NaN")
    assert_same(hi, rkn.maximum_filter(Z, fp), "maximum with NaN")
    S = rkn.samples(Z, fp)
    assert np.array_equal(np.isnan(lo), np.isnan(S).all(-1)) and np.array_equal(np.isnan(hi), np.isnan(S).any(-1))
    assert np.isnan(hi).sum() > np.isnan(lo).sum()
    # the NaN-aware launch on a raster without NaN: the same bits as the plain one
    X = raster(rng, (70, 129), dtype)
    for tag in ("rand4x7", "diamond5", "3x3"):
        n = int(fps[tag].sum())
        for impl in impls(n):
            if not impl & ~GLOBAL:
                continue                       # AUTO takes rank 0 of a plain launch to another kernel
            for rank in ranks_of(n):
                assert same_bits(rk.rank_filter(X, rank, footprint=fps[tag], impl=impl | FORCE_NAN),
                                 rk.rank_filter(X, rank, footprint=fps[tag], impl=impl)), (tag, impl, rank)


# ------------------------------------------------------------------------------------------
# the LDS cap
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_at_the_lds_cap_and_past_it(gpu_device, dtype):
    """the largest square whose tile fits the cap the library reports: the automatic choice stages it; one wider: it reads
    global memory and a forced tile is refused; both equal SciPy"""
    import ctypes as C
    import neilpy_amd as na
    from neilpy_amd import morphology as mo
    rk = _rk()
    lib = rk._library()
    cap, item = lib.smrf_rank_tile_bytes(), np.dtype(dtype).itemsize
    w = 1
    while (mo.TY + w) * (mo.TX + w) * item + 4 * (w + 1) ** 2 <= cap:           # the keys of tile and halo, the members' offsets
        w += 1
    path = lambda width, impl: lib.smrf_rank_path(mo.plan(mo.square(width)).head.ctypes.data_as(C.c_void_p), item, impl)   # noqa: E731
    assert path(w, AUTO) == rk.PATH_BISECT | rk.PATH_TILE and path(w + 1, AUTO) == rk.PATH_BISECT | rk.PATH_GLOBAL
    X = raster(np.random.default_rng(20261217), (70, 129), dtype)
    for width in (w, w + 1):
        want = ndi.median_filter(X, size=width)
        assert_same(rk.median_filter(X, size=width), want, (width, "auto"))
        if width == w:
            assert_same(rk.median_filter(X, size=width, impl=TILE), want, (width, "tile"))
        else:
            with pytest.raises(na.SmrfHipError, match="LDS"):
                rk.median_filter(X, size=width, impl=TILE)


# ------------------------------------------------------------------------------------------
# tensors
# ------------------------------------------------------------------------------------------
def test_tensors_and_views(gpu_device):
    import torch
    rk = _rk()
    rng = np.random.default_rng(20261218)
    Z = raster(rng, (90, 140), np.float64)
    Z[5, 7] = np.nan
    Zt = torch.from_numpy(Z).to(gpu_device)
    keep = Zt.clone()
    fp = footprints()["rand4x7"]
    calls = {"median_filter": (), "rank_filter": (3,), "percentile_filter": (75,), "minimum_filter": (), "maximum_filter": ()}
    for name, lead in calls.items():
        f = lambda A: getattr(rk, name)(A, *lead, footprint=fp, mode="nearest")                # noqa: E731
        t, n = f(Zt), f(Z)
        assert isinstance(t, torch.Tensor) and t.device == Zt.device and t.dtype == Zt.dtype and isinstance(n, np.ndarray)
        assert same_bits(t.cpu().numpy(), n), name
        assert f(Zt.float()).dtype == torch.float32
        # a transposed and an offset-strided view: the contiguous call's bits
        base = torch.from_numpy(np.ascontiguousarray(Z.T)).to(gpu_device)
        assert same_bits(f(base.T).cpu().numpy(), n), (name, "transposed")
        wide = torch.full((Z.shape[0] + 3, 2 * Z.shape[1] + 5), -1.0, dtype=torch.float64, device=gpu_device)
        view = wide[2:2 + Z.shape[0], 3:3 + 2 * Z.shape[1]:2]
        view.copy_(Zt)
        assert not view.is_contiguous() and same_bits(f(view).cpu().numpy(), n), (name, "strided")
    assert torch.equal(Zt.view(torch.int64), keep.view(torch.int64))           # the input is unchanged
    # integer rasters are widened to float64; an empty raster comes back empty
    Zi = np.round(Z[:, 10:] * 3).astype(np.int32)
    assert_same(rk.median_filter(Zi, footprint=fp), ndi.median_filter(Zi.astype(np.float64), footprint=fp), "int raster")
    for name, lead in calls.items():
        for shape in ((0, 5), (4, 0)):
            e = getattr(rk, name)(np.zeros(shape, np.float32), *lead, size=3)
            assert e.shape == shape and e.dtype == np.float32
        e = getattr(rk, name)(torch.zeros((0, 0), dtype=torch.float64, device=gpu_device), *lead, size=3)
        assert isinstance(e, torch.Tensor) and e.shape == (0, 0) and e.dtype == torch.float64


# ------------------------------------------------------------------------------------------
# guarded memory and a side stream, on cases built here
# ------------------------------------------------------------------------------------------
def harness_cases(dtype):
    """one median and one percentile case: the 2 % NaN raster of the case table's shape, the even, holed rand4x7"""
    from family_cases import NAN_SHAPE, raster as table_raster
    rk = _rk()
    fp = footprints()["rand4x7"]
    Z = table_raster(NAN_SHAPE, dtype, nan=True, seed=7)
    assert np.isnan(Z).any()
    yield dict(name="median_filter", fn=lambda Zt: rk.median_filter(Zt, footprint=fp), inputs=[Z], ctx=("median", np.dtype(dtype).name),
               reference=lambda got: assert_same(got, rkn.median_filter(Z, fp), "median"))
    yield dict(name="percentile_filter", fn=lambda Zt: rk.percentile_filter(Zt, 33.3, footprint=fp, mode="nearest", impl=BISECT),
               inputs=[Z], ctx=("percentile", np.dtype(dtype).name),
               reference=lambda got: assert_same(got, rkn.percentile_filter(Z, 33.3, fp, "nearest"), "percentile"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_guarded_memory(gpu_device, dtype):
    from test_gpu_guarded import run_guarded
    for case in harness_cases(dtype):
        run_guarded(**case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_a_side_stream(gpu_device, dtype):
    """the launch carries the current stream: the handle of smrf_rank_filter_* is recorded beside the shared header's"""
    import streamed as S
    from test_gpu_streams import streamed
    slots = dict(S.stream_slots(), **S.stream_slots(open(os.path.join(ROOT, "include", "smrf_rank.h")).read()))
    assert slots["smrf_rank_filter_f32"] == slots["smrf_rank_filter_f64"] == 10
    for case in harness_cases(dtype):
        streamed(case["fn"], case["inputs"], name=case["name"], ctx=case["ctx"], reference=case["reference"], slots=slots)
