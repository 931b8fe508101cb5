"""Rank filters without a GPU (neilpy_amd/rank.py, csrc/rank.hip, csrc/float_key.h): the NumPy
restatement tests/rank_numpy.py against scipy.ndimage, the NaN rule and the one recorded deviation from SciPy, the rank
resolution, the signatures, the argument refusals, the host logic behind the C ABI of include/smrf_rank.h, and the key
transform and the two selections compiled with g++.  Every comparison is by value, NaN equal to NaN, no tolerance."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.ndimage as ndi

import footprint_numpy as fpn
import rank_numpy as rkn
from conftest import ROOT

DTYPES = [np.float32, np.float64]
MODES = ["reflect", "nearest"]
PERCENTILES = (0, 10, 33.3, 50, 75, 99.9, 100, -20)
NAMES = ("median_filter", "rank_filter", "percentile_filter", "minimum_filter", "maximum_filter")
E_ARG, E_UNSUPPORTED = -1, -5


def assert_same(got, want, ctx):
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), (ctx, got, want)


def random_footprint(rng):
    kh, kw = int(rng.integers(1, 7)), int(rng.integers(1, 7))
    fp = rng.random((kh, kw)) < 0.6
    fp[rng.integers(kh), rng.integers(kw)] = True
    return fp


def random_raster(rng, shape, dtype, kind):
    X = rng.normal(size=shape) * 8
    if kind == "ties":
        X = np.round(X)
    X = X.astype(dtype)
    if kind == "inf":
        X[rng.random(shape) < 0.15] = np.inf
        X[rng.random(shape) < 0.15] = -np.inf
    return X


# ------------------------------------------------------------------------------------------
# the restatement against SciPy
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_restatement_equals_scipy(dtype, mode):
    """rows and cols 1..11, random footprints up to 6 x 6 (even, non-square, larger than the raster where SciPy can serve),
    plain, tied and +-inf values, ranks {0, n // 2, n - 1, random}, the median and the percentiles"""
    rng = np.random.default_rng(20261201 + (dtype is np.float64) + 2 * (mode == "nearest"))
    compared = 0
    for rows in range(1, 12):
        for cols in range(1, 12):
            kind = ("plain", "ties", "inf")[(rows + cols) % 3]
            X = random_raster(rng, (rows, cols), dtype, kind)
            fp = random_footprint(rng)
            if not fpn.scipy_comparable(fp, X.shape):
                continue
            n = int(fp.sum())
            for rank in sorted({0, n // 2, n - 1, int(rng.integers(n))}):
                assert_same(rkn.rank_filter(X, rank, fp, mode), ndi.rank_filter(X, rank, footprint=fp, mode=mode),
                            (X.shape, fp.shape, rank))
                compared += 1
            assert_same(rkn.rank_filter(X, -1, fp, mode), ndi.rank_filter(X, -1, footprint=fp, mode=mode), "rank -1")
            assert_same(rkn.median_filter(X, fp, mode), ndi.median_filter(X, footprint=fp, mode=mode), (X.shape, fp.shape))
            p = PERCENTILES[(rows * 11 + cols) % len(PERCENTILES)]
            assert_same(rkn.percentile_filter(X, p, fp, mode), ndi.percentile_filter(X, p, footprint=fp, mode=mode),
                        (X.shape, fp.shape, p))
            compared += 3
    assert compared >= 500, compared                     # four parametrisations: at least 2000 comparisons in all


@pytest.mark.parametrize("dtype", DTYPES)
def test_percentiles_and_footprints_larger_than_the_raster(dtype):
    rng = np.random.default_rng(20261205)
    for shape, fshape in (((3, 4), (5, 6)), ((2, 7), (6, 3)), ((4, 4), (6, 6)), ((9, 10), (4, 5))):
        X = random_raster(rng, shape, dtype, "ties")
        fp = rng.random(fshape) < 0.7
        fp[0, 0] = fp[-1, -1] = True
        assert fpn.scipy_comparable(fp, shape)
        for mode in MODES:
            for p in PERCENTILES:
                assert_same(rkn.percentile_filter(X, p, fp, mode), ndi.percentile_filter(X, p, footprint=fp, mode=mode),
                            (shape, fshape, mode, p))


@pytest.mark.parametrize("dtype", DTYPES)
def test_minimum_and_maximum_equal_scipys(dtype):
    """size= (SciPy's separable filters) and holed footprints, rasters without NaN"""
    rng = np.random.default_rng(20261206)
    holed = np.array([[1, 0, 1, 1], [0, 1, 0, 0], [1, 1, 0, 1]], dtype=bool)
    for shape in ((1, 1), (5, 9), (11, 4)):
        X = random_raster(rng, shape, dtype, "inf" if shape == (5, 9) else "plain")
        for mode in MODES:
            for size in (1, 3, (2, 5), (4, 1)):
                fp = np.ones((size, size) if isinstance(size, int) else size, dtype=bool)
                assert_same(rkn.minimum_filter(X, fp, mode), ndi.minimum_filter(X, size=size, mode=mode), (shape, size))
                assert_same(rkn.maximum_filter(X, fp, mode), ndi.maximum_filter(X, size=size, mode=mode), (shape, size))
            assert_same(rkn.minimum_filter(X, holed, mode), ndi.minimum_filter(X, footprint=holed, mode=mode), shape)
            assert_same(rkn.maximum_filter(X, holed, mode), ndi.maximum_filter(X, footprint=holed, mode=mode), shape)


# ------------------------------------------------------------------------------------------
# NaN
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rule_is_the_masked_count(dtype):
    """np.sort puts NaN last: a cell is NaN iff fewer than rank + 1 of its samples are not NaN, of either sign of NaN"""
    rng = np.random.default_rng(20261207)
    for shape in ((3, 4), (6, 7)):
        X = random_raster(rng, shape, dtype, "ties")
        X[rng.random(shape) < 0.3] = np.nan
        X[rng.random(shape) < 0.1] = -np.nan
        X.flat[0] = np.copysign(np.nan, -1)
        for _ in range(4):
            fp = random_footprint(rng)
            n = int(fp.sum())
            for rank in sorted({0, n // 2, n - 1}):
                for mode in MODES:
                    assert_same(rkn.rank_filter(X, rank, fp, mode), rkn.masked_count_rule(X, rank, fp, mode), (shape, rank))


# a 3 x 4 raster with one NaN under a holed footprint: SciPy's selection compares with `<`, so where the NaN lands
# depends on its visiting order
NAN_X = np.array([[5., 1., 7., 3.], [2., np.nan, 6., 0.], [9., 4., 8., 10.]])
NAN_FP = np.array([[1, 1, 0], [1, 1, 1], [0, 1, 1]], dtype=bool)


def test_scipy_differs_with_nan_present():
    """the stated deviation, on record: SciPy's values with a NaN among the samples are not np.sort's at some rank"""
    n = int(NAN_FP.sum())
    differs = []
    for rank in range(n):
        want = rkn.rank_filter(NAN_X, rank, NAN_FP)
        assert_same(want, rkn.masked_count_rule(NAN_X, rank, NAN_FP), rank)
        with np.errstate(invalid="ignore"):
            got = ndi.rank_filter(NAN_X, rank, footprint=NAN_FP)
        if not np.array_equal(got, want, equal_nan=True):
            differs.append(rank)
    if not differs:
        pytest.skip("this SciPy sorts NaN last, as this package does")
    print("scipy.ndimage.rank_filter differs from np.sort's order at ranks", differs)


# ------------------------------------------------------------------------------------------
# the rank
# ------------------------------------------------------------------------------------------
def _scipy_rank(n, op, value):
    """the rank SciPy uses, read off its result: a footprint of n members over a row of distinct ascending values"""
    X = np.arange(3 * n, dtype=np.float64).reshape(1, -1)
    fp = np.ones((1, n), dtype=bool)
    if op == "median":
        out = ndi.median_filter(X, footprint=fp, mode="nearest")
    elif op == "percentile":
        out = ndi.percentile_filter(X, value, footprint=fp, mode="nearest")
    else:
        out = ndi.rank_filter(X, value, footprint=fp, mode="nearest")
    j = n + n // 2                                           # far from the borders: samples j - n // 2 .. ascending
    return int(out[0, j]) - (j - n // 2)


def test_resolve_is_scipys():
    from neilpy_amd import rank as rk
    for n in list(range(1, 40)) + [961]:
        assert rk.resolve("minimum", n) == 0 and rk.resolve("maximum", n) == n - 1
        assert rk.resolve("median", n) == rkn.resolve("median", n) == n // 2
        for p in PERCENTILES + (12.5, 66.7, -0.1, -100):
            assert rk.resolve("percentile", n, p) == rkn.resolve("percentile", n, p), (n, p)
        for r in (0, n // 2, n - 1, -1, -n):
            assert rk.resolve("rank", n, r) == rkn.resolve("rank", n, r) == r % n, (n, r)
    for n in (1, 2, 7, 10, 30):
        assert rk.resolve("median", n) == _scipy_rank(n, "median", None)
        for p in PERCENTILES:
            assert rk.resolve("percentile", n, p) == _scipy_rank(n, "percentile", p), (n, p)
        for r in (0, n - 1, -1, -n, n // 3):
            assert rk.resolve("rank", n, r) == _scipy_rank(n, "rank", r), (n, r)
    for f in (rk.resolve, rkn.resolve):
        for n, r in ((4, 4), (4, -5), (1, 1)):
            with pytest.raises(RuntimeError, match="rank not within filter footprint size"):
                f("rank", n, r)
        with pytest.raises(RuntimeError, match="invalid percentile"):
            f("percentile", 9, 100.5)
    with pytest.raises(RuntimeError, match="rank not within filter footprint size"):
        ndi.rank_filter(np.zeros((3, 3)), 4, size=2)


# ------------------------------------------------------------------------------------------
# the interface
# ------------------------------------------------------------------------------------------
def test_signatures_are_scipys_plus_keyword_only():
    from neilpy_amd import rank as rk
    for name in NAMES:
        want = list(inspect.signature(getattr(ndi, name)).parameters.values())
        got = list(inspect.signature(getattr(rk, name)).parameters.values())
        assert len(got) >= len(want), name
        for w, g in zip(want, got):
            assert (g.name, g.kind, g.default) == (w.name, w.kind, w.default), (name, g, w)
        extras = got[len(want):]
        assert [g.name for g in extras] == ["impl"] and all(g.kind is inspect.Parameter.KEYWORD_ONLY for g in extras), name
    import neilpy_amd
    assert not set(NAMES) & set(dir(neilpy_amd)), "the family is not re-exported from the package"


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_come_from_the_host(name):
    """every refusal is decided before the device is touched: it is the same with and without a GPU"""
    from neilpy_amd import morphology as mo, rank as rk
    lead = {"rank_filter": (1,), "percentile_filter": (50,)}.get(name, ())
    f = lambda X, *a, **k: getattr(rk, name)(X, *lead, *a, **k)            # noqa: E731
    X = np.zeros((4, 5), np.float32)
    with pytest.raises(RuntimeError, match="no footprint or filter size"):
        f(X)
    for bad in (dict(footprint=np.ones((2, 2, 2))), dict(footprint=np.ones(3)), dict(footprint=np.zeros((3, 3))),
                dict(size=0), dict(size=(1, 2, 3)), dict(size=3, impl=3), dict(size=3, impl=8 | 16), dict(size=3, impl=32)):
        with pytest.raises(ValueError):
            f(X, **bad)
    for mode in ("constant", "mirror", "wrap", "grid-wrap"):
        with pytest.raises(NotImplementedError):
            f(X, size=3, mode=mode)
    for bad in (dict(output=np.empty_like(X)), dict(origin=1), dict(origin=(0, -1)), dict(axes=(0,)), dict(axes=(0, 1)),
                dict(size=(1, mo.MAX_EXTENT + 1))):
        with pytest.raises(NotImplementedError):
            f(X, **{"size": 3, **bad})
    for Y in (np.zeros((2, 3, 4)), np.zeros(5)):
        with pytest.raises(NotImplementedError):
            f(Y, size=3)                                                   # not a 2-D raster
    with pytest.raises(RuntimeError, match="rank not within filter footprint size"):
        rk.rank_filter(X, 9, size=3)
    with pytest.raises(RuntimeError, match="rank not within filter footprint size"):
        rk.rank_filter(X, -10, footprint=np.ones((3, 3)))
    with pytest.raises(RuntimeError, match="invalid percentile"):
        rk.percentile_filter(X, 101, size=3)


def test_valid_call_without_a_gpu_raises():
    import torch
    import neilpy_amd
    from neilpy_amd import rank as rk
    if torch.cuda.is_available():
        return                                                 # tests/test_gpu_rank.py runs the valid calls
    for X, kw in ((np.zeros((4, 5), np.float32), dict(size=(2, 3), cval=7.0, origin=0)),
                  (np.zeros((4, 5)), dict(footprint=[[0, 1, 1]], mode="nearest"))):
        for name in ("median_filter", "minimum_filter", "maximum_filter"):
            with pytest.raises(neilpy_amd.SmrfHipError):
                getattr(rk, name)(X, **kw)
        with pytest.raises(neilpy_amd.SmrfHipError):
            rk.rank_filter(X, -1, **kw)
        with pytest.raises(neilpy_amd.SmrfHipError):
            rk.percentile_filter(X, 33.3, **kw)


# ------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    """every name include/smrf_rank.h declares is exported and bound in rank.py with the declaration's arity; nothing of
    it sits in the shared header or the shared signature table"""
    import streamed as S
    from neilpy_amd import _lib, rank as rk
    decl = S.declarations(open(os.path.join(ROOT, "include", "smrf_rank.h")).read())
    assert set(decl) == set(rk.SIGNATURES) == {"smrf_rank_" + n for n in (
        "tile_bytes", "count_max_taps", "path", "filter_f32", "filter_f64")}
    lib = rk._library()
    for name, params in decl.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(params) == len(rk.SIGNATURES[name][1]), name
    for name in ("smrf_rank_filter_f32", "smrf_rank_filter_f64"):
        assert decl[name][-1] == "stream" and rk.SIGNATURES[name][1][-1] is C.c_void_p
    assert not [n for n in _lib.SIGNATURES if "rank" in n] and not [n for n in S.declarations() if "rank" in n]
    text = open(os.path.join(ROOT, "include", "smrf_rank.h")).read()
    macro = lambda n: int(re.search(r"#define SMRF_RANK_%s (\d+)" % n, text).group(1))          # noqa: E731
    assert (rk.IMPL_AUTO, rk.IMPL_COUNT, rk.IMPL_BISECT, rk.IMPL_GLOBAL, rk.IMPL_TILE) == tuple(
        macro("IMPL_" + n) for n in ("AUTO", "COUNT", "BISECT", "GLOBAL", "TILE"))
    assert rk.FORCE_NAN_AWARE == 4 and not rk.FORCE_NAN_AWARE & (rk.IMPL_COUNT | rk.IMPL_BISECT | rk.IMPL_GLOBAL | rk.IMPL_TILE)
    assert (rk.PATH_COUNT, rk.PATH_BISECT, rk.PATH_TILE, rk.PATH_GLOBAL) == tuple(
        macro("PATH_" + n) for n in ("COUNT", "BISECT", "TILE", "GLOBAL"))
    assert rk.TILE_BYTES == macro("TILE_BYTES") == lib.smrf_rank_tile_bytes()
    assert rk.COUNT_BLOCK == macro("COUNT_BLOCK")
    for elem, sfx in ((4, "F32"), (8, "F64")):
        assert rk.COUNT_MAX_TAPS[elem] == macro("COUNT_MAX_TAPS_" + sfx) == lib.smrf_rank_count_max_taps(elem)
    assert lib.smrf_rank_count_max_taps(2) == E_ARG


def _head(fp):
    from neilpy_amd import morphology as mo
    return mo.plan(fp).head


def _path(head, elem, impl):
    from neilpy_amd import rank as rk
    return rk._library().smrf_rank_path(head.ctypes.data_as(C.c_void_p), elem, impl)


@pytest.mark.parametrize("elem", [4, 8])
def test_path_follows_the_cap_and_the_member_count(elem):
    from neilpy_amd import morphology as mo, rank as rk
    cap = rk._library().smrf_rank_tile_bytes()
    fits = lambda w: (mo.TY + w - 1) * (mo.TX + w - 1) * elem + 4 * w * w <= cap               # noqa: E731: keys and offsets
    w = 1
    while fits(w + 1):
        w += 1
    assert w == {4: 64, 8: 45}[elem]
    for method in (rk.IMPL_AUTO, rk.IMPL_COUNT, rk.IMPL_BISECT):
        want = rk.PATH_COUNT if method == rk.IMPL_COUNT else rk.PATH_BISECT
        assert _path(_head(mo.square(w)), elem, method) == want | rk.PATH_TILE
        assert _path(_head(mo.square(w)), elem, method | rk.IMPL_TILE) == want | rk.PATH_TILE
        assert _path(_head(mo.square(w)), elem, method | rk.IMPL_GLOBAL) == want | rk.PATH_GLOBAL
        assert _path(_head(mo.square(w + 1)), elem, method) == want | rk.PATH_GLOBAL
        assert _path(_head(mo.square(w + 1)), elem, method | rk.IMPL_TILE) == E_UNSUPPORTED
        assert b"LDS" in _lib().smrf_last_error()
    # a holed footprint's tile is its bounding box's
    b = w
    while (mo.TY + b - 1) * (mo.TX + b - 1) * elem + 4 * 2 <= cap:
        b += 1
    for side, source in ((b - 1, rk.PATH_TILE), (b, rk.PATH_GLOBAL)):
        wide = np.zeros((side, side), dtype=bool)
        wide[0, 0] = wide[-1, -1] = True
        assert _path(_head(wide), elem, rk.IMPL_AUTO) == rk.PATH_COUNT | source, side
    m = rk._library().smrf_rank_count_max_taps(elem)
    assert m == rk.COUNT_MAX_TAPS[elem] and 1 <= m <= w * w
    for n, want in ((1, rk.PATH_COUNT), (m, rk.PATH_COUNT), (m + 1, rk.PATH_BISECT), (4 * m, rk.PATH_BISECT)):
        assert _path(_head(np.ones((1, n))), elem, rk.IMPL_AUTO) == want | rk.PATH_TILE, n
        assert _path(_head(np.ones((1, n))), elem, rk.IMPL_COUNT) == rk.PATH_COUNT
        assert _path(_head(np.ones((1, n))), elem, rk.IMPL_BISECT | rk.IMPL_GLOBAL) == rk.PATH_BISECT | rk.PATH_GLOBAL


def _lib():
    from neilpy_amd import _lib as L
    return L.load()


def test_abi_argument_errors():
    """refusals by status code, before any launch and so without a GPU"""
    from neilpy_amd import morphology as mo, rank as rk
    lib = rk._library()
    p, null = C.c_void_p(4096), C.c_void_p(0)                        # never dereferenced: every call is refused first
    head = _head(np.ones((3, 3)))
    h = head.ctypes.data_as(C.c_void_p)
    for f in (lib.smrf_rank_filter_f32, lib.smrf_rank_filter_f64):
        assert f(p, p, -1, 5, p, h, 0, 0, 0, 0, null) == E_ARG
        assert f(p, p, 5, 5, p, null, 0, 0, 0, 0, null) == E_ARG                  # no plan head
        assert f(p, p, 5, 5, p, h, 0, 2, 0, 0, null) == E_ARG                     # unknown mode
        for impl in (3, 4, 8 | 16, 32, -1):
            assert f(p, p, 5, 5, p, h, 0, 0, 0, impl, null) == E_ARG, impl        # unknown impl
        assert f(p, p, 5, 5, p, h, 9, 0, 0, 0, null) == E_ARG                     # rank out of range
        assert f(p, p, 5, 5, p, h, -1, 0, 0, 0, null) == E_ARG
        assert f(p, p, 0, 5, p, h, 9, 0, 0, 0, null) == E_ARG                     # also on an empty raster
        assert f(null, p, 5, 5, p, h, 4, 0, 0, 0, null) == E_ARG
        assert f(p, null, 5, 5, p, h, 4, 0, 0, 0, null) == E_ARG
        assert f(p, p, 5, 5, null, h, 4, 0, 0, 0, null) == E_ARG
        assert f(p, p, (1 << 30) + 1, 5, p, h, 4, 0, 0, 0, null) == E_UNSUPPORTED
        big = _head(np.ones((90, 90))).ctypes.data_as(C.c_void_p)
        assert f(p, p, 5, 5, p, big, 4, 0, 0, rk.IMPL_TILE, null) == E_UNSUPPORTED
        assert f(p, p, 0, 5, p, h, 8, 1, 1, rk.IMPL_COUNT | rk.IMPL_GLOBAL, null) == 0     # an empty raster: nothing launched
        for k, v in ((0, 0), (0, 10), (2, -(1 << 20) - 1), (3, (1 << 20) + 1), (4, 0), (5, (1 << 20) + 1)):
            bad = head.copy()
            bad[k] = v
            assert f(p, p, 5, 5, p, bad.ctypes.data_as(C.c_void_p), 0, 0, 0, 0, null) == E_ARG, (k, v)
            assert _path(bad, 4, 0) == E_ARG, (k, v)
    assert _path(head, 2, 0) == E_ARG and lib.smrf_rank_path(null, 4, 0) == E_ARG
    assert mo.MAX_EXTENT == 1 << 20


def test_kernels_compile_without_scratch(tmp_path):
    """csrc/rank.hip for gfx950: dtype x border mode x sample source x selection, every kernel in registers"""
    import family_checks as fc
    text, kernels = fc.device_asm("rank", tmp_path)
    assert len(kernels) == 16 and all("rank_kernel" in k for k in kernels)
    fc.assert_no_scratch(text, kernels)


# ------------------------------------------------------------------------------------------
# csrc/float_key.h on the CPU
# ------------------------------------------------------------------------------------------
_KEY_CPP = r'''
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "float_key.h"

template <typename T>
static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

template <typename T>
static long check_keys() {
  using K = typename SmrfKey<T>::type;
  using L = std::numeric_limits<T>;
  const T nan = L::quiet_NaN();
  // ascending, every neighbour pair strictly so (as keys): NaN of negative sign first without nan_last
  std::vector<T> v = {-L::infinity(), -L::max(), T(-2.5), T(-1), -L::min(), -L::denorm_min(), T(-0.0), T(0.0), L::denorm_min(),
                      L::min(), T(1), T(1) + L::epsilon(), T(2.5), L::max(), L::infinity()};
  long wrong = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    for (int nl = 0; nl < 2; ++nl) {
      wrong += !same_bits(smrf_unkey<T>(smrf_key<T>(v[i], nl)), v[i]);
      if (i) wrong += !(smrf_key<T>(v[i - 1], nl) < smrf_key<T>(v[i], nl));
    }
    wrong += smrf_key<T>(v[i], false) != smrf_key<T>(v[i], true);
  }
  const T pnan = std::copysign(nan, T(1)), nnan = std::copysign(nan, T(-1));
  wrong += !(smrf_key<T>(nnan, false) < smrf_key<T>(v.front(), false));      // without nan_last the sign decides
  wrong += !(smrf_key<T>(pnan, false) > smrf_key<T>(v.back(), false));
  wrong += !same_bits(smrf_unkey<T>(smrf_key<T>(pnan, false)), pnan) + !same_bits(smrf_unkey<T>(smrf_key<T>(nnan, false)), nnan);
  for (T x : {pnan, nnan}) {
    wrong += smrf_key<T>(x, true) != ~(K)0;
    wrong += !(smrf_key<T>(x, true) > smrf_key<T>(v.back(), true));
    wrong += !std::isnan(smrf_unkey<T>(smrf_key<T>(x, true)));
  }
  return wrong;
}

template <typename T, int BLOCK>
static long check_select(unsigned seed) {
  using K = typename SmrfKey<T>::type;
  std::mt19937 gen(seed);
  long wrong = 0;
  for (int trial = 0; trial < 1500; ++trial) {
    const int n = 1 + gen() % (trial % 10 == 0 ? 70 : 20);
    const int kind = trial % 4;
    std::vector<T> v(n);
    for (T& x : v) {
      const double u = (double)(gen() % 2001) / 1000.0 - 1.0;
      x = kind == 0 ? (T)(u * 100) : kind == 1 ? (T)std::round(u * 3) : kind == 2 ? (T)(1000.0 + u * 1e-3) : (T)(u * 1e30);
      if (kind == 1 && gen() % 7 == 0) x = gen() % 2 ? L_inf<T>() : -L_inf<T>();
      if (kind == 1 && gen() % 9 == 0) x = gen() % 2 ? T(0.0) : T(-0.0);
    }
    if (trial % 25 == 0) std::fill(v.begin(), v.end(), v[0]);
    std::vector<K> keys(n);
    for (int i = 0; i < n; ++i) keys[i] = smrf_key<T>(v[i], trial % 2);
    auto at = [&](int j) { return keys[j]; };
    for (int rank = 0; rank < n; ++rank) {
      std::vector<T> s = v;
      std::nth_element(s.begin(), s.begin() + rank, s.end());
      const T b = smrf_unkey<T>(smrf_select_bisect<K>(n, rank, at));
      const T c = smrf_unkey<T>(smrf_select_count<K, BLOCK>(n, rank, at, [](bool f) { return f; }));
      const T d = smrf_unkey<T>(smrf_select_count<K, BLOCK>(n, rank, at, [](bool) { return false; }));
      wrong += !(b == s[rank]) + !same_bits(b, c) + !same_bits(c, d);
    }
  }
  return wrong;
}

int main() {
  std::printf("%ld %ld %ld %ld %ld %ld\n", check_keys<float>(), check_keys<double>(), check_select<float, 8>(1),
              check_select<double, 8>(2), check_select<float, 3>(3), check_select<double, 1>(4));
  return 0;
}
'''


def test_float_key_header_on_the_cpu(tmp_path):
    """csrc/float_key.h compiled with g++: the key's round trip and strict monotonicity over sorted float32 and float64
    lists with +-0, +-inf, denormals and NaN of both signs; BISECT and COUNT (the kernel's text, at the kernel's block of
    8 and at blocks of 3 and 1) against std::nth_element on NaN-free lists with ties, +-inf and +-0, at every rank"""
    src = tmp_path / "key.cpp"
    src.write_text(_KEY_CPP.replace("L_inf<T>()", "std::numeric_limits<T>::infinity()"))
    exe = tmp_path / "key"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "neilpy_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0"] * 6, out
