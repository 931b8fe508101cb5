"""Focal statistics on the MI355X: goldens of the reference through the public functions, seeded random cases against
the NumPy restatement (tests/focal_numpy.py) with the tiled and the direct kernel path forced, tensor handling, a
larger raster and run-to-run identity.

Outputs built from + - * / and sqrt only are bit-exact: focal_convolve, std, unstandardised TPI and reduce_peaks with
blend_rate 2.  Standardised TPI is within K + 2 ulps of the restatement whose sums are exactly rounded (math.fsum),
K = ceil(log2(rows * cols)) + 16 (tests/test_focal_host.py shows the reference within K of the same): the device sums
in float64 in a fixed tree order.  reduce_peaks with another power goes through pow (the device's is not glibc's) and is
within ULPS = 8 of the golden.  NaN and inf positions are identical and no cell is exempt."""
import json

import numpy as np
import pytest

import focal_numpy as fn
from conftest import golden

pytestmark = pytest.mark.gpu

ULPS = 8          # tests/family_checks.py's
AUTO, TILED, DIRECT = 0, 1, 2


def _na():
    import neilpy_amd
    return neilpy_amd


def assert_bits(got, want, ctx):
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), \
        (ctx, int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want))))))


def assert_ulps(got, want, ulps, ctx):
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), ctx
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), ctx
    fin = np.isfinite(want)
    if fin.any():
        tol = ulps * np.spacing(np.abs(want[fin])).astype(np.float64)
        err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
        worst = float(np.max(err / tol))
        print(ctx, "worst error / tolerance: %.3f" % worst)
        assert np.all(err <= tol), (ctx, worst)


def check_tpi(X, got, kw, ctx):
    if kw.get("standardize", True):
        assert_ulps(got, fn.topographic_position_index(X, **kw), fn.tpi_ulps(X.shape) + 2, ctx)
    else:
        assert_bits(got, fn.topographic_position_index(X, **kw), ctx)


def test_goldens(gpu_device):
    na = _na()
    G = golden("focal.npz")
    cs = json.loads(str(G["cases"]))
    for c in cs:
        X = G["in_" + c["input"]]
        want = G["out_" + c["id"]]
        ctx = (c["id"], c["fn"], c["input"], c["kernel"], c["kw"])
        if c["fn"] == "convolve":
            assert_bits(na.focal_convolve(X, G["k_" + c["kernel"]]), want, ctx)
        elif c["fn"] == "std":
            assert_bits(na.std(X, G["k_" + c["kernel"]]), want, ctx)
        elif c["fn"] == "topographic_position_index":
            got = na.topographic_position_index(X, **c["kw"])
            if c["kw"].get("standardize", True):
                check_tpi(X, got, c["kw"], ctx)
            else:
                assert_bits(got, want, ctx)
        else:
            got = na.reduce_peaks(X, **c["kw"])
            if fn.exact_kind(c["fn"], c["kw"]):
                assert_bits(got, want, ctx)
            else:
                assert_ulps(got, want, ULPS, ctx)
    assert len(cs) > 100


SHAPES = ((1, 1), (1, 70), (70, 1), (67, 131), (9, 200), (5, 6))     # (5, 6): smaller than the 7 x 7 kernel's halo reach
KERNELS = ((3, 3), (7, 7), (1, 9), (9, 1), (2, 2), (6, 4))


def _raster(rng, shape, dtype, nan=False):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    Z = np.sin(x / 7.0) * 9 + np.cos(y / 5.0) * 6 + rng.normal(size=shape) * 2 + 50
    if nan:
        Z[rng.random(shape) < 0.02] = np.nan
    return Z.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_random_kernels_both_paths(gpu_device, dtype):
    na = _na()
    rng = np.random.default_rng(20261021)
    for shape in SHAPES:
        for k, kshape in enumerate(KERNELS):
            X = _raster(rng, shape, dtype, nan=(k % 3 == 0 and shape[0] * shape[1] > 100))
            w = rng.normal(size=kshape)
            if w.size > 4:
                w[rng.random(kshape) < 0.2] = 0.0
            want = fn.convolve(X, w)
            for impl in (AUTO, TILED, DIRECT):
                assert_bits(na.focal_convolve(X, w, impl=impl), want, ("convolve", shape, kshape, impl))
            pos = np.abs(w) + (w != 0) * 0.1
            want = fn.std(X, pos)
            for impl in (TILED, DIRECT):
                assert_bits(na.std(X, pos, impl=impl), want, ("std", shape, kshape, impl))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_disk_at_the_tile_cap_and_past_it(gpu_device, dtype):
    """the largest disk whose halo the tile holds, and the next: automatic, tiled (past the cap: the part of the halo
    that fits, the other taps from global memory) and direct give the restatement's bits"""
    na = _na()
    from neilpy_amd import _lib
    lib = _lib.load()
    elem = np.dtype(dtype).itemsize
    r = 1
    while lib.smrf_focal_fits_tile(2 * r + 3, 2 * r + 3, elem):
        r += 1
    assert lib.smrf_focal_fits_tile(2 * r + 1, 2 * r + 1, elem) and not lib.smrf_focal_fits_tile(2 * r + 3, 2 * r + 3, elem)
    rng = np.random.default_rng(20261022)
    X = _raster(rng, (67, 131), dtype)
    for radius in (r, r + 1):
        strel = fn.disk(radius)
        want = fn.std(X, strel)
        for impl in (AUTO, TILED, DIRECT):
            assert_bits(na.std(X, strel, impl=impl), want, ("std disk", radius, impl))
    w = fn.tpi_weights(r + 1)
    assert_bits(na.focal_convolve(X, w, impl=TILED), fn.convolve(X, w), ("convolve disk", r + 1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tpi_and_reduce_peaks_random(gpu_device, dtype):
    na = _na()
    rng = np.random.default_rng(20261023)
    for shape, radius in (((67, 131), 1), ((67, 131), 4), ((9, 200), 2), ((1, 70), 3), ((70, 1), 2), ((1, 1), 1),
                          ((3, 4), 5)):
        X = _raster(rng, shape, dtype)
        for st in (True, False):
            kw = dict(radius=radius, standardize=st)
            a = na.topographic_position_index(X, impl=TILED, **kw)
            b = na.topographic_position_index(X, impl=DIRECT, **kw)
            assert_bits(a, b, ("tpi tiled / direct", shape, kw))
            assert_bits(na.topographic_position_index(X, **kw), a, ("tpi auto", shape, kw))
            check_tpi(X, a, kw, ("tpi", shape, kw))
    for shape, radius, nan in (((67, 131), 3, False), ((40, 70), 6, True), ((1, 70), 2, False), ((5, 6), 4, False)):
        Z = _raster(rng, shape, dtype, nan=nan)
        want = fn.reduce_peaks(Z, radius)
        for impl in (AUTO, TILED, DIRECT):
            assert_bits(na.reduce_peaks(Z, radius, impl=impl), want, ("reduce_peaks", shape, radius, impl))
        assert_bits(na.reduce_peaks(Z, radius, blend_rate=1, kernel_rate=1.3),
                    fn.reduce_peaks(Z, radius, blend_rate=1, kernel_rate=1.3), ("reduce_peaks b1", shape))
        assert_ulps(na.reduce_peaks(Z, radius, blend_rate=2.5), fn.reduce_peaks(Z, radius, blend_rate=2.5), ULPS,
                    ("reduce_peaks b2.5", shape))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sum_and_sum_of_squares_from_one_read(gpu_device, dtype):
    """the SUM_SQ mode of the C entry point: conv(X) and conv(X*X), the square rounded in the raster's dtype"""
    import torch
    from neilpy_amd import _lib, focal
    rng = np.random.default_rng(20261024)
    X = _raster(rng, (67, 131), dtype, nan=True)
    w = rng.normal(size=(5, 4))
    Xd = torch.from_numpy(X).to(gpu_device)
    for impl in (TILED, DIRECT):
        a, b = torch.empty_like(Xd), torch.empty_like(Xd)
        focal._launch(Xd, _lib.FOCAL_SUM_SQ, w, [a, b], impl=impl)
        assert_bits(a.cpu().numpy(), fn.convolve(X, w), ("sum", impl))
        assert_bits(b.cpu().numpy(), fn.convolve(X * X, w), ("sum of squares", impl))


def test_tensors_and_layouts(gpu_device):
    import torch
    na = _na()
    rng = np.random.default_rng(7)
    Z = _raster(rng, (70, 90), np.float64)
    Z[5, 7] = np.nan
    Zt = torch.from_numpy(Z).to(gpu_device)
    w = rng.normal(size=(3, 5))
    calls = {"focal_convolve": lambda A: na.focal_convolve(A, w), "std": lambda A: na.std(A, fn.disk(2)),
             "tpi": lambda A: na.topographic_position_index(A, 2), "tpi_raw": lambda A: na.topographic_position_index(A, 2, False),
             "reduce_peaks": lambda A: na.reduce_peaks(A, 3)}
    for name, f in calls.items():
        t, n = f(Zt), f(Z)
        assert isinstance(t, torch.Tensor) and t.device == Zt.device and isinstance(n, np.ndarray), name
        assert_bits(t.cpu().numpy(), n, name)
        # a transposed tensor and a strided view: the bits of their contiguous copies
        assert_bits(f(Zt.t()).cpu().numpy(), f(np.ascontiguousarray(Z.T)), name + " transposed")
        assert_bits(f(Zt[::2, 3::3]).cpu().numpy(), f(np.ascontiguousarray(Z[::2, 3::3])), name + " strided")
        assert_bits(f(Z[::2, 3::3]), f(np.ascontiguousarray(Z[::2, 3::3])), name + " strided numpy")
    Z32 = Zt.float()
    assert na.focal_convolve(Z32, w).dtype == torch.float32 and na.topographic_position_index(Z32).dtype == torch.float32
    assert na.std(Z32, fn.disk(1)).dtype == torch.float64 and na.reduce_peaks(Z32, 2).dtype == torch.float64
    # integer rasters are widened to float64
    Zi = np.round(Z[:, 10:] * 3).astype(np.int32)
    assert_bits(na.std(Zi, fn.disk(2)), na.std(Zi.astype(np.float64), fn.disk(2)), "int raster")
    for f in calls.values():
        e = f(np.zeros((0, 5)))
        assert e.shape == (0, 5) and e.dtype == np.float64
    assert na.focal_convolve(np.zeros((0, 5), np.float32), w).dtype == np.float32


def test_large_raster_std(gpu_device):
    """1500 x 1100 float32 with disk(10): crops (corners, edges, interior) against the restatement; a crop carries the
    kernel's reach of cells around it wherever the raster goes on, and the raster's own edge where it ends"""
    import torch
    na = _na()
    rows, cols, R = 1500, 1100, 10
    gen = torch.Generator(device=gpu_device).manual_seed(13)
    y = torch.arange(rows, device=gpu_device, dtype=torch.float32)[:, None]
    x = torch.arange(cols, device=gpu_device, dtype=torch.float32)[None, :]
    Zt = (torch.sin(x / 37.0) * 9 + torch.cos(y / 53.0) * 7 + 200 +
          torch.rand((rows, cols), device=gpu_device, generator=gen, dtype=torch.float32) * 0.5)
    strel = fn.disk(R)
    got = na.std(Zt, strel)
    assert got.dtype == torch.float64 and got.device == Zt.device
    for r0, c0 in ((0, 0), (700, 500), (rows - 60, 300), (401, cols - 60), (rows - 60, cols - 60), (0, 1000)):
        h0, h1, w0, w1 = max(r0 - R, 0), min(r0 + 60 + R, rows), max(c0 - R, 0), min(c0 + 60 + R, cols)
        want = fn.std(Zt[h0:h1, w0:w1].cpu().numpy(), strel)
        sl = (slice(R if h0 > 0 else 0, (h1 - h0) - (R if h1 < rows else 0)),
              slice(R if w0 > 0 else 0, (w1 - w0) - (R if w1 < cols else 0)))
        assert_bits(got[h0:h1, w0:w1].cpu().numpy()[sl], want[sl], ("large", r0, c0))


def test_tpi_is_bit_identical_from_run_to_run(gpu_device):
    na = _na()
    rng = np.random.default_rng(9)
    for dtype in (np.float32, np.float64):
        X = _raster(rng, (300, 517), dtype)
        a = na.topographic_position_index(X, 3)
        b = na.topographic_position_index(X, 3)
        assert_bits(a, b, ("run to run", dtype))
        assert np.isfinite(a).all()


def test_tpi_radius_raises_before_any_launch(gpu_device):
    na = _na()
    with pytest.raises(ValueError):
        na.topographic_position_index(np.zeros((4, 4)), 0)
    with pytest.raises(ValueError):
        na.topographic_position_index("not a raster", 0)      # the radius is looked at first
