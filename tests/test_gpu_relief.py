"""Relief colouring and raster statistics on the MI355X: raster_stats against the NumPy restatement
(tests/relief_numpy.py: exact count, min, max and median; mean and sum of squares bit for bit against the replayed
summation order), the colour gather against the device's own hillshade on every cell, the reference's goldens, normalize
against np.interp bit for bit, brassel within ulps (float) or a rounding margin (uint8), tensor handling and the
device-resident route from smrf().

Margins.  A uint8 shade of the device can differ from the reference's where 255 * H lies within MARGIN / MARGIN_F32
(tests/test_gpu_surface.py) of a half-integer; the goldens were generated to hold no such cell.  brassel's uint8 output
goes through the device's pow: cells whose 255 * H_new in the restatement lies within 1e-9 of a half-integer are exempt
(none among the goldens, at most 1e-4 of the cells of a random case)."""
import json

import numpy as np
import pytest

import relief_numpy as rn
import surface_numpy as sn
from conftest import golden, load_sample
from family_checks import assert_close
from test_gpu_surface import MARGIN, MARGIN_F32

pytestmark = pytest.mark.gpu

BRASSEL_MARGIN = 1e-9


def _na():
    import neilpy_amd
    return neilpy_amd


@pytest.fixture(scope="module")
def G():
    return golden("relief.npz")


# ------------------------------------------------------------------------------------------
# raster_stats
# ------------------------------------------------------------------------------------------
def same_float_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and (a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)))


def check_stats(X, ctx):
    na = _na()
    got = na.raster_stats(X)
    want = rn.raster_stats(X)
    assert set(got) == set(want) == {'count', 'min', 'max', 'mean', 'median', 'sum_sq', 'has_nan'}, ctx
    assert got['count'] == want['count'] and isinstance(got['count'], int), (ctx, got, want)
    assert got['has_nan'] == want['has_nan'], ctx
    for k in ('min', 'max', 'median'):
        assert got[k].dtype == want[k].dtype == X.dtype, (ctx, k)
        assert np.array_equal(got[k], want[k], equal_nan=True), (ctx, k, got[k], want[k])
    for k in ('mean', 'sum_sq'):
        assert same_float_bits(got[k], want[k]), (ctx, k, got[k], want[k])
    if want['count']:
        with np.errstate(all='ignore'):
            assert np.array_equal(got['median'], np.nanmedian(X), equal_nan=True), ctx
    again = na.raster_stats(X)
    for k in ('mean', 'sum_sq', 'median', 'min', 'max'):
        assert same_float_bits(got[k], again[k]), (ctx, k)          # deterministic: the same bits on a second call


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_raster_stats_sizes(gpu_device, dtype):
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257):
        check_stats((rng.normal(size=(1, n)) * 100).astype(dtype), n)
    # 500 x 600 > 1024 x 256 cells: the grid-stride loop runs twice
    X = (rng.normal(size=(500, 600)) * 30 + 400).astype(dtype)
    check_stats(X, "500x600")
    X[rng.random(X.shape) < 0.3] = np.nan
    check_stats(X, "500x600, 30 % NaN")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_raster_stats_values(gpu_device, dtype):
    rng = np.random.default_rng(2)
    info = np.finfo(dtype)
    check_stats(np.full((7, 9), 3.25, dtype), "all equal")
    check_stats(np.full((7, 10), np.nan, dtype), "all NaN")
    Z = np.zeros((9, 11), dtype)
    Z[rng.random(Z.shape) < 0.5] = -0.0
    check_stats(Z, "+-0")
    got = _na().raster_stats(np.array([[-0.0, 0.0, -0.0, 0.0, 5.0]], dtype), ('median',))
    assert got['median'] == 0 and not got['has_nan']
    X = (rng.normal(size=(30, 31)) * 5).astype(dtype)
    X[3, 4], X[8, 9], X[10, 1] = np.inf, -np.inf, np.nan
    with np.errstate(all='ignore'):
        check_stats(X, "+-inf")
        check_stats(np.array([[np.inf, 1.0, 2.0, np.inf]], dtype), "inf in the middle")
        check_stats(np.array([[-np.inf, np.inf]], dtype), "inf - inf")
    # values that differ only in their lowest 8 mantissa bits: the last pass decides
    base = np.array([1234.5], dtype).view(np.uint32 if dtype == np.float32 else np.uint64)
    for n in (256, 255, 1000, 1001):
        low = rng.integers(0, 256, size=n).astype(base.dtype)
        check_stats(((base & ~base.dtype.type(255)) | low).view(dtype).reshape(1, n), ("low bits", n))
    # the two middle values in different buckets of the top digit (other signs, other exponents)
    for n in (2, 4, 100, 101, 1000, 1001):
        h = n // 2
        X = np.concatenate([-rng.uniform(1, 2, h) * 1e10, rng.uniform(1, 2, n - h) * 1e-10]).astype(dtype)
        check_stats(rng.permutation(X).reshape(1, n), ("split top digit", n))
        X = np.concatenate([rng.uniform(1, 2, h), rng.uniform(1, 2, n - h) * 4096]).astype(dtype)
        check_stats(rng.permutation(X).reshape(1, n), ("split exponent", n))
    check_stats(np.array([[info.max, info.max, -info.max, info.tiny]], dtype), "extremes")
    e = _na().raster_stats(np.zeros((0, 5), dtype))
    assert e['count'] == 0 and not e['has_nan'] and all(np.isnan(e[k]) for k in ('min', 'max', 'mean', 'median', 'sum_sq'))
    assert _na().raster_stats(X.reshape(1, -1), 'max') == {'max': X.max(), 'has_nan': False}


def test_rmse(gpu_device):
    import torch
    na = _na()
    rng = np.random.default_rng(4)
    for dtype in (np.float32, np.float64):
        X = (rng.normal(size=(40, 50)) * 3).astype(dtype)
        X[rng.random(X.shape) < 0.2] = np.nan
        got = na.rmse(X)
        assert isinstance(got, dtype) and got == rn.rmse(X)
        t = na.rmse(torch.from_numpy(X).to(gpu_device))
        assert isinstance(t, torch.Tensor) and t.dim() == 0 and t.device.type == "cuda" and t.item() == got
        assert na.rmse(np.full((3, 3), np.nan, dtype)) == 0
    assert np.isnan(na.rmse(np.zeros((0, 4))))


def test_rmse_goldens(gpu_device, G):
    from test_relief_host import rmse_tolerance
    for c in json.loads(str(G["cases"])):
        if c["fn"] == "rmse":
            Z, want = G["in_" + c["input"]], G["out_" + c["id"]]
            with np.errstate(all='ignore'):
                got = _na().rmse(Z)
            assert got.dtype == want.dtype
            assert got == want or abs(float(got) - float(want)) <= rmse_tolerance(Z) * abs(float(want)), (c, got, want)


# ------------------------------------------------------------------------------------------
# colortable_shade / swiss_shading
# ------------------------------------------------------------------------------------------
def _terrain(rng, shape, dtype):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    Z = np.sin(x / 7.0) * 9 + np.cos(y / 5.0) * 6 + rng.normal(size=shape)
    return (np.round(Z * 40) if np.issubdtype(dtype, np.integer) else Z * 40).astype(dtype)


def test_gather_against_the_devices_own_shade(gpu_device, G):
    """got == lut[zi, hillshade(Z, cellsize)] on EVERY cell: the shade is the device's own, zi is NumPy's"""
    na = _na()
    rng = np.random.default_rng(5)
    tabs = {"2d": G["lut_ghc"], "3ch": G["lut_swiss"], "4ch": G["lut_rand4"]}
    n = 0
    for shape in ((2, 2), (2, 5), (7, 2), (9, 65), (17, 130), (150, 301)):
        for dtype in (np.float32, np.float64, np.int32):
            for cs in (0.5, 2):
                Z = _terrain(rng, shape, dtype)
                name = ("2d", "3ch", "4ch")[n % 3]
                n += 1
                H = na.hillshade(Z, cs)
                want = rn.table3(tabs[name])[rn.table_index(Z), H]
                got = na.colortable_shade(Z, tabs[name], cs)
                assert got.dtype == np.uint8 and got.shape == shape + (3,)
                assert np.array_equal(got, want), (shape, dtype, cs, name, int((got != want).sum()))
                if name != "2d":
                    assert np.array_equal(na.swiss_shading(Z, cs, lut=tabs[name]), want)
    for Z in (np.full((9, 65), 2.5), np.full((5, 4), -1.0, np.float32)):
        got = na.colortable_shade(Z, tabs["4ch"])
        assert np.array_equal(got, rn.table3(tabs["4ch"])[np.zeros(Z.shape, int), na.hillshade(Z)])
    Z = _terrain(rng, (17, 130), np.float64)
    Z[3, 100] = np.nan
    got = na.colortable_shade(Z, tabs["3ch"], 2)
    assert np.array_equal(got, tabs["3ch"][np.zeros(Z.shape, int), na.hillshade(Z, 2)])
    # a table that is not uint8 is cast as NumPy assignment casts
    f = rng.uniform(0, 255.9, size=(256, 256, 3))
    assert np.array_equal(na.colortable_shade(Z, f), na.colortable_shade(Z, f.astype(np.uint8)))
    with pytest.raises(ValueError, match="numerical gradient"):      # as hillshade: an empty axis has no gradient
        na.colortable_shade(np.zeros((0, 5)), tabs["2d"])


def test_shading_goldens(gpu_device, G):
    na = _na()
    exempt = {}
    n = 0
    for c in json.loads(str(G["cases"])):
        if c["fn"] not in ("colortable_shade", "swiss_shading"):
            continue
        n += 1
        Z, kw = G["in_" + c["input"]], c["kw"]
        lut = G["lut_" + c["table"]]
        with np.errstate(all='ignore'):
            got = na.colortable_shade(Z, lut, **kw) if c["fn"] == "colortable_shade" else na.swiss_shading(Z, lut=lut, **kw)
            cs = kw.get("cellsize", 1)
            ok = sn.half_margin(sn.hillshade_value(Z, cs), sn.flat_cells(Z, cs)) >= \
                (MARGIN_F32 if Z.dtype == np.float32 else MARGIN)
        want = G["out_" + c["id"]]
        assert got.dtype == want.dtype and got.shape == want.shape, c
        assert np.array_equal(got[ok], want[ok]), (c, int((got[ok] != want[ok]).sum()))
        if not ok.all():
            exempt[c["id"]] = int((~ok).sum())
    assert n >= 60 and not exempt, exempt


# ------------------------------------------------------------------------------------------
# normalize
# ------------------------------------------------------------------------------------------
def test_normalize_is_np_interp(gpu_device):
    na = _na()
    rng = np.random.default_rng(6)
    for dtype in (np.float32, np.float64):
        X = (rng.normal(size=(37, 70)) * 20 + 100).astype(dtype)
        X[rng.random(X.shape) < 0.1] = np.nan
        X[0, 0], X[0, 1] = 90, 110                                  # cells equal to a numeric knot
        for xr, yr in ((['min', 'max'], [0, 1]), (['min', 'median', 'max'], [-1, 0, 1]),
                       (['min', 'mean', 'max'], [-1, 0, 1]), ([90, 110], [5, -5]), ([90, 100.5, 110, 130], [0, 3, 3, -1]),
                       (['min', 95, 'median', 'max'], [0, 1, 2, 3]), ([90, 90, 110], [0, 1, 2])):
            got, knots = na.normalize(X, xr, yr, return_knots=True)
            st = na.raster_stats(X)
            assert knots.dtype == np.float64
            assert np.array_equal(knots, [np.float64(st[k]) if isinstance(k, str) else float(k) for k in xr])
            want = np.interp(X, knots, yr)
            assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True), (dtype, xr)
            assert np.array_equal(na.normalize(X, xr, yr), got, equal_nan=True)
            assert np.isnan(got[np.isnan(X)]).all()
            if 'mean' not in xr:
                assert np.array_equal(got, rn.normalize(X, xr, yr), equal_nan=True)
        assert (X > 110).any() and (X < 90).any()                   # cells outside the numeric knots
        got = na.normalize(X)
        assert got[X == np.nanmin(X)][0] == 0 and got[X == np.nanmax(X)][0] == 1
    c = na.normalize(np.full((4, 5), 2.0))
    assert np.array_equal(c, np.interp(np.full((4, 5), 2.0), [2.0, 2.0], [0, 1]))
    assert na.normalize(np.zeros((0, 3))).shape == (0, 3)


def test_normalize_goldens(gpu_device, G):
    from test_relief_host import mean_knot_tolerance
    na = _na()
    n = 0
    for c in json.loads(str(G["cases"])):
        if c["fn"] != "normalize":
            continue
        n += 1
        Z, want = G["in_" + c["input"]], G["out_" + c["id"]]
        got, knots = na.normalize(Z, **c["kw"], return_knots=True)
        assert got.dtype == want.dtype and got.shape == want.shape
        if 'mean' in c["kw"].get("xrange", []):
            ok = ~np.isnan(want)
            assert np.array_equal(np.isnan(got), ~ok)
            assert np.all(np.abs(got[ok] - want[ok]) <= mean_knot_tolerance(Z, knots, c["kw"]["yrange"])), c
        else:
            assert np.array_equal(got, want, equal_nan=True), c
    assert n >= 50


# ------------------------------------------------------------------------------------------
# brassel
# ------------------------------------------------------------------------------------------
def check_brassel(H, Z, kw, want=None):
    """asserts; returns (cells exempt by the rounding margin, cells)"""
    got = _na().brassel_atmospheric_perspective(H, Z, **kw)
    with np.errstate(all='ignore'):
        v, was_int = rn.brassel_value(H, Z, **kw)
        want = rn.brassel_atmospheric_perspective(H, Z, **kw) if want is None else want
    assert got.dtype == want.dtype == (np.uint8 if was_int else np.float64) and got.shape == want.shape, kw
    if not was_int:
        assert_close(got, want, 1.0, (kw, Z.dtype, H.dtype))
        return 0, got.size
    with np.errstate(all='ignore'):
        v = 255 * v
        ok = ~(np.abs(v - (np.floor(v) + 0.5)) < BRASSEL_MARGIN)
    assert np.array_equal(got[ok], want[ok]), (kw, Z.dtype, int((got[ok] != want[ok]).sum()))
    return int((~ok).sum()), got.size


def test_brassel_goldens(gpu_device, G):
    n = 0
    for c in json.loads(str(G["cases"])):
        if c["fn"] == "brassel_atmospheric_perspective":
            n += 1
            exempt, _ = check_brassel(G[c["shade"] + "_" + c["input"]], G["in_" + c["input"]], c["kw"],
                                      G["out_" + c["id"]])
            assert exempt == 0, c
    assert n >= 90


def test_brassel_random_cases(gpu_device):
    rng = np.random.default_rng(8)
    exempt = cells = 0
    wraps = set()
    for shape in ((1, 1), (2, 3), (9, 65), (64, 257), (150, 301)):
        for zdt in (np.float32, np.float64):
            for hkind in ("u8", "f32", "f64", "f32_255"):
                Z = _terrain(rng, shape, zdt)
                if rng.random() < 0.5 and Z.size > 4:
                    Z[rng.random(shape) < 0.1] = np.nan
                h = rng.uniform(0, 1, size=shape)
                H = {"u8": np.round(255 * h).astype(np.uint8), "f32": h.astype(np.float32), "f64": h,
                     "f32_255": (255 * h).astype(np.float32)}[hkind]
                kw = dict(k=float(rng.choice([1, 1.371, 2.303, 5.7])))
                if rng.random() < 0.5:
                    kw["flat"] = float(rng.choice([0.6, 200, 1]))
                if rng.random() < 0.5 and Z.size > 6:
                    kw["Zmid"] = float(np.nanmean(Z) + rng.normal())
                if rng.random() < 0.5:
                    kw["reverse"] = True
                if rng.random() < 0.6:
                    kw["C2"] = float(rng.choice([0.41, -0.41, -0.9, 0.77]))
                    wraps.add(np.sign(kw["C2"]))
                e, n = check_brassel(H, Z, kw)
                exempt += e
                cells += n
    assert wraps == {1.0, -1.0}
    print("brassel random cells exempt by margin: %d of %d" % (exempt, cells))
    assert exempt <= 1e-4 * cells


# ------------------------------------------------------------------------------------------
# tensors, errors, the device route
# ------------------------------------------------------------------------------------------
def test_tensors_in_tensors_out(gpu_device, G):
    import torch
    na = _na()
    Z = G["in_nan"]
    H = G["h_nan"]
    lut = G["lut_rand4"]
    Zt, Ht, lt = (torch.from_numpy(v).to(gpu_device) for v in (Z, H, lut))
    keep = (Zt.clone(), Ht.clone(), lt.clone())
    pairs = [(na.colortable_shade(Zt, lt, 2), na.colortable_shade(Z, lut, 2)),
             (na.colortable_shade(Zt, lut), na.colortable_shade(Z, lut)),
             (na.swiss_shading(Zt, lut=lt), na.swiss_shading(Z, lut=lut)),
             (na.normalize(Zt, ['min', 'median', 'max'], [-1, 0, 1]), na.normalize(Z, ['min', 'median', 'max'], [-1, 0, 1])),
             (na.brassel_atmospheric_perspective(Ht, Zt, 2.303, C2=0.41), na.brassel_atmospheric_perspective(H, Z, 2.303, C2=0.41)),
             (na.brassel_atmospheric_perspective(torch.from_numpy(H / 255).to(gpu_device), Zt, 2.303),
              na.brassel_atmospheric_perspective(H / 255, Z, 2.303))]
    for t, n in pairs:
        assert isinstance(t, torch.Tensor) and t.device == Zt.device and isinstance(n, np.ndarray)
        assert np.array_equal(t.cpu().numpy(), n, equal_nan=n.dtype.kind == 'f')
    for a, b in zip(keep, (Zt, Ht, lt)):
        assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all()       # inputs unmodified
    assert torch.equal(torch.nan_to_num(keep[0], nan=-1.0), torch.nan_to_num(Zt, nan=-1.0))
    assert na.raster_stats(Zt) .keys() == na.raster_stats(Z).keys()
    st, sn_ = na.raster_stats(Zt), na.raster_stats(Z)
    assert all(np.array_equal(st[k], sn_[k], equal_nan=True) for k in st)
    # a transposed (non-contiguous) tensor: same answer as its contiguous copy
    assert np.array_equal(na.colortable_shade(Zt.t(), lt).cpu().numpy(), na.colortable_shade(np.ascontiguousarray(Z.T), lut))
    pieces = na.cutter(Zt[:, :24], 2, 3)
    assert pieces[1][2].data_ptr() == Zt[10:, 16:24].data_ptr() and pieces[1][2].shape == (10, 8)


def test_errors_raise_before_any_launch(gpu_device, G):
    import torch
    na = _na()
    Zt = torch.zeros((6, 6), device=gpu_device)
    lt = torch.zeros((256, 256, 3), dtype=torch.uint8, device=gpu_device)
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError):
        na.colortable_shade(Zt, 'swiss')
    with pytest.raises(ValueError, match="colour table"):
        na.colortable_shade(Zt, lt[:, :, :2])
    with pytest.raises(ValueError, match="numerical gradient"):
        na.colortable_shade(Zt[:1], lt)
    with pytest.raises(ValueError, match="greater than one"):
        na.brassel_atmospheric_perspective(Zt, Zt, 0.99)
    with pytest.raises(ValueError, match="shape"):
        na.brassel_atmospheric_perspective(Zt[:, :5], Zt, 2)
    with pytest.raises(ValueError, match="unknown knot"):
        na.normalize(Zt, ['min', 'mode'], [0, 1])
    with pytest.raises(TypeError):
        na.swiss_shading(Zt)                                         # the table is a required keyword


def test_device_route_from_smrf(gpu_device, G):
    """smrf() tensors -> hillshade -> brassel -> colortable_shade, no host array in between"""
    import torch
    na = _na()
    x, y, z, _ = load_sample("samp21")
    xt, yt, zt = (torch.from_numpy(np.ascontiguousarray(v)).to(gpu_device) for v in (x, y, z))
    dtm_t, _, _, _ = na.smrf(xt, yt, zt, cellsize=1, windows=18)
    h_t = na.hillshade(dtm_t)
    b_t = na.brassel_atmospheric_perspective(h_t, dtm_t, 2.303)
    lut_t = torch.from_numpy(G["lut_swiss"]).to(gpu_device)
    rgb_t = na.colortable_shade(dtm_t, lut_t)
    for t, dt in ((h_t, torch.uint8), (b_t, torch.uint8), (rgb_t, torch.uint8)):
        assert isinstance(t, torch.Tensor) and t.device == dtm_t.device and t.dtype == dt
    assert rgb_t.shape == dtm_t.shape + (3,) and b_t.shape == dtm_t.shape
    dtm = dtm_t.cpu().numpy()
    assert np.array_equal(rgb_t.cpu().numpy(), G["lut_swiss"][rn.table_index(dtm), h_t.cpu().numpy()])
    assert np.array_equal(b_t.cpu().numpy(), na.brassel_atmospheric_perspective(h_t.cpu().numpy(), dtm, 2.303))
