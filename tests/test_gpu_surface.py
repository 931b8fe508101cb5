"""Surface derivatives on the MI355X: goldens of the reference, seeded random cases against the NumPy restatement
(tests/surface_numpy.py), tensor handling, a large raster and the device-resident route from smrf().

Outputs built from + - * / and sqrt only are bit-exact.  Outputs that go through atan, atan2, cos, sin or pow (the
device's are not glibc's) match within ULPS units in the last place of the output dtype, plus the same number of
ulps of the output's natural scale where the reference subtracts (aspect: pi/2 - atan2; hillshade: the illumination
sum), with NaN and inf positions identical.  uint8 shades are equal on every cell whose pre-rounding value 255 * H in
the restatement lies at least MARGIN (float64 raster) or MARGIN_F32 (float32 raster) from a half-integer."""
import json

import numpy as np
import pytest

import surface_numpy as sn
from conftest import golden, load_sample
from family_checks import assert_close

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
MARGIN_F32 = 1e-4

# per function: output index -> "exact" or the absolute scale of the ulp tolerance (0: relative only)
EXACT, REL = "exact", 0.0


def kinds(fn, kw):
    ra = kw.get("return_as", "degrees")
    if fn == "slope":
        return [EXACT if ra == "percent" else REL]
    if fn == "aspect":
        return [360.0 if ra == "degrees" else 2 * np.pi]
    if fn == "hillshade":
        return ["uint8" if kw.get("return_uint8", True) else 1.0]
    if fn == "multiple_illumination":
        return ["uint8"]
    if fn == "esri_slope":
        return [REL if ra == "degrees" else EXACT]
    if fn == "curvature":
        return [EXACT]
    if fn == "esri_curvature":
        return [EXACT] * 3
    if fn in ("zevenbergen_and_thorne_curvature", "evans_curvature"):
        return [EXACT, REL, REL, EXACT, EXACT, EXACT]
    return [EXACT, REL, REL, EXACT]      # wilson_gallant_curvature: K and Kt exact, Kp and Kc through pow


def _na():
    import neilpy_amd
    return neilpy_amd


def call(fn, Z, kw):
    return getattr(_na(), fn)(Z, **sn.decode_kw(kw))


def margin_of(fn, Z, kw):
    kw = sn.decode_kw(kw)
    if fn == "hillshade":
        kw = {k: v for k, v in kw.items() if k != "return_uint8"}
        return sn.half_margin(sn.hillshade_value(Z, **kw),
                              sn.flat_cells(Z, kw.get("cellsize", 1), kw.get("z_factor", 1)))
    return sn.multiple_illumination(Z, **kw, return_margin=True)[1]


def compare(fn, Z, kw, got, want):
    """asserts; returns the number of uint8 cells exempt by margin"""
    got = got if fn in sn.N_OUT else (got,)
    want = want if fn in sn.N_OUT else (want,)
    assert len(got) == len(want), fn
    exempt = 0
    for k, (g, w, kind) in enumerate(zip(got, want, kinds(fn, kw))):
        ctx = (fn, kw, Z.shape, Z.dtype, k)
        if kind == EXACT:
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True), \
                (ctx, int(np.sum(~((g == w) | (np.isnan(g) & np.isnan(w))))))
        elif kind == "uint8":
            assert g.dtype == w.dtype == np.uint8 and g.shape == w.shape, ctx
            ok = margin_of(fn, Z, kw) >= (MARGIN_F32 if Z.dtype == np.float32 else MARGIN)
            assert np.array_equal(g[ok], w[ok]), (ctx, int(np.sum(g[ok] != w[ok])))
            exempt += int(np.sum(~ok))
        else:
            assert_close(g, w, kind, ctx, Z.dtype if fn == "hillshade" else None)
    return exempt


def test_goldens(gpu_device):
    G = golden("surface.npz")
    exempt = {}
    for c in json.loads(str(G["cases"])):
        Z = G["in_" + c["input"]]
        got = call(c["fn"], Z, c["kw"])
        want = tuple(G["out_%s_%d" % (c["id"], k)] for k in range(sn.N_OUT[c["fn"]])) if c["fn"] in sn.N_OUT \
            else G["out_" + c["id"]]
        n = compare(c["fn"], Z, c["kw"], got, want)
        if n:
            exempt[c["id"]] = n
    print("golden cells exempt by margin:", exempt or "none")
    assert not exempt, exempt


GRADIENT = ("slope", "aspect", "hillshade", "multiple_illumination")


def _random_case(rng):
    fn = str(rng.choice(list(sn.FUNCS)))
    lo = 2 if fn in GRADIENT else 1
    hi = 120 if fn == "multiple_illumination" else 300
    shape = tuple(int(v) for v in np.exp(rng.uniform(0, np.log(hi), size=2)).astype(int).clip(lo, hi))
    dtype = rng.choice([np.float32, np.float64])
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    Z = (np.sin(x / rng.uniform(3, 30)) * rng.uniform(1, 20) + np.cos(y / rng.uniform(3, 30)) * rng.uniform(1, 20) +
         rng.normal(size=shape) * rng.uniform(0, 2))
    if rng.random() < 0.3:
        Z = np.round(Z)                                  # exact flats
    if rng.random() < 0.3:
        Z[rng.random(shape) < rng.uniform(0, 0.3)] = np.nan
    Z = Z.astype(dtype)
    kw = {}
    cs = float(rng.choice([1, 0.5, 2.0, rng.uniform(0.1, 5)]))
    zf = float(rng.choice([1, 3.0, rng.uniform(0.2, 4)]))
    if fn != "aspect":
        kw["cellsize"] = cs
    if fn in ("slope", "hillshade", "multiple_illumination", "esri_slope"):
        kw["z_factor"] = zf
    if fn == "slope":
        kw["return_as"] = str(rng.choice(["degrees", "radians", "percent"]))
    if fn == "esri_slope":
        kw["return_as"] = str(rng.choice(["degrees", "percent"]))
    if fn == "aspect":
        kw["return_as"] = str(rng.choice(["degrees", "radians"]))
        kw["flat_as"] = "nan" if rng.random() < 0.5 else float(rng.choice([0, -1, 361]))
    if fn == "hillshade":
        kw["zenith"] = float(rng.uniform(5, 85))
        kw["azimuth"] = float(rng.uniform(0, 360))
        kw["return_uint8"] = bool(rng.random() < 0.6)
    if fn == "multiple_illumination":
        kw["zeniths"] = int(rng.integers(0, 4)) if rng.random() < 0.5 else [float(v) for v in rng.uniform(5, 85, 2)]
        kw["azimuths"] = int(rng.integers(1, 9)) if rng.random() < 0.5 else [float(v) for v in rng.uniform(0, 360, 3)]
    return fn, Z, kw


def test_random_cases_against_the_restatement(gpu_device):
    rng = np.random.default_rng(20261016)
    exempt = 0
    seen = set()
    for i in range(200):
        fn, Z, kw = _random_case(rng)
        seen.add(fn)
        got = call(fn, Z, kw)
        want = sn.run(fn, Z, kw)
        exempt += compare(fn, Z, kw, got, want)
    assert seen == set(sn.FUNCS)
    print("random cells exempt by margin:", exempt)


def test_multiple_illumination_is_the_max_of_hillshades(gpu_device):
    na = _na()
    G = golden("surface.npz")
    for name in ("dtm11", "nan_f32", "terrace"):
        Z = G["in_" + name]
        for zs, az in ((np.array([45]), 4), (2, 6), (np.array([30.0, 60.0]), np.array([0, 90, 225]))):
            m = na.multiple_illumination(Z, 1.5, 2, zs, az)
            z2, a2 = sn.angle_lists(zs, az)
            want = np.zeros(Z.shape, np.uint8)
            for z in z2:
                for a in a2:
                    want = np.maximum(want, na.hillshade(Z, 1.5, 2, z, a))
            assert m.dtype == np.uint8 and np.array_equal(m, want), (name, zs, az)
    assert np.array_equal(na.multiple_illumination(G["in_dtm11"], zeniths=0, azimuths=3),
                          np.zeros(G["in_dtm11"].shape, np.uint8))


def test_numpy_scalar_parameters(gpu_device):
    """NumPy scalars are taken as Python floats: a float32 raster stays float32 with the float32 contract"""
    na = _na()
    Z = golden("surface.npz")["in_dtm21_f32"]
    a = na.slope(Z, np.float64(0.3), np.float64(1.0), 'percent')
    b = na.slope(Z, 0.3, 1.0, 'percent')
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert np.array_equal(na.curvature(Z, np.float32(0.3)), na.curvature(Z, float(np.float32(0.3))))


def test_tensors_and_layouts(gpu_device):
    import torch
    na = _na()
    rng = np.random.default_rng(3)
    Z = rng.normal(size=(70, 90)).cumsum(axis=0)
    Z[5, 7] = np.nan
    Zt = torch.from_numpy(Z).to(gpu_device)
    for fn in sn.FUNCS:
        t = call(fn, Zt, {})
        n = call(fn, Z, {})
        ts = t if fn in sn.N_OUT else (t,)
        ns = n if fn in sn.N_OUT else (n,)
        assert isinstance(t, tuple) == (fn in sn.N_OUT), fn
        for a, b in zip(ts, ns):
            assert isinstance(a, torch.Tensor) and a.device == Zt.device, fn
            assert isinstance(b, np.ndarray), fn
            assert np.array_equal(a.cpu().numpy(), b, equal_nan=True), fn
        # a transposed (non-contiguous) tensor: same answer as its contiguous copy
        nc = call(fn, Zt.t(), {})
        cc = call(fn, np.ascontiguousarray(Z.T), {})
        for a, b in zip(nc if fn in sn.N_OUT else (nc,), cc if fn in sn.N_OUT else (cc,)):
            assert np.array_equal(a.cpu().numpy(), b, equal_nan=True), fn
    s32 = na.slope(Zt.float())
    assert s32.dtype == torch.float32 and na.hillshade(Zt.float(), return_uint8=False).dtype == torch.float64
    # integer rasters are widened to float64
    Zi = np.round(Z[:, 10:] * 3).astype(np.int32)
    assert np.array_equal(na.curvature(Zi), na.curvature(Zi.astype(np.float64)))
    e = na.curvature(np.zeros((0, 5)))
    assert e.shape == (0, 5) and e.dtype == np.float64


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_large_raster(gpu_device, dtype):
    """8192^2: every function on the device, checked on four crops against the restatement (crop borders dropped)"""
    import torch
    na = _na()
    n = 8192
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    gen = torch.Generator(device=gpu_device).manual_seed(11)
    y = torch.arange(n, device=gpu_device, dtype=tdt)[:, None]
    x = torch.arange(n, device=gpu_device, dtype=tdt)[None, :]
    Zt = (torch.sin(x / 37.0) * 9 + torch.cos(y / 53.0) * 7 + torch.sin((x + y) / 11.0) * 2 +
          torch.rand((n, n), device=gpu_device, generator=gen, dtype=tdt) * 0.5)
    crops = ((0, 0), (4000, 5000), (n - 70, 300), (777, n - 70))
    exempt = 0
    for fn in sn.FUNCS:
        kw = {"cellsize": 2.0} if fn != "aspect" else {}
        got = call(fn, Zt, kw)
        got = got if fn in sn.N_OUT else (got,)
        for r0, c0 in crops:
            h0, h1, w0, w1 = max(r0 - 1, 0), min(r0 + 71, n), max(c0 - 1, 0), min(c0 + 71, n)
            crop = Zt[h0:h1, w0:w1].cpu().numpy()
            want = sn.run(fn, crop, kw)
            want = want if fn in sn.N_OUT else (want,)
            # inner cells: their 3 x 3 window lies in the crop, or the raster's own edge rule applies on both sides
            sl = (slice(1 if h0 > 0 else 0, (h1 - h0) - (1 if h1 < n else 0)),
                  slice(1 if w0 > 0 else 0, (w1 - w0) - (1 if w1 < n else 0)))
            g = tuple(t[h0:h1, w0:w1].cpu().numpy()[sl] for t in got)
            w = tuple(v[sl] for v in want)
            sub = crop[sl]
            if fn in ("hillshade", "multiple_illumination"):
                m = margin_of(fn, crop, kw)[sl]
                ok = m >= (MARGIN_F32 if dtype == np.float32 else MARGIN)
                assert np.array_equal(g[0][ok], w[0][ok]), (fn, r0, c0)
                exempt += int(np.sum(~ok))
            else:
                compare(fn, sub, kw, g if fn in sn.N_OUT else g[0], w if fn in sn.N_OUT else w[0])
    print("large raster cells exempt by margin:", exempt)


def test_device_route_from_smrf(gpu_device):
    import torch
    na = _na()
    x, y, z, _ = load_sample("samp21")
    dtm, t, obj, pts = na.smrf(x, y, z, cellsize=1, windows=18)
    xt, yt, zt = (torch.from_numpy(np.ascontiguousarray(v)).to(gpu_device) for v in (x, y, z))
    dtm_t, _, _, _ = na.smrf(xt, yt, zt, cellsize=1, windows=18)
    assert isinstance(dtm_t, torch.Tensor) and dtm_t.is_cuda
    h_t = na.hillshade(dtm_t)
    assert isinstance(h_t, torch.Tensor) and h_t.device == dtm_t.device and h_t.dtype == torch.uint8
    assert np.array_equal(h_t.cpu().numpy(), na.hillshade(dtm))
    k_t = na.zevenbergen_and_thorne_curvature(dtm_t)
    k_n = na.zevenbergen_and_thorne_curvature(dtm)
    for a, b in zip(k_t, k_n):
        assert isinstance(a, torch.Tensor) and a.device == dtm_t.device
        assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)
