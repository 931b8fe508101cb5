"""Terrain functions on the MI355X: goldens of the reference, seeded random cases against the NumPy restatement
(tests/terrain_numpy.py), tiled / direct identity, tensor handling, a large raster and the device-resident route
from smrf().  The device arctan / sin are not glibc's, so floats are compared within 1e-12 and the threshold
decisions on every cell whose margin to the threshold is at least 1e-9 degrees.  An O_i that is 0 from identical
arctan arguments (a flat with threshold 0: the terraced golden) is exact on both sides and does not shrink the margin."""
import json

import numpy as np
import pytest

import terrain_numpy as tn
from conftest import golden, load_sample

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
TIGHT = 1e-12
DECISIONS = ("count_openness", "geomorphons", "ternary_pattern_from_openness")


def _na():
    import neilpy_amd
    return neilpy_amd


def call(fn, Z, kw, **extra):
    kw = dict(kw)
    if "neighbors" in kw:
        kw["neighbors"] = np.array(kw["neighbors"])
    f = getattr(_na(), fn)
    if fn == "count_openness":
        return f(Z, kw.pop("cellsize"), kw.pop("lookup_pixels"), kw.pop("threshold_angle"), **kw, **extra)
    return f(Z, **kw, **extra)


def decision_margin(fn, Z, kw):
    """per-cell margin of the decisions from the restatement (enhance: both marches)"""
    kw = dict(kw)
    thr = kw.get("threshold_angle", 1 if fn == "geomorphons" else 0)
    cs = kw.get("cellsize", 1)
    L = kw.get("lookup_pixels", 1)
    steps = tn.steps_of(L, kw.get("fast", False), kw.get("how_fast", 20))
    O, exact = tn.openness_differences(Z, cs, steps, kw.get("use_negative_openness", True), with_exact=True)
    m = tn.margin(O, thr, exact)
    if fn == "geomorphons" and kw.get("enhance") and L > 16:
        O, exact = tn.openness_differences(Z, cs, tn.steps_of(max(L // 4, 4)), with_exact=True)
        m = np.minimum(m, tn.margin(O, thr, exact))
    return m


def assert_close(got, want, ctx):
    assert got.dtype == np.float64 and got.shape == want.shape, ctx
    assert np.array_equal(np.isnan(got), np.isnan(want)), ctx
    assert np.array_equal(np.isinf(got), np.isinf(want)), ctx
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), ctx
    if fin.any():
        err = np.max(np.abs(got[fin] - want[fin]))
        assert err <= TIGHT, (ctx, err)


def assert_decisions(got, want, margin, ctx):
    assert got.dtype == want.dtype and got.shape == want.shape, ctx
    ok = margin >= MARGIN
    assert np.array_equal(got[ok], want[ok]), (ctx, int(np.sum(got[ok] != want[ok])))
    return int(np.sum(~ok))


def compare(fn, Z, kw, got, want):
    if fn in ("openness", "skyview_factor"):
        assert_close(got, want, (fn, kw))
        return 0
    m = decision_margin(fn, Z, kw)
    if fn == "count_openness":
        return assert_decisions(got[0], want[0], m, (fn, kw)) + assert_decisions(got[1], want[1], m, (fn, kw))
    return assert_decisions(got, want, m, (fn, kw))


def test_goldens(gpu_device):
    G = golden("terrain.npz")
    exempt = {}
    for c in json.loads(str(G["cases"])):
        Z = G["in_" + c["input"]]
        got = call(c["fn"], Z, c["kw"])
        want = (G["out_%s_pos" % c["id"]], G["out_%s_neg" % c["id"]]) if c["fn"] == "count_openness" \
            else G["out_" + c["id"]]
        n = compare(c["fn"], Z, c["kw"], got, want)
        if n:
            exempt[c["id"]] = n
    print("golden cells exempt by margin:", exempt or "none")
    assert not exempt, exempt                      # the goldens have no cell within 1e-9 degrees of a threshold


def _random_case(rng):
    fn = rng.choice(["openness", "skyview_factor", "count_openness", "geomorphons", "ternary_pattern_from_openness"])
    shape = tuple(int(v) for v in np.exp(rng.uniform(0, np.log(300), size=2)).astype(int).clip(1, 300))
    dtype = rng.choice([np.float32, np.float64])
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    Z = (np.sin(x / rng.uniform(3, 30)) * rng.uniform(1, 20) + np.cos(y / rng.uniform(3, 30)) * rng.uniform(1, 20) +
         rng.normal(size=shape) * rng.uniform(0, 2))
    if rng.random() < 0.3:
        Z = np.round(Z)
    if rng.random() < 0.3:
        Z[rng.random(shape) < rng.uniform(0, 0.3)] = np.nan
    Z = Z.astype(dtype)
    L = int(rng.integers(0, 41))
    kw = dict(cellsize=float(rng.choice([1, 0.5, 2.0, rng.uniform(0.1, 5)])), lookup_pixels=L)
    if fn in ("openness", "count_openness", "geomorphons") and rng.random() < 0.4:
        kw["fast"] = True
        kw["how_fast"] = int(rng.choice([10, 20, 35]))
    if fn == "openness" and rng.random() < 0.5:
        kw["neighbors"] = [int(v) for v in rng.integers(0, 8, size=int(rng.integers(1, 10)))]
    if fn in DECISIONS:
        kw["threshold_angle"] = float(rng.choice([0, 0.5, 1, 3, rng.uniform(0, 5)]))
    if fn == "geomorphons" and rng.random() < 0.5:
        kw["enhance"] = True
    if fn == "ternary_pattern_from_openness":
        kw["use_negative_openness"] = bool(rng.random() < 0.7)
        kw["lowest"] = bool(rng.random() < 0.5)
    return fn, Z, kw


def test_random_cases_against_the_restatement(gpu_device):
    rng = np.random.default_rng(4242)
    exempt = 0
    for i in range(200):
        fn, Z, kw = _random_case(rng)
        impl = int(rng.choice([1, 2]))
        got = call(fn, Z, kw, impl=impl)
        want = tn.run(fn, Z, kw)
        exempt += compare(fn, Z, kw, got, want)
    print("random cells exempt by margin:", exempt)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiled_and_direct_give_the_same_bits(gpu_device, dtype):
    from neilpy_amd import _lib
    cap = _lib.TERRAIN_HALO_CAP["f32" if dtype == np.float32 else "f64"]
    rng = np.random.default_rng(7)
    Z = (np.cumsum(rng.normal(size=(203, 331)), axis=1) + rng.normal(size=(203, 331))).astype(dtype)
    Z[rng.random(Z.shape) < 0.02] = np.nan
    for L in (1, cap - 1, cap, cap + 1, cap + 9):
        for fn, kw in (("openness", dict(lookup_pixels=L)), ("skyview_factor", dict(lookup_pixels=L)),
                       ("geomorphons", dict(lookup_pixels=L, threshold_angle=1, enhance=True)),
                       ("geomorphons", dict(lookup_pixels=L, threshold_angle=1, enhance=True, fast=True)),
                       ("ternary_pattern_from_openness", dict(lookup_pixels=L, threshold_angle=1, lowest=True))):
            a = call(fn, Z, kw, impl=1)
            b = call(fn, Z, kw, impl=2)
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (fn, L)
    with pytest.raises(ValueError):
        _na().openness(Z, impl=7)


def test_tensors_and_layouts(gpu_device):
    import torch
    na = _na()
    rng = np.random.default_rng(3)
    Z = rng.normal(size=(70, 90)).cumsum(axis=0)
    Zt = torch.from_numpy(Z).to(gpu_device)
    for fn, kw in (("openness", dict(lookup_pixels=4)), ("skyview_factor", dict(lookup_pixels=4)),
                   ("geomorphons", dict(lookup_pixels=4)), ("ternary_pattern_from_openness", dict(lookup_pixels=4))):
        t = call(fn, Zt, kw)
        n = call(fn, Z, kw)
        assert isinstance(t, torch.Tensor) and t.device == Zt.device, fn
        assert isinstance(n, np.ndarray), fn
        assert np.array_equal(t.cpu().numpy(), n, equal_nan=True), fn
        # non-contiguous input: same answer as its contiguous copy
        nc = call(fn, Zt.t(), kw)
        assert np.array_equal(nc.cpu().numpy(), call(fn, np.ascontiguousarray(Z.T), kw), equal_nan=True), fn
    p, q = na.count_openness(Zt, 1, 4, 1)
    assert p.dtype == torch.uint8 and p.device == Zt.device and q.device == Zt.device
    codes = na.ternary_pattern_from_openness(Zt, 1, 4, 1, lowest=True)
    g = na.terrain_code_to_geomorphon(codes, 'loose')
    assert g.device == Zt.device and g.dtype == torch.uint8
    # integer rasters are widened to float64
    Zi = np.round(Z * 3).astype(np.int32)
    assert np.array_equal(na.openness(Zi, 1, 3), na.openness(Zi.astype(np.float64), 1, 3))
    e = na.openness(np.zeros((0, 5)), 1, 3)
    assert e.shape == (0, 5) and e.dtype == np.float64


def test_large_raster(gpu_device):
    """8192^2 float32 geomorphons(L = 20, enhance) against the restatement on four crops (interior cells), twice"""
    import torch
    na = _na()
    n, L = 8192, 20
    gen = torch.Generator(device=gpu_device).manual_seed(11)
    y = torch.arange(n, device=gpu_device, dtype=torch.float32)[:, None]
    x = torch.arange(n, device=gpu_device, dtype=torch.float32)[None, :]
    Zt = (torch.sin(x / 37.0) * 9 + torch.cos(y / 53.0) * 7 + torch.sin((x + y) / 11.0) * 2 +
          torch.rand((n, n), device=gpu_device, generator=gen) * 0.5)
    a = na.geomorphons(Zt, 1, L, 1, True)
    b = na.geomorphons(Zt, 1, L, 1, True)
    assert torch.equal(a, b)
    exempt = 0
    for r0, c0 in ((0, 0), (4000, 5000), (8192 - 120, 300), (777, 8192 - 120)):
        r1, c1 = min(r0 + 120, n), min(c0 + 120, n)
        h0, h1, w0, w1 = max(r0 - L, 0), min(r1 + L, n), max(c0 - L, 0), min(c1 + L, n)
        crop = Zt[h0:h1, w0:w1].cpu().numpy()
        want, m = tn.geomorphons(crop, 1, L, 1, True, return_margin=True)
        got = a[h0:h1, w0:w1].cpu().numpy()
        R, C = np.indices(crop.shape)
        gr, gc = R + h0, C + w0
        # cells whose rays stay inside the crop (or leave the raster itself, where both sides use the edge rule)
        inner = (((gr - h0 >= L) | (gr < L)) & ((h1 - 1 - gr >= L) | (gr >= n - L)) &
                 ((gc - w0 >= L) | (gc < L)) & ((w1 - 1 - gc >= L) | (gc >= n - L)))
        inner &= (gr >= r0) & (gr < r1) & (gc >= c0) & (gc < c1)
        exempt += assert_decisions(got[inner], want[inner], m[inner], (r0, c0))
    print("large raster cells exempt by margin:", exempt)


def test_device_to_device_from_smrf(gpu_device):
    import torch
    na = _na()
    x, y, z, _ = load_sample("samp21")
    dtm, t, obj, pts = na.smrf(x, y, z, cellsize=1, windows=18)
    xt, yt, zt = (torch.from_numpy(np.ascontiguousarray(v)).to(gpu_device) for v in (x, y, z))
    dtm_t, _, _, _ = na.smrf(xt, yt, zt, cellsize=1, windows=18)
    assert isinstance(dtm_t, torch.Tensor) and dtm_t.is_cuda
    g_t = na.geomorphons(dtm_t, 1, 10, 1)
    assert isinstance(g_t, torch.Tensor) and g_t.device == dtm_t.device
    assert np.array_equal(g_t.cpu().numpy(), na.geomorphons(dtm, 1, 10, 1))


def test_geomorphons_consistency(gpu_device):
    """geomorphons == table[count_openness] == terrain_code_to_geomorphon(ternary(lowest=True), 'loose') (the
    reference's geomorphons2 identity)"""
    from neilpy_amd.terrain import GEOMORPHON_TABLE
    na = _na()
    G = golden("terrain.npz")
    for name in ("dtm11", "dtm41", "terrace", "nan"):
        Z = G["in_" + name]
        for L, thr in ((3, 1), (8, 0.5), (6, 0)):
            g = na.geomorphons(Z, 1, L, thr)
            p, q = na.count_openness(Z, 1, L, thr)
            assert np.array_equal(g, GEOMORPHON_TABLE[p, q]), (name, L)
            codes = na.ternary_pattern_from_openness(Z, 1, L, thr, lowest=True)
            assert np.array_equal(g, na.terrain_code_to_geomorphon(codes, 'loose')), (name, L)
