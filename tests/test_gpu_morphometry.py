"""scaled_morphometry, vip_score and ashift on the MI355X: goldens of the reference, seeded random cases against the
NumPy restatement (tests/morphometry_numpy.py), the outputs= subset, tensor handling, a larger raster and the
device-resident route from smrf().

Outputs built from + - * / and sqrt only are bit-exact: K, K_cross, K_long, K_tan, all of vip_score, and ashift.  S,
K_profile and K_plan go through atan or pow (the device's are not glibc's) and match within ULPS units in the last place
of the output dtype, with NaN and inf positions identical: the rule and the constant of tests/family_checks.py.  A
(atan2, then 270 - a, mod 360) matches within ULPS ulps of itself plus ULPS ulps of 360, on the circular difference
min(|d|, 360 - |d|): the wrap sits at atan2 = -90 degrees."""
import json

import numpy as np
import pytest

import morphometry_numpy as mn
from conftest import golden, load_sample
from family_checks import assert_close, assert_exact

pytestmark = pytest.mark.gpu

EXACT = ("K", "K_cross", "K_long", "K_tan")
CLOSE = ("S", "K_profile", "K_plan")


def _na():
    import neilpy_amd
    return neilpy_amd


def compare_morphometry(got, want, ctx):
    assert list(got) == list(want), ctx
    for k in got:
        if k in EXACT:
            assert_exact(got[k], want[k], ctx + (k,))
        elif k == "A":
            assert_close(got[k], want[k], 360.0, ctx + (k,), circular=360.0)
        else:
            assert k in CLOSE
            assert_close(got[k], want[k], 0.0, ctx + (k,))


def test_goldens(gpu_device):
    na = _na()
    G = golden("morphometry.npz")
    seen = set()
    for c in json.loads(str(G["cases"])):
        Z = G["in_" + c["input"]]
        before = Z.copy()
        ctx = (c["fn"], c["input"], tuple(sorted(c["kw"].items())))
        seen.add(c["fn"])
        if c["fn"] == "scaled_morphometry":
            want = {k: G["out_%s_%s" % (c["id"], k)] for k in mn.KEYS}
            compare_morphometry(na.scaled_morphometry(Z, **c["kw"]), want, ctx)
        elif c["fn"] == "vip_score":
            assert_exact(na.vip_score(Z, **c["kw"]), G["out_" + c["id"]], ctx)
        else:
            assert_exact(na.ashift(Z, **c["kw"]), G["out_" + c["id"]], ctx)
        assert np.array_equal(Z, before, equal_nan=True), ctx            # the input is untouched
    assert seen == {"scaled_morphometry", "vip_score", "ashift"}


def _random_raster(rng, shape, dtype):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    Z = (np.sin(x / rng.uniform(3, 30)) * rng.uniform(1, 20) + np.cos(y / rng.uniform(3, 30)) * rng.uniform(1, 20) +
         rng.normal(size=shape) * rng.uniform(0, 2))
    if rng.random() < 0.3:
        Z = np.round(Z)                                  # exact flats
    if rng.random() < 0.6:
        p = rng.uniform(0, 0.1)
        Z[rng.random(shape) < p] = np.nan
        Z[rng.random(shape) < p / 3] = np.inf
        Z[rng.random(shape) < p / 3] = -np.inf
    return Z.astype(dtype)


def test_random_cases_against_the_restatement(gpu_device):
    """rows and cols from 1..150 with the lane and workgroup edges 63, 64, 65 and 129 columns; strides below, at and
    above a wave's width and above the raster; both dtypes; NaN and +-inf cells"""
    na = _na()
    rng = np.random.default_rng(20261018)
    strides = (1, 2, 7, 63, 64, 65, 149, 150, 300)
    forced_cols = (63, 64, 65, 129, 1, 150)
    dtypes = set()
    for i in range(72):
        rows = int(rng.integers(1, 151))
        cols = forced_cols[i % 12] if i % 12 < len(forced_cols) else int(rng.integers(1, 151))
        n = strides[i % len(strides)]
        dtype = (np.float32, np.float64)[(i // len(strides)) % 2]
        dtypes.add(dtype)
        Z = _random_raster(rng, (rows, cols), dtype)
        cs = float(rng.choice([1, 0.5, 2.5, rng.uniform(0.1, 5)]))
        ctx = (i, rows, cols, n, np.dtype(dtype).name, cs)
        compare_morphometry(na.scaled_morphometry(Z, cs, n), mn.scaled_morphometry(Z, cs, n), ctx)
        assert_exact(na.vip_score(Z, cs), mn.vip_score(Z, cs), ctx)
        d = int(rng.integers(0, 10))
        assert_exact(na.ashift(Z, d, n), mn.ashift(Z, d, n), ctx + (d,))
    assert len(dtypes) == 2


def test_outputs_subset(gpu_device):
    na = _na()
    G = golden("morphometry.npz")
    for name, n in (("dtm21_f32", 2), ("nan", 5)):
        Z = G["in_" + name]
        full = na.scaled_morphometry(Z, 0.5, n)
        assert list(full) == list(mn.KEYS)
        for names, wrap in ((["K"], tuple), (["K_plan", "A"], tuple), (["S", "K_tan", "K_cross"], list),
                            (["K_long", "K_profile"], iter), (list(mn.KEYS[::-1]), set), (["K_cross"], lambda v: v[0])):
            got = na.scaled_morphometry(Z, 0.5, n, outputs=wrap(names))
            assert list(got) == [k for k in mn.KEYS if k in names], names
            for k in got:
                assert_exact(got[k], full[k], (name, n, tuple(names), k))
        assert na.scaled_morphometry(Z, 0.5, n, outputs=()) == {}
    with pytest.raises(ValueError):
        na.scaled_morphometry(G["in_nan"], outputs=("K", "nope"))


def test_tensors_and_layouts(gpu_device):
    import torch
    na = _na()
    rng = np.random.default_rng(3)
    Z = rng.normal(size=(70, 90)).cumsum(axis=0)
    Z[5, 7] = np.nan
    Zt = torch.from_numpy(Z).to(gpu_device)
    calls = (lambda z: na.scaled_morphometry(z, 2.0, 3), lambda z: {"vip": na.vip_score(z, 2.0)},
             lambda z: {"shift": na.ashift(z, 6, 4)})
    for f in calls:
        t, h = f(Zt), f(Z)
        assert list(t) == list(h)
        for k in t:
            assert isinstance(t[k], torch.Tensor) and t[k].device == Zt.device, k
            assert isinstance(h[k], np.ndarray), k
            assert np.array_equal(t[k].cpu().numpy(), h[k], equal_nan=True), k
        # a transposed tensor and a strided NumPy view: the same bits as their contiguous copies
        nc, cc = f(Zt.t()), f(np.ascontiguousarray(Z.T))
        sv, sc = f(Z[::2, 1::3]), f(np.ascontiguousarray(Z[::2, 1::3]))
        for k in nc:
            assert np.array_equal(nc[k].cpu().numpy(), cc[k], equal_nan=True), k
            assert np.array_equal(sv[k], sc[k], equal_nan=True), k
    assert np.array_equal(Zt.cpu().numpy(), Z, equal_nan=True)
    t32 = Zt.float()
    assert all(v.dtype == torch.float32 for v in na.scaled_morphometry(t32).values())
    assert na.vip_score(t32).dtype == torch.float64 and na.ashift(t32, 0).dtype == torch.float32
    # integer rasters are widened to float64
    Zi = np.round(Z[:, 10:] * 3).astype(np.int32)
    for f in calls:
        a, b = f(Zi), f(Zi.astype(np.float64))
        for k in a:
            assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k], equal_nan=True), k
    # empty rasters: empty results
    for shape in ((0, 5), (4, 0)):
        e = na.scaled_morphometry(np.zeros(shape, np.float32), outputs=("K", "A"))
        assert list(e) == ["A", "K"] and all(v.shape == shape and v.dtype == np.float32 for v in e.values())
        assert na.vip_score(np.zeros(shape, np.float32)).shape == shape
        assert na.vip_score(np.zeros(shape, np.float32)).dtype == np.float64
        assert na.ashift(np.zeros(shape), 2, 3).shape == shape
    # NumPy-scalar parameters: the float32 contract whatever the scalar type
    Z32 = golden("morphometry.npz")["in_dtm21_f32"]
    a, b = na.scaled_morphometry(Z32, np.float64(0.5), np.int64(2)), na.scaled_morphometry(Z32, 0.5, 2)
    assert all(a[k].dtype == np.float32 and np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    assert np.array_equal(na.vip_score(Z32, np.float32(2.5)), na.vip_score(Z32, float(np.float32(2.5))))


@pytest.mark.parametrize("n", [1, 17])
def test_larger_raster(gpu_device, n):
    """1500 x 2100 float32: 40 x 40 windows, the four corners included, against the restatement run on each window
    grown by n cells where the raster goes on (the grown rim is dropped again)"""
    import torch
    na = _na()
    R, C, W = 1500, 2100, 40
    gen = torch.Generator(device=gpu_device).manual_seed(11)
    y = torch.arange(R, device=gpu_device, dtype=torch.float32)[:, None]
    x = torch.arange(C, device=gpu_device, dtype=torch.float32)[None, :]
    Zt = (torch.sin(x / 37.0) * 9 + torch.cos(y / 53.0) * 7 + torch.sin((x + y) / 11.0) * 2 +
          torch.rand((R, C), device=gpu_device, generator=gen, dtype=torch.float32) * 0.5)
    got = na.scaled_morphometry(Zt, 2.0, n)
    vip = na.vip_score(Zt, 2.0)
    sh = na.ashift(Zt, 4, n)
    for r0, c0 in ((0, 0), (0, C - W), (R - W, 0), (R - W, C - W), (700, 1000), (63, 1985)):
        def grown(m):
            h0, h1, w0, w1 = max(r0 - m, 0), min(r0 + W + m, R), max(c0 - m, 0), min(c0 + W + m, C)
            return (h0, h1, w0, w1), (slice(r0 - h0, r0 - h0 + W), slice(c0 - w0, c0 - w0 + W))
        (h0, h1, w0, w1), inner = grown(n)
        crop = Zt[h0:h1, w0:w1].cpu().numpy()
        want = {k: v[inner] for k, v in mn.scaled_morphometry(crop, 2.0, n).items()}
        win = {k: v[r0:r0 + W, c0:c0 + W].cpu().numpy() for k, v in got.items()}
        compare_morphometry(win, want, (n, r0, c0))
        assert_exact(sh[r0:r0 + W, c0:c0 + W].cpu().numpy(), mn.ashift(crop, 4, n)[inner], (n, r0, c0, "ashift"))
        (h0, h1, w0, w1), inner = grown(1)
        crop = Zt[h0:h1, w0:w1].cpu().numpy()
        assert_exact(vip[r0:r0 + W, c0:c0 + W].cpu().numpy(), mn.vip_score(crop, 2.0)[inner], (n, r0, c0, "vip"))


def test_device_route_from_smrf(gpu_device):
    import torch
    na = _na()
    x, y, z, _ = load_sample("samp11")
    dtm, _, _, _ = na.smrf(x, y, z, cellsize=1, windows=18)
    xt, yt, zt = (torch.from_numpy(np.ascontiguousarray(v)).to(gpu_device) for v in (x, y, z))
    dtm_t, _, _, _ = na.smrf(xt, yt, zt, cellsize=1, windows=18)
    assert isinstance(dtm_t, torch.Tensor) and dtm_t.is_cuda
    v_t = na.vip_score(dtm_t)
    assert isinstance(v_t, torch.Tensor) and v_t.device == dtm_t.device and v_t.dtype == torch.float64
    assert np.array_equal(v_t.cpu().numpy(), na.vip_score(dtm), equal_nan=True)
    m_t, m_n = na.scaled_morphometry(dtm_t, 1, 5), na.scaled_morphometry(dtm, 1, 5)
    assert list(m_t) == list(mn.KEYS) == list(m_n)
    for k in m_t:
        assert isinstance(m_t[k], torch.Tensor) and m_t[k].device == dtm_t.device
        assert np.array_equal(m_t[k].cpu().numpy(), m_n[k], equal_nan=True), k
