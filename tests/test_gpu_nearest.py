"""Nearest-source infill on the MI355X: goldens, random cases against the brute-force restatement
(tests/nearest_numpy.py), the tie rule, large rasters against SciPy's exact transform, in-place and layout handling and
determinism.  Every comparison is on bits."""
import json
import time

import numpy as np
import pytest
from scipy import ndimage

import nearest_numpy as nn
from conftest import golden, load_sample

pytestmark = pytest.mark.gpu


def _na():
    import neilpy_amd
    return neilpy_amd


def check_against_restatement(X, tag):
    """fill, index planes and distances of one raster against the restatement, every cell, on bits"""
    na = _na()
    X = np.ascontiguousarray(X)
    index, dist2, _ = nn.feature_transform(X)
    want = nn.inpaint_nearest(X)
    work = X.copy()
    got = na.inpaint_nearest(work)
    assert got is work, tag
    assert nn.same_bits(got, want), tag
    dist, rc = na.nearest_source(X)
    assert dist.dtype == np.float64 and rc.dtype == np.int64 and rc.shape == (2,) + X.shape, tag
    rows, cols = X.shape
    if (index < 0).all():
        assert np.isinf(dist).all() and (rc == -1).all(), tag
        return
    assert np.array_equal(rc[0] * cols + rc[1], index), tag
    assert np.array_equal(dist, np.sqrt(dist2.astype(np.float64))), tag
    rr, cc = np.mgrid[0:rows, 0:cols]
    assert np.array_equal((rc[0] - rr) ** 2 + (rc[1] - cc) ** 2, dist2), tag
    assert nn.same_bits(X[rc[0], rc[1]], got), tag


def test_goldens(gpu_device):
    """the device result equals the restatement on every cell and the reference on every untied hole, fp32 and fp64"""
    na = _na()
    G = golden("nearest.npz")
    seen = set()
    for c in json.loads(str(G["cases"])):
        X, ref = G["in_" + c["name"]], G["out_" + c["name"]]
        work = X.copy()
        got = na.inpaint_nearest(work)
        assert got is work and got.dtype == X.dtype, c
        if X.dtype.kind != "f":
            assert np.array_equal(got, X), c
            continue
        seen.add(X.dtype.name)
        assert nn.same_bits(got, nn.inpaint_nearest(X)), c
        _, _, nties = nn.feature_transform(X)
        untied = ~np.isfinite(X) & (nties == 1)
        assert nn.same_bits(got[untied], ref[untied]), c
        if not np.isfinite(X).any():
            assert nn.same_bits(got, ref), c
        check_against_restatement(X, c["name"])
    assert seen == {"float32", "float64"}


def random_rasters():
    """(tag, raster): shapes around the kernels' sizes (32-row mask words, 64-row / 64-column tiles, 256-cell lookup
    blocks, 1024-column envelope segments), hole shares from 0 to 100 %, planted +-inf and -0.0, sources confined to a
    corner, a column or a row, holes on every border"""
    rng = np.random.default_rng(20261017)

    def base(shape, dtype):
        return (rng.normal(size=shape) * 5 + 100).astype(dtype)

    shapes = [(1, 1), (1, 2), (2, 1), (1, 300), (200, 1), (31, 33), (32, 64), (33, 65), (63, 63), (64, 64), (65, 129),
              (96, 70), (127, 40), (128, 3), (129, 17), (5, 255), (4, 256), (3, 257), (200, 30), (40, 300), (7, 1023),
              (6, 1024), (5, 1025), (3, 2049), (2, 3100)]
    shares = [0.0, 0.02, 0.3, 0.6, 0.9, 0.99, 1.0]
    k = 0
    for shape in shapes:
        for share in (shares[k % 7], shares[(k + 3) % 7]):
            dtype = np.float32 if k % 2 else np.float64
            X = base(shape, dtype)
            X[rng.random(shape) < share] = np.nan
            flat = X.reshape(-1)
            for v in (np.inf, -np.inf, -0.0):
                flat[rng.integers(flat.size)] = v
            yield "rand %s %.2f %s" % (shape, share, dtype.__name__), X
            k += 1
    for shape in ((70, 90), (33, 1100), (130, 66)):
        rows, cols = shape
        for name, keep in (("corner", (slice(rows - 2, rows), slice(cols - 3, cols))),
                           ("corner0", (slice(0, 1), slice(0, 1))),
                           ("column", (slice(None), slice(cols // 3, cols // 3 + 1))),
                           ("row", (slice(rows // 2, rows // 2 + 1), slice(None))),
                           ("last_row", (slice(rows - 1, rows), slice(None))),
                           ("last_column", (slice(None), slice(cols - 1, cols)))):
            X = np.full(shape, np.nan)
            X[keep] = base(shape, np.float64)[keep]
            yield "%s %s" % (name, shape), X
        if cols > 1000:
            shape = (20, cols)
        X = base(shape, np.float32)                     # holes touching every border, sources inside
        X[:3, :] = np.nan
        X[-2:, :] = np.nan
        X[:, :4] = np.nan
        X[:, -1:] = np.nan
        X[rng.random(shape) < 0.2] = -np.inf
        yield "borders %s" % (shape,), X


def test_random_cases_against_the_restatement(gpu_device):
    n = 0
    for tag, X in random_rasters():
        check_against_restatement(X, tag)
        n += 1
    assert n >= 70


def test_tie_rule(gpu_device):
    """a plateau of distinct values around symmetric holes: the chosen index is the lowest flat index among the sources at
    the minimal distance"""
    na = _na()
    n = 41
    rr, cc = np.mgrid[0:n, 0:n]
    plateau = (rr * n + cc).astype(np.float64)          # the value names the cell
    shapes = {}
    iso = plateau.copy()
    iso[5::7, 4::9] = np.nan                            # isolated holes: four sources at distance 1
    shapes["isolated"] = iso
    plus = plateau.copy()
    plus[20, 8:33] = np.nan
    plus[8:33, 20] = np.nan
    shapes["plus"] = plus
    ring = plateau.copy()
    d2 = (rr - 20) ** 2 + (cc - 20) ** 2
    ring[(d2 <= 15 ** 2) & (d2 >= 9 ** 2)] = np.nan     # a ring of holes around a disk of sources
    shapes["ring"] = ring
    disk = plateau.copy()
    disk[d2 <= 13 ** 2] = np.nan                        # its centre is equally far from many sources
    shapes["disk"] = disk
    square = plateau.copy()
    square[10:31, 10:31] = np.nan
    shapes["square"] = square
    checker = plateau.copy()
    checker[(rr + cc) % 2 == 0] = np.nan
    shapes["checkerboard"] = checker
    for name, X in shapes.items():
        for dtype in (np.float64, np.float32):
            Xd = X.astype(dtype)
            index, dist2, nties = nn.feature_transform(Xd)
            hole = np.isnan(Xd)
            assert (nties[hole] > 1).sum() >= 20, name              # the shape does put the rule to work
            dist, rc = na.nearest_source(Xd)
            flat = rc[0] * n + rc[1]
            assert np.array_equal(flat, index), (name, dtype)
            # spelled out: no source at the minimal distance has a lower flat index
            sr, sc = np.nonzero(~hole)
            for r, c in zip(*np.nonzero(hole)):
                d = (sr - r) ** 2 + (sc - c) ** 2
                assert flat[r, c] == (sr[d == d.min()] * n + sc[d == d.min()]).min(), (name, r, c)
            filled = na.inpaint_nearest(Xd.copy())
            assert np.array_equal(filled, index.astype(dtype)), (name, dtype)      # the value names the source
    assert na.inpaint_nearest(iso.copy())[5, 4] == 4 * n + 4                       # the upper of the four


def _edt_check(X, dist, rc, filled):
    """device planes of a large raster against SciPy's exact transform on the host"""
    finite = np.isfinite(X)
    edt = ndimage.distance_transform_edt(~finite)
    want2 = np.rint(edt ** 2).astype(np.int64)
    rows, cols = X.shape
    rr = np.arange(rows, dtype=np.int64)[:, None]
    cc = np.arange(cols, dtype=np.int64)[None, :]
    got2 = (rc[0] - rr) ** 2 + (rc[1] - cc) ** 2
    assert np.array_equal(got2, want2)
    assert np.array_equal(dist, np.sqrt(want2.astype(np.float64)))
    assert finite[rc[0], rc[1]].all()
    assert nn.same_bits(filled, X[rc[0], rc[1]])


def test_large_raster_against_scipy(gpu_device):
    """4096 x 4100 float32, scattered holes plus a 1500-cell-wide block: squared distances equal
    distance_transform_edt's; the filled value is the value at the returned index"""
    na = _na()
    rng = np.random.default_rng(3)
    rows, cols = 4096, 4100
    X = (rng.standard_normal((rows, cols), dtype=np.float32) * 5 + 100)
    X[rng.random((rows, cols), dtype=np.float32) < 0.05] = np.nan
    X[1000:2700, 1200:2700] = np.nan
    X[7, 9] = np.inf
    dist, rc = na.nearest_source(X)
    filled = na.inpaint_nearest(X.copy())
    assert np.isfinite(filled).all()
    _edt_check(X, dist, rc, filled)


def test_single_source_is_bounded_work(gpu_device):
    """2048^2 with one source: every cell equals it.  The guard on the work bound: it runs under the suite's ordinary
    time limit like any other test"""
    na = _na()
    X = np.full((2048, 2048), np.nan, dtype=np.float32)
    X[1234, 777] = np.float32(3.25)
    t0 = time.perf_counter()
    dist, rc = na.nearest_source(X)
    out = na.inpaint_nearest(X)
    print("single source 2048^2: %.2f s with transfers" % (time.perf_counter() - t0))
    assert out is X and (out == np.float32(3.25)).all()
    assert (rc[0] == 1234).all() and (rc[1] == 777).all()
    rr, cc = np.mgrid[0:2048, 0:2048]
    assert np.array_equal(dist, np.sqrt(((rr - 1234) ** 2 + (cc - 777) ** 2).astype(np.float64)))


@pytest.mark.parametrize("shape", [(16384, 8), (8, 16384)])
def test_long_thin_rasters(gpu_device, shape):
    na = _na()
    rng = np.random.default_rng(shape[0])
    X = rng.normal(size=shape) * 5 + 100
    X[rng.random(shape) < 0.7] = np.nan
    lo = 3000
    if shape[0] > shape[1]:
        X[lo:lo + 5000, :] = np.nan
    else:
        X[:, lo:lo + 5000] = np.nan
    dist, rc = na.nearest_source(X)
    filled = na.inpaint_nearest(X.copy())
    _edt_check(X, dist, rc, filled)


def test_in_place_and_layouts(gpu_device):
    import torch
    na = _na()
    rng = np.random.default_rng(5)
    X = rng.normal(size=(70, 130)) * 5 + 100
    X[rng.random(X.shape) < 0.4] = np.nan
    want = nn.inpaint_nearest(X)
    # NumPy in: the same object out, filled
    a = X.copy()
    assert na.inpaint_nearest(a) is a and nn.same_bits(a, want)
    # a CUDA tensor is filled in place on the device
    t = torch.from_numpy(X).to(gpu_device)
    p = t.data_ptr()
    r = na.inpaint_nearest(t)
    assert r is t and t.data_ptr() == p and t.is_cuda and nn.same_bits(t.cpu().numpy(), want)
    # non-contiguous inputs: a transposed tensor, a strided NumPy view, a CPU tensor
    tt = torch.from_numpy(np.ascontiguousarray(X.T)).to(gpu_device).t()
    assert not tt.is_contiguous()
    assert na.inpaint_nearest(tt) is tt and nn.same_bits(tt.cpu().numpy(), want)
    big = np.full((140, 260), 7.0)
    view = big[::2, ::2]
    view[...] = X
    assert na.inpaint_nearest(view) is view and nn.same_bits(np.ascontiguousarray(view), want)
    assert (big[1::2, :] == 7.0).all() and (big[:, 1::2] == 7.0).all()
    ct = torch.from_numpy(X.copy())
    assert na.inpaint_nearest(ct) is ct and nn.same_bits(ct.numpy(), want)
    # float32 and float16 keep their dtype; integers come back as they are
    for dt in (np.float32, np.float16):
        h = X.astype(dt)
        w = nn.inpaint_nearest(h)
        assert na.inpaint_nearest(h) is h and h.dtype == dt and nn.same_bits(h, w)
    i = np.arange(12).reshape(3, 4)
    assert na.inpaint_nearest(i) is i and i.dtype == np.arange(12).dtype
    it = torch.arange(12, device=gpu_device).reshape(3, 4)
    assert na.inpaint_nearest(it) is it
    # nearest_source: tensor in -> tensors out, the argument untouched, either plane alone
    t = torch.from_numpy(X).to(gpu_device)
    dist, rc = na.nearest_source(t)
    assert dist.is_cuda and rc.is_cuda and rc.shape == (2, 70, 130) and nn.same_bits(t.cpu().numpy(), X)
    d_only = na.nearest_source(t, return_indices=False)
    i_only = na.nearest_source(X, return_distances=False)
    assert torch.equal(d_only, dist) and np.array_equal(i_only, rc.cpu().numpy())
    e_d, e_i = ndimage.distance_transform_edt(~np.isfinite(X), return_indices=True)
    assert np.array_equal(np.rint(dist.cpu().numpy() ** 2), np.rint(e_d ** 2))
    assert i_only.shape == e_i.shape
    with pytest.raises(ValueError):
        na.nearest_source(X, return_distances=False, return_indices=False)
    with pytest.raises(ValueError):
        na.inpaint_nearest(np.zeros(5))
    # no hole and no source: unchanged
    full = rng.normal(size=(9, 9))
    assert nn.same_bits(na.inpaint_nearest(full.copy()), full)
    none = np.full((9, 9), np.nan)
    none[4, 4] = np.inf
    assert nn.same_bits(na.inpaint_nearest(none.copy()), none)


def test_device_route_from_smrf(gpu_device):
    """a DTM straight from smrf() on the device is accepted, filled in place, and equals the NumPy route"""
    import torch
    na = _na()
    x, y, z, _ = load_sample("samp21")
    xt, yt, zt = (torch.from_numpy(np.ascontiguousarray(v)).to(gpu_device) for v in (x, y, z))
    dtm_t, _, obj_t, _ = na.smrf(xt, yt, zt, cellsize=1, windows=18)
    assert isinstance(dtm_t, torch.Tensor) and dtm_t.is_cuda
    dtm_t[obj_t] = float("nan")                        # drop the object cells again: holes of every size
    host = dtm_t.cpu().numpy()
    assert np.isnan(host).sum() > 100
    out = na.inpaint_nearest(dtm_t)
    assert out is dtm_t and torch.isfinite(dtm_t).all()
    assert nn.same_bits(dtm_t.cpu().numpy(), na.inpaint_nearest(host.copy()))
    dist, rc = na.nearest_source(torch.from_numpy(host).to(gpu_device))
    assert np.array_equal(np.rint(dist.cpu().numpy() ** 2),
                          np.rint(ndimage.distance_transform_edt(np.isnan(host)) ** 2))


def test_determinism(gpu_device):
    """twenty calls on one 2048^2 input give identical bits"""
    import torch
    na = _na()
    gen = torch.Generator(device=gpu_device).manual_seed(17)
    X = torch.rand((2048, 2048), device=gpu_device, generator=gen, dtype=torch.float32) * 50
    X[torch.rand((2048, 2048), device=gpu_device, generator=gen) < 0.3] = float("nan")
    X[300:1100, 500:1500] = float("nan")
    first = first_idx = None
    for k in range(20):
        t = X.clone()
        na.inpaint_nearest(t)
        idx = na.nearest_source(X, return_distances=False)
        if first is None:
            first, first_idx = t, idx
            assert torch.isfinite(t).all()
        else:
            assert torch.equal(t.view(torch.int32), first.view(torch.int32)), k
            assert torch.equal(idx, first_idx), k
