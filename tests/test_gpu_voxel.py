"""voxelize on the device against the reference's goldens (tests/golden/voxel.npz) and the NumPy restatement
(tests/voxel_numpy.py).  DESIGN.md section 15.  Every comparison is np.array_equal on the whole volume; every cloud is a
few thousand points and every volume at most about 10**5 voxels."""
import ctypes as C
import json

import numpy as np
import pytest

import voxel_numpy as vn
from conftest import golden, unpack

pytestmark = pytest.mark.gpu

COUNTS = (2, 63, 64, 65, 257, 5000)
RESOLUTIONS = (1, 2, 31, 32, 33, 65)
LEVELS = (1, 31, 32, 33, 64, 65)


@pytest.fixture(scope="module")
def G():
    return golden("voxel.npz")


def cloud(n, seed, T=np.float64, zspan=8.0):
    """n points over 32 x 20 x zspan with both corners of the box among them, so the extents are exactly these"""
    rng = np.random.default_rng(seed)
    x, y, z = rng.uniform(0, 32.0, n), rng.uniform(0, 20.0, n), rng.uniform(0, zspan, n)
    x[0], y[0], z[0] = 0.0, 0.0, 0.0
    if n > 1:
        x[-1], y[-1], z[-1] = 32.0, 20.0, zspan
    return (x + 700.0).astype(T), (y - 40.0).astype(T), (z + 12.0).astype(T)


def check(x, y, z, resolution, **kw):
    """the device's volume equals the restatement's, shape, dtype and every voxel; returns it"""
    import neilpy_amd as na
    H = na.voxelize(None, x, y, z, resolution, **kw)
    want = vn.voxelize(None, x, y, z, resolution, **kw)
    assert isinstance(H, np.ndarray) and H.dtype == bool and H.flags.c_contiguous
    assert H.shape == want.shape, (H.shape, want.shape)
    assert np.array_equal(H, want), "%d of %d voxels differ, first at %s" % (
        (H != want).sum(), want.size, np.argwhere(H != want)[0])
    return H


def test_goldens(gpu_device, G):
    import neilpy_amd as na
    cases = json.loads(str(G["cases"]))
    assert len(cases) >= 14
    for c in cases:
        x, y, z = (G[k + "_" + c["cloud"]] for k in "xyz")
        kw = dict(c["kwargs"])
        H = na.voxelize(None, x, y, z, kw.pop("resolution"), **kw)
        want = unpack(G["bits_" + c["name"]], tuple(G["shape_" + c["name"]]))
        assert H.dtype == bool and H.shape == want.shape, (c["name"], H.shape, want.shape)
        assert np.array_equal(H, want), (c["name"], int((H != want).sum()))


@pytest.mark.parametrize("T", [np.float64, np.float32])
def test_point_counts_and_resolutions(gpu_device, T):
    """2 .. 5000 points (one wave, the wave boundary, more than one workgroup) x resolution 1 .. 65, both fill modes"""
    for n in COUNTS:
        for resolution in RESOLUTIONS:
            x, y, z = cloud(n, 10 * n + resolution, T)
            H = check(x, y, z, resolution, bottom_fill=bool(resolution & 1))
            assert H.shape[0] in (resolution, resolution + 1) and H.any()      # np.arange may round one edge in


def test_one_point_has_no_extent(gpu_device):
    """a single point, or any cloud on one vertical line, has no extent in x and y: refused after the bounds reduction"""
    import neilpy_amd as na
    one = np.array([3.0])
    with pytest.raises(ValueError, match="no extent"):
        na.voxelize(None, one, one, one, 4)
    with pytest.raises(ValueError, match="no extent"):
        na.voxelize(None, np.full(100, 2.5), np.full(100, -1.0), np.arange(100.0), 4)


@pytest.mark.parametrize("fill", [True, False])
def test_word_boundaries_of_the_bit_set(gpu_device, fill):
    """ve chosen so that nz is 1, 31, 32, 33, 64, 65 over a z extent of 8 at unit cells; then every pad 0 .. 5, so that
    nz + pad takes every residue mod 4 on both sides of a dword of the expand store"""
    x, y, z = cloud(4000, 77)
    for nz in LEVELS:
        H = check(x, y, z, 32, ve=nz / 8.0, bottom_fill=fill)
        assert H.shape == (32, 20, nz), (nz, H.shape)
        for pad in range(1, 6):
            H = check(x, y, z, 32, ve=nz / 8.0, bottom_fill=fill, pad=pad, threshold=1 + (pad & 1))
            assert H.shape == (32, 20, nz + pad) and H[:, :, :pad].all()
    # rows of 1, 3, 4 and 5 bytes: a dword of the output spans up to four columns
    for pad in (0, 2, 3, 4):
        assert check(x, y, z, 32, ve=1 / 8.0, bottom_fill=fill, pad=pad).shape == (32, 20, 1 + pad)


@pytest.mark.parametrize("fill", [True, False])
def test_thresholds_on_repeated_points(gpu_device, fill):
    """each point 1 to 6 times: the counts straddle thresholds 2 and 5"""
    x, y, z = cloud(900, 5)
    rep = np.random.default_rng(6).integers(1, 7, 900)
    order = np.random.default_rng(7).permutation(int(rep.sum()))
    x, y, z = (np.repeat(a, rep)[order] for a in (x, y, z))
    filled = []
    for threshold in (1, 2, 5):
        for resolution, ve in ((33, 1), (64, 4.125)):
            H = check(x, y, z, resolution, threshold=threshold, ve=ve, bottom_fill=fill)
            filled.append(int(H.sum()))
    assert min(filled) > 0
    if not fill:                                  # with the fill a higher threshold can raise a column's lowest voxel
        assert filled[0] > filled[2] > filled[4] and filled[1] > filled[3] > filled[5]


def test_float32_and_mixed_dtypes(gpu_device):
    x, y, z = cloud(3000, 21, np.float32, zspan=13.0)
    check(x, y, z, 40, ve=2.5, pad=1)
    check(x + np.float32(5e4), y, z, 40, threshold=2)                  # 16 bits of the float32 mantissa gone to the offset
    check(x.astype(np.float64), y, z, 17)                               # mixed: widened to float64, as the restatement does
    check(x.astype(np.int64), y.astype(np.int32), z, 9)


def _marks(ws, nx, ny, nz, threshold):
    """the marks at the head of a workspace as counts, or as 0 / 1 for the bit set"""
    if threshold > 1:
        return ws[:nx * ny * nz * 4].cpu().numpy().view(np.uint32).reshape(nx, ny, nz).astype(np.int64)
    words = (nz + 31) // 32
    raw = ws[:nx * ny * words * 4].cpu().numpy().view(np.uint32).reshape(nx, ny, words)
    bits = np.unpackbits(raw.view(np.uint8), bitorder="little").reshape(nx, ny, words * 32)
    assert not bits[:, :, nz:].any()                                     # no bit past the column's last cell
    return bits[:, :, :nz].astype(np.int64)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_mark_with_hand_made_edges(gpu_device, sfx):
    """the mark entry of the C ABI on edges of uneven width (one of them doubled): points below the first edge and above
    the last are dropped, a point on the last edge goes to the last bin, a point on an interior edge to the upper bin"""
    import torch
    from neilpy_amd import _lib
    from neilpy_amd._raster import _ptr, _stream
    lib = _lib.load()
    T = np.float64 if sfx == "f64" else np.float32
    xe = np.array([0.0, 1.0, 2.5, 2.5, 4.0, 10.0])
    ye = np.array([-2.0, -1.0, 3.0])
    ze = np.concatenate([np.arange(0.0, 16.0, 0.5), np.arange(16.0, 40.0, 4.0), [40.0, 41.0, 45.0]])   # 40 bins: two words
    nx, ny, nz = len(xe) - 1, len(ye) - 1, len(ze) - 1
    assert nz == 40
    rng = np.random.default_rng(31)
    n = 3000
    d = [rng.uniform(e[0] - 1.0, e[-1] + 1.0, n) for e in (xe, ye, ze)]            # some outside on every axis
    for a, e in zip(d, (xe, ye, ze)):
        a[:len(e)] = e                                                              # every edge itself, the last included
        a[len(e):len(e) + 4] = [e[0] - 0.25, e[-1] + 0.25, np.nextafter(e[0], -np.inf), np.nextafter(e[-1], np.inf)]
        rng.shuffle(a)
    offsets = np.array([16.0, -8.0, 0.0])
    pts = [(a + o).astype(T) for a, o in zip(d, offsets)]
    dd = [(p - T(o)).astype(np.float64) for p, o in zip(pts, offsets)]             # what the kernel subtracts
    want = vn.counts_of((xe, ye, ze), dd)
    inside = [(a >= e[0]) & (a <= e[-1]) for a, e in zip(dd, (xe, ye, ze))]
    assert 0 < want.sum() == int((inside[0] & inside[1] & inside[2]).sum()) < n    # outliers dropped, the edges closed
    assert want[2].sum() == 0                                                       # the empty bin between the doubled edges

    dev = [torch.from_numpy(p).to(gpu_device) for p in pts]
    edges = [torch.from_numpy(e).to(gpu_device) for e in (xe, ye, ze)]
    off = (C.c_double * 3)(*offsets)
    for threshold in (1, 2):
        nbytes = lib.smrf_voxel_workspace_bytes(nx, ny, nz, threshold)
        ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=gpu_device)     # the entry clears its marks itself
        _lib.check(getattr(lib, "smrf_voxel_mark_" + sfx)(_ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), n, off, _ptr(edges[0]),
                                                          _ptr(edges[1]), _ptr(edges[2]), nx, ny, nz, threshold, _ptr(ws),
                                                          nbytes, _stream()))
        torch.cuda.synchronize()
        got = _marks(ws, nx, ny, nz, threshold)
        assert np.array_equal(got, want if threshold > 1 else (want >= 1)), threshold
        for fill, pad in ((1, 0), (0, 3), (1, 2)):
            out = torch.full((nx, ny, nz + pad), 7, dtype=torch.uint8, device=gpu_device)
            _lib.check(lib.smrf_voxel_expand(_ptr(ws), nbytes, nx, ny, nz, threshold, fill, pad, _ptr(out), _stream()))
            assert np.array_equal(out.cpu().numpy(), vn.solid(want, threshold, bool(fill), pad).astype(np.uint8))
        # a workspace one byte short is refused, nothing is launched
        rc = lib.smrf_voxel_expand(_ptr(ws), nbytes - 1, nx, ny, nz, threshold, 1, 0, _ptr(out), _stream())
        assert rc != 0 and b"workspace" in lib.smrf_last_error()


def test_tensors_in_tensors_out(gpu_device):
    import torch
    import neilpy_amd as na
    for T in (np.float64, np.float32):
        x, y, z = cloud(2500, 41, T)
        want = check(x, y, z, 33, ve=2, pad=2)
        tx, ty, tz = (torch.from_numpy(a).to(gpu_device) for a in (x, y, z))
        H = na.voxelize(None, tx, ty, tz, 33, ve=2, pad=2)
        assert isinstance(H, torch.Tensor) and H.dtype == torch.bool and H.device == gpu_device and H.is_contiguous()
        assert np.array_equal(H.cpu().numpy(), want)
        H2 = na.voxelize(None, tx[::2], ty[::2], tz[::2], 16, threshold=2)             # strided views of the cloud
        assert np.array_equal(H2.cpu().numpy(), vn.voxelize(None, x[::2], y[::2], z[::2], 16, threshold=2))


def test_return_edges(gpu_device):
    """the edges and offsets that were used, bit for bit the restatement's; they place the voxels back on the cloud"""
    import neilpy_amd as na
    for T in (np.float64, np.float32):
        x, y, z = cloud(2000, 51, T, zspan=11.3)
        H, edges, mins = na.voxelize(None, x, y, z, 37, ve=1.5, pad=1, return_edges=True)
        want, wedges, wmins = vn.voxelize(None, x, y, z, 37, ve=1.5, pad=1, return_edges=True)
        assert np.array_equal(H, want) and len(edges) == 3 and len(mins) == 3
        for a, b in zip(edges, wedges):
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.tobytes() == b.tobytes()
        assert all(type(m) is T and m == w for m, w in zip(mins, wmins))
        assert H.shape == (len(edges[0]) - 1, len(edges[1]) - 1, len(edges[2]) - 1 + 1)
        i = np.searchsorted(edges[0], (x - mins[0])[5], side="right") - 1
        j = np.searchsorted(edges[1], (y - mins[1])[5], side="right") - 1
        k = np.searchsorted(edges[2], (z - mins[2])[5], side="right") - 1
        assert H[i, j, 1 + k]


def test_two_calls_give_identical_bytes(gpu_device):
    x, y, z = cloud(5000, 61)
    for kw in (dict(), dict(threshold=2, ve=3.0, pad=1)):
        a = check(x, y, z, 48, **kw)
        b = check(x, y, z, 48, **kw)
        assert a.tobytes() == b.tobytes()


def test_flat_cloud_has_no_levels(gpu_device):
    """all z equal: the reference's np.arange gives one z edge, so no z bins; the result is the pad alone"""
    x, y, z = cloud(500, 71)
    z[:] = 4.0
    assert check(x, y, z, 8).shape == (8, 5, 0)
    H = check(x, y, z, 8, pad=3)
    assert H.shape == (8, 5, 3) and H.all()


def test_nonfinite_coordinates_raise(gpu_device):
    import neilpy_amd as na
    for T in (np.float64, np.float32):
        good = cloud(300, 81, T)
        for value in (np.nan, np.inf, -np.inf):
            for axis in range(3):
                bad = [a.copy() for a in good]
                bad[axis][123] = value
                with pytest.raises(ValueError, match="NaN or infinite"):
                    na.voxelize(None, *bad, 8)
