"""The small kernels between smrf()'s big stages, each called by name through the C ABI and held to the bit against
the one NumPy line its header comment quotes (include/smrf_hip.h), under -m gpu.

Every one of them is a grid-stride loop with a block cap (8192, 2048 or 1024 blocks of 256 threads), so the 1-D
lengths end in 8192 * 256 + 257: the second trip of every capped loop runs, with a remainder that is no multiple of the
block.  The raster kernel (gradient + slope) gets the same through 4100 x 513 cells.
"""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 8192 * 256 + 257
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1000, BIG]
E_ARG, E_WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def nz(gpu_device):
    import neilpy_amd
    neilpy_amd.load_library()
    return neilpy_amd


@pytest.fixture(scope="module")
def lib(nz):
    from neilpy_amd import _lib
    return _lib.load()


def ok(rc):
    from neilpy_amd import _lib
    _lib.check(rc)


def dev(a, gpu_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def doubles(*v):
    return (C.c_double * len(v))(*v)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_values(got, want):
    """equal as NumPy values, NaN where NaN, and the same sign on every zero"""
    return np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got) & (got == 0), np.signbit(want) & (want == 0))


# ---------------------------------------------------------------------------------------------- smrf_points_extent_f64
def _extent(lib, gpu_device, x, y, ws_bytes=4 * 1024 * 8):
    import torch
    ws = torch.full((max(ws_bytes, 1),), 255, dtype=torch.uint8, device=gpu_device)
    out = doubles(0, 0, 0, 0)
    x_d, y_d = dev(x, gpu_device), dev(y, gpu_device)
    rc = lib.smrf_points_extent_f64(p(x_d), p(y_d), x.size, out, p(ws), ws_bytes, stream())
    return rc, np.array(out[:])


@pytest.mark.parametrize("n", LENGTHS)
def test_points_extent(lib, gpu_device, n):
    rng = np.random.default_rng(n)
    x = rng.normal(8.6e5, 300.0, n)
    y = rng.normal(1.9e6, 300.0, n)
    rc, got = _extent(lib, gpu_device, x, y)
    assert rc == 0 and same_bits(got, np.array([np.min(x), np.max(x), np.min(y), np.max(y)]))
    # +-inf are ordinary values of np.min / np.max
    xi, yi = x.copy(), y.copy()
    xi[n // 2] = np.inf
    yi[(2 * n) // 3] = -np.inf
    rc, got = _extent(lib, gpu_device, xi, yi)
    assert rc == 0 and same_bits(got, np.array([np.min(xi), np.inf, -np.inf, np.max(yi)]))
    if n > 1:
        xi[0] = -np.inf
        yi[-1] = np.inf
        rc, got = _extent(lib, gpu_device, xi, yi)
        assert rc == 0 and same_bits(got, np.array([-np.inf, np.inf, -np.inf, np.inf]))
    # one NaN anywhere, in x or in y, makes all four NaN: the first element, the last, and (the capped loop: 1024 blocks
    # of 256) an element that only the second trip reads
    spots = [0, n - 1] + ([1024 * 256 + 77, n - 300] if n == BIG else [])
    for k, i in enumerate(spots):
        xn, yn = x.copy(), y.copy()
        (xn if k % 2 == 0 else yn)[i] = np.nan
        rc, got = _extent(lib, gpu_device, xn, yn)
        assert rc == 0 and np.isnan(got).all(), (n, i)
        assert np.isnan(np.min(xn) + np.min(yn))


def test_points_extent_short_workspace(lib, gpu_device):
    x = np.arange(1000.0)
    need = 4 * 4 * 8                                                  # 4 blocks of partial (min, max, min, max)
    assert _extent(lib, gpu_device, x, x, need)[0] == 0
    rc, out = _extent(lib, gpu_device, x, x, need - 1)
    assert rc == E_WORKSPACE and np.array_equal(out, np.zeros(4))     # refused before any launch: h_out untouched
    x = np.arange(float(BIG))
    assert _extent(lib, gpu_device, x, x, 4 * 1024 * 8 - 1)[0] == E_WORKSPACE


# ------------------------------------------------------------------- smrf_points_nn_bounds_f64, smrf_voxel_bounds_f32/64
# the other two callers of csrc/cloud_reduce.h: non-finite coordinates are counted, the box skips a NaN and takes an
# infinity.  Their loop is capped at 1024 workgroups, so the last length reaches its second trip.
PARTS_LENGTHS = LENGTHS[:-1] + [1024 * 256 + 257]


def _box_numpy(cols, n):
    """(min, max) per column as float64.  np.nanmin / np.nanmax, which a column of one NaN (n = 1) has none of: the
    reduction then leaves its identity, (inf, -inf)"""
    out = []
    for c in cols:
        c = c.astype(np.float64)
        if n > 1:
            assert np.fmin.reduce(c) == np.nanmin(c) and np.fmax.reduce(c) == np.nanmax(c)
        out += [np.fmin.reduce(c, initial=np.inf), np.fmax.reduce(c, initial=-np.inf)]
    return np.array(out)


def _nn_bounds(lib, gpu_device, pts, ws_bytes=1024 * 5 * 8):
    import torch
    ws = torch.full((max(ws_bytes, 1),), 255, dtype=torch.uint8, device=gpu_device)
    box, bad = doubles(0, 0, 0, 0), C.c_int64(-7)
    pts_d = dev(pts, gpu_device)
    rc = lib.smrf_points_nn_bounds_f64(p(pts_d), pts.shape[0], pts.shape[1], box, C.byref(bad), p(ws), ws_bytes, stream())
    return rc, np.array(box[:]), bad.value


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", PARTS_LENGTHS)
def test_points_nn_bounds(lib, gpu_device, n, dim):
    rng = np.random.default_rng(n + dim)
    pts = rng.normal(8.6e5, 300.0, (n, dim))
    pts[:, dim - 1] *= 3.0                                            # the last column reaches past the others
    rc, box, bad = _nn_bounds(lib, gpu_device, pts)
    assert rc == 0 and bad == 0
    assert same_bits(box, np.array([pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()]))
    # NaN and +-inf are counted over all columns; the box is of columns 0 and 1, skips the NaN and takes the infinity
    pts[0, 0] = np.nan
    pts[n // 2, 1] = np.inf
    if dim == 3:
        pts[n - 1, 2] = -np.inf
    rc, box, bad = _nn_bounds(lib, gpu_device, pts)
    assert rc == 0 and bad == dim
    assert same_bits(box, _box_numpy([pts[:, 0], pts[:, 1]], n)) and box[3] == np.inf and box[2] != -np.inf


def test_points_nn_bounds_signed_zero(lib, gpu_device):
    """min0 over (0.0, -0.0, 1.0, ...) is a zero whose sign the order of the reduction decides: lane 0 holds +0.0,
    lane 1 -0.0, and the last step of the shuffle tree is fmin(+0.0, -0.0) = -0.0 on gfx950.  The sign asserted is
    the one points_bounds_kernel returned before the bounds kernels became one (profiles/cloud_boundary.md section 2)"""
    pts = np.ones((1000, 2))
    pts[0, 0], pts[1, 0] = 0.0, -0.0
    rc, box, bad = _nn_bounds(lib, gpu_device, pts)
    print("min0 = %r, signbit %s" % (box[0], np.signbit(box[0])))
    assert rc == 0 and bad == 0 and same_bits(box, np.array([-0.0, 1.0, 1.0, 1.0]))


def test_points_nn_bounds_short_workspace(lib, gpu_device):
    pts = np.arange(2000.0).reshape(1000, 2)
    assert _nn_bounds(lib, gpu_device, pts, 1024 * 5 * 8)[0] == 0
    rc, box, bad = _nn_bounds(lib, gpu_device, pts, 1024 * 5 * 8 - 1)
    assert rc == E_WORKSPACE and np.array_equal(box, np.zeros(4)) and bad == -7     # refused before any launch


def _voxel_bounds(lib, gpu_device, x, y, z, ws_bytes=57344):
    import torch
    ws = torch.full((max(ws_bytes, 1),), 255, dtype=torch.uint8, device=gpu_device)
    box, bad = doubles(0, 0, 0, 0, 0, 0), C.c_int64(-7)
    x_d, y_d, z_d = dev(x, gpu_device), dev(y, gpu_device), dev(z, gpu_device)
    fn = lib.smrf_voxel_bounds_f32 if x.dtype == np.float32 else lib.smrf_voxel_bounds_f64
    rc = fn(p(x_d), p(y_d), p(z_d), x.size, box, C.byref(bad), p(ws), ws_bytes, stream())
    return rc, np.array(box[:]), bad.value


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", PARTS_LENGTHS)
def test_voxel_bounds(lib, gpu_device, n, dtype):
    rng = np.random.default_rng(n)
    x, y, z = (rng.normal(c, 300.0, n).astype(dtype) for c in (8.6e5, 1.9e6, 120.0))
    rc, box, bad = _voxel_bounds(lib, gpu_device, x, y, z)
    assert rc == 0 and bad == 0
    assert same_bits(box, np.array([x.min(), x.max(), y.min(), y.max(), z.min(), z.max()], dtype=np.float64))
    x[0] = np.nan
    y[n // 2] = np.inf
    z[n - 1] = -np.inf
    rc, box, bad = _voxel_bounds(lib, gpu_device, x, y, z)
    assert rc == 0 and bad == 3
    assert same_bits(box, _box_numpy([x, y, z], n)) and box[3] == np.inf and box[4] == -np.inf


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxel_bounds_signed_zero(lib, gpu_device, dtype):
    """zeros of both signs at the ends of a column: the box holds what voxel_bounds_kernel returned for this input
    before the bounds kernels became one (profiles/cloud_boundary.md section 2): -0.0 for both minima whichever zero
    comes first, and -0.0 for the maximum of z, whose +0.0 sits in the last row"""
    n = 1000
    x, y, z = np.ones(n, dtype), np.ones(n, dtype), -np.ones(n, dtype)
    x[0], x[1] = 0.0, -0.0
    y[0], y[1] = -0.0, 0.0
    z[0], z[n - 1] = -0.0, 0.0
    rc, box, bad = _voxel_bounds(lib, gpu_device, x, y, z)
    print("box = %r, signbit %s" % (box, np.signbit(box)))
    assert rc == 0 and bad == 0 and same_bits(box, np.array([-0.0, 1.0, -0.0, 1.0, -1.0, -0.0]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxel_bounds_short_workspace(lib, gpu_device, dtype):
    x = np.arange(1000, dtype=dtype)
    assert _voxel_bounds(lib, gpu_device, x, x, x, 57344)[0] == 0
    rc, box, bad = _voxel_bounds(lib, gpu_device, x, x, x, 57344 - 1)
    assert rc == E_WORKSPACE and np.array_equal(box, np.zeros(6)) and bad == -7       # refused before any launch


# ----------------------------------------------------------------------------------------------- smrf_affine_apply_f64
def _inverse(cellsize, theta, x0=8.6e5, y0=1.9e6):
    """(a, b, c, d, e, f) of the inverse of a north-up (theta = 0) or rotated transform with its origin at (x0, y0)"""
    a, b = np.cos(theta) / cellsize, np.sin(theta) / cellsize
    d, e = np.sin(theta) / cellsize, -np.cos(theta) / cellsize
    return (float(a), float(b), float(-(a * x0 + b * y0)), float(d), float(e), float(-(d * x0 + e * y0)))


def _rnd(q):
    return Fraction(float(q))          # Fraction -> float is one correctly rounded division of two integers


def _fused_differs(x, y, a, b, c):
    """does one of the two contractions of (x*a + y*b) + c give other bits than the separately rounded form?"""
    X, Y, A_, B_, C_ = (Fraction(float(v)) for v in (x, y, a, b, c))
    plain = _rnd(_rnd(_rnd(X * A_) + _rnd(Y * B_)) + C_)
    fma_x = _rnd(_rnd(X * A_ + _rnd(Y * B_)) + C_)                    # fma(x, a, y*b) + c
    fma_y = _rnd(_rnd(_rnd(X * A_) + Y * B_) + C_)                    # fma(y, b, x*a) + c
    return plain != fma_x, plain != fma_y


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cellsize,theta", [(.3, 0.0), (.5, 0.0), (.3, .1), (.5, .25)])
def test_affine_apply(lib, gpu_device, n, cellsize, theta):
    import torch
    rng = np.random.default_rng(n + int(cellsize * 10))
    x = 8.6e5 + rng.uniform(0, 900, n)
    y = 1.9e6 - rng.uniform(0, 700, n)
    inv = _inverse(cellsize, theta)
    if theta != 0.0 and n == 1000:
        # the data can show a contraction: on a rotated transform a fused multiply-add moves the result.  (North-up
        # transforms have b = d = 0 and every contraction of them is exact, so they cannot.)
        hits = np.array([_fused_differs(x[i], y[i], *inv[:3]) + _fused_differs(x[i], y[i], *inv[3:]) for i in range(n)])
        assert (hits.mean(0) >= .01).all(), hits.mean(0)
    col = torch.full((n,), np.nan, dtype=torch.float64, device=gpu_device)
    row = torch.full((n,), np.nan, dtype=torch.float64, device=gpu_device)
    x_d, y_d = dev(x, gpu_device), dev(y, gpu_device)
    ok(lib.smrf_affine_apply_f64(p(x_d), p(y_d), n, doubles(*inv), p(col), p(row), stream()))
    a, b, c, d, e, f = inv
    assert same_bits(col.cpu().numpy(), (x * a + y * b) + c)
    assert same_bits(row.cpu().numpy(), (x * d + y * e) + f)


# --------------------------------------------------------------------------------------------- smrf_las_decode_xyz_f64
@pytest.mark.parametrize("reclen", (20, 28, 34, 67))
def test_las_decode(lib, gpu_device, reclen):
    import torch
    so = [(.01, .001, .01, 1e5, 2e6, 4.5e5), (.001, .01, .001, 2e6, 1e5, 1234.5)][reclen % 2]
    for n in LENGTHS[:-1] + ([BIG] if reclen == 34 else []):
        rng = np.random.default_rng(n + reclen)
        XYZ = rng.integers(-2 ** 31, 2 ** 31, (n, 3), dtype=np.int64).astype(np.int32)
        edge = np.array([-2 ** 31, 2 ** 31 - 1, -1, 0], dtype=np.int32)
        for k in range(min(n, 12)):                                   # every extreme in every coordinate, first and last records
            XYZ[(k // 3) if k < 6 else n - 1 - (k - 6) // 3, k % 3] = edge[(k + k // 3) % 4]
        if n >= 4:
            XYZ[:4] = edge[:, None]
            XYZ[-4:] = edge[::-1, None]
        rec = np.empty((n, reclen), dtype=np.uint8)
        rec[:] = ((np.arange(reclen) * 37 + 11) % 256).astype(np.uint8)           # the fields after x, y, z
        rec[:, :12] = XYZ.astype("<i4").view(np.uint8).reshape(n, 12)
        buf = np.zeros(n * reclen + 1, dtype=np.uint8)                # the records start one byte into the allocation
        buf[1:] = rec.ravel()
        buf_d = dev(buf, gpu_device)
        out = [torch.full((n,), np.nan, dtype=torch.float64, device=gpu_device) for _ in range(3)]
        ok(lib.smrf_las_decode_xyz_f64(C.c_void_p(buf_d.data_ptr() + 1), n, reclen, doubles(*so), p(out[0]), p(out[1]),
                                       p(out[2]), stream()))
        for k in range(3):
            assert same_bits(out[k].cpu().numpy(), XYZ[:, k].astype(np.float64) * so[k] + so[3 + k]), (n, reclen, k)


# ------------------------------------------------------- smrf_grid_clear_u64, smrf_grid_bin_f64, smrf_grid_finalize_f64
def grid_numpy(x, y, z, inv, filt, rows, cols, is_max):
    """(grid, empty, points outside the grid) as create_dem's groupby gives them (neilpy.py:1128, :1141-1156)"""
    a, b, c, d, e, f = inv
    keep = np.ones(x.size, dtype=bool)
    if filt is not None:
        keep = ~((x < filt[0]) | (x > filt[1]) | (y > filt[3]) | (y < filt[2]))
    with np.errstate(invalid="ignore"):
        ci = np.floor((x * a + y * b) + c)
        ri = np.floor((x * d + y * e) + f)
        inside = (ci >= 0) & (ci < cols) & (ri >= 0) & (ri < rows)
    sel = keep & inside & ~np.isnan(z)
    flat = ri[sel].astype(np.int64) * cols + ci[sel].astype(np.int64)
    g = np.full(rows * cols, -np.inf if is_max else np.inf)
    (np.maximum if is_max else np.minimum).at(g, flat, z[sel])
    empty = np.bincount(flat, minlength=rows * cols) == 0
    g[empty] = np.nan
    return g.reshape(rows, cols), empty.reshape(rows, cols), int((keep & ~inside).sum())


class DeviceCloud:
    def __init__(self, lib, gpu_device, x, y, z):
        self.lib, self.device, self.n = lib, gpu_device, x.size
        self.x, self.y, self.z = (dev(v, gpu_device) for v in (x, y, z))

    def grid(self, inv, filt, rows, cols, is_max, row0=0, rows_local=None, want_empty=True):
        import torch
        lib = self.lib
        rows_local = rows if rows_local is None else rows_local
        cells = rows_local * cols
        keys = torch.zeros(max(cells, 1), dtype=torch.int64, device=self.device)
        n_out = torch.zeros(1, dtype=torch.int64, device=self.device)
        ok(lib.smrf_grid_clear_u64(p(keys), cells, stream()))
        if cells:
            assert bool((keys[:cells] == -1).all())                    # all-ones = empty
        ok(lib.smrf_grid_bin_f64(p(self.x), p(self.y), p(self.z), self.n, doubles(*inv),
                                 doubles(*filt) if filt is not None else None, p(keys), rows, cols, row0, rows_local,
                                 int(is_max), p(n_out), stream()))
        grid = torch.full((max(cells, 1),), 7.0, dtype=torch.float64, device=self.device)
        empty = torch.full((max(cells, 1),), 9, dtype=torch.uint8, device=self.device) if want_empty else None
        ok(lib.smrf_grid_finalize_f64(p(keys), p(grid), p(empty), cells, int(is_max), stream()))
        g = grid.cpu().numpy()[:cells].reshape(rows_local, cols)
        e = empty.cpu().numpy()[:cells].reshape(rows_local, cols) if want_empty else None
        return g, e, int(n_out.item())


def _cloud(n, rows, cols, cellsize, seed, spread=1.06):
    """n points over (and a little beyond) a rows x cols grid of the north-up transform at (8.6e5, 1.9e6); z holds NaN,
    +-inf and negative values, and no zero of either sign (pandas' choice between -0.0 and 0.0 depends on order)"""
    rng = np.random.default_rng(seed)
    w, h = cols * cellsize, rows * cellsize
    x = 8.6e5 + (rng.uniform(0, spread, n) + .02) * w                  # the westmost 2 % of the grid stay empty
    y = 1.9e6 - (rng.uniform(0, spread, n) - (spread - 1) / 2) * h
    z = rng.normal(-3.0, 40.0, n)
    z[z == 0] = 1.0
    z[rng.random(n) < .05] = np.nan
    z[rng.random(n) < .001] = np.inf
    z[rng.random(n) < .001] = -np.inf
    if n > 2:
        z[0], z[1], z[2] = np.nan, np.inf, -np.inf
    return x, y, z


def _check_grid(cloud, host, inv, filt, rows, cols, is_max, bands=None):
    want, want_empty, want_out = grid_numpy(*host, inv, filt, rows, cols, is_max)
    got, empty, n_out = cloud.grid(inv, filt, rows, cols, is_max)
    assert same_values(got, want) and np.array_equal(empty, want_empty.astype(np.uint8)) and n_out == want_out
    got2, none, n_out2 = cloud.grid(inv, filt, rows, cols, is_max, want_empty=False)          # d_empty = NULL
    assert none is None and same_bits(got2, got) and n_out2 == want_out
    if bands:
        parts = [cloud.grid(inv, filt, rows, cols, is_max, row0, nloc) for row0, nloc in bands]
        assert sum(nloc for _, nloc in bands) == rows
        assert same_bits(np.vstack([g for g, _, _ in parts]), got)
        assert np.array_equal(np.vstack([e for _, e, _ in parts]), empty)
        assert [k for _, _, k in parts] == [want_out] * len(bands)    # every band call counts the points outside the WHOLE grid
    return want, want_out


@pytest.mark.parametrize("is_max", (0, 1))
def test_grid_contention(lib, gpu_device, is_max):
    """10^6 points into 7 x 5 cells: every atomic min / max contended"""
    host = _cloud(10 ** 6, 7, 5, .5, 21)
    cloud = DeviceCloud(lib, gpu_device, *host)
    want, n_out = _check_grid(cloud, host, _inverse(.5, 0.0), None, 7, 5, is_max, bands=[(0, 2), (2, 4), (6, 1)])
    assert n_out > 1000 and np.isinf(want).all()                      # +-inf win every cell they reach


@pytest.mark.parametrize("is_max", (0, 1))
@pytest.mark.parametrize("cellsize,theta", [(.3, 0.0), (.5, .1)])
def test_grid_second_trip(lib, gpu_device, is_max, cellsize, theta):
    """8192 * 256 + 257 points (the bin loop's second trip) into 300 x 257 cells, in three row bands too; rotated as
    well as north-up, where the row and column sums have two non-zero products"""
    host = _cloud(BIG, 300, 257, cellsize, 22, spread=1.5 if theta else 1.06)
    cloud = DeviceCloud(lib, gpu_device, *host)
    want, n_out = _check_grid(cloud, host, _inverse(cellsize, theta), None, 300, 257, is_max,
                              bands=[(0, 100), (100, 199), (299, 1)])
    assert n_out > 1000 and 0 < np.isnan(want).sum() < want.size and np.isfinite(want).sum() > want.size // 2


@pytest.mark.parametrize("is_max", (0, 1))
def test_grid_boundaries_and_filter(lib, gpu_device, is_max):
    """Points exactly on cell boundaries (cell size 0.5 and an origin that is a multiple of it: every product and sum is
    exact, so a point on a boundary belongs to the cell to its east / south, and one on the grid's east or south edge
    is outside), and the filter rectangle with points exactly on its four bounds, which are inclusive (:1128)."""
    rows, cols, cs = 9, 12, .5
    inv = _inverse(cs, 0.0)
    gx = 8.6e5 + cs * np.arange(-1, cols + 2)                         # every column boundary, one beyond each side
    gy = 1.9e6 - cs * np.arange(-1, rows + 2)
    x, y = (v.ravel() for v in np.meshgrid(gx, gy))
    rng = np.random.default_rng(23)
    xr, yr, zr = _cloud(5000, rows, cols, cs, 24, spread=1.3)
    x, y = np.concatenate([x, xr]), np.concatenate([y, yr])
    z = np.concatenate([rng.normal(10.0, 5.0, gx.size * gy.size), zr])
    # the filter's bounds sit on cell boundaries and a few points lie exactly on each
    filt = (8.6e5 + 2 * cs, 8.6e5 + 9 * cs, 1.9e6 - 7 * cs, 1.9e6 - 1 * cs)   # xedges[0], xedges[-1], yedges[-1], yedges[0]
    on = [(x == filt[0]).sum(), (x == filt[1]).sum(), (y == filt[2]).sum(), (y == filt[3]).sum()]
    assert min(on) >= rows
    host = (x, y, z)
    cloud = DeviceCloud(lib, gpu_device, *host)
    bands = [(0, 3), (3, 5), (8, 1)]
    whole, n_out = _check_grid(cloud, host, inv, None, rows, cols, is_max, bands)
    assert n_out >= 2 * (rows + cols)
    part, n_out_f = _check_grid(cloud, host, inv, filt, rows, cols, is_max, bands)
    assert n_out_f == 0                                               # the filter drops before the grid test counts
    # inclusive bounds: the cells just inside hold the points ON the bounds; outside the rectangle nothing is binned
    assert not np.isnan(part[1:7, 2:9]).any() and np.isnan(part[:1]).all() and np.isnan(part[:, :2]).all()
    assert np.isnan(part[8:]).all() and np.isnan(part[:, 10:]).all()
    assert not np.isnan(part[7, 2:10]).any() and not np.isnan(part[1:8, 9]).any()    # y == yedges[-1] and x == xedges[-1] are kept
    # a filter wider than the grid keeps the points outside, and they are counted
    wide = (8.6e5 - 10, 8.6e5 + 10, 1.9e6 - 10, 1.9e6 + 10)
    assert _check_grid(cloud, host, inv, wide, rows, cols, is_max)[1] > 0


# --------------------------------------------------------------------------------------------- smrf_gradient_slope_f64
def _slope(lib, gpu_device, Z, h):
    import torch
    Z_d = dev(Z, gpu_device)
    S_d = torch.full(Z.shape, -1.0, dtype=torch.float64, device=gpu_device)
    rc = lib.smrf_gradient_slope_f64(p(Z_d), p(S_d), Z.shape[0], Z.shape[1], h, stream())
    return rc, S_d.cpu().numpy()


@pytest.mark.parametrize("shape", [(2, 2), (2, 300), (300, 2), (3, 3), (257, 515), (4100, 513)])
def test_gradient_slope(lib, gpu_device, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    Z = rng.normal(0, 1, shape).cumsum(0).cumsum(1) * .37 + 1234.5
    m, n = shape
    if m * n > 9:
        # NaN, inf and -inf inside, and on each edge that is long enough to keep clean cells beside them (on a raster two
        # cells wide one NaN in the first row would blank the whole row, and the edge rule with it)
        cells = [(m // 2, (2 * n) // 3), (m // 3, n // 3), (m // 4, n // 5)]
        cells += [(0, n // 2), (m - 1, n // 4), (m - 1, n // 2 + 3)] if n > 4 else []
        cells += [(m // 2, 0), (m // 5, n - 1), (m // 2 + 3, n - 1)] if m > 4 else []
        for k, rc in enumerate(cells):
            Z[rc] = (np.nan, np.inf, -np.inf)[k % 3]
    for h in (1.0, .5, .3, 2.5):
        with np.errstate(invalid="ignore"):
            gy, gx = np.gradient(Z, h)
            want = np.sqrt(gy ** 2 + gx ** 2)
        rc, got = _slope(lib, gpu_device, Z, h)
        assert rc == 0
        assert np.array_equal(got, want, equal_nan=True), (shape, h, int((got != want).sum()))
    assert all(np.isfinite(edge).sum() * 2 > edge.size for edge in (want[0], want[-1], want[:, 0], want[:, -1]))
    if m * n > 9:
        assert np.isnan(want).any() and np.isinf(want).any()


def test_gradient_slope_refuses_single_lines(lib, gpu_device):
    for shape in ((1, 5), (5, 1)):
        rc, got = _slope(lib, gpu_device, np.ones(shape), 1.0)
        assert rc == E_ARG and (got == -1.0).all()


# -------------------------------------------------------------------------------------------- smrf_classify_points_f64
@pytest.mark.parametrize("n", LENGTHS)
def test_classify_points(lib, gpu_device, n):
    import torch
    thr, scaler = .5, 1.25
    rng = np.random.default_rng(n)
    slope = np.abs(rng.normal(0, .4, n))
    z = rng.normal(300.0, 20.0, n)
    elev = z + rng.normal(0, 1.0, n)
    # planted, cyclically from the end: |elev - z| exactly the right-hand side (False), one ulp above (True) and one below
    # (False), on either side of z = 0 (the subtraction is then exact), and a NaN in each input (False)
    req = thr + scaler * slope
    kinds = min(n, 9)
    for i in range(min(n, 90)):
        j, kind = n - 1 - i, i % kinds
        if kind < 6:
            sign = 1.0 if kind < 3 else -1.0
            z[j] = 0.0
            elev[j] = sign * (req[j], np.nextafter(req[j], np.inf), np.nextafter(req[j], 0.0))[kind % 3]
        else:
            (elev, slope, z)[kind - 6][j] = np.nan
    with np.errstate(invalid="ignore"):
        want = np.abs(elev - z) > thr + scaler * slope
    if n >= 9:
        planted = want[n - 9:][::-1]
        assert list(planted) == [False, True, False, False, True, False, False, False, False]
    out = torch.full((n,), 7, dtype=torch.uint8, device=gpu_device)
    e_d, s_d, z_d = (dev(v, gpu_device) for v in (elev, slope, z))
    ok(lib.smrf_classify_points_f64(p(e_d), p(s_d), p(z_d), n, thr, scaler, p(out), stream()))
    assert np.array_equal(out.cpu().numpy(), want.astype(np.uint8))
    if n >= 1000:
        assert 0 < want.sum() < n


# ----------------------------------------------------------------------------------------------------- smrf_negate_f64
@pytest.mark.parametrize("n", LENGTHS)
def test_negate(lib, gpu_device, n):
    import torch
    a = np.random.default_rng(n).normal(0, 100.0, n)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1.7976931348623157e308])
    k = min(n, special.size)
    a[:k] = special[:k]
    a[n - k:] = special[:k][::-1]
    out = torch.full((n,), 7.0, dtype=torch.float64, device=gpu_device)
    a_d = dev(a, gpu_device)
    ok(lib.smrf_negate_f64(p(a_d), p(out), n, stream()))
    got = out.cpu().numpy()
    assert same_values(got, -a)
    assert np.array_equal(np.signbit(got[~np.isnan(a)]), ~np.signbit(a[~np.isnan(a)]))


# ------------------------------------------------------------------------------------------------- smrf_mask_apply_f64
@pytest.mark.parametrize("n", LENGTHS)
def test_mask_apply(lib, gpu_device, n):
    import torch
    rng = np.random.default_rng(n)
    Z = rng.normal(0, 100.0, n)
    k = min(n, 4)
    Z[:k] = np.array([np.inf, -np.inf, -0.0, 0.0])[:k]
    byte = np.array([0, 0, 0, 0, 0, 1, 2, 255], dtype=np.uint8)       # any non-zero byte sets
    masks = [byte[rng.integers(0, byte.size, n)] for _ in range(3)]
    masks[0][-1], masks[1][-1], masks[2][-1] = 0, 0, 255              # the last element: set by c alone
    masks[0][0], masks[1][0], masks[2][0] = 2, 0, 0                   # the first: by a alone
    Z_h = dev(Z, gpu_device)
    m_d = [dev(m, gpu_device) for m in masks]
    for use_b, use_c, use_u in itertools.product((False, True), repeat=3):
        want_u = (masks[0] != 0) | ((masks[1] != 0) & use_b) | ((masks[2] != 0) & use_c)
        Z_d = Z_h.clone()
        u_d = torch.full((n,), 7, dtype=torch.uint8, device=gpu_device) if use_u else None
        ok(lib.smrf_mask_apply_f64(p(Z_d), p(m_d[0]), p(m_d[1]) if use_b else None, p(m_d[2]) if use_c else None, p(u_d), n,
                                   stream()))
        got = Z_d.cpu().numpy()
        assert np.array_equal(np.isnan(got), want_u), (use_b, use_c, use_u)       # NaN exactly where the union is set
        assert same_bits(got[~want_u], Z[~want_u])                                # and the same bits elsewhere
        if use_u:
            assert np.array_equal(u_d.cpu().numpy(), want_u.astype(np.uint8))     # written as 0 / 1
    for m, m_dev in zip(masks, m_d):
        assert np.array_equal(m_dev.cpu().numpy(), m)                             # the inputs are read only


# -------------------------------------------------------------------------------- smrf_count_nan_f32, smrf_count_nan_f64
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("n", [0] + LENGTHS)
def test_count_nan(lib, gpu_device, n, dtype):
    fn = lib.smrf_count_nan_f32 if dtype is np.float32 else lib.smrf_count_nan_f64
    count = C.c_int64(-5)
    if n == 0:
        ok(fn(None, 0, C.byref(count), stream()))
        assert count.value == 0
        return
    rng = np.random.default_rng(n)
    a = rng.normal(0, 1, n).astype(dtype)
    a[rng.random(n) < .1] = np.nan
    a[rng.random(n) < .1] = np.inf                                    # not counted
    a[rng.random(n) < .05] = -np.inf
    a[0] = np.nan
    a[-1] = dtype(np.copysign(np.nan, -1.0))                          # a negative NaN, last
    if n > 2:
        a[n // 2] = dtype(np.copysign(np.nan, -1.0))
        a[1] = np.inf
    assert np.signbit(a[-1]) and np.isnan(a[-1])
    a_d = dev(a, gpu_device)
    ok(fn(p(a_d), n, C.byref(count), stream()))
    assert count.value == int(np.isnan(a).sum())
    b = np.where(np.isnan(a), dtype(1.0), a)                          # inf alone counts nothing
    b_d = dev(b, gpu_device)
    ok(fn(p(b_d), n, C.byref(count), stream()))
    assert count.value == 0 and (n < 100 or np.isinf(b).any())
