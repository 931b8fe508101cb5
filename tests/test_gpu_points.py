"""nearest_points / chamfer_distance on the device against the brute-force restatement (tests/points_numpy.py) and the
reference's goldens (tests/golden/points.npz).  DESIGN.md section 14.

Every nearest_points case is compared on bits, ``dist`` and ``index``, for every query point.  The restatement is exact
by construction, so it alone decides."""
import json

import numpy as np
import pytest

import points_numpy as pn
from conftest import golden

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257)
DIRECTIONS = ("y_to_x", "x_to_y", "bi")


@pytest.fixture(scope="module")
def G():
    return golden("points.npz")


def check(query, points):
    """nearest_points equals the restatement bit for bit at every query point; returns the device's result"""
    import neilpy_amd as na
    dist, index = na.nearest_points(query, points)
    wd, wi = pn.nearest_points(query, points)
    assert isinstance(dist, np.ndarray) and isinstance(index, np.ndarray)
    assert dist.dtype == np.float64 and index.dtype == np.int64 and dist.shape == wd.shape and index.shape == wi.shape
    bad = np.flatnonzero((index != wi) | (dist.view(np.uint64) != wd.view(np.uint64)))
    assert bad.size == 0, "%d of %d differ, first at %d: got (%r, %d), want (%r, %d)" % (
        bad.size, wd.size, bad[0], dist[bad[0]], index[bad[0]], wd[bad[0]], wi[bad[0]])
    return dist, index


def degenerate_cases():
    """{name: (query, points)}: the shapes of cloud at which a cell index, a ring bound or the tie rule can go wrong"""
    rng = np.random.default_rng(141)
    out = {}
    # all points equal: a zero-extent box, one cell
    p = np.tile(np.array([[12.5, -3.25, 7.0]]), (100, 1))
    out["all_equal"] = (np.vstack([rng.uniform(-50, 50, (200, 3)), p[:1]]), p)
    out["all_equal_2d"] = (np.vstack([rng.uniform(-50, 50, (200, 2)), p[:1, :2]]), p[:, :2])
    # all points on one line parallel to an axis: one axis of the box has no extent
    t = rng.uniform(0, 300, 300)
    for name, line in (("line_x", np.column_stack([t, np.full(300, 5.0)])), ("line_y", np.column_stack([np.full(300, -2.0), t]))):
        q = np.vstack([rng.uniform(-20, 320, (300, 2)), line[::7], line[::11] + np.array([0.0, 1e-9])])
        out[name] = (q, line)
        # the same cloud with one point 10**6 units away: the box is stretched until nearly all points share one cell
        far = np.vstack([line, [[1e6, 1e6]]])
        out[name + "_outlier"] = (np.vstack([q, [[1e6, 1e6 - 1.0], [5e5, 5e5]]]), far)
    cloud = rng.uniform(0, 100, (400, 3))
    out["cloud_outlier"] = (rng.uniform(-10, 110, (300, 3)), np.vstack([cloud, [[1e6, -1e6, 0.0]]]))
    # each point three times, queries the points: distance 0, the lowest of the three rows
    base = rng.uniform(0, 50, (200, 3))
    out["triple"] = (base, np.tile(base, (3, 1)))
    base2 = rng.uniform(0, 50, (200, 2))
    perm = rng.permutation(600)
    out["triple_shuffled_2d"] = (base2, np.tile(base2, (3, 1))[perm])
    # an integer lattice in shuffled row order, queries at cell centres (four-way ties) and edge midpoints (two-way):
    # equal float distances, many across cell borders
    ii, jj = np.meshgrid(np.arange(40.0), np.arange(40.0), indexing="ij")
    lattice = np.column_stack([ii.ravel(), jj.ravel()])[rng.permutation(1600)]
    ci, cj = np.meshgrid(np.arange(39.0), np.arange(39.0), indexing="ij")
    centres = np.column_stack([ci.ravel() + 0.5, cj.ravel() + 0.5])
    mid_a = np.column_stack([ci.ravel() + 0.5, cj.ravel()])
    mid_b = np.column_stack([ci.ravel(), cj.ravel() + 0.5])
    out["lattice"] = (np.vstack([centres, mid_a, mid_b]), lattice)
    out["lattice_3d"] = (np.column_stack([np.vstack([centres, mid_a]), np.full(2 * 39 * 39, 0.25)]),
                         np.column_stack([lattice, np.zeros(1600)]))
    # two clusters 10**4 units apart: queries halfway between walk many rings of empty cells
    a, b = rng.normal(0, 5, (500, 2)), rng.normal(0, 5, (500, 2)) + np.array([1e4, 0.0])
    q = np.vstack([rng.normal(0, 20, (100, 2)) + np.array([5e3, 0.0]), np.array([[5e3, 0.0], [5e3, 40.0]]),
                   rng.normal(0, 5, (100, 2)), rng.normal(0, 5, (100, 2)) + np.array([1e4, 0.0])])
    out["two_clusters"] = (q, np.vstack([a, b]))
    # queries far outside the box on every side and at its corners, and exactly on its corners
    p = rng.uniform(0, 100, (1000, 2))
    lo, hi = p.min(axis=0), p.max(axis=0)
    far = [[-1e3, 50], [1e3, 50], [50, -1e3], [50, 1e3], [-1e6, -1e6], [1e6, 1e6], [-1e6, 1e6], [1e6, -1e6],
           [-1e6, 50], [50, 1e6], [hi[0], hi[1]], [lo[0], lo[1]], [hi[0], lo[1]], [lo[0], hi[1]], [hi[0], 50], [50, hi[1]],
           [np.nextafter(hi[0], np.inf), np.nextafter(hi[1], np.inf)]]
    out["outside"] = (np.vstack([np.array(far, dtype=np.float64), rng.uniform(-300, 400, (300, 2))]), p)
    p3 = np.column_stack([p, rng.uniform(0, 5, 1000)])
    out["outside_3d"] = (np.column_stack([np.array(far, dtype=np.float64), np.linspace(-50, 50, len(far))]), p3)
    return out


@pytest.mark.parametrize("d", [2, 3])
def test_small_sizes_crossed(gpu_device, d):
    """np, nq in {1, 2, 63, 64, 65, 257}, crossed: one point, one cell, the wave boundary, more than one workgroup"""
    rng = np.random.default_rng(100 + d)
    for n_p in SIZES:
        for n_q in SIZES:
            p = rng.uniform(0, 10, (n_p, d))
            q = rng.uniform(-1, 11, (n_q, d))
            check(q, p)


@pytest.mark.parametrize("name", sorted(degenerate_cases()))
def test_degenerate_clouds(gpu_device, name):
    query, points = degenerate_cases()[name]
    dist, index = check(query, points)
    if name.startswith("triple"):
        assert (dist == 0.0).all()
        if name == "triple":
            assert np.array_equal(index, np.arange(200))             # rows i, i + 200, i + 400 hold point i
    if name.startswith("lattice"):
        assert (np.unique(dist).size <= 3)                            # sqrt(0.5), 0.5 and their 3-D versions


def test_offset_cloud(gpu_device, G):
    """the 3-D golden clouds offset by (5.4e6, 5.1e5, 300): 23 bits of the mantissa gone to the offset"""
    x, y = G["x_flat3d_offset"], G["y_flat3d_offset"]
    assert x.min() > 3e2 and x[:, 0].min() > 5e6
    check(y, x)
    check(x, y)


@pytest.fixture(scope="module")
def big():
    """{d: (query, points, restatement dist, restatement index)} at 20000 x 20000: many workgroups, many cells"""
    out = {}
    for d in (2, 3):
        rng = np.random.default_rng(2000 + d)
        p = rng.uniform(0, 1000, (20000, d))
        q = rng.uniform(-5, 1005, (20000, d))
        if d == 3:
            p[:, 2] *= 0.05
            q[:, 2] *= 0.05
        out[d] = (q, p) + pn.nearest_points(q, p)
    return out


@pytest.mark.parametrize("d", [2, 3])
def test_20000_points(gpu_device, big, d):
    import neilpy_amd as na
    q, p, wd, wi = big[d]
    dist, index = na.nearest_points(q, p)
    assert pn.same_bits(dist, wd) and pn.same_bits(index, wi), int(((index != wi) | (dist != wd)).sum())
    assert np.unique(index).size > 5000


def test_deterministic(gpu_device, big):
    """five runs of the 20000-point case: the same dist, index and chamfer bits (the sort's atomics decide nothing, the sum
    has a fixed order)"""
    import neilpy_amd as na
    q, p, wd, wi = big[3]
    values = set()
    for _ in range(5):
        dist, index = na.nearest_points(q, p)
        assert pn.same_bits(dist, wd) and pn.same_bits(index, wi)
        values.add(na.chamfer_distance(q, p).tobytes())
    assert len(values) == 1


def _bound(r, g, n):
    """any summation order over n non-negative terms: |r - g| <= n * 2**-53 * g"""
    return abs(r - g) <= n * 2.0 ** -53 * g


def test_chamfer_goldens(gpu_device, G):
    import neilpy_amd as na
    cases = [c["name"] for c in json.loads(str(G["cases"]))]
    assert set(cases) >= {"uniform2d", "flat3d", "flat3d_offset", "f32", "equal"}
    for name in cases:
        x, y, want = G["x_" + name], G["y_" + name], G["cd_" + name]
        n = max(len(x), len(y))
        for k, direction in enumerate(DIRECTIONS):
            r = na.chamfer_distance(x, y, direction=direction)
            print(name, direction, repr(r), repr(want[k]), abs(r - want[k]))
            assert type(r) is np.float64, (name, direction, type(r))
            assert _bound(r, want[k], n), (name, direction, r, want[k])
        assert _bound(na.chamfer_distance(x, y), want[2], n)                  # the defaults: 'l2', 'bi'
        assert na.chamfer_distance(x, y, 'euclidean', 'x_to_y') == na.chamfer_distance(x, y, 'l2', 'x_to_y')


def test_chamfer_equal_clouds(gpu_device, G):
    import neilpy_amd as na
    x = G["x_equal"]
    for direction in DIRECTIONS:
        r = na.chamfer_distance(x, G["y_equal"], direction=direction)
        assert type(r) is np.float64 and r == 0.0
        assert na.chamfer_distance(x, x, direction=direction) == 0.0


def test_dtypes_and_tensors(gpu_device, G):
    """float32, integer and CUDA-tensor input give what float64 NumPy input gives; tensors in, tensors out"""
    import torch
    import neilpy_amd as na
    x32, y32 = G["x_f32"], G["y_f32"]
    assert x32.dtype == np.float32
    x64, y64 = x32.astype(np.float64), y32.astype(np.float64)
    want = [na.chamfer_distance(x64, y64, direction=d) for d in DIRECTIONS]
    wd, wi = check(y64, x64)
    for d, w in zip(DIRECTIONS, want):
        assert na.chamfer_distance(x32, y32, direction=d).tobytes() == w.tobytes()
        for xt, yt in ((torch.from_numpy(x64).to(gpu_device), torch.from_numpy(y64).to(gpu_device)),
                       (torch.from_numpy(x32).to(gpu_device), torch.from_numpy(y32).to(gpu_device))):
            r = na.chamfer_distance(xt, yt, direction=d)
            assert type(r) is np.float64 and r.tobytes() == w.tobytes()
    dist, index = na.nearest_points(y32, x32)
    assert pn.same_bits(dist, wd) and pn.same_bits(index, wi)
    td, ti = na.nearest_points(torch.from_numpy(y32).to(gpu_device), torch.from_numpy(x32).to(gpu_device))
    assert td.is_cuda and ti.is_cuda and td.dtype == torch.float64 and ti.dtype == torch.int64
    assert td.device == gpu_device and pn.same_bits(td.cpu().numpy(), wd) and pn.same_bits(ti.cpu().numpy(), wi)
    rng = np.random.default_rng(5)
    pi, qi = rng.integers(-40, 40, (300, 2)), rng.integers(-50, 50, (200, 2))
    dist, index = na.nearest_points(qi, pi)
    wd, wi = pn.nearest_points(qi, pi)
    assert pn.same_bits(dist, wd) and pn.same_bits(index, wi)
    dist, index = na.nearest_points(torch.from_numpy(qi).to(gpu_device), pi.astype(np.int32))
    assert pn.same_bits(dist.cpu().numpy(), wd) and pn.same_bits(index.cpu().numpy(), wi)


def test_layouts(gpu_device):
    """a non-contiguous slice and a Fortran-ordered (n, d) array give the contiguous result"""
    import torch
    import neilpy_amd as na
    rng = np.random.default_rng(9)
    wide_p, wide_q = rng.uniform(0, 60, (700, 5)), rng.uniform(0, 60, (1200, 6))
    p, q = wide_p[::2, 1:4], wide_q[::3, ::2]
    assert not p.flags.c_contiguous and not q.flags.c_contiguous
    wd, wi = check(np.ascontiguousarray(q), np.ascontiguousarray(p))
    want = na.chamfer_distance(np.ascontiguousarray(q), np.ascontiguousarray(p))
    for qq, pp in ((q, p), (np.asfortranarray(q), np.asfortranarray(p))):
        dist, index = na.nearest_points(qq, pp)
        assert pn.same_bits(dist, wd) and pn.same_bits(index, wi)
        assert na.chamfer_distance(qq, pp).tobytes() == want.tobytes()
    tq, tp = torch.from_numpy(wide_q).to(gpu_device)[::3, ::2], torch.from_numpy(wide_p).to(gpu_device)[::2, 1:4]
    assert not tq.is_contiguous()
    dist, index = na.nearest_points(tq, tp)
    assert pn.same_bits(dist.cpu().numpy(), wd) and pn.same_bits(index.cpu().numpy(), wi)
    assert na.chamfer_distance(tq, tp).tobytes() == want.tobytes()


def test_nonfinite_coordinates_raise(gpu_device):
    import neilpy_amd as na
    good = np.random.default_rng(3).uniform(0, 1, (50, 3))
    for value in (np.nan, np.inf, -np.inf):
        for col in (0, 2):
            bad = good.copy()
            bad[17, col] = value
            for call in (lambda: na.nearest_points(bad, good), lambda: na.nearest_points(good, bad),
                         lambda: na.chamfer_distance(bad, good), lambda: na.chamfer_distance(good, bad, direction='x_to_y')):
                with pytest.raises(ValueError, match="NaN or infinite"):
                    call()
