"""voxelize without a GPU: the NumPy restatement of the contract against the reference's goldens,
the public signature, the host argument checks, the ABI names and the no-fallback rule."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import voxel_numpy as vn
from conftest import ROOT, golden, unpack

ABI_NAMES = ("smrf_voxel_bounds_f32", "smrf_voxel_bounds_f64", "smrf_voxel_workspace_bytes", "smrf_voxel_mark_f32",
             "smrf_voxel_mark_f64", "smrf_voxel_expand")


@pytest.fixture(scope="module")
def G():
    return golden("voxel.npz")


def _cases(G):
    return json.loads(str(G["cases"]))


def _cloud(G, name):
    return G["x_" + name], G["y_" + name], G["z_" + name]


def test_golden_cases_are_the_ones_promised(G):
    cases = {c["name"]: c for c in _cases(G)}
    x, y, z = _cloud(G, "strip")
    assert x.dtype == np.float64 and x.shape == y.shape == z.shape == (5000,)
    assert 1000 <= x.min() and x.max() <= 1100 and 500 <= y.min() and y.max() <= 560
    assert cases["strip"]["kwargs"] == {"resolution": 50}
    varied = {k: sorted(c["kwargs"][k] for c in cases.values()
                        if c["cloud"] == "strip" and set(c["kwargs"]) == {"resolution", k} and c["kwargs"]["resolution"] == 50)
              for k in ("bottom_fill", "threshold", "ve", "pad")}
    assert varied == {"bottom_fill": [False], "threshold": [2, 3], "ve": [0.5, 2.5], "pad": [1, 3]}
    assert all(a.dtype == np.float32 for a in _cloud(G, "strip_f32")) and cases["strip_f32"]["cloud"] == "strip_f32"
    ox, oy, oz = _cloud(G, "offset")
    assert ox.min() > 5.4e6 and oy.min() > 5.1e5 and oz.min() > 250 and ox.dtype == np.float64
    tx, ty, _ = _cloud(G, "tall_y")
    assert np.ptp(ty) > np.ptp(tx)
    ex, ey, ez = _cloud(G, "on_edges")
    for v in (ex, ey, ez):                       # integer extents, several points exactly on the maximum
        assert np.ptp(v) == np.round(np.ptp(v)) and (v == v.max()).sum() >= 2
    cx, cy, _ = _cloud(G, "column")
    assert (cx != cx[0]).sum() == 1 and (cy != cy[0]).sum() == 1
    assert cases["resolution_1"]["kwargs"]["resolution"] == 1 and tuple(G["shape_resolution_1"]) == (1, 1, 1)
    assert str(G["numpy_version"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "voxel.npz")) < 600 * 1024


def test_restatement_equals_every_golden(G):
    """exact equality of the whole volume, every case"""
    for c in _cases(G):
        kw = dict(c["kwargs"])
        H = vn.voxelize(None, *_cloud(G, c["cloud"]), kw.pop("resolution"), **kw)
        want = unpack(G["bits_" + c["name"]], tuple(G["shape_" + c["name"]]))
        assert H.dtype == bool and H.flags.c_contiguous and H.shape == want.shape, (c["name"], H.shape, want.shape)
        assert np.array_equal(H, want), (c["name"], int((H != want).sum()))


def test_restatement_pieces():
    """the bin rule and the fill on inputs small enough to check by eye"""
    e = np.array([0.0, 1.0, 2.5, 2.5, 4.0])
    d = np.array([-1e-9, 0.0, 0.999, 1.0, 2.5, 3.999, 4.0, 4.000001, np.nextafter(4.0, 0)])
    assert list(vn.bins_of(e, d)) == [-1, 0, 0, 1, 3, 3, 3, -1, 3]
    assert list(vn.bins_of(np.array([0.0]), np.array([0.0, 1.0]))) == [-1, -1]          # one edge: no bin
    counts = np.zeros((1, 3, 5), dtype=np.int64)
    counts[0, 0, [2, 4]] = 1
    counts[0, 1, 0] = 3
    H = vn.solid(counts, 1, True, 2)
    assert H.shape == (1, 3, 7)
    assert H[0].astype(int).tolist() == [[1, 1, 1, 1, 1, 0, 1], [1, 1, 1, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0]]
    assert vn.solid(counts, 2, True, 0)[0].astype(int).tolist() == [[0] * 5, [1, 0, 0, 0, 0], [0] * 5]
    assert vn.solid(counts, 1, False, 0)[0, 0].astype(int).tolist() == [0, 0, 1, 0, 1]


def test_signature_equals_the_reference(G):
    import neilpy_amd as na
    want = json.loads(str(G["signature"]))
    assert [p["name"] for p in want] == ["filename", "x", "y", "z", "resolution", "bottom_fill", "threshold", "material",
                                         "ve", "pad"]
    got = list(inspect.signature(na.voxelize).parameters.values())
    for p, g in zip(want, got):
        assert (g.name, g.kind.name) == (p["name"], p["kind"]), (g, p)
        assert (None if g.default is inspect.Parameter.empty else repr(g.default)) == p["default"], (g, p)
    extra = got[len(want):]
    assert [g.name for g in extra] == ["return_edges"] and all(g.kind is inspect.Parameter.KEYWORD_ONLY for g in extra)
    assert extra[0].default is False


def test_host_argument_checks():
    """every deviation that can be seen from the arguments raises before the library or a GPU is needed"""
    import torch
    import neilpy_amd as na
    x, y, z = np.arange(5.0), np.arange(5.0) * 2, np.ones(5)
    for bad in (0, -3, 2.0, 2.5, "4", None):
        with pytest.raises(ValueError, match="resolution"):
            na.voxelize(None, x, y, z, bad)
    for bad in (0, -1, 1.0, 1.5):
        with pytest.raises(ValueError, match="threshold"):
            na.voxelize(None, x, y, z, 4, threshold=bad)
        with pytest.raises(ValueError, match="threshold"):
            na.voxelize(None, x, y, z, 4, True, bad)
    for bad in (-1, 1.0, 0.5):
        with pytest.raises(ValueError, match="pad"):
            na.voxelize(None, x, y, z, 4, pad=bad)
    for bad in (0, 0.0, -1, -0.5, float("nan"), float("inf"), "tall", None):
        with pytest.raises(ValueError, match="ve"):
            na.voxelize(None, x, y, z, 4, ve=bad)
    for bad in (np.zeros((5, 1)), np.zeros((1, 5)), np.float64(3.0), np.zeros((5, 2))):
        for args in ((bad, y, z), (x, bad, z), (x, y, bad)):
            with pytest.raises(ValueError, match="1-D"):
                na.voxelize(None, *args, 4)
    for args in ((x[:4], y, z), (x, y[:3], z), (x, y, z[:1])):
        with pytest.raises(ValueError, match="differ in length"):
            na.voxelize(None, *args, 4)
    with pytest.raises(ValueError, match="empty"):
        na.voxelize(None, x[:0], y[:0], z[:0], 4)
    with pytest.raises(ValueError, match="empty"):
        na.voxelize(None, torch.zeros(0), torch.zeros(0), torch.zeros(0), 4)
    with pytest.raises(ValueError, match="1-D"):
        na.voxelize(None, torch.zeros((3, 2)), torch.zeros(3), torch.zeros(3), 4)
    huge = np.broadcast_to(np.float64(1.0), (2 ** 31,))           # 2**31 points that take no memory
    with pytest.raises(ValueError, match=r"2\*\*31 - 1"):
        na.voxelize(None, huge, huge, huge, 4)
    # np.integer values are integers; a bool threshold is not worth an error
    for kw in (dict(resolution=np.int64(0)), dict(resolution=4, pad=np.int32(-2))):
        with pytest.raises(ValueError):
            na.voxelize(None, x, y, z, **kw)


def test_filename_is_refused():
    import neilpy_amd as na
    x = np.arange(5.0)
    for name in ("a.stl", b"a.stl", 0, ""):
        with pytest.raises(NotImplementedError):
            na.voxelize(name, x, x, x, 4)
    with pytest.raises(NotImplementedError):                      # before anything else is looked at
        na.voxelize("a.stl", None, None, None, -1)


def test_edges_on_the_host():
    """bin_edges(), the host half of the public function: the restatement's edges from the cloud's box alone, bit for bit,
    for both dtypes, and the zero-extent refusal"""
    from neilpy_amd.voxel import bin_edges
    rng = np.random.default_rng(15)
    for T in (np.float64, np.float32):
        x, y, z = (rng.uniform(lo, hi, 500).astype(T) for lo, hi in ((5.4e6, 5.4e6 + 91.3), (100, 143.7), (3, 20.2)))
        box = [float(v) for a in (x, y, z) for v in (a.min(), a.max())]
        for resolution, ve in ((1, 1), (7, 0.5), (33, 2.5), (100, 1), (1000, 3)):
            edges, mins = bin_edges(box, T, resolution, float(ve))
            want, wmins, _ = vn.edges_of(x, y, z, resolution, ve)
            for a, b in zip(edges, want):
                assert a.dtype == np.float64 and a.tobytes() == b.tobytes(), (T, resolution, ve)
            assert all(type(m) is T and m == w for m, w in zip(mins, wmins))
    with pytest.raises(ValueError, match="no extent"):
        bin_edges([3.0, 3.0, -1.0, -1.0, 0.0, 9.0], np.float64, 4, 1.0)
    edges, _ = bin_edges([3.0, 3.0, -1.0, 1.0, 2.0, 2.0], np.float64, 4, 1.0)      # one axis flat: no bins on it
    assert [len(e) - 1 for e in edges] == [0, 4, 0]


def test_abi_names_declared():
    from neilpy_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from neilpy_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "smrf_hip.h")).read()
    for n in ABI_NAMES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
        assert re.search(r"^SMRF_API [\w \*]*?\b%s\(" % n, hdr, flags=re.M), n
        assert _lib.SIGNATURES[n][1][-1] is ctypes.c_void_p or n == "smrf_voxel_workspace_bytes"       # trailing stream
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("smrf_voxel_")) == sorted(ABI_NAMES)
    assert _lib.load().smrf_abi_version() == 1 and "#define SMRF_ABI_VERSION 1" in hdr
    from neilpy_amd import voxel
    assert re.search(r"^#define SMRF_VOXEL_BOUNDS_BYTES %d$" % voxel.BOUNDS_BYTES, hdr, flags=re.M)
    # the workspace query is host code: 1/8 B per voxel as a bit set, 4 B per voxel as counts, 4 B per column, 0 out of range
    fn = _lib.load().smrf_voxel_workspace_bytes
    assert fn(-1, 2, 2, 1) == 0 and fn(2, 2, -1, 1) == 0 and fn(2, 2, 2, 0) == 0 and fn(1 << 20, 1 << 20, 64, 1) == 0
    assert fn(0, 5, 5, 1) > 0 and fn(5, 5, 0, 2) > 0
    nx, ny, nz = 1024, 1024, 4096
    cols, slack = nx * ny, 1024
    assert cols * (nz // 8 + 4) <= fn(nx, ny, nz, 1) <= cols * (nz // 8 + 4) + slack
    assert cols * (nz * 4 + 4) <= fn(nx, ny, nz, 2) <= cols * (nz * 4 + 4) + slack
    assert fn(nx, ny, nz, 2) == fn(nx, ny, nz, 7)
    assert fn(10, 10, 33, 1) >= 100 * 2 * 4 + 100 * 4                                # 33 levels take two words


def test_no_cpu_fallback():
    import torch
    import neilpy_amd as na
    x = np.arange(5.0)
    if not torch.cuda.is_available():
        for call in (lambda: na.voxelize(None, x, x, x, 4), lambda: na.voxelize(None, x.astype(np.float32), x, x, 2, pad=1),
                     lambda: na.voxelize(None, x, x, x, 4, return_edges=True)):
            with pytest.raises(na.SmrfHipError):
                call()
    src = open(os.path.join(ROOT, "neilpy_amd", "voxel.py")).read()
    assert "histogramdd(" not in src and "bincount" not in src and "searchsorted" not in src
