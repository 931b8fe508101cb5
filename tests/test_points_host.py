"""nearest_points / chamfer_distance without a GPU: the NumPy restatement of the contract against
the reference's goldens and scikit-learn's KD-tree, the host argument checks, the signature, the ABI names, the no-fallback
rule and the generated code of csrc/points.hip."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import points_numpy as pn
from conftest import ROOT, golden
from family_checks import assert_no_scratch, device_asm

DIRECTIONS = ("y_to_x", "x_to_y", "bi")
ABI_NAMES = ("smrf_points_nn_workspace_bytes", "smrf_points_nn_bounds_f64", "smrf_points_nn_build_f64",
             "smrf_points_nn_search_f64", "smrf_points_nn_sum_f64")


@pytest.fixture(scope="module")
def G():
    return golden("points.npz")


def _names(G):
    return [c["name"] for c in json.loads(str(G["cases"]))]


def test_golden_cases_are_the_ones_promised(G):
    assert _names(G) == ["uniform2d", "flat3d", "flat3d_offset", "f32", "equal"]
    assert G["x_uniform2d"].shape == (3000, 2) and G["y_uniform2d"].shape == (2500, 2)
    x, y = G["x_flat3d"], G["y_flat3d"]
    assert x.shape == (3000, 3) and y.shape == (2500, 3) and np.ptp(x[:, 2]) < 0.051 * np.ptp(x[:, 0])
    off = G["x_flat3d_offset"] - x
    assert np.allclose(off, [5.4e6, 5.1e5, 300.0], rtol=0, atol=1e-6) and G["x_flat3d_offset"].dtype == np.float64
    assert G["x_f32"].dtype == np.float32 and G["y_f32"].dtype == np.float32
    assert np.array_equal(G["x_equal"], G["y_equal"])
    assert set(json.loads(str(G["result_types"])).values()) == {"numpy.float64"}      # also for the float32 pair
    assert json.loads(str(G["raises"])) == {"direction": "ValueError", "empty": "ValueError"}
    assert str(G["sklearn_version"]) and str(G["numpy_version"])


def test_restatement_equals_every_golden(G):
    """exact equality, all five cloud pairs, all three directions"""
    for name in _names(G):
        x, y, want = G["x_" + name], G["y_" + name], G["cd_" + name]
        assert want.dtype == np.float64 and want.shape == (3,)
        for k, direction in enumerate(DIRECTIONS):
            got = pn.chamfer_distance(x, y, direction=direction)
            assert type(got) is np.float64 and got == want[k], (name, direction, got, want[k])
    assert (G["cd_equal"] == 0.0).all()


def test_restatement_distances_equal_sklearn(G):
    """per point, bit for bit, against the KD-tree query the reference makes"""
    from sklearn.neighbors import NearestNeighbors
    for name in _names(G):
        x, y = G["x_" + name], G["y_" + name]
        for q, p in ((y, x), (x, y)):
            nn = NearestNeighbors(n_neighbors=1, leaf_size=1, algorithm='kd_tree', metric='l2').fit(p)
            d, i = nn.kneighbors(q)
            dist, index = pn.nearest_points(q, p)
            assert pn.same_bits(d[:, 0], dist), name
            if name != "equal":                      # no ties in the random clouds: the same neighbour
                assert np.array_equal(i[:, 0], index), name


def test_restatement_tie_rule():
    p = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [0.0, 1.0]])
    dist, index = pn.nearest_points(np.array([[0.0, 0.0], [0.0, 0.9], [0.5, 0.5]]), p[::-1])
    assert list(index) == [0, 0, 0] and dist[0] == 1.0           # row 0 of the reversed cloud is (0, 1)
    dist, index = pn.nearest_points(np.array([[0.0, 0.0]]), p[[2, 0, 1]])
    assert index[0] == 0


def test_host_argument_checks():
    """every check the host makes raises ValueError before the library or a GPU is needed"""
    import neilpy_amd as na
    x, y = np.zeros((5, 2)), np.ones((4, 2))
    with pytest.raises(ValueError, match="metric"):
        na.chamfer_distance(x, y, metric='l1')
    with pytest.raises(ValueError, match="metric"):
        na.chamfer_distance(x, y, 'manhattan', 'bi')
    with pytest.raises(ValueError, match="direction"):
        na.chamfer_distance(x, y, direction='both')
    with pytest.raises(ValueError, match="direction"):
        na.chamfer_distance(x, y, 'l2', 'y_x')
    for bad in (np.zeros((5, 1)), np.zeros((5, 4)), np.zeros(5), np.zeros((2, 2, 2))):
        for call in (lambda: na.chamfer_distance(bad, y), lambda: na.chamfer_distance(x, bad),
                     lambda: na.nearest_points(bad, y), lambda: na.nearest_points(x, bad)):
            with pytest.raises(ValueError):
                call()
    for call in (lambda: na.chamfer_distance(x[:0], y), lambda: na.chamfer_distance(x, y[:0], direction='x_to_y'),
                 lambda: na.nearest_points(x[:0], y), lambda: na.nearest_points(x, y[:0])):
        with pytest.raises(ValueError, match="empty"):
            call()
    with pytest.raises(ValueError, match="dimension"):
        na.nearest_points(np.zeros((5, 3)), y)
    with pytest.raises(ValueError, match="dimension"):
        na.chamfer_distance(x, np.zeros((5, 3)))
    import torch
    with pytest.raises(ValueError, match="empty"):
        na.nearest_points(torch.zeros((0, 3)), torch.zeros((4, 3)))
    with pytest.raises(ValueError):
        na.chamfer_distance(torch.zeros((3, 5)), torch.zeros((4, 5)))


def test_signatures():
    import neilpy_amd as na
    ps = list(inspect.signature(na.chamfer_distance).parameters.values())
    assert [(p.name, p.default) for p in ps] == [("x", inspect.Parameter.empty), ("y", inspect.Parameter.empty),
                                                 ("metric", "l2"), ("direction", "bi")]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in ps)
    assert list(inspect.signature(na.nearest_points).parameters) == ["query", "points"]


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
        assert _lib.SIGNATURES[n][1][-1] is ctypes.c_void_p or n == "smrf_points_nn_workspace_bytes"   # trailing stream
    assert _lib.load().smrf_abi_version() == 1 and "#define SMRF_ABI_VERSION 1" in hdr
    # the workspace query is host code: nothing for arguments out of range, 40 KB of partials plus the grid otherwise
    fn = _lib.load().smrf_points_nn_workspace_bytes
    assert fn(0, 2) == 0 and fn(10, 1) == 0 and fn(10, 4) == 0 and fn((1 << 30) + 1, 3) == 0
    assert fn(1, 2) >= 1024 * 5 * 8
    n = 10 ** 7
    assert n * (3 * 8 + 4) < fn(n, 3) < n * (3 * 8 + 4 + 14) and fn(n, 2) < fn(n, 3)


def test_no_cpu_fallback():
    import torch
    import neilpy_amd as na
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x, y = np.zeros((5, 2)), np.ones((4, 2))
    for call in (lambda: na.nearest_points(x, y), lambda: na.chamfer_distance(x, y),
                 lambda: na.chamfer_distance(x.astype(np.float32), y.astype(np.int64), 'euclidean', 'y_to_x')):
        with pytest.raises(na.SmrfHipError):
            call()


def test_points_kernels_compile_without_scratch(tmp_path):
    """every kernel of csrc/points.hip keeps its state in registers, the squares and sums of the distance stay separate
    instructions, and the only atomics are the sort's integer counters (no GPU needed)"""
    text, kernels = device_asm("points", tmp_path)
    names = sorted(kernels)
    assert len(names) == 10, names     # bounds x 2 dimensions, count, scan x 3, scatter, search x 2 dimensions, sum
    for stem, n in (("cloud_bounds_kernel", 2), ("points_count_kernel", 1), ("points_scan_", 3),
                    ("points_scatter_kernel", 1), ("points_search_kernel", 2), ("points_sum_kernel", 1)):
        assert sum(stem in k for k in names) == n, (stem, names)
    assert_no_scratch(text, kernels)
    for name, body in kernels.items():
        if "points_search_kernel" in name:
            assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) == 0, name
    atomics = set(re.findall(r"^\s*((?:global|flat|buffer|ds)_atomic\w*)", text, re.M))
    assert atomics and all(re.fullmatch(r"global_atomic_(add|sub)(_u32)?", a) for a in atomics), atomics
    # the search kernels' code: the distance is formed with separate v_mul_f64 / v_add_f64 (the fused multiply-adds that
    # remain belong to the division and square-root expansions)
    for name in names:
        if "points_search_kernel" in name:
            at = text.index("\n%s:" % name)
            body = text[at:text.index(".end_amdhsa_kernel", at)]
            assert "v_mul_f64" in body and "v_add_f64" in body, name
