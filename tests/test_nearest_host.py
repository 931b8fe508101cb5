"""Nearest-source infill without a GPU: the NumPy restatement of the contract against the
reference's goldens and SciPy's exact distance transform, the signature, the ABI exports, the no-fallback rule and the
generated code of csrc/nearest.hip."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import nearest_numpy as nn
from conftest import ROOT, golden
from family_checks import assert_no_scratch, device_asm, signatures_match


@pytest.fixture(scope="module")
def G():
    return golden("nearest.npz")


def _cases(G):
    return json.loads(str(G["cases"]))


def restatement_cases():
    """rasters the reference cannot run (it only accepts squares) and the degenerate ones: {name: raster}"""
    rng = np.random.default_rng(7)
    out = {}

    def holes(shape, share, dtype=np.float64):
        X = (rng.normal(size=shape) * 5 + 100).astype(dtype)
        X[rng.random(shape) < share] = np.nan
        return X
    out["r7x19"] = holes((7, 19), 0.4)
    out["r23x5_f32"] = holes((23, 5), 0.6, np.float32)
    out["row1x17"] = holes((1, 17), 0.5)
    out["col17x1"] = holes((17, 1), 0.5)
    out["one_hole"] = np.array([[np.nan]])
    out["one_source"] = np.array([[2.5]])
    out["allhole"] = np.full((5, 9), np.nan)
    out["nohole"] = holes((6, 4), 0.0)
    X = holes((12, 15), 0.97)
    X[3, 4] = np.inf
    X[9, 2] = -np.inf
    X[0, 0] = -0.0
    out["sparse_inf"] = X
    X = np.full((9, 11), np.nan)
    X[8, 10] = 4.0
    out["corner_source"] = X
    return out


def test_restatement_reproduces_the_reference(G):
    """every hole of every golden case: a hole with one nearest source has the reference's bits; a tied hole has the value
    of some source at the minimal distance in the reference's result"""
    n_unique = 0
    for c in _cases(G):
        X, want = G["in_" + c["name"]], G["out_" + c["name"]]
        assert want.dtype == X.dtype and want.shape == X.shape, c
        if X.dtype.kind != "f":
            assert np.array_equal(want, X), c
            continue
        got = nn.inpaint_nearest(X)
        _, dist2, nties = nn.feature_transform(X)
        hole = ~np.isfinite(X)
        assert nn.same_bits(got[~hole], X[~hole]) and nn.same_bits(want[~hole], X[~hole]), c
        if not (~hole).any():
            assert nn.same_bits(got, X) and nn.same_bits(want, X), c       # no source: unchanged, as the reference
            continue
        untied = hole & (nties == 1)
        assert nn.same_bits(got[untied], want[untied]), c
        n_unique += int(untied.sum())
        for r, col, values in nn.candidates(X, dist2):
            assert (values == want[r, col]).any(), (c, r, col)
            assert (values == got[r, col]).any(), (c, r, col)
    assert n_unique > 3000


def test_golden_cases_carry_their_condition(G):
    """the bit-for-bit clause only counts where enough holes are untied: at least half in every case marked for it"""
    cases = _cases(G)
    marked = [c for c in cases if c["unique"]]
    assert {c["name"] for c in marked} >= {"blocks96", "blocks96_f32", "sparse48", "sparse48_f32"}
    for c in marked:
        X = G["in_" + c["name"]]
        hole = ~np.isfinite(X)
        _, _, nties = nn.feature_transform(X)
        assert hole.sum() > 1000 and (nties[hole] == 1).mean() >= 0.5, c
        assert np.isposinf(X).sum() == 1, c
    assert G["in_blocks96"].shape == (96, 96) and np.isnan(G["in_blocks96"][10:40, 20:70]).all()
    assert np.isnan(G["in_blocks96"][60:96, 0:17]).all()
    assert G["in_blocks96_f32"].dtype == np.float32 and G["out_blocks96_f32"].dtype == np.float32
    X = G["in_scatter64"]
    _, _, nties = nn.feature_transform(X)
    assert (nties[~np.isfinite(X)] == 1).mean() < 0.5                       # the valid-choice clause only
    assert np.isneginf(X).any() and np.signbit(X[40, 40]) and X[40, 40] == 0
    # the reference's behaviour at the edges of the contract, recorded
    assert np.isnan(G["out_allnan8"]).all()
    assert G["out_int8x8"].dtype == np.int64 and np.array_equal(G["out_int8x8"], G["in_int8x8"])
    assert nn.same_bits(G["out_nohole8"], G["in_nohole8"])
    assert all(json.loads(str(G["returns_argument"])).values())             # it returns the array it was given


def test_reference_is_square_only():
    """np.meshgrid's 'xy' indexing gives (cols, rows) planes: the reference's mask of another shape does not fit them"""
    X = np.zeros((3, 5))
    RI, CI = np.meshgrid(np.arange(X.shape[0]), np.arange(X.shape[1]))
    assert RI.shape == (5, 3)
    with pytest.raises(IndexError):
        RI[np.isfinite(X)]


def test_restatement_distances_equal_scipy(G):
    """squared distances against scipy.ndimage.distance_transform_edt, on the goldens and on the restatement's own
    cases; the index plane points at a source at that distance"""
    rasters = {c["name"]: G["in_" + c["name"]] for c in _cases(G) if G["in_" + c["name"]].dtype.kind == "f"}
    rasters.update(restatement_cases())
    for name, X in rasters.items():
        finite = np.isfinite(X)
        index, dist2, _ = nn.feature_transform(X)
        if not finite.any():
            assert (index == -1).all() and (dist2 == nn.NO_SOURCE_DIST2).all(), name
            assert nn.same_bits(nn.inpaint_nearest(X), X), name
            continue
        edt = ndimage.distance_transform_edt(~finite)
        assert np.array_equal(np.rint(edt ** 2).astype(np.int64), dist2), name
        r, c = np.divmod(index, X.shape[1])
        rr, cc = np.mgrid[0:X.shape[0], 0:X.shape[1]]
        assert finite[r, c].all() and np.array_equal((r - rr) ** 2 + (c - cc) ** 2, dist2), name
        assert nn.same_bits(nn.inpaint_nearest(X), X[r, c]), name


def test_restatement_tie_rule():
    """an isolated hole has four sources at distance 1: the upper one wins; in a row, the left one"""
    X = np.arange(9.0).reshape(3, 3)
    X[1, 1] = np.nan
    assert nn.inpaint_nearest(X)[1, 1] == 1.0
    Y = np.array([[1.0, np.nan, 3.0]])
    assert nn.inpaint_nearest(Y)[0, 1] == 1.0
    Z = np.array([[np.nan, -0.0], [5.0, np.nan]])
    out = nn.inpaint_nearest(Z)
    assert np.signbit(out[0, 0]) and out[0, 0] == 0 and np.signbit(out[1, 1])


def test_signature_matches_the_reference():
    import neilpy_amd
    assert list(signatures_match("nearest_signatures.json", 1)) == ["inpaint_nearest"]
    ns = inspect.signature(neilpy_amd.nearest_source).parameters
    assert list(ns) == ["X", "return_distances", "return_indices"]
    assert ns["return_distances"].default is True and ns["return_indices"].default is True


def test_abi_names_exported():
    from neilpy_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from neilpy_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "smrf_hip.h")).read()
    for n in ("smrf_nearest_workspace_bytes", "smrf_nearest_f32", "smrf_nearest_f64", "smrf_nearest_planes"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
        assert re.search(r"^SMRF_API [\w \*]*?\b%s\(" % n, hdr, flags=re.M), n
    declared = sorted(set(re.findall(r"^SMRF_API [\w \*]*?\b(smrf_\w+)\(", hdr, flags=re.M)))
    assert sorted(_lib.SIGNATURES) == declared
    assert _lib.load().smrf_abi_version() == 1
    # the workspace query is host code: integer planes only, the same for both element sizes, nothing for an empty raster
    fn = lib.smrf_nearest_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    assert fn(0, 5, 4) == 0 and fn(5, 0, 8) == 0
    assert fn(100, 300, 4) == fn(100, 300, 8) >= 100 * 300 * 12
    assert fn(16384, 16384, 4) < 13 * 16384 * 16384


def test_no_cpu_fallback():
    import torch
    import neilpy_amd as na
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    X = np.ones((6, 6))
    X[2, 2] = np.nan
    for call in (lambda: na.inpaint_nearest(X), lambda: na.nearest_source(X),
                 lambda: na.inpaint_nearest(np.ones((4, 4), np.int64))):
        with pytest.raises(na.SmrfHipError):
            call()
    assert np.isnan(X[2, 2])


def test_nearest_kernels_compile_without_scratch(tmp_path):
    """every kernel of csrc/nearest.hip keeps its state in registers (ScratchSize 0) and decides no winner with an
    atomic (no GPU needed)"""
    text, kernels = device_asm("nearest", tmp_path)
    names = sorted(kernels)
    assert len(names) == 7, names             # mask x 2 dtypes, carry, envelope, lookup x 2 dtypes, planes
    for stem, n in (("nearest_mask_kernel", 2), ("nearest_carry_kernel", 1), ("nearest_envelope_kernel", 1),
                    ("nearest_lookup_kernel", 2), ("nearest_planes_kernel", 1)):
        assert sum(stem in k for k in names) == n, (stem, names)
    assert_no_scratch(text, kernels)
    assert not re.search(r"^\s*(global|flat|buffer|ds)_atomic|^\s*ds_(add|min|max|cmpst)", text, re.M)
    env = [b for k, b in kernels.items() if "nearest_envelope_kernel" in k][0]
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", env).group(1)) == 64 * 65 * 4   # the transposing tile
