"""Terrain functions without a GPU: the NumPy restatement of the contract against the reference's goldens, the host
helpers and tables, signatures, ABI exports, the no-fallback rule and the generated code of csrc/terrain.hip."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import terrain_numpy as tn
from conftest import ROOT, golden
from family_checks import assert_no_scratch, device_asm, signatures_match


@pytest.fixture(scope="module")
def G():
    return golden("terrain.npz")


def _cases(G):
    return json.loads(str(G["cases"]))


def test_restatement_equals_every_golden(G):
    """the contract of DESIGN.md section 9 reproduces the reference bit for bit, NaN and inf placement included"""
    cases = _cases(G)
    assert len(cases) >= 80
    for c in cases:
        Z = G["in_" + c["input"]]
        got = tn.run(c["fn"], Z, c["kw"])
        if c["fn"] == "count_openness":
            for g, part in zip(got, ("pos", "neg")):
                want = G["out_%s_%s" % (c["id"], part)]
                assert g.dtype == want.dtype == np.uint8 and np.array_equal(g, want), c
        else:
            want = G["out_" + c["id"]]
            assert got.dtype == want.dtype and got.shape == want.shape, (c, got.dtype, want.dtype)
            assert np.array_equal(got, want, equal_nan=True), c


def test_golden_inputs_cover_the_contract(G):
    cases = _cases(G)
    Ls = {c["kw"].get("lookup_pixels") for c in cases}
    assert {0, 1, 3, 10, 20, 25} <= Ls
    assert any(c["kw"].get("fast") for c in cases) and any(c["kw"].get("enhance") for c in cases)
    assert np.isnan(G["in_nan"]).any() and G["in_dtm21_f32"].dtype == np.float32
    assert str(G["numpy_version"]).startswith("2.")
    ternary = [G["out_" + c["id"]] for c in cases if c["fn"] == "ternary_pattern_from_openness"]
    assert all(t.dtype == np.int64 for t in ternary)


def test_host_helpers_match_the_reference(G):
    import neilpy_amd as na
    from neilpy_amd import terrain
    for key in G.files:
        if key.startswith("pw_"):
            a, b, p = (int(v) for v in key[3:].split("_"))
            got = na.progressive_window(a, b, p)
            assert got.dtype == G[key].dtype and np.array_equal(got, G[key]), key
    assert list(na.progressive_window(1, 25, 20))[-1] == 22
    for x, b, want in json.loads(str(G["int2base"])):
        assert na.int2base(x, b) == want
    lowest = G["lowest_table"]
    assert np.array_equal(terrain._lowest_table(), lowest)
    assert all(na.get_lowest_equivalent(int(x)) == lowest[x] for x in (0, 1, 241, 5129, 1449, 6560))
    assert na.get_lowest_equivalent(241) == 161
    codes = np.arange(3 ** 8)
    for m in ("strict", "loose"):
        got = na.terrain_code_to_geomorphon(codes, m)
        assert got.dtype == np.uint8 and np.array_equal(got, G["geo_" + m]), m
    with pytest.raises(ValueError):
        na.terrain_code_to_geomorphon(codes, "medium")
    assert {str(k): list(v) for k, v in na.geomorphon_cmap().items()} == json.loads(str(G["cmap"]))
    assert np.array_equal(terrain.GEOMORPHON_TABLE, tn.GEO)


def test_march_tables():
    """the host step list / flags / distance table of one launch (enhance: the short march is a prefix)"""
    from neilpy_amd import terrain
    m = terrain._March(terrain._as_steps(25, True, 20), list(np.arange(1, 7)), cellsize=0.3)
    assert list(m.steps) == [1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 18, 22]
    assert list(m.flags) == [3, 3, 3, 3, 3, 3, 1, 1, 1, 1, 1, 1]
    m = terrain._March(terrain._as_steps(25, True, 20), list(np.arange(1, 8)), cellsize=0.3)
    assert list(m.flags[:8]) == [3, 3, 3, 3, 3, 3, 2, 1]
    n = m.n
    assert m.dist[6] == (0.3 * 7) * np.sqrt(2) and m.dist[n + 6] == 0.3 * 7 * 1.0
    assert terrain._March(terrain._as_steps(0), cellsize=1).n == 0
    assert list(terrain._March(terrain._as_steps(0, True), cellsize=1).steps) == [1]


def test_signatures_match_the_reference():
    signatures_match("terrain_signatures.json", 10)


def test_abi_names_exported():
    from neilpy_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from neilpy_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("smrf_terrain_rays_f32", "smrf_terrain_rays_f64"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "smrf_hip.h")).read()
    for k, v in _lib.TERRAIN_HALO_CAP.items():
        assert re.search(r"#define SMRF_TERRAIN_HALO_CAP_%s %d\b" % (k.upper(), v), hdr), k


def test_no_cpu_fallback():
    import torch
    import neilpy_amd as na
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    Z = np.zeros((6, 6))
    for call in (lambda: na.openness(Z, 1, 2), lambda: na.skyview_factor(Z, 1, 2),
                 lambda: na.count_openness(Z, 1, 2, 1), lambda: na.geomorphons(Z, 1, 2),
                 lambda: na.ternary_pattern_from_openness(Z, 1, 2)):
        with pytest.raises(na.SmrfHipError):
            call()


def test_neighbors_are_validated():
    import neilpy_amd as na
    for nb in ([], [8], [-1], [0, 9]):
        with pytest.raises(ValueError):
            na.openness(np.zeros((4, 4)), neighbors=np.array(nb, dtype=np.int64))


def test_terrain_kernels_compile_without_scratch(tmp_path):
    """every instance of csrc/terrain.hip keeps its state in registers: ScratchSize 0 (no GPU needed)"""
    text, kernels = device_asm("terrain", tmp_path)
    assert len(kernels) == 16                 # 2 dtypes x 4 modes x {tiled, direct}
    assert_no_scratch(text, kernels)
