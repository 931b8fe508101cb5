"""The strided-stencil contract on the host (no GPU): the NumPy restatement (tests/morphometry_numpy.py) against the
goldens of the reference, signatures, ABI exports, the no-fallback rule, the documented deviations and the host helper
triangle_height."""
import ctypes
import inspect
import json
import os
import warnings

import numpy as np
import pytest

import morphometry_numpy as mn
from conftest import golden
from family_checks import same_bits, signatures_match


@pytest.fixture(scope="module")
def G():
    return golden("morphometry.npz")


def _cases(G):
    return json.loads(str(G["cases"]))


def test_restatement_equals_every_golden(G):
    """the contract of DESIGN.md section 13 reproduces the reference bit for bit, signed zeros and NaN placement
    included"""
    cases = _cases(G)
    assert len(cases) >= 150
    assert json.loads(str(G["keys"])) == list(mn.KEYS)
    for c in cases:
        Z = G["in_" + c["input"]]
        if c["fn"] == "scaled_morphometry":
            got = mn.scaled_morphometry(Z, **c["kw"])
            assert list(got) == list(mn.KEYS)
            for k in mn.KEYS:
                assert same_bits(got[k], G["out_%s_%s" % (c["id"], k)]), (c, k)
        elif c["fn"] == "vip_score":
            assert same_bits(mn.vip_score(Z, **c["kw"]), G["out_" + c["id"]]), c
        else:
            assert same_bits(mn.ashift(Z, **c["kw"]), G["out_" + c["id"]]), c


def test_golden_cases_cover_the_contract(G):
    cases = _cases(G)
    sm = [c for c in cases if c["fn"] == "scaled_morphometry"]
    assert {c["kw"].get("lookup_pixels", 1) for c in sm} == {1, 2, 5, 19, 20, 26, 40}
    assert {c["kw"].get("cellsize", 1) for c in sm} == {1, 0.5, 2.5}
    inputs = {k[3:] for k in G.files if k.startswith("in_")}
    assert {c["input"] for c in cases if c["fn"] == "vip_score"} == inputs
    assert inputs >= {"one", "row7", "col7", "sq2", "r2x5", "nan", "nan_f32", "terrace", "terrace_f32", "dtm21_f32"}
    assert G["in_dtm11"].shape == (20, 26) and np.isnan(G["in_nan"][[0, 0, -1, -1], [0, -1, 0, -1]]).all()
    sh = [c for c in cases if c["fn"] == "ashift"]
    assert {(c["kw"]["direction"], c["kw"]["n"]) for c in sh} == {(d, n) for d in range(10) for n in (1, 3, 25)}
    # dtypes: float32 is kept by scaled_morphometry and promoted by vip_score
    c = next(c for c in sm if c["input"] == "dtm21_f32")
    assert all(G["out_%s_%s" % (c["id"], k)].dtype == np.float32 for k in mn.KEYS)
    c = next(c for c in cases if c["fn"] == "vip_score" and c["input"] == "dtm21_f32")
    assert G["out_" + c["id"]].dtype == np.float64
    # a flat interior cell: A = 270, S = 0, K = -0.0, NaN in the five ratios (no NaN repair)
    c = next(c for c in sm if c["input"] == "terrace" and c["kw"].get("lookup_pixels", 1) == 1)
    out = {k: G["out_%s_%s" % (c["id"], k)] for k in mn.KEYS}
    assert G["in_terrace"][7:10, 6:9].std() == 0
    assert out["A"][8, 7] == 270 and out["S"][8, 7] == 0 and out["K"][8, 7] == 0 and np.signbit(out["K"][8, 7])
    assert all(np.isnan(out[k][8, 7]) for k in ("K_profile", "K_cross", "K_long", "K_tan", "K_plan"))
    # directions 8 and 9 do not move; a stride beyond the raster is a copy
    for c in sh:
        if c["kw"]["direction"] >= 8 or (c["input"] == "r2x5" and c["kw"]["n"] == 25):
            assert np.array_equal(G["out_" + c["id"]], G["in_" + c["input"]]), c
    assert str(G["numpy_version"]).startswith("2.")


def test_signatures_match_the_reference():
    import neilpy_amd
    want = signatures_match("morphometry_signatures.json", 4)
    assert set(want) == {"scaled_morphometry", "vip_score", "ashift", "triangle_height"}
    assert "outputs" in inspect.signature(neilpy_amd.scaled_morphometry).parameters


def test_abi_names_exported():
    from neilpy_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from neilpy_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("smrf_morphometry_f32", "smrf_morphometry_f64", "smrf_vip_f32", "smrf_vip_f64", "smrf_ashift_f32",
              "smrf_ashift_f64"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["smrf_morphometry_f32"][1]) == 17
    assert len(_lib.SIGNATURES["smrf_vip_f64"][1]) == 9 and len(_lib.SIGNATURES["smrf_ashift_f32"][1]) == 7


def test_no_cpu_fallback():
    import torch
    import neilpy_amd as na
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    Z = np.zeros((6, 6))
    for call in (lambda: na.scaled_morphometry(Z), lambda: na.scaled_morphometry(Z, 1, 3, outputs=("K",)),
                 lambda: na.vip_score(Z), lambda: na.ashift(Z, 0), lambda: na.ashift(Z, 9, 2)):
        with pytest.raises(na.SmrfHipError):
            call()


# ------------------------------------------------------------------------------------------
# documented deviations
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, -1, -3, 2.0, 1.5, np.float64(2), "2", None, True])
def test_strides_must_be_integers_from_one(bad):
    """the reference raises a broadcast ValueError at 0, a TypeError on floats and scrambles the raster on negatives;
    here all of them are a ValueError, raised before the device is touched (so it is a ValueError without a GPU too)"""
    import neilpy_amd as na
    Z = np.arange(30.0).reshape(5, 6)
    with pytest.raises(ValueError, match="integer >= 1"):
        na.scaled_morphometry(Z, 1, bad)
    with pytest.raises(ValueError, match="integer >= 1"):
        na.ashift(Z, 1, bad)


def test_unknown_output_key_raises_before_the_device():
    import neilpy_amd as na
    Z = np.zeros((4, 4))
    with pytest.raises(ValueError, match="unknown output"):
        na.scaled_morphometry(Z, outputs=("K", "K_mean"))
    with pytest.raises(ValueError, match="unknown output"):
        na.scaled_morphometry(Z, outputs="slope")


def test_numpy_scalar_cellsize_is_a_python_float(G):
    """under NEP 50 an np.float64 cellsize makes the reference's divisors float64 scalars and promotes a float32 raster
    to float64; the contract takes the cellsize as a Python float, so float32 stays float32 with the same bits"""
    Z = G["in_dtm21_f32"]
    L = np.float64(0.5) * 2
    assert (Z / (6 * L ** 2)).dtype == np.float64 and (Z / (6 * float(L) ** 2)).dtype == np.float32
    a = mn.scaled_morphometry(Z, np.float64(0.5), 2)
    b = mn.scaled_morphometry(Z, 0.5, 2)
    assert all(a[k].dtype == np.float32 and same_bits(a[k], b[k]) for k in mn.KEYS)
    assert same_bits(mn.vip_score(Z, np.float32(2.5)), mn.vip_score(Z, 2.5))


def test_error_state_is_left_alone(G):
    """the reference ends scaled_morphometry with np.seterr(divide='warn', invalid='warn'); neither the product nor the
    restatement touches the process's error state"""
    import neilpy_amd as na
    Z = G["in_terrace"]
    for state in (dict(divide="raise", invalid="ignore"), dict(divide="ignore", invalid="raise")):
        before = np.geterr()
        np.seterr(**state)
        try:
            want = np.geterr()
            mn.scaled_morphometry(Z, 1, 2)
            mn.vip_score(Z)
            assert np.geterr() == want
            for call in (lambda: na.scaled_morphometry(Z, 1, 2), lambda: na.vip_score(Z), lambda: na.ashift(Z, 3, 2)):
                try:
                    call()
                except na.SmrfHipError:
                    pass                      # no GPU here: the state must be untouched all the same
                assert np.geterr() == want
            na.triangle_height(np.arange(4.0), np.ones(4))
            assert np.geterr() == want
        finally:
            np.seterr(**before)


def test_triangle_height_equals_golden_without_a_warning(G):
    import neilpy_amd as na
    h0, h1 = G["th_h0"], G["th_h1"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="ignore"):
            for t in json.loads(str(G["th_cases"])):
                for f in (na.triangle_height, mn.triangle_height):
                    assert same_bits(f(h0, h1, t["x_dist"]), G["th_" + t["id"]]), t
            assert same_bits(na.triangle_height(h0, h1), G["th_default"])
            got = na.triangle_height(h0.astype(np.float32), h1.astype(np.float32))
            assert got.dtype == np.float64 and same_bits(got, G["th_f32"])
            assert same_bits(mn.triangle_height(h0.astype(np.float32), h1.astype(np.float32)), G["th_f32"])
    assert np.isnan(G["th_t0"][1]) and G["th_t0"][0] == 0


def test_vip_score_is_the_mean_of_triangle_heights(G):
    """the restatement's fused loop equals the reference's composition: four triangle_height calls on ashift
    differences, summed in direction order, divided by 4"""
    import neilpy_amd as na
    for name, cs in (("dtm21_f32", 1), ("nan", 2.5), ("terrace", 0.5)):
        Z = G["in_" + name]
        x, _ = mn.vip_constants(cs)
        acc = np.zeros(Z.size)
        with np.errstate(all="ignore"):
            for d in range(4):
                acc += na.triangle_height((mn.ashift(Z, d) - Z).ravel(), (mn.ashift(Z, d + 4) - Z).ravel(), x[d % 2])
            want = (acc / 4).reshape(Z.shape)
        assert same_bits(mn.vip_score(Z, cs), want), name
