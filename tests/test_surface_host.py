"""Surface derivatives without a GPU: the NumPy restatement of the contract against the reference's goldens, the host
helpers, signatures, ABI exports, the no-fallback rule, the documented deviations and the generated code of
csrc/surface.hip."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import surface_numpy as sn
from conftest import ROOT, golden
from family_checks import assert_no_scratch, device_asm, signatures_match


@pytest.fixture(scope="module")
def G():
    return golden("surface.npz")


def _cases(G):
    return json.loads(str(G["cases"]))


def golden_outputs(G, c):
    if c["fn"] in sn.N_OUT:
        return tuple(G["out_%s_%d" % (c["id"], k)] for k in range(sn.N_OUT[c["fn"]]))
    return (G["out_" + c["id"]],)


def test_restatement_equals_every_golden(G):
    """the contract of DESIGN.md section 10 reproduces the reference bit for bit, NaN and inf placement included"""
    cases = _cases(G)
    assert len(cases) >= 150
    for c in cases:
        got = sn.run(c["fn"], G["in_" + c["input"]], c["kw"])
        got = got if c["fn"] in sn.N_OUT else (got,)
        for k, (g, want) in enumerate(zip(got, golden_outputs(G, c))):
            assert g.dtype == want.dtype and g.shape == want.shape, (c, k, g.dtype, want.dtype)
            assert np.array_equal(g, want, equal_nan=True), (c, k)


def test_golden_inputs_cover_the_contract(G):
    cases = _cases(G)
    fns = {c["fn"] for c in cases}
    assert fns == set(sn.FUNCS)
    inputs = {c["input"] for c in cases}
    for name in ("one", "row7", "col7", "sq2", "r2x5", "nan", "nan_f32", "terrace", "terrace_f32", "dtm21_f32"):
        assert name in inputs, name
    assert G["in_one"].shape == (1, 1) and G["in_row7"].shape == (1, 7) and G["in_col7"].shape == (7, 1)
    assert G["in_sq2"].shape == (2, 2) and G["in_r2x5"].shape == (2, 5)
    nan = G["in_nan"]
    assert np.isnan(nan[[0, 0, -1, -1], [0, -1, 0, -1]]).all()            # NaN corners
    assert np.isnan(nan[8:11, 12:16]).all() and 0.02 < np.isnan(nan).mean() < 0.3   # a block and scattered NaNs
    assert G["in_dtm21_f32"].dtype == np.float32 and G["in_nan_f32"].dtype == np.float32
    # exact flats: zero gradients (flat_as) and 0 / 0 in the curvature ratios
    terr = G["in_terrace"]
    assert (np.diff(terr, axis=1) == 0).mean() > 0.3
    for ra in ("degrees", "radians", "percent"):
        assert any(c["fn"] == "slope" and c["kw"].get("return_as", "degrees") == ra for c in cases)
    assert any(c["fn"] == "aspect" and c["kw"].get("flat_as", "nan") == "nan" for c in cases)
    assert any(c["fn"] == "aspect" and c["kw"].get("flat_as") in (0, -1) for c in cases)
    assert any(c["fn"] == "hillshade" and c["kw"].get("return_uint8") is False for c in cases)
    mi = [c["kw"] for c in cases if c["fn"] == "multiple_illumination"]
    assert {} in mi and any(np.isscalar(k.get("zeniths", [0])) for k in mi)
    assert any(isinstance(k.get("azimuths"), list) for k in mi)
    assert len({(c["kw"].get("cellsize", 1), c["kw"].get("z_factor", 1)) for c in cases}) >= 3
    assert str(G["numpy_version"]).startswith("2.")
    # the flat rules show in the goldens
    flat = [c for c in cases if c["fn"] == "aspect" and c["input"] == "terrace" and "flat_as" not in c["kw"]]
    assert flat and np.isnan(G["out_" + flat[0]["id"]]).any()
    hs = [c for c in cases if c["fn"] == "hillshade" and c["input"] == "nan" and c["kw"] == {}]
    assert hs and G["out_" + hs[0]["id"]].dtype == np.uint8
    undefined = np.isnan(sn.hillshade_value(nan))                       # a NaN shade is 0 in the uint8 output
    assert undefined.sum() > 10 and (G["out_" + hs[0]["id"]][undefined] == 0).all()
    zt = [c for c in cases if c["fn"] == "zevenbergen_and_thorne_curvature" and c["input"] == "terrace"][0]
    assert (G["out_%s_4" % zt["id"]] == 0).any() and np.isnan(G["out_%s_1" % zt["id"]]).any()


def test_f32_float_hillshade_is_float64(G):
    """NumPy 2: np.cos(zenith) is a float64 scalar, so the float shade of a float32 raster is float64"""
    c = [c for c in _cases(G) if c["fn"] == "hillshade" and c["input"] == "dtm21_f32" and
         c["kw"].get("return_uint8") is False][0]
    assert G["out_" + c["id"]].dtype == np.float64
    s = [c for c in _cases(G) if c["fn"] == "slope" and c["input"] == "dtm21_f32"][0]
    assert G["out_" + s["id"]].dtype == np.float32


def test_z_factor_and_angle_lists_match_the_reference(G):
    import neilpy_amd as na
    from neilpy_amd import surface
    got = na.z_factor(G["z_factor_lat"])
    assert np.array_equal(got, G["z_factor"])
    assert na.z_factor(45.0) == G["z_factor"][2]
    for zs, az, seen in json.loads(str(G["angles"])):
        zs = np.array(zs) if isinstance(zs, list) else zs
        az = np.array(az) if isinstance(az, list) else az
        z2, a2 = surface._angle_lists(zs, az)
        pairs = [(float(z), float(a)) for z in z2 for a in a2]
        assert pairs == [tuple(p) for p in seen], (zs, az)
        assert [tuple(p) for p in seen] == [(float(z), float(a)) for z in sn.angle_lists(zs, az)[0]
                                              for a in sn.angle_lists(zs, az)[1]]
    assert surface._angle_row(45, 315) == list(sn.angles(45, 315))


def test_signatures_match_the_reference():
    signatures_match("surface_signatures.json", 11)


def test_abi_names_exported():
    from neilpy_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from neilpy_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("smrf_surface_f32", "smrf_surface_f64"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "smrf_hip.h")).read()
    for name in ("SLOPE", "ASPECT", "HILLSHADE", "HORN", "LAPLACE", "ESRI", "ZT", "EVANS", "WG"):
        v = getattr(_lib, "SURFACE_" + name)
        assert re.search(r"#define SMRF_SURFACE_%s %d\b" % (name, v), hdr), name
    for name in ("RADIANS", "DEGREES"):
        assert re.search(r"#define SMRF_SURFACE_OPT_%s %d\b" % (name, getattr(_lib, "SURFACE_OPT_" + name)), hdr)


def test_no_cpu_fallback():
    import torch
    import neilpy_amd as na
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    Z = np.zeros((6, 6))
    for call in (lambda: na.slope(Z), lambda: na.aspect(Z), lambda: na.hillshade(Z), lambda: na.esri_slope(Z),
                 lambda: na.multiple_illumination(Z), lambda: na.curvature(Z), lambda: na.esri_curvature(Z),
                 lambda: na.zevenbergen_and_thorne_curvature(Z), lambda: na.evans_curvature(Z),
                 lambda: na.wilson_gallant_curvature(Z)):
        with pytest.raises(na.SmrfHipError):
            call()


# ------------------------------------------------------------------------------------------
# documented deviations
# ------------------------------------------------------------------------------------------
def test_unsupported_return_as_raises():
    """the reference prints a message and then fails on an unbound name (slope) or returns None (aspect)"""
    import neilpy_amd as na
    Z = np.zeros((4, 4))
    with pytest.raises(ValueError):
        na.slope(Z, return_as="grads")
    with pytest.raises(ValueError):
        na.aspect(Z, return_as="percent")


def test_gradient_functions_need_two_cells_per_axis():
    """np.gradient's own message, raised before the device is touched (as pssm does)"""
    import neilpy_amd as na
    for shape in ((1, 7), (7, 1), (1, 1)):
        Z = np.zeros(shape)
        with pytest.raises(ValueError, match="too small to calculate a numerical gradient"):
            np.gradient(Z)
        for fn in (na.slope, na.aspect, na.hillshade, na.multiple_illumination):
            with pytest.raises(ValueError, match="too small to calculate a numerical gradient"):
                fn(Z)


def test_numpy_scalar_parameters_are_python_floats():
    """under NEP 50 an np.float64 spacing promotes np.gradient of a float32 raster to a float64 division; the library
    takes every parameter as a Python float, so the float32 contract holds whatever scalar type is passed"""
    rng = np.random.default_rng(5)
    Z = rng.normal(size=(40, 40)).astype(np.float32) * 100
    a = np.gradient(Z, 0.3)[1]
    b = np.gradient(Z, np.float64(0.3))[1]
    assert a.dtype == b.dtype == np.float32 and not np.array_equal(a, b)
    assert np.array_equal(sn.slope(Z, np.float64(0.3), np.float64(1), 'percent'), sn.slope(Z, 0.3, 1, 'percent'))


def test_esri_slope_squares_by_a_product(G):
    """the reference's per-cell callback squares NumPy float64 scalars through C pow, which is not correctly rounded;
    the contract squares by a product.  On the goldens both give the same bits; elsewhere they differ by at most one
    float64 ulp in a small fraction of cells, and the float32 results agree"""
    for c in _cases(G):
        if c["fn"] == "esri_slope":
            Z = G["in_" + c["input"]]
            assert np.array_equal(sn.run("esri_slope", Z, c["kw"], scalar_pow=True), G["out_" + c["id"]],
                                  equal_nan=True), c
    rng = np.random.default_rng(9)
    Z = np.cumsum(rng.normal(size=(60, 60)), axis=0) * 7.3
    a = sn.esri_slope(Z, return_as="percent")
    b = sn.esri_slope(Z, return_as="percent", scalar_pow=True)
    diff = a != b
    assert diff.mean() < 0.02
    assert np.all(np.abs(a[diff] - b[diff]) <= np.spacing(np.maximum(np.abs(a[diff]), np.abs(b[diff]))))


def test_surface_kernels_compile_without_scratch(tmp_path):
    """every instance of csrc/surface.hip keeps its state in registers (ScratchSize 0), and the fp32 divides and square
    roots are the correctly rounded sequences (no GPU needed)"""
    text, kernels = device_asm("surface", tmp_path)
    assert len(kernels) == 18                 # 2 dtypes x 9 modes
    assert_no_scratch(text, kernels)
    # laplace in fp32 (Li4) is arithmetic only: its five divides are the div_scale / div_fmas / div_fixup sequence
    parts = re.split(r"\n\s*\.type\s+(_ZN4smrf14surface_kernel\S+),@function\n", text)
    bodies = {parts[i]: parts[i + 1].split(".Lfunc_end")[0] for i in range(1, len(parts), 2)}
    lap32 = [b for n, b in bodies.items() if "IfLi4E" in n][0]
    assert lap32.count("v_div_fixup_f32") == 5
    # the fp32 gradient slope's square root carries the correction steps after v_sqrt_f32
    sl32 = [b for n, b in bodies.items() if "IfLi0E" in n][0]
    i = sl32.index("v_sqrt_f32")
    assert "v_fma_f32" in sl32[i:i + 400]
