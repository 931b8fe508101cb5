"""The array boundary of the raster functions (neilpy_amd/_raster.py) without a GPU: the one 2-D rule, made before the
device is touched, and the helpers other modules and the tools reach through ``api``."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

W = np.ones((3, 3))

# every raster function of the surface, focal, terrain, morphometry and nearest families and the disk filters and pssm
# of api, with the arguments it cannot be called without
RASTER_CALLS = {
    "slope": lambda na, Z: na.slope(Z),
    "aspect": lambda na, Z: na.aspect(Z),
    "hillshade": lambda na, Z: na.hillshade(Z),
    "multiple_illumination": lambda na, Z: na.multiple_illumination(Z),
    "esri_slope": lambda na, Z: na.esri_slope(Z),
    "curvature": lambda na, Z: na.curvature(Z),
    "esri_curvature": lambda na, Z: na.esri_curvature(Z),
    "zevenbergen_and_thorne_curvature": lambda na, Z: na.zevenbergen_and_thorne_curvature(Z),
    "evans_curvature": lambda na, Z: na.evans_curvature(Z),
    "wilson_gallant_curvature": lambda na, Z: na.wilson_gallant_curvature(Z),
    "focal_convolve": lambda na, Z: na.focal_convolve(Z, W),
    "std": lambda na, Z: na.std(Z, W),
    "topographic_position_index": lambda na, Z: na.topographic_position_index(Z),
    "reduce_peaks": lambda na, Z: na.reduce_peaks(Z, 3),
    "openness": lambda na, Z: na.openness(Z, 1, 2),
    "skyview_factor": lambda na, Z: na.skyview_factor(Z, 1, 2),
    "count_openness": lambda na, Z: na.count_openness(Z, 1, 2, 1),
    "geomorphons": lambda na, Z: na.geomorphons(Z, 1, 2),
    "ternary_pattern_from_openness": lambda na, Z: na.ternary_pattern_from_openness(Z, 1, 2),
    "scaled_morphometry": lambda na, Z: na.scaled_morphometry(Z),
    "vip_score": lambda na, Z: na.vip_score(Z),
    "ashift": lambda na, Z: na.ashift(Z, 0),
    "inpaint_nearest": lambda na, Z: na.inpaint_nearest(Z),
    "nearest_source": lambda na, Z: na.nearest_source(Z),
    "erosion": lambda na, Z: na.erosion(Z, radius=1),
    "dilation": lambda na, Z: na.dilation(Z, radius=1),
    "opening": lambda na, Z: na.opening(Z, radius=1),
    "pssm": lambda na, Z: na.pssm(Z),
}


def test_every_raster_function_is_listed():
    """the families' public raster functions, from their ``__all__``, minus the host helpers that take no raster"""
    from neilpy_amd import focal, morphometry, nearest, surface, terrain
    helpers = {"z_factor", "distance_kernel", "triangle_height", "progressive_window", "int2base",
               "get_lowest_equivalent", "terrain_code_to_geomorphon", "geomorphon_cmap", "GEOMORPHON_TABLE"}
    public = set()
    for mod in (surface, focal, terrain, morphometry, nearest):
        public |= set(mod.__all__)
    assert public - helpers == set(RASTER_CALLS) - {"erosion", "dilation", "opening", "pssm"}


@pytest.mark.parametrize("name", sorted(RASTER_CALLS))
def test_a_raster_is_two_dimensional(name):
    """ValueError from the argument's shape alone: the same on a machine without a GPU, where touching the device
    would raise SmrfHipError first"""
    import neilpy_amd as na
    for Z in (np.zeros(6), np.zeros((2, 3, 4)), np.zeros(6, np.float32), np.zeros((2, 3, 4), np.int32)):
        with pytest.raises(ValueError, match="expected a 2-D raster"):
            RASTER_CALLS[name](na, Z)


def test_tensors_are_checked_by_dim():
    import torch
    import neilpy_amd as na
    for name in ("slope", "focal_convolve", "openness", "ashift", "inpaint_nearest", "nearest_source", "opening", "pssm"):
        for Z in (torch.zeros(6), torch.zeros((2, 3, 4), dtype=torch.float64)):
            with pytest.raises(ValueError, match="expected a 2-D raster"):
                RASTER_CALLS[name](na, Z)


def test_checks_that_come_before_the_raster_still_do():
    """a function's own argument checks keep their place ahead of the 2-D rule"""
    import neilpy_amd as na
    Z = np.zeros(6)
    with pytest.raises(ValueError, match="return_as"):
        na.slope(Z, return_as="grads")
    with pytest.raises(ValueError, match="integer >= 1"):
        na.ashift(Z, 0, 0)
    with pytest.raises(ValueError, match="integer >= 1"):
        na.scaled_morphometry(Z, 1, 0)
    with pytest.raises(ValueError, match="unknown output"):
        na.scaled_morphometry(Z, outputs=("nope",))
    with pytest.raises(ValueError, match="radius must be"):
        na.topographic_position_index(Z, 0)
    with pytest.raises(ValueError, match="neighbors"):
        na.openness(Z, neighbors=np.array([8]))
    with pytest.raises(ValueError, match="2-D kernel"):
        na.focal_convolve(Z, np.ones(3))
    with pytest.raises(ValueError, match="too small to calculate a numerical gradient"):
        na.slope(np.zeros((1, 6)))


def test_helpers_resolve_through_api():
    """tools/smrf_stages.py and neilpy_amd/sharded.py reach the general helpers as ``api._ptr`` and so on"""
    from neilpy_amd import _raster, api
    for name in ("_ptr", "_stream", "_to_device", "_suffix", "_torch"):
        assert getattr(api, name) is getattr(_raster, name), name
    assert api._ptr(None).value is None
    assert _raster._pyfloat(np.float32(2.5)) == 2.5 and type(_raster._pyfloat(np.float64(0.3))) is float


def test_one_definition_of_the_boundary():
    """no module of the package but _raster defines the boundary helpers"""
    import ast
    import glob
    import os
    for path in glob.glob(os.path.join(ROOT, "neilpy_amd", "*.py")):
        if os.path.basename(path) == "_raster.py":
            continue
        defs = {n.name for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.FunctionDef)}
        assert not defs & {"_raster", "_out", "_empty", "_check_2d", "_stream", "_sfx", "_st", "_ptr", "_suffix"}, path


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_two_restatements_of_evans_quadratic_agree(dtype):
    """what tests/test_gpu_raster_boundary.py holds the two kernels to: on its raster (no NaN, no flat cell)
    evans_curvature and scaled_morphometry at stride 1 restate the same six curvatures, bit for bit"""
    import morphometry_numpy as mn
    import surface_numpy as sn
    from family_checks import same_bits
    rng = np.random.default_rng(20261101)
    X = (rng.normal(size=(8, 9)) * 10).astype(dtype)
    for cellsize in (1, 2.5):
        sm = mn.scaled_morphometry(X, cellsize, 1)
        assert sm["S"].min() > 0
        for k, v in zip(("K", "K_profile", "K_plan", "K_tan", "K_long", "K_cross"), sn.evans_curvature(X, cellsize)):
            assert same_bits(v, sm[k]) and not np.isnan(v).any(), (k, cellsize)


def test_importing_the_package_does_not_import_torch():
    code = "import sys; import neilpy_amd; sys.exit(1 if 'torch' in sys.modules else 0)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
