"""Seeded random point clouds through the whole smrf(): HIP path against the oracle (which the goldens
pin to the reference).  Varies point density, cell size (incl. non-integers, where the index
arithmetic of create_dem is delicate), window lists, thresholds and the low-outlier option."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nz(gpu_device):
    import neilpy_amd
    neilpy_amd.load_library()
    return neilpy_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import smrf_oracle
    return smrf_oracle


def cloud(rng, npts, extent):
    x = rng.uniform(1000.0, 1000.0 + extent[0], npts)
    y = rng.uniform(5000.0, 5000.0 + extent[1], npts)
    ground = 50 + 0.05 * (x - 1000) + 3 * np.sin((y - 5000) / 7.0)
    z = ground + np.where(rng.random(npts) < .25, rng.uniform(2, 15, npts), rng.normal(0, .05, npts))
    z[rng.random(npts) < .005] -= rng.uniform(5, 30)                       # low outliers
    return np.round(x, 2), np.round(y, 2), np.round(z, 2)


CASES = [
    # seed, points, extent, cellsize, windows, slope, elev_thr, scaler, low_fill
    (1, 3000, (60, 45), 1, 5, .15, .5, 1.25, False),
    (2, 800, (50, 70), 2, 3, .2, .3, 1.0, False),
    (3, 5000, (40, 40), .5, np.array([1, 2, 4, 7]), .15, .5, 1.25, True),
    (4, 2500, (33, 57), .3, 6, .1, .4, 2.0, False),
    (5, 1200, (90, 20), 1.5, np.array([3, 1, 2]), .3, .6, 0.0, False),
    (6, 6000, (70, 70), 1, 12, .15, .5, 1.25, True),
    (7, 400, (25, 25), 1, 2, .15, .5, 1.25, False),
    (8, 2000, (48, 52), .7, 4, .25, 1.0, .5, False),
]


@pytest.mark.parametrize("case", CASES, ids=[str(c[0]) for c in CASES])
def test_smrf_random_cloud(nz, orc, case):
    seed, npts, extent, cellsize, windows, slope, ethr, scaler, low_fill = case
    x, y, z = cloud(np.random.default_rng(seed), npts, extent)
    kw = dict(cellsize=cellsize, windows=windows, slope_threshold=slope, elevation_threshold=ethr,
              elevation_scaler=scaler, low_outlier_fill=low_fill)
    want = orc.smrf(x, y, z, **kw)
    got = nz.smrf(x, y, z, **kw)
    assert got[0].shape == want[0].shape and tuple(got[1])[:6] == tuple(want[1])[:6]
    assert np.array_equal(got[2], want[2])                                  # object cells, bit-exact
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-7)          # DTM
    assert np.array_equal(np.asarray(got[3]), np.asarray(want[3]))          # point flags


def test_return_extras_far_edge_index_error(nz, orc):
    """A point that rounds onto the raster's far edge makes the reference's when_dropped lookup raise
    (neilpy.py:1780, drop_raster[round(r), round(c)]); NumPy and CUDA inputs both raise IndexError here,
    and without return_extras the same cloud runs."""
    import torch
    x, y, z = cloud(np.random.default_rng(2), 800, (50, 70))
    kw = dict(cellsize=2, windows=3, slope_threshold=.2, elevation_threshold=.3, elevation_scaler=1.0)
    with pytest.raises(IndexError):
        orc.smrf(x, y, z, return_extras=True, **kw)
    with pytest.raises(IndexError):
        nz.smrf(x, y, z, return_extras=True, **kw)
    with pytest.raises(IndexError):
        nz.smrf(*(torch.from_numpy(v).cuda() for v in (x, y, z)), return_extras=True, **kw)
    assert len(nz.smrf(x, y, z, **kw)) == 4


@pytest.mark.parametrize("seed,shape,known", [(11, (37, 53), .5), (12, (90, 41), .1), (13, (64, 64), .03), (14, (5, 130), .3),
                                              (15, (120, 7), .6), (16, (77, 77), .9)])
def test_inpaint_random_holes(nz, orc, seed, shape, known):
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 1, shape).cumsum(0).cumsum(1) * 0.1 + 100
    A[rng.random(shape) >= known] = np.nan
    want, istop, itn = orc.inpaint_nans_by_springs(A, return_info=True)
    got = nz.inpaint_nans_by_springs(A)
    st = nz.last_stats["inpaint"]
    assert (st["istop"], st["itn"]) == (istop, itn)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-7)


@pytest.mark.parametrize("seed,shape,dtype,windows", [(21, (70, 90), np.float32, [1, 2, 3, 5, 9]), (22, (33, 200), np.float64, [4, 2, 11]),
                                                      (23, (150, 64), np.float32, list(range(1, 15))), (24, (9, 9), np.float64, [1, 6])])
def test_progressive_filter_random(nz, orc, seed, shape, dtype, windows):
    rng = np.random.default_rng(seed)
    Z = (rng.normal(0, 1, shape).cumsum(0).cumsum(1) * 0.05 + 200 + (rng.random(shape) < .06) * rng.uniform(1, 25, shape)).astype(dtype)
    win = np.asarray(windows)
    m, w = nz.progressive_filter(Z, win, .5, .2, return_when_dropped=True)
    m2, w2 = orc.progressive_filter(Z, win, .5, .2, return_when_dropped=True)
    assert np.array_equal(m, m2) and np.array_equal(w, w2)


# Large radii, awkward shapes, forced routes (windows from 0..64, half with a consecutive run; rows 1..300, columns 1..700
# biased to 1, 2, 7, 8, 9, 255..257, 511..513, plus three rasters of 10 or more strips by at most 60 rows; the second half
# under one drawn combination of the routing switches).  Drawn once from numpy's default_rng(20261016) and kept as a literal,
# so a failure names its case and replays alone; tools/fuzz_campaign.py draws its `pf` cases from the same space.
LARGE = [
    # seed, shape, dtype, windows, switches
    (300, (8, 390), 'f32', [46, 61, 10, 11, 12, 13, 16], {}),
    (301, (60, 233), 'f64', [7, 8, 53, 48, 46, 0, 52], {}),
    (302, (81, 658), 'f32', [25, 21, 27, 9], {}),
    (303, (8, 273), 'f32', [24, 4, 22, 45, 35, 34, 60], {}),
    (304, (157, 9), 'f64', [44, 45, 46, 47, 48, 49], {}),
    (305, (87, 9), 'f64', [61, 62, 63], {}),
    (306, (9, 210), 'f32', [64, 55, 4, 1, 35, 4, 35], {}),
    (307, (257, 143), 'f64', [27], {}),
    (308, (1, 526), 'f32', [20, 21, 22, 23, 24, 25], {}),
    (309, (257, 8), 'f64', [53, 54, 9, 3, 34, 56, 8], {}),
    (310, (230, 327), 'f32', [39, 22, 18], {}),
    (311, (134, 605), 'f32', [61, 38, 44, 19, 45], {}),
    (312, (39, 4097), 'f64', [39], {}),
    (313, (1, 257), 'f64', [8], {}),
    (314, (99, 1), 'f32', [49, 21, 63, 30], {}),
    (315, (64, 255), 'f64', [41, 6, 61, 24, 52, 24, 7], {}),
    (316, (1, 201), 'f32', [33, 34], {}),
    (317, (223, 255), 'f64', [6, 54, 0, 1, 2], {}),
    (318, (46, 1), 'f32', [4, 31, 10, 48, 12], {}),
    (319, (255, 91), 'f32', [32, 30, 3, 8, 6, 51, 55], {}),
    (320, (85, 511), 'f64', [49, 50, 51, 52], {'SMRF_NT': 1, 'SMRF_SEG_RULE': 2, 'SMRF_XCD_REMAP': 0}),
    (321, (201, 34), 'f64', [15, 16], {'SMRF_FUSED': 0, 'SMRF_CHAIN': 0, 'SMRF_ERO_INC': 0, 'SMRF_RING_SEG': 50, 'SMRF_SEG_RULE': 1}),
    (322, (7, 141), 'f32', [57], {'SMRF_FUSED': 0, 'SMRF_NT': 1}),
    (323, (29, 405), 'f64', [16, 43, 0, 62, 52, 56, 30, 51], {'SMRF_RING_DUAL': 1, 'SMRF_SEG_RULE': 2}),
    (324, (1, 7), 'f32', [42, 43], {'SMRF_FUSED': 2, 'SMRF_NT': 1, 'SMRF_RING_SEG': 50, 'SMRF_XCD_REMAP': 0}),
    (325, (7, 4353), 'f64', [22, 23], {'SMRF_FUSED': 0, 'SMRF_RING_SEG': 50}),
    (326, (257, 270), 'f32', [8, 5, 12, 25, 53, 60, 41, 14], {'SMRF_FUSED': 2, 'SMRF_CHAIN': 0, 'SMRF_ERO_INC': 2, 'SMRF_RING_DUAL': 0, 'SMRF_SEG_RULE': 2, 'SMRF_XCD_REMAP': 0}),
    (327, (155, 370), 'f32', [22, 3, 5, 44, 8, 27, 36], {'SMRF_FUSED': 2, 'SMRF_CHAIN': 0, 'SMRF_RING_DUAL': 0, 'SMRF_NT': 0, 'SMRF_XCD_REMAP': 0}),
    (328, (7, 1), 'f64', [6, 7, 8], {'SMRF_CHAIN': 0, 'SMRF_ERO_INC': 0, 'SMRF_SEG_RULE': 1, 'SMRF_XCD_REMAP': 0}),
    (329, (74, 8), 'f64', [57, 16, 17, 18, 19, 20, 14, 30], {'SMRF_FUSED': 2}),
    (330, (4, 604), 'f32', [50, 46, 59, 6], {'SMRF_RING_DUAL': 1, 'SMRF_RING_SEG': 50, 'SMRF_XCD_REMAP': 0}),
    (331, (9, 663), 'f64', [0, 42, 3, 47, 54, 53, 44], {'SMRF_ERO_INC': 0, 'SMRF_RING_DUAL': 0, 'SMRF_RING_SEG': 8, 'SMRF_SEG_RULE': 1, 'SMRF_XCD_REMAP': 0}),
    (332, (122, 699), 'f32', [44, 53, 3, 4, 54], {'SMRF_FUSED': 0, 'SMRF_ERO_INC': 2, 'SMRF_RING_DUAL': 0}),
    (333, (81, 80), 'f64', [57, 51, 52, 53, 54, 23, 15], {'SMRF_FUSED': 0, 'SMRF_ERO_INC': 0, 'SMRF_NT': 1, 'SMRF_RING_SEG': 50, 'SMRF_XCD_REMAP': 0}),
    (334, (19, 512), 'f32', [19, 31, 22, 42, 19, 61, 60, 7], {'SMRF_FUSED': 2, 'SMRF_CHAIN': 0, 'SMRF_ERO_INC': 0, 'SMRF_RING_SEG': 136, 'SMRF_SEG_RULE': 1}),
    (335, (53, 541), 'f32', [9], {'SMRF_FUSED': 2, 'SMRF_ERO_INC': 2, 'SMRF_RING_DUAL': 1, 'SMRF_RING_SEG': 136, 'SMRF_SEG_RULE': 1}),
    (336, (2, 170), 'f64', [25, 35, 13, 14], {'SMRF_CHAIN': 0, 'SMRF_NT': 1, 'SMRF_SEG_RULE': 1, 'SMRF_XCD_REMAP': 0}),
    (337, (114, 8), 'f64', [39, 22, 14, 41, 27, 7, 8], {'SMRF_CHAIN': 0, 'SMRF_SEG_RULE': 1}),
    (338, (28, 2305), 'f32', [7, 51, 9], {'SMRF_CHAIN': 0, 'SMRF_ERO_INC': 2, 'SMRF_RING_SEG': 24}),
    (339, (257, 199), 'f64', [52, 1], {'SMRF_RING_DUAL': 0, 'SMRF_RING_SEG': 50, 'SMRF_SEG_RULE': 2, 'SMRF_XCD_REMAP': 0}),
]


def large_raster(seed, shape, dtype):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, shape).cumsum(0).cumsum(1) * 0.05 + 200 + (rng.random(shape) < .06) * rng.uniform(1, 25, shape)).astype(dtype)


@pytest.mark.parametrize("case", LARGE, ids=[str(c[0]) for c in LARGE])
def test_progressive_filter_random_large_radii(nz, monkeypatch, case):
    """mask and when_dropped against tests/morph_numpy.py (the period-2n reflect at any radius), bit for bit"""
    import morph_numpy as mn
    from conftest import switch
    seed, shape, dtype, windows, switches = case
    assert 1 <= len(windows) <= 8 and min(windows) >= 0 and max(windows) <= 64
    Z = large_raster(seed, shape, np.float32 if dtype == "f32" else np.float64)
    win = np.asarray(windows)
    for name, value in switches.items():
        switch(monkeypatch, name, value)
    m, w = nz.progressive_filter(Z, win, 1, .15, return_when_dropped=True)
    m2, w2 = mn.progressive_filter(Z, win, 1, .15, return_when_dropped=True)
    assert np.array_equal(m, m2) and np.array_equal(w, w2)
