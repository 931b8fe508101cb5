"""The focal contract on the host (no GPU): the NumPy restatement (tests/focal_numpy.py) against the goldens of the
reference and against scipy.ndimage.convolve, the exported signatures, the tap list the host builds, the tile cap and
the tolerance that the GPU test allows standardised TPI."""
import inspect
import json
import math

import numpy as np
import pytest

import focal_numpy as fn
from conftest import golden
from family_checks import assert_no_scratch, device_asm, same_bits, signatures_match


def cases():
    G = golden("focal.npz")
    return G, json.loads(str(G["cases"]))


def restate(G, c):
    X = G["in_" + c["input"]]
    if c["fn"] == "convolve":
        return fn.convolve(X, G["k_" + c["kernel"]])
    if c["fn"] == "std":
        return fn.std(X, G["k_" + c["kernel"]])
    return getattr(fn, c["fn"])(X, **c["kw"])


def test_golden_covers_the_issue_cases():
    G, cs = cases()
    fns = {c["fn"] for c in cs}
    assert fns == {"convolve", "std", "topographic_position_index", "reduce_peaks"}
    assert {G["in_" + c["input"]].dtype for c in cs} == {np.dtype(np.float32), np.dtype(np.float64)}
    shapes = {G["in_" + c["input"]].shape for c in cs}
    assert shapes >= {(1, 1), (1, 7), (7, 1), (2, 5), (3, 2), (20, 26)}
    # float32 raster, integer strel: float64 out (NEP 50: np.sum(strel) is a NumPy integer scalar)
    c = next(c for c in cs if c["fn"] == "std" and c["input"] == "dtm21_f32" and c["kernel"] == "disk3")
    assert G["out_" + c["id"]].dtype == np.float64
    # zero weights over NaN cells leave finite cells that a full kernel would not
    c0 = next(c for c in cs if c["fn"] == "std" and c["input"] == "nan" and c["kernel"] == "cross0")
    c1 = next(c for c in cs if c["fn"] == "std" and c["input"] == "nan" and c["kernel"] == "ones33")
    nan = np.isnan(G["in_nan"])
    assert (np.isfinite(G["out_" + c0["id"]]) & nan).any() and not (np.isfinite(G["out_" + c1["id"]]) & nan).any()


def test_restatement_equals_every_golden():
    G, cs = cases()
    n_std = 0
    for c in cs:
        want = G["out_" + c["id"]]
        got = restate(G, c)
        assert got.dtype == want.dtype and got.shape == want.shape, c
        assert np.array_equal(np.isnan(got), np.isnan(want)), c
        if fn.exact_kind(c["fn"], c["kw"]):
            assert same_bits(got, want), (c, int(np.sum(~((got == want) | np.isnan(want)))))
        elif c["fn"] == "reduce_peaks":
            # NumPy's pow on both sides
            assert same_bits(got, want), c
        else:
            n_std += 1        # standardised TPI: see test_standardised_tpi_tolerance
    assert n_std >= 10


def test_restatement_equals_scipy_on_random_kernels():
    import scipy.ndimage as ndi
    rng = np.random.default_rng(20261020)
    for i in range(60):
        shape = tuple(int(v) for v in rng.integers(1, 24, size=2))
        kshape = tuple(int(v) for v in rng.integers(1, 9, size=2))
        X = (rng.normal(size=shape) * 10).astype(rng.choice([np.float32, np.float64]))
        w = rng.normal(size=kshape)
        if rng.random() < 0.5:
            w[rng.random(kshape) < 0.3] = 0.0
        if rng.random() < 0.3:
            X[rng.random(shape) < 0.1] = np.nan
        want = ndi.convolve(X, w, mode='nearest')
        assert same_bits(fn.convolve(X, w), want), (shape, kshape, X.dtype)


def test_distance_kernel_equals_golden_and_needs_no_gpu():
    import neilpy_amd
    G = golden("focal.npz")
    dks = json.loads(str(G["dk_cases"]))
    assert {c["kw"].get("method", "binary") for c in dks} >= {"binary", "distance", "idw", "other"}
    for c in dks:
        want = G["dk_" + c["id"]]
        with np.errstate(all="ignore"):
            for got in (neilpy_amd.distance_kernel(**c["kw"]), fn.distance_kernel(**c["kw"])):
                assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), c


def test_signatures_match_the_reference():
    import neilpy_amd
    want = signatures_match("focal_signatures.json", 4)
    assert set(want) == {"std", "topographic_position_index", "reduce_peaks", "distance_kernel"}
    got = list(inspect.signature(neilpy_amd.focal_convolve).parameters.values())
    assert [g.name for g in got[:2]] == ["X", "weights"]
    assert all(g.kind is inspect.Parameter.KEYWORD_ONLY for g in got[2:])


def test_tap_list_order_and_zero_skipping():
    from neilpy_amd import focal
    w = np.array([[1.0, 0.0, 3.0],
                  [4.0, 5.0, 0.0]])                 # 2 x 3: rows reach 0 .. 1, columns -1 .. 1
    t = focal._taps(w)
    assert t.dtype.itemsize == 16
    got = [(int(a), int(b), float(c)) for a, b, c in t]
    # s = 1, 0 outer; t = 2, 1, 0 inner; drow = 1 - s, dcol = 1 - t; zeros dropped
    assert got == [(0, 0, 5.0), (0, 1, 4.0), (1, -1, 3.0), (1, 1, 1.0)]
    rng = np.random.default_rng(5)
    for kshape in ((1, 1), (3, 3), (4, 3), (2, 2), (1, 9), (7, 1)):
        w = rng.normal(size=kshape)
        w[rng.random(kshape) < 0.3] = 0.0
        got = [(int(a), int(b), float(c)) for a, b, c in focal._taps(w)]
        assert got == [(a, b, float(c)) for a, b, c in fn.taps(w)], kshape
        assert len(got) == int(np.count_nonzero(w))
    assert len(focal._taps(np.zeros((3, 3)))) == 0
    w = np.ones((3, 3))
    w[1, 1] = np.nan                                # a NaN weight is not a zero
    assert len(focal._taps(w)) == 9
    with pytest.raises(ValueError):
        focal._taps(np.ones(3))


def test_tile_cap_is_host_logic():
    """the whole halo fits the tile up to a radius per dtype; from the next radius on the automatic path is direct"""
    from neilpy_amd import _lib
    lib = _lib.load()

    def largest(elem):
        r = 1
        while lib.smrf_focal_fits_tile(2 * r + 3, 2 * r + 3, elem):
            r += 1
        return r
    for elem in (4, 8):
        r = largest(elem)
        assert (64 + 2 * r) * (8 + 2 * r) * elem <= 53248 < (64 + 2 * r + 2) * (8 + 2 * r + 2) * elem
        assert 3 * ((64 + 2 * r) * (8 + 2 * r) * elem + 64) <= 160 * 1024      # three workgroups per CU
    assert largest(4) == 41 and largest(8) == 25
    assert lib.smrf_focal_fits_tile(1, 1, 4) == 1 and lib.smrf_focal_fits_tile(1, 2001, 4) == 0
    assert lib.smrf_focal_fits_tile(0, 3, 4) == 0 and lib.smrf_focal_fits_tile(3, 3, 2) == 0
    assert lib.smrf_focal_workspace_bytes(0, 5) == 0
    assert lib.smrf_focal_workspace_bytes(8, 64) == (4 + 2 * 1024) * 8
    assert lib.smrf_focal_workspace_bytes(8 * 2000, 64 * 3 + 1) == (4 + 2 * 2000 * 4) * 8


def test_no_cpu_fallback():
    import torch
    import neilpy_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    X = np.zeros((8, 8), np.float32)
    with pytest.raises(neilpy_amd.SmrfHipError):
        neilpy_amd.focal_convolve(X, np.ones((3, 3)))
    with pytest.raises(neilpy_amd.SmrfHipError):
        neilpy_amd.std(X, np.ones((3, 3)))
    with pytest.raises(neilpy_amd.SmrfHipError):
        neilpy_amd.topographic_position_index(X)
    with pytest.raises(neilpy_amd.SmrfHipError):
        neilpy_amd.reduce_peaks(X, 3)
    assert neilpy_amd.distance_kernel(3).shape == (7, 7)


def test_tpi_radius_is_checked_before_the_device():
    import neilpy_amd
    X = np.zeros((8, 8))
    for r in (0, -1, 1.5, 2.0, True, "2"):
        with pytest.raises(ValueError):
            neilpy_amd.topographic_position_index(X, r)


def test_standardised_tpi_tolerance():
    """The GPU test holds standardised TPI within K + 2 ulps of the restatement with exactly rounded sums (math.fsum),
    K = ceil(log2(rows * cols)) + 16: log2 n for a pairwise or tree sum, 16 for NumPy's 128-element sequential blocks
    summed in 8 lanes.  The reference's own sd (recovered from its goldens as unstandardised / standardised, which adds
    the rounding of one division) lies within K of the fsum sd on every golden: the tolerance admits the reference."""
    G, cs = cases()
    tp = [c for c in cs if c["fn"] == "topographic_position_index"]
    pairs = 0
    for c in tp:
        if not c["kw"].get("standardize", True):
            continue
        raw_kw = dict(c["kw"], standardize=False)
        raw = next(G["out_" + d["id"]] for d in tp if d["input"] == c["input"] and dict(d["kw"]) == raw_kw) \
            if "standardize" in c["kw"] else fn.tpi_planes(G["in_" + c["input"]], c["kw"].get("radius", 1))[0]
        st = G["out_" + c["id"]]
        X = G["in_" + c["input"]]
        result, sq = fn.tpi_planes(X, c["kw"].get("radius", 1))
        assert same_bits(result, raw), c
        sd = fn.tpi_sd_fsum(result, sq)
        assert sd.dtype == X.dtype
        if np.isnan(X).any():
            assert np.isnan(sd) and np.isnan(st).all(), c
            continue
        ok = np.isfinite(st) & (st != 0)
        assert ok.any(), c
        with np.errstate(all="ignore"):
            sd_ref = np.median(raw[ok].astype(np.float64) / st[ok].astype(np.float64))
        K = fn.tpi_ulps(X.shape)
        assert K == math.ceil(math.log2(X.size)) + 16
        err = abs(float(sd_ref) - float(sd)) / float(np.spacing(sd))
        print(c["id"], c["input"], c["kw"], "sd", float(sd), "reference - fsum in ulps: %.2f of K = %d" % (err, K))
        assert err <= K, (c, err, K)
        pairs += 1
    assert pairs >= 10


def test_focal_kernels_compile_without_scratch(tmp_path):
    """every kernel of csrc/focal.hip keeps its state in registers, and no fused multiply-add reaches the tap loop's
    sums: the only fp64 FMAs are those of the divide, sqrt and pow expansions of the tails (no GPU needed)"""
    import re
    text, kernels = device_asm("focal", tmp_path)
    assert len(kernels) == 24       # focal: 2 dtypes x 4 modes x {tiled, direct}; 2 TPI reduce, 2 divide, 2 min / max, 2 mix
    assert_no_scratch(text, kernels)
    # SUM / SUM_SQ instances have no tail: not one FMA in them
    bodies = dict(re.findall(r"^(_ZN\S*focal_kernel\S*):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M))
    plain = [b for n, b in bodies.items() if re.search(r"focal_kernelI[fd]Li[01]ELb[01]E", n)]
    assert len(plain) == 8
    for b in plain:
        assert "v_fma" not in b and "v_mul_f64" in b and "v_add_f64" in b
