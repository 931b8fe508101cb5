"""Relief colouring and raster statistics without a GPU: the NumPy restatement of the contract
against the reference's goldens, the replayed summation order against math.fsum, the bucket walk of csrc/select_plan.h
compiled with g++ and fuzzed against a sort, signatures, ABI exports, the error paths, the host-only cutter and the
generated code of csrc/relief.hip.

Summation bounds used here.  A sum of n terms evaluated as any tree of additions of depth d has an error of at most
d * u * sum(|x|) to first order (u = the unit roundoff: 2^-53 in float64, 2^-24 in float32); two more roundings cover
a division and a final rounding.  The device's order has d = relief_numpy.chain_depth(n); the reference's sums
(np.nanmean, np.nansum: pairwise, in the raster's dtype) are bounded by the depth of ANY order, n - 1.
"""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import relief_numpy as rn
from conftest import ROOT, golden
from family_checks import assert_no_scratch, device_asm, signatures_match

CSRC = os.path.join(ROOT, "neilpy_amd", "csrc")
U64 = 2.0 ** -53
NEW_SYMBOLS = ["smrf_raster_stats_workspace_bytes", "smrf_raster_stats_f32", "smrf_raster_stats_f64",
               "smrf_raster_stats_u8", "smrf_normalize_f32", "smrf_normalize_f64", "smrf_colortable_f32",
               "smrf_colortable_f64", "smrf_brassel_f32", "smrf_brassel_f64"]


def unit(dtype):
    return 2.0 ** -24 if dtype == np.float32 else U64


@pytest.fixture(scope="module")
def G():
    return golden("relief.npz")


def _cases(G):
    return json.loads(str(G["cases"]))


def run_restatement(G, c):
    Z = G["in_" + c["input"]]
    kw = c["kw"]
    if c["fn"] == "colortable_shade":
        return rn.colortable_shade(Z, G["lut_" + c["table"]], **kw)
    if c["fn"] == "swiss_shading":
        return rn.swiss_shading(Z, lut=G["lut_" + c["table"]], **kw)
    if c["fn"] == "brassel_atmospheric_perspective":
        return rn.brassel_atmospheric_perspective(G[c["shade"] + "_" + c["input"]], Z, **kw)
    if c["fn"] == "cutter":
        return np.array(rn.cutter(Z, **kw))
    return getattr(rn, c["fn"])(Z, **kw)


def mean_knot_tolerance(Z, knots, yrange):
    """how far np.interp's result may move when the 'mean' knot is the device's float64 mean instead of np.nanmean's:
    the two means differ by at most delta = ((d + 2) u64 + (n - 1 + 2) u_T) fsum(|x|) / n; a knot that moves by delta
    moves a result of its two segments by at most delta * |fp[j+1] - fp[j]| / |xp[j+1] - xp[j]| to first order (twice
    that is allowed for the second order), plus 4 roundings of the interpolation itself"""
    v = Z[~np.isnan(Z)].astype(np.float64)
    n = v.size
    delta = ((rn.chain_depth(Z.size) + 2) * U64 + (n + 1) * unit(Z.dtype)) * math.fsum(np.abs(v)) / n
    fp = np.asarray(yrange, dtype=np.float64)
    steep = np.max(np.abs(np.diff(fp)) / np.abs(np.diff(knots)))
    return 2 * delta * steep + 4 * U64 * np.max(np.abs(fp))


def rmse_tolerance(Z):
    """relative: half the relative error of the sum of squares (a square root halves it) of both sides, plus the
    roundings of the division, the root and the result in the raster's dtype"""
    n = int((~np.isnan(Z)).sum())
    return ((n - 1) / 2 + 3) * unit(Z.dtype) + ((rn.chain_depth(Z.size) + 2) / 2 + 1) * U64


def test_restatement_equals_every_golden(G):
    cases = _cases(G)
    assert len(cases) >= 200
    for c in cases:
        want = G["out_" + c["id"]]
        got = np.asarray(run_restatement(G, c))
        assert got.dtype == want.dtype and got.shape == want.shape, (c, got.dtype, want.dtype)
        Z = G["in_" + c["input"]]
        if c["fn"] == "normalize" and 'mean' in c["kw"].get("xrange", []):
            knots = rn.knots_of(Z, c["kw"]["xrange"])
            tol = mean_knot_tolerance(Z, knots, c["kw"]["yrange"])
            assert np.array_equal(np.isnan(got), np.isnan(want)), c
            ok = ~np.isnan(want)
            assert np.all(np.abs(got[ok] - want[ok]) <= tol), (c, float(np.max(np.abs(got[ok] - want[ok]))), tol)
        elif c["fn"] == "rmse":
            tol = rmse_tolerance(Z) * abs(float(want))
            assert abs(float(got) - float(want)) <= tol or (np.isnan(got) and np.isnan(want)) or got == want, (c, got, want)
        else:
            assert np.array_equal(got, want, equal_nan=(want.dtype.kind == 'f')), c


def test_golden_set_covers_the_contract(G):
    cases = _cases(G)
    assert {c["fn"] for c in cases} == {"colortable_shade", "swiss_shading", "rmse", "cutter", "normalize",
                                        "brassel_atmospheric_perspective"}
    shaded = {c["input"] for c in cases if c["fn"] == "colortable_shade"}
    for name in ("nan", "nan_f32", "const", "inf", "dtm21_f32", "terrace", "sq2", "r2x5"):
        assert name in shaded, name
    assert np.isnan(G["in_nan"]).any() and np.isinf(G["in_inf"]).any()
    assert np.ptp(G["in_const"]) == 0 and G["in_dtm21_f32"].dtype == np.float32
    assert G["in_sq2"].shape == (2, 2) and G["in_r2x5"].shape == (2, 5)
    assert {c["table"] for c in cases if c["fn"] == "colortable_shade"} == {"swiss", "ghc", "gray", "rand4"}
    assert G["lut_ghc"].shape == (256, 256) and G["lut_swiss"].shape == (256, 256, 3)
    assert G["lut_rand4"].shape == (256, 256, 4) and G["lut_swiss"].dtype == np.uint8
    # a NaN or constant raster indexes row 0 of the table everywhere
    for d in ("nan", "const"):
        assert (rn.table_index(G["in_" + d]) == 0).all()
    norm = [c["kw"] for c in cases if c["fn"] == "normalize"]
    names = {k for kw in norm for k in kw.get("xrange", ['min', 'max']) if isinstance(k, str)}
    assert names == {"min", "max", "mean", "median"}
    assert {len(kw.get("xrange", [0, 0])) for kw in norm} == {2, 3, 4}
    assert any(all(not isinstance(k, str) for k in kw.get("xrange", ['min'])) for kw in norm)
    br = [c for c in cases if c["fn"] == "brassel_atmospheric_perspective"]
    assert {c["shade"] for c in br} == {"h", "hf", "hf32"}
    assert {G["out_" + c["id"]].dtype for c in br} == {np.dtype(np.uint8), np.dtype(np.float64)}      # was_int both ways
    assert any(c["kw"].get("reverse") for c in br) and any("Zmid" in c["kw"] for c in br)
    assert {c["kw"].get("flat", 180) > 1 for c in br} == {True, False}
    assert any(c["input"] == "nan" for c in br)
    below = above = False
    for c in br:
        if c["shade"] == "h" and c["kw"].get("C2"):
            v, was_int = rn.brassel_value(G["h_" + c["input"]], G["in_" + c["input"]], **c["kw"])
            assert was_int
            with np.errstate(invalid='ignore'):
                below |= bool((np.round(255 * v) < 0).any())
                above |= bool((np.round(255 * v) > 255).any())
    assert below and above                      # both wrap directions of the uint8 cast
    assert np.array_equal(rn.wrap_u8(np.array([-3, 260, -300, 70000, np.nan])), np.array([253, 4, 212, 112, 0]))
    assert str(G["numpy_version"]).startswith("2.")


def test_interp_formula_is_np_interp():
    """the per-cell formula the device evaluates, against np.interp on knots of every kind the contract names"""
    rng = np.random.default_rng(7)
    xp = np.array([-1.5, 0.25, 0.25, 3.0, 8.0])
    fp = np.array([2.0, -1.0, 4.0, 4.0, 0.5])
    x = np.concatenate([rng.uniform(-3, 10, 3000), xp, [np.nan, -np.inf, np.inf, -0.0]])
    assert np.array_equal(rn.interp(x, xp, fp), np.interp(x, xp, fp), equal_nan=True)
    xp2, fp2 = np.array([1.0, np.inf]), np.array([0.0, 1.0])
    x2 = np.array([0.0, 1.0, 5.0, np.inf, np.nan])
    with np.errstate(all='ignore'):
        assert np.array_equal(rn.interp(x2, xp2, fp2), np.interp(x2, xp2, fp2), equal_nan=True)
    assert np.array_equal(rn.interp(np.array([7.0, 6.0, 8.0]), [7.0, 7.0], [0.0, 1.0]),
                          np.interp(np.array([7.0, 6.0, 8.0]), [7.0, 7.0], [0.0, 1.0]))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 5000, 300001])
def test_replayed_summation_order_agrees_with_fsum(n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 6, size=n)
    d = rn.chain_depth(n)
    assert d == -(-n // (rn.blocks_of(n) * 256)) + 8 + rn.blocks_of(n)
    exact = math.fsum(x)
    bound = (d + 2) * U64 * math.fsum(np.abs(x))
    assert abs(float(rn.ordered_sum(x)) - exact) <= bound
    st = rn.raster_stats(x.reshape(1, n), ('mean', 'sum_sq'))
    assert abs(float(st['mean']) - exact / n) <= bound / n
    assert abs(float(st['sum_sq']) - math.fsum(x * x)) <= (d + 2) * U64 * math.fsum(x * x)


def test_restated_statistics_follow_numpy():
    rng = np.random.default_rng(3)
    for dt in (np.float32, np.float64):
        for n in (1, 2, 3, 8, 101, 1000):
            X = (rng.normal(size=(1, n)) * 50).astype(dt)
            if n > 3:
                X[0, rng.random(n) < 0.3] = np.nan
                X[0, 0] = 1.0
            st = rn.raster_stats(X)
            assert st['median'] == np.nanmedian(X) and st['median'].dtype == dt
            assert st['min'] == np.nanmin(X) and st['max'] == np.nanmax(X)
            assert st['count'] == int((~np.isnan(X)).sum()) and st['has_nan'] == bool(np.isnan(X).any())
    st = rn.raster_stats(np.full((2, 3), np.nan))
    assert st['count'] == 0 and all(np.isnan(st[k]) for k in ('min', 'max', 'mean', 'median', 'sum_sq'))


def test_signatures_match_the_reference():
    signatures_match("relief_signatures.json", 6)


def test_abi_names_declared_and_exported():
    from neilpy_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from neilpy_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "smrf_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and ("SMRF_API" in hdr and (" " + n + "(") in hdr), n
    import re
    for name in ("STATS_MOMENTS", "STATS_MEDIAN", "STATS_ROW", "STATS_COUNT", "STATS_NAN", "STATS_MIN", "STATS_MAX",
                 "STATS_MEAN", "STATS_SUM_SQ", "STATS_MEDIAN_AT", "SHADE_U8", "SHADE_F32", "SHADE_F64",
                 "BRASSEL_WAS_INT", "BRASSEL_ZMID", "BRASSEL_REVERSE"):
        assert re.search(r"#define SMRF_%s %d\b" % (name, getattr(_lib, name)), hdr), name
    assert "#define SMRF_ABI_VERSION 1" in hdr


def test_no_cpu_fallback():
    import torch
    import neilpy_amd as na
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    Z = np.zeros((6, 6))
    lut = np.zeros((256, 256), np.uint8)
    for call in (lambda: na.raster_stats(Z), lambda: na.normalize(Z), lambda: na.rmse(Z),
                 lambda: na.colortable_shade(Z, lut), lambda: na.swiss_shading(Z, lut=np.zeros((256, 256, 3))),
                 lambda: na.brassel_atmospheric_perspective(Z, Z, 2)):
        with pytest.raises(na.SmrfHipError):
            call()


def test_error_paths_need_no_device():
    """every documented error is raised on the arguments alone, before the device is asked for"""
    import neilpy_amd as na
    Z = np.zeros((6, 6))
    lut = np.zeros((256, 256, 3), np.uint8)
    for name in ('swiss', 'gray', 'gray_high_contrast', 'x.png'):
        with pytest.raises(NotImplementedError, match="as an array"):
            na.colortable_shade(Z, name)
    with pytest.raises(NotImplementedError):
        na.colortable_shade(Z)                         # the reference's default is a named table
    for bad in (np.zeros((256, 255)), np.zeros((256, 256, 2)), np.zeros((255, 256, 3)), np.zeros((256, 256, 3, 1)),
                np.zeros(256)):
        with pytest.raises(ValueError, match="colour table"):
            na.colortable_shade(Z, bad)
        with pytest.raises(ValueError, match="colour table"):
            na.swiss_shading(Z, lut=bad)
    for shape in ((1, 7), (7, 1), (1, 1)):
        with pytest.raises(ValueError, match="too small to calculate a numerical gradient"):
            na.colortable_shade(np.zeros(shape), lut)
        with pytest.raises(ValueError, match="too small to calculate a numerical gradient"):
            na.swiss_shading(np.zeros(shape), lut=lut)
    with pytest.raises(ValueError, match="greater than one"):
        na.brassel_atmospheric_perspective(Z, Z, 0.5)
    with pytest.raises(ValueError, match="shape"):
        na.brassel_atmospheric_perspective(np.zeros((6, 5)), Z, 2)
    with pytest.raises(ValueError):
        na.normalize(Z, ['min'], [0])
    with pytest.raises(ValueError):
        na.normalize(Z, ['min', 'max'], [0, 1, 2])
    with pytest.raises(ValueError, match="unknown knot"):
        na.normalize(Z, ['min', 'mode'], [0, 1])
    with pytest.raises(ValueError, match="unknown statistic"):
        na.raster_stats(Z, ('min', 'mode'))
    with pytest.raises(ValueError, match="2-D"):
        na.rmse(np.zeros(5))


def test_cutter_is_views_of_arrays_and_tensors():
    import torch
    import neilpy_amd as na
    x = np.arange(20 * 26, dtype=np.float32).reshape(20, 26)
    for r, c in ((2, 2), (5, 13), (1, 1), (20, 26)):
        got = na.cutter(x, r, c)
        want = [np.hsplit(i, c) for i in np.vsplit(x, r)]
        t = na.cutter(torch.from_numpy(x), r, c)
        assert len(got) == len(t) == r and all(len(g) == c for g in got) and all(len(g) == c for g in t)
        for i in range(r):
            for j in range(c):
                assert np.array_equal(got[i][j], want[i][j]) and np.shares_memory(got[i][j], x)
                assert np.array_equal(t[i][j].numpy(), want[i][j]) and np.shares_memory(t[i][j].numpy(), x)
    for r, c in ((3, 2), (2, 4), (7, 13)):
        with pytest.raises(ValueError) as e_np:
            [np.hsplit(i, c) for i in np.vsplit(x, r)]
        for arg in (x, torch.from_numpy(x)):
            with pytest.raises(ValueError) as e:
                na.cutter(arg, r, c)
            assert str(e.value) == str(e_np.value)
    with pytest.raises(ValueError, match="2 or more dimensions"):
        na.cutter(torch.zeros(6), 2, 1)


def test_relief_kernels_compile_without_scratch(tmp_path):
    text, kernels = device_asm("relief", tmp_path)
    # moments x 3 dtypes, histogram and walk x 2, normalize x 2, colortable x 2, brassel x 3 shades x 2
    assert len(kernels) == 3 + 2 + 2 + 2 + 2 + 6
    assert_no_scratch(text, kernels)


# ------------------------------------------------------------------------------------------
# csrc/select_plan.h on the CPU
# ------------------------------------------------------------------------------------------
_SHIM = r"""
#include "select_plan.h"
using namespace smrf;
extern "C" {
int sp_buckets() { return SELECT_BUCKETS; }
int sp_passes(int kb) { return select_passes(kb); }
int sp_lo(int kb, int p) { return select_lo(kb, p); }
int sp_hi(int kb, int p) { return select_hi(kb, p); }
uint64_t sp_total(const uint64_t* row) { return select_total(row); }
void sp_begin(SelectState* s, uint64_t n) { select_begin(*s, n); }
void sp_step(const uint64_t* rows, int lo, SelectState* s) { select_step(rows, lo, *s); }
int sp_walk(const uint64_t* row, uint64_t* rank) { return select_walk(row, *rank); }
}
"""


class State(ctypes.Structure):
    _fields_ = [("prefix", ctypes.c_uint64 * 2), ("rank", ctypes.c_uint64 * 2), ("count", ctypes.c_uint64)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("select_plan")
    src = tmp / "shim.cpp"
    src.write_text(_SHIM)
    so = tmp / "select_plan.so"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                        str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    lib = ctypes.CDLL(str(so))
    lib.sp_total.restype = ctypes.c_uint64
    lib.sp_begin.argtypes = [ctypes.POINTER(State), ctypes.c_uint64]
    return lib


def _row_ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def select(plan, keys, kb):
    """the device's passes on the host: histograms by NumPy, every walk by select_plan.h; asserts the invariants"""
    B = plan.sp_buckets()
    keys = np.asarray(keys, dtype=np.uint64)
    st = State()
    for p in range(plan.sp_passes(kb)):
        lo, hi = plan.sp_lo(kb, p), plan.sp_hi(kb, p)
        assert 0 <= lo < hi <= kb and hi - lo <= 11 and (p > 0 or hi == kb)
        rows = np.zeros((2, B), dtype=np.uint64)
        split = p > 0 and st.prefix[0] != st.prefix[1]
        for k in range(2 if split else 1):
            sel = keys if p == 0 else keys[(keys >> np.uint64(hi)) == np.uint64(st.prefix[k] >> hi)]
            dig = ((sel >> np.uint64(lo)) & np.uint64((1 << (hi - lo)) - 1)).astype(np.int64)
            rows[k] = np.bincount(dig, minlength=B).astype(np.uint64)
        if p == 0:
            assert plan.sp_total(_row_ptr(rows)) == len(keys)
            plan.sp_begin(ctypes.byref(st), len(keys))
            assert (st.rank[0], st.rank[1]) == ((len(keys) - 1) // 2, len(keys) // 2)
        plan.sp_step(_row_ptr(rows), lo, ctypes.byref(st))
        for k in range(2):
            d = (st.prefix[k] >> lo) & ((1 << (hi - lo)) - 1)
            assert st.rank[k] < rows[k if split else 0][d], (p, k)       # the residue stays inside the chosen bucket
    assert plan.sp_lo(kb, plan.sp_passes(kb) - 1) == 0
    return st.prefix[0], st.prefix[1]


def _check(plan, keys, kb):
    s = np.sort(np.asarray(keys, dtype=np.uint64))
    n = len(s)
    assert select(plan, keys, kb) == (int(s[(n - 1) // 2]), int(s[n // 2])), (n, kb)


def test_select_plan_walk_on_random_histograms(plan):
    rng = np.random.default_rng(11)
    B = plan.sp_buckets()
    assert B == 2048 and plan.sp_passes(32) == 3 and plan.sp_passes(64) == 6
    for trial in range(200):
        row = rng.integers(0, 50, size=B).astype(np.uint64)
        row[rng.random(B) < rng.uniform(0, 0.99)] = 0
        if trial % 10 == 0:
            row[:] = 0
            row[rng.integers(0, B)] = rng.integers(1, 2 ** 40)            # all mass in one bucket
        total = int(row.sum())
        if total == 0:
            continue
        cum = np.cumsum(row)
        for rank in {0, total - 1, total // 2, int(rng.integers(0, total))}:
            r = ctypes.c_uint64(rank)
            d = plan.sp_walk(_row_ptr(row), ctypes.byref(r))
            want = int(np.searchsorted(cum, rank, side='right'))
            assert d == want and r.value == rank - (int(cum[want - 1]) if want else 0) and r.value < row[d]


@pytest.mark.parametrize("kb", [32, 64])
def test_select_plan_finds_both_middle_keys(plan, kb):
    rng = np.random.default_rng(kb)
    top = (1 << kb) - 1
    for n in (1, 2, 3, 4, 5, 64, 1000, 1001):
        _check(plan, rng.integers(0, top, size=n, dtype=np.uint64, endpoint=True), kb)
        _check(plan, np.full(n, rng.integers(0, top, dtype=np.uint64)), kb)                    # all keys equal
        _check(plan, rng.integers(0, 256, size=n, dtype=np.uint64), kb)                        # the last pass decides
        base = int(rng.integers(0, top >> 12)) << 12
        _check(plan, np.uint64(base) + rng.integers(0, 4096, size=n, dtype=np.uint64), kb)     # one bucket until the end
    # the two middle ranks straddle a bucket boundary of the top digit, of a middle digit and of the last one
    for shift in (kb - 11, kb - 22, 0):
        for half in (1, 2, 500):
            lo = (np.uint64(5) << np.uint64(shift)) - rng.integers(1, 3, size=half, dtype=np.uint64)
            hi = (np.uint64(5) << np.uint64(shift)) + rng.integers(0, 3, size=half, dtype=np.uint64)
            _check(plan, np.concatenate([lo, hi]), kb)
            _check(plan, np.concatenate([lo, hi, hi[:1]]), kb)
    _check(plan, np.array([0, top], dtype=np.uint64), kb)
    _check(plan, np.array([top], dtype=np.uint64), kb)
    for trial in range(30):
        n = int(rng.integers(1, 400))
        bits = int(rng.integers(1, kb + 1))
        _check(plan, rng.integers(0, (1 << bits) - 1, size=n, dtype=np.uint64, endpoint=True), kb)
