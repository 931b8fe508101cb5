"""Every kernel family on poisoned, guard-banded device memory (tests/guarded.py; its own proof is
tests/test_guarded_host.py).

``run_guarded`` calls a public function twice on the same inputs, once with every byte the package allocates (and the
surroundings of every input) poisoned with 0xFF - NaN in every float type, 255 in uint8 - and once with 0x5A, an ordinary
finite number in every float type, and asserts:

* Reference: the result matches the family's NumPy restatement or the oracle under the comparison and the margins of that
  family's own GPU test, imported from there;
* Identity: the two runs agree bit for bit in every returned array - an output cell nobody wrote, a read of scratch
  nobody wrote and an over-read of an input's surroundings that reaches the output all differ between the poisons;
* Guards: no byte of the 4096 in front of and behind any allocation changed (outputs, workspaces, scratch planes, inputs);
* Ownership: every returned tensor lives in an arena of the harness, NOT_OWNED below being the explicit exceptions;
* Inputs: every input has the bits it came with (for the in-place fills: the cells that were known).

No function here is exempt from Identity: every kernel of the package is bit-reproducible from run to run.

Workspaces.  The public wrappers of ``smrf_raster_stats_*``, ``smrf_nearest_*``, ``smrf_points_nn_*``, ``smrf_voxel_*``,
``smrf_springs_lsqr_f64``, ``smrf_fda_lsqr_f64`` and ``smrf_progressive_filter_*`` allocate ``*_workspace_bytes(...)`` bytes
as they are (``exact_workspace`` asserts that such an allocation was served); the TPI workspace of ``smrf_focal_*`` is
rounded by its wrapper.  The last section calls every one of these entry points once more straight through ctypes with
a workspace of exactly that many bytes carved by the harness, so that the tail guard sits on the first byte the library
did not ask for whatever a wrapper does.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import focal_numpy as fnp
import morph_numpy as mn
import morphometry_numpy as mnp
import nearest_numpy as nn
import points_numpy as pn
import relief_numpy as rn
import surface_numpy as sn
import terrain_numpy as tn
import voxel_numpy as vn
from conftest import GOLDEN, golden, load_sample
from family_checks import assert_close, assert_exact
from guarded import POISONS, guarded, same_bits

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------
# the package's exports, classified (tests/test_guarded_host.py compares the three lists with neilpy_amd's namespace)
# ------------------------------------------------------------------------------------------
# called below under the harness
GUARDED = ("slope", "aspect", "hillshade", "multiple_illumination", "esri_slope", "curvature", "esri_curvature",
           "zevenbergen_and_thorne_curvature", "evans_curvature", "wilson_gallant_curvature",
           "focal_convolve", "std", "topographic_position_index", "reduce_peaks",
           "openness", "skyview_factor", "count_openness", "geomorphons", "ternary_pattern_from_openness",
           "scaled_morphometry", "vip_score", "ashift",
           "raster_stats", "normalize", "rmse", "colortable_shade", "swiss_shading", "brassel_atmospheric_perspective",
           "progressive_filter", "erosion", "dilation", "opening",
           "create_dem", "inpaint_nearest", "nearest_source", "inpaint_nans_by_springs", "inpaint_nans_by_fda",
           "nearest_points", "chamfer_distance", "voxelize", "pssm", "smrf", "read_las_xyz")
# launches a kernel and is not called here: name -> reason
LEFT_OUT = {}
# exported and launches nothing: host helpers, constants, views and table look-ups by torch indexing
NO_KERNEL = ("SmrfHipError", "load_library", "LIB_PATH", "Affine", "edges_from_IT", "from_origin", "write_worldfile", "disk",
             "last_stats", "distance_kernel", "read_las", "write_las", "triangle_height", "cutter", "z_factor", "synth_dem",
             "synth_points", "geomorphon_cmap", "get_lowest_equivalent", "int2base", "progressive_window",
             "terrain_code_to_geomorphon")

# Returned tensors that do not live in an arena: (function, path of the leaf in the result) -> the torch op that made it.
# Every entry names a torch op, not a kernel; an entry whose tensor IS owned fails too, so the table cannot go stale.
NOT_OWNED = {
    ("rmse", ""): "torch.tensor(float(v)): the 0-dim result is built from the host's statistics row",
    ("smrf", "[4]['above_ground_height']"): "zd - elev_d, a torch subtraction of two vectors the kernels wrote",
    ("smrf", "[4]['when_dropped']"): "drop[ri, ci], a torch gather from the kernels' drop raster",
    ("sharded", "[0]"): "mask.bool() in tests/sharded_one_gpu.py, after copy_ stitched the bands' masks together",
}

DEVICE = "cuda:0"
AUTO, TILED, DIRECT = 0, 1, 2
F32, F64 = np.float32, np.float64


def F(name):
    """a guarded export by name: as a literal name, or as F(fn) with fn drawn from SURFACE, TERRAIN or DISK below -
    tests/test_guarded_host.py reads GUARDED against exactly these"""
    import neilpy_amd
    assert name in GUARDED, name
    return getattr(neilpy_amd, name)


# ------------------------------------------------------------------------------------------
# run_guarded
# ------------------------------------------------------------------------------------------
def _is_affine(v):
    return type(v).__name__ == "Affine"


def _leaves(v, path=""):
    if _is_affine(v):
        yield path, v
    elif isinstance(v, (tuple, list)):
        for i, e in enumerate(v):
            yield from _leaves(e, "%s[%d]" % (path, i))
    elif isinstance(v, dict):
        for k, e in v.items():
            yield from _leaves(e, "%s[%r]" % (path, k))
    else:
        yield path, v


def _np(v):
    import torch
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    if _is_affine(v):
        return np.array(tuple(v)[:6], dtype=np.float64)
    return v if v is None else np.asarray(v)


def _rebuild(v, f):
    if _is_affine(v):
        return f(v)
    if isinstance(v, (tuple, list)):
        return type(v)(_rebuild(e, f) for e in v)
    if isinstance(v, dict):
        return {k: _rebuild(e, f) for k, e in v.items()}
    return f(v)


def run_guarded(fn, inputs, kw=None, *, name, reference=None, known=None, ctx=None, after=None):
    """``fn(*inputs as harness tensors, **kw)`` under both poisons with the five assertions of the module docstring.
    ``name`` keys NOT_OWNED; ``reference(result as NumPy)`` asserts against the restatement; ``known(i, array)`` is the
    mask of cells of input ``i`` that must keep their bits (default: all of them); ``after(g)`` looks at the harness.
    Returns the result as NumPy arrays."""
    import torch
    runs = []
    for poison in POISONS:
        with guarded(DEVICE, poison) as g:
            tens = [g.tensor(a) if isinstance(a, np.ndarray) else a for a in inputs]
            res = fn(*tens, **(kw or {}))
            torch.cuda.synchronize()
        tag = (name, ctx, "poison 0x%02X" % poison)
        g.check()                                                                        # Guards
        for path, v in _leaves(res):                                                     # Ownership
            if isinstance(v, torch.Tensor):
                if (name, path) in NOT_OWNED:
                    assert not g.owns(v), (tag, path, "is owned: drop its NOT_OWNED entry")
                else:
                    assert g.owns(v), (tag, path or "result", "was not allocated through the harness")
        for i, (a, t) in enumerate(zip(inputs, tens)):                                   # Inputs
            if isinstance(a, np.ndarray):
                assert g.unchanged(t, where=known(i, a) if known else None), (tag, "input %d was modified" % i)
        if after:
            after(g)
        runs.append(_rebuild(res, _np))
        del g, tens, res
    a, b = (list(_leaves(r)) for r in runs)                                              # Identity
    assert [p for p, _ in a] == [p for p, _ in b], (name, ctx)
    for (path, u), (_, v) in zip(a, b):
        if u is None or v is None:
            assert u is None and v is None, (name, ctx, path)
            continue
        diff = int(np.sum(u.view(np.uint8) != v.view(np.uint8))) if u.shape == v.shape and u.dtype == v.dtype and u.ndim else -1
        assert same_bits(u, v), (name, ctx, path, "the runs under 0xFF and 0x5A differ in %d bytes" % diff)
    if reference is not None:                                                            # Reference
        reference(runs[0])
    return runs[0]


def exact_workspace(nbytes):
    """an ``after=`` that asserts the harness served a uint8 allocation of exactly ``nbytes`` bytes"""
    import torch

    def look(g):
        sizes = [a.nbytes for a in g.arenas if a.dtype == torch.uint8 and len(a.shape) == 1]
        assert int(nbytes) in sizes, (int(nbytes), sizes)
    return look


def lib():
    from neilpy_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------
# rasters
# ------------------------------------------------------------------------------------------
TILE_SHAPES = ((1, 1), (1, 65), (65, 1), (9, 65), (67, 131))      # 64 x 8 tiles: one cell past a tile in both axes, several tiles
GRADIENT_SHAPES = ((2, 65), (65, 2), (9, 65), (67, 131))
NAN_SHAPE = (67, 131)


def raster(shape, dtype, nan=False, seed=0):
    from test_gpu_focal import _raster
    return _raster(np.random.default_rng(20261101 + seed + 1000 * shape[0] + shape[1]), shape, dtype, nan=nan)


def cases_of(shapes, dtypes=(F32, F64)):
    """every shape and dtype without NaN, and the largest shape once more with 2 % NaN cells"""
    for dtype in dtypes:
        for shape in shapes:
            yield raster(shape, dtype), (shape, np.dtype(dtype).name)
        yield raster(NAN_SHAPE, dtype, nan=True, seed=7), (NAN_SHAPE, np.dtype(dtype).name, "nan")


def golden_kw(npz, fn):
    """the keywords of the golden case of ``fn`` that sets the most of them (the first such case)"""
    cs = [c for c in json.loads(str(golden(npz)["cases"])) if c["fn"] == fn]
    return dict(max(cs, key=lambda c: len(c["kw"]))["kw"])


# ------------------------------------------------------------------------------------------
# surface
# ------------------------------------------------------------------------------------------
SURFACE = tuple(sorted(sn.FUNCS))


@pytest.mark.parametrize("fn", SURFACE)
def test_surface(gpu_device, fn):
    from test_gpu_surface import GRADIENT, compare
    kw = golden_kw("surface.npz", fn)
    for Z, ctx in cases_of(GRADIENT_SHAPES if fn in GRADIENT else TILE_SHAPES):
        run_guarded(lambda Zt: F(fn)(Zt, **sn.decode_kw(kw)), [Z], name=fn, ctx=(ctx, kw),
                    reference=lambda got: compare(fn, Z, kw, got, sn.run(fn, Z, kw)))


# ------------------------------------------------------------------------------------------
# focal
# ------------------------------------------------------------------------------------------
def focal_kernels():
    rng = np.random.default_rng(20261102)
    w7 = rng.normal(size=(7, 7))
    w7[rng.random((7, 7)) < 0.3] = 0.0                       # zero taps are skipped by the tap table
    assert (w7 == 0).any()
    return {"7x7 with zero taps": w7, "1x9": rng.normal(size=(1, 9)), "6x4": rng.normal(size=(6, 4))}


@pytest.mark.parametrize("dtype", [F32, F64])
def test_focal_convolve_and_std(gpu_device, dtype):
    from test_gpu_focal import assert_bits
    for Z, ctx in cases_of(TILE_SHAPES, (dtype,)):
        for kname, w in focal_kernels().items():
            pos = np.abs(w) + (w != 0) * 0.1
            want_c, want_s = fnp.convolve(Z, w), fnp.std(Z, pos)
            for impl in (AUTO, TILED, DIRECT):
                c = (ctx, kname, impl)
                run_guarded(lambda Zt: F("focal_convolve")(Zt, w, impl=impl), [Z], name="focal_convolve", ctx=c,
                            reference=lambda got: assert_bits(got, want_c, c))
                run_guarded(lambda Zt: F("std")(Zt, pos, impl=impl), [Z], name="std", ctx=c,
                            reference=lambda got: assert_bits(got, want_s, c))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_focal_tpi_and_reduce_peaks(gpu_device, dtype):
    """TPI: the partials workspace and the single-workgroup reduce behind the standardising sd"""
    from test_gpu_focal import assert_bits, check_tpi
    for Z, ctx in cases_of(TILE_SHAPES, (dtype,)):
        for kw in (dict(radius=1, standardize=True), dict(radius=4, standardize=True), dict(radius=4, standardize=False)):
            for impl in (AUTO, TILED, DIRECT):
                c = (ctx, kw, impl)
                run_guarded(lambda Zt: F("topographic_position_index")(Zt, impl=impl, **kw), [Z],
                            name="topographic_position_index", ctx=c, reference=lambda got: check_tpi(Z, got, kw, c))
        want = fnp.reduce_peaks(Z, 3)
        for impl in (AUTO, TILED, DIRECT):
            c = (ctx, "reduce_peaks", impl)
            run_guarded(lambda Zt: F("reduce_peaks")(Zt, 3, impl=impl), [Z], name="reduce_peaks", ctx=c,
                        reference=lambda got: assert_bits(got, want, c))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_focal_tpi_workspace_exact(gpu_device, dtype):
    """smrf_focal_* (TPI) straight through ctypes with a workspace of exactly smrf_focal_workspace_bytes: the tail guard
    sits on the first byte the library did not ask for"""
    import torch
    from neilpy_amd import _lib, focal
    from test_gpu_focal import check_tpi
    L = lib()
    sfx = "f32" if dtype == F32 else "f64"
    for shape in TILE_SHAPES + ((300, 517),):
        Z = raster(shape, dtype)
        for radius, impl in ((1, TILED), (4, DIRECT)):
            kw = dict(radius=radius, standardize=True)
            w = fnp.tpi_weights(radius)
            taps = focal._taps(w)
            nbytes = int(L.smrf_focal_workspace_bytes(shape[0], shape[1]))
            assert nbytes >= 32

            def call(Zt):
                g = __import__("guarded")._active[0]
                ws = g.bytes_of(nbytes)
                tab = g.tensor(taps.view(np.uint8))
                out = torch.empty_like(Zt)
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
                _lib.check(getattr(L, "smrf_focal_" + sfx)(p(Zt), None, shape[0], shape[1], _lib.FOCAL_TPI, p(tab), len(taps),
                                                           w.shape[0], w.shape[1], 0.0, p(out), None, p(ws), nbytes, impl, st))
                _lib.check(getattr(L, "smrf_focal_divide_" + sfx)(p(out), out.numel(), C.c_void_p(ws.data_ptr() + 16), st))
                return out
            c = (shape, sfx, radius, impl)
            run_guarded(call, [Z], name="smrf_focal", ctx=c, reference=lambda got: check_tpi(Z, got, kw, c))


# ------------------------------------------------------------------------------------------
# terrain
# ------------------------------------------------------------------------------------------
TERRAIN = ("openness", "skyview_factor", "count_openness", "geomorphons", "ternary_pattern_from_openness")


def terrain_call(fn, Z, kw, impl):
    """tests/test_gpu_terrain.py's call(): count_openness takes its first three parameters by position"""
    kw = dict(kw)
    if fn == "count_openness":
        return F(fn)(Z, kw.pop("cellsize"), kw.pop("lookup_pixels"), kw.pop("threshold_angle"), **kw, impl=impl)
    return F(fn)(Z, **kw, impl=impl)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("fn", TERRAIN)
def test_terrain(gpu_device, fn, dtype):
    """lookup_pixels 1, the LDS tile's halo cap and cap + 1 (the taps past the halo come from global memory), every impl;
    geomorphons with enhance (both marches from one launch, L > 16) and, like openness and count_openness, once fast"""
    from neilpy_amd import _lib
    from test_gpu_terrain import compare
    cap = _lib.TERRAIN_HALO_CAP["f32" if dtype == F32 else "f64"]
    base = golden_kw("terrain.npz", fn)
    for Z, ctx in cases_of(TILE_SHAPES, (dtype,)):
        variants = [(L, {}) for L in (1, cap, cap + 1)]
        if fn in ("openness", "count_openness", "geomorphons"):
            variants.append((cap + 1, dict(fast=True, how_fast=20)))
        for L, extra in variants:
            kw = dict(base, lookup_pixels=L, **extra)
            if fn == "geomorphons":
                kw["enhance"] = True
            kw.pop("neighbors", None)
            want = tn.run(fn, Z, kw)
            for impl in (AUTO, TILED, DIRECT):
                c = (ctx, kw, impl)
                run_guarded(lambda Zt: terrain_call(fn, Zt, kw, impl), [Z], name=fn, ctx=c,
                            reference=lambda got: compare(fn, Z, kw, got, want))


# ------------------------------------------------------------------------------------------
# morphometry
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_morphometry(gpu_device, dtype):
    from test_gpu_morphometry import compare_morphometry
    kw_m, kw_v, kw_a = (golden_kw("morphometry.npz", f) for f in ("scaled_morphometry", "vip_score", "ashift"))
    for Z, ctx in cases_of(TILE_SHAPES, (dtype,)):
        for kw in (kw_m, dict(kw_m, lookup_pixels=64), dict(kw_m, lookup_pixels=65)):      # a wave's width and past it
            run_guarded(lambda Zt: F("scaled_morphometry")(Zt, **kw), [Z], name="scaled_morphometry", ctx=(ctx, kw),
                        reference=lambda got: compare_morphometry(got, mnp.scaled_morphometry(Z, **kw), (ctx,)))
        run_guarded(lambda Zt: F("vip_score")(Zt, **kw_v), [Z], name="vip_score", ctx=ctx,
                    reference=lambda got: assert_exact(got, mnp.vip_score(Z, **kw_v), ctx))
        for kw in (kw_a, dict(direction=4, n=3), dict(direction=7, n=64)):
            run_guarded(lambda Zt: F("ashift")(Zt, **kw), [Z], name="ashift", ctx=(ctx, kw),
                        reference=lambda got: assert_exact(got, mnp.ashift(Z, **kw), (ctx, kw)))


# ------------------------------------------------------------------------------------------
# relief
# ------------------------------------------------------------------------------------------
def stats_match(got, X, ctx):
    """tests/test_gpu_relief.py's check_stats on a result in hand"""
    from test_gpu_relief import same_float_bits
    want = rn.raster_stats(X)
    assert set(got) == set(want) == {'count', 'min', 'max', 'mean', 'median', 'sum_sq', 'has_nan'}, ctx
    assert int(got['count']) == want['count'] and bool(got['has_nan']) == want['has_nan'], (ctx, got, want)
    for k in ('min', 'max', 'median'):
        assert got[k].dtype == want[k].dtype == X.dtype, (ctx, k)
        assert np.array_equal(got[k], want[k], equal_nan=True), (ctx, k, got[k], want[k])
    for k in ('mean', 'sum_sq'):
        assert same_float_bits(got[k], want[k]), (ctx, k, got[k], want[k])
    if want['count']:
        with np.errstate(all='ignore'):
            assert np.array_equal(got['median'], np.nanmedian(X), equal_nan=True), ctx


@pytest.mark.parametrize("dtype", [F32, F64])
def test_raster_stats(gpu_device, dtype):
    """n = 1, 65, 257 and 500 x 600, the grid-stride loop's second trip; moments and the radix select's workspace"""
    from neilpy_amd import _lib
    rng = np.random.default_rng(1)
    cases = [((rng.normal(size=(1, n)) * 100).astype(dtype), n) for n in (1, 65, 257)]
    X = (rng.normal(size=(500, 600)) * 30 + 400).astype(dtype)
    cases.append((X, "500x600"))
    Xn = X.copy()
    Xn[rng.random(X.shape) < 0.02] = np.nan
    cases.append((Xn, "500x600, 2 % NaN"))
    nbytes = lib().smrf_raster_stats_workspace_bytes(np.dtype(dtype).itemsize, _lib.STATS_MOMENTS | _lib.STATS_MEDIAN)
    for X, ctx in cases:
        run_guarded(lambda Xt: F("raster_stats")(Xt), [X], name="raster_stats", ctx=ctx, after=exact_workspace(nbytes),
                    reference=lambda got: stats_match(got, X, ctx))
        run_guarded(lambda Xt: F("rmse")(Xt), [X], name="rmse", ctx=ctx,
                    reference=lambda got: (got.dtype == X.dtype and got == rn.rmse(X)) or pytest.fail("rmse %r" % (ctx,)))


def brassel_reference(Hs, Z, kw, ctx):
    """tests/test_gpu_relief.py's comparison of brassel_atmospheric_perspective on a result in hand"""
    from test_gpu_relief import BRASSEL_MARGIN

    def ref(got):
        with np.errstate(all='ignore'):
            v, was_int = rn.brassel_value(Hs, Z, **kw)
            want = rn.brassel_atmospheric_perspective(Hs, Z, **kw)
        assert got.dtype == want.dtype == (np.uint8 if was_int else np.float64) and got.shape == want.shape, kw
        if not was_int:
            return assert_close(got, want, 1.0, (kw, Z.dtype, Hs.dtype))
        with np.errstate(all='ignore'):
            ok = ~(np.abs(255 * v - (np.floor(255 * v) + 0.5)) < BRASSEL_MARGIN)
        assert np.array_equal(got[ok], want[ok]), (ctx, int((got[ok] != want[ok]).sum()))
    return ref


@pytest.mark.parametrize("dtype", [F32, F64])
def test_relief_images(gpu_device, dtype):
    """normalize with a median knot, the colour gather against the device's own shade, brassel with uint8 and float shades"""
    import neilpy_amd as na
    G = golden("relief.npz")
    for Z, ctx in cases_of(GRADIENT_SHAPES, (dtype,)):
        xr, yr = ['min', 'median', 'max'], [-1, 0, 1]
        run_guarded(lambda Zt: F("normalize")(Zt, xr, yr), [Z], name="normalize", ctx=ctx,
                    reference=lambda got: assert_exact(got, rn.normalize(Z, xr, yr), ctx))
        H = na.hillshade(Z, 2)                      # the device's own shade (guarded in test_surface), zi is NumPy's
        for fn, table, call in (("colortable_shade", "lut_ghc", lambda Zt, lt: F("colortable_shade")(Zt, lt, 2)),
                                ("colortable_shade", "lut_rand4", lambda Zt, lt: F("colortable_shade")(Zt, lt, 2)),
                                ("swiss_shading", "lut_swiss", lambda Zt, lt: F("swiss_shading")(Zt, 2, lut=lt))):
            if "nan" in ctx:
                want = rn.table3(G[table])[np.zeros(Z.shape, int), H]          # np.min / np.max of a raster with a NaN
            else:
                want = rn.table3(G[table])[rn.table_index(Z), H]
            run_guarded(call, [Z, G[table]], name=fn, ctx=(ctx, table),
                        reference=lambda got: (got.dtype == np.uint8 and np.array_equal(got, want)) or pytest.fail(
                            "%s %r: %d cells differ" % (fn, ctx, int((got != want).sum()))))
        rng = np.random.default_rng(8)
        h = rng.uniform(0, 1, size=Z.shape)
        for hkind, Hs in (("u8", np.round(255 * h).astype(np.uint8)), ("f32", h.astype(F32)), ("f64", h)):
            kw = dict(k=2.303, C2=0.41) if hkind != "f32" else dict(k=1.371, flat=200, reverse=True)
            ref = brassel_reference(Hs, Z, kw, (ctx, hkind))
            run_guarded(lambda Ht, Zt: F("brassel_atmospheric_perspective")(Ht, Zt, **kw), [Hs, Z],
                        name="brassel_atmospheric_perspective", ctx=(ctx, hkind), reference=ref)


# ------------------------------------------------------------------------------------------
# progressive filter and disk filters
# ------------------------------------------------------------------------------------------
PF_SHAPES = ((70, 300), (203, 331))
DISK = ("erosion", "dilation", "opening")


def pf_raster(shape, dtype, nan):
    from test_gpu_fuzz import large_raster
    Z = large_raster(400 + shape[0], shape, dtype)
    if nan:
        Z[np.random.default_rng(shape[1]).random(shape) < 0.02] = np.nan
    return Z


def pf_plan(elem, windows, shape, has_nan, impl):
    """[(route, took the incremental erosion)] per window from the library's own planner (csrc/pf_route.h)"""
    from neilpy_amd import _lib
    win = np.ascontiguousarray(np.asarray(windows, dtype=np.int32))
    route = np.full(win.size, -1, dtype=np.int32)
    taken = np.full(win.size, 9, dtype=np.uint8)
    _lib.check(lib().smrf_pf_plan(int(elem), win.ctypes.data_as(C.c_void_p), int(win.size), shape[0], shape[0] * shape[1],
                                  int(has_nan), int(impl), 0, route.ctypes.data_as(C.c_void_p),
                                  taken.ctypes.data_as(C.c_void_p)))
    return [(int(r), int(t)) for r, t in zip(route, taken)]


def pf_candidates():
    """window lists the routes are drawn from, smallest radii first: single windows 0 .. 65, consecutive pairs and triples
    (chains, the incremental erosion that needs the previous window's radius + 1)"""
    out = [[r] for r in range(0, 66)]
    out += [[r, r + 1] for r in range(1, 64)]
    out += [[r, r + 1, r + 2] for r in range(1, 63)]
    return out


def pf_routes(shape, dtype, nan):
    """{(route, incremental): (windows, impl)}: for every route the plan can return for this shape and dtype, the first
    candidate list (smallest radii) and impl (automatic, forced ring, forced direct) that takes it"""
    first = {}
    for win in pf_candidates():
        for impl in (0, 1, 2):
            for key in pf_plan(np.dtype(dtype).itemsize, win, shape, nan, impl):
                first.setdefault(key, (tuple(win), impl))
    return first


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", PF_SHAPES)
def test_progressive_filter_routes(gpu_device, shape, dtype, nan):
    """one window list per route smrf_pf_plan reports: ring passes, chains, the fused opening, the incremental erosion,
    the direct kernel and the copy.  Finite rasters against tests/morph_numpy.py, rasters with NaN against the oracle
    (SciPy's NaN rule), masks and when_dropped bit for bit as in tests/test_gpu_fuzz.py."""
    from neilpy_amd import _lib
    from oracle import smrf_oracle as orc
    Z = pf_raster(shape, dtype, nan)
    routes = pf_routes(shape, dtype, nan)
    nbytes = lib().smrf_progressive_filter_workspace_bytes(shape[0], shape[1], np.dtype(dtype).itemsize)
    covered = set()
    refs = {}
    for win, impl in sorted(set(routes.values())):
        w = np.asarray(win)
        covered |= set(pf_plan(np.dtype(dtype).itemsize, win, shape, nan, impl))
        if win not in refs:
            refs[win] = (orc if nan else mn).progressive_filter(Z, w, 1, .15, return_when_dropped=True)
        want_m, want_w = refs[win]
        run_guarded(lambda Zt: F("progressive_filter")(Zt, w, 1, .15, return_when_dropped=True, impl=impl), [Z],
                    name="progressive_filter", ctx=(shape, np.dtype(dtype).name, nan, win, impl), after=exact_workspace(nbytes),
                    reference=lambda got: (np.array_equal(got[0], want_m) and np.array_equal(got[1], want_w)) or pytest.fail(
                        "progressive_filter %r impl %d: mask %d, when %d cells differ" % (
                            win, impl, int((got[0] != want_m).sum()), int((got[1] != want_w).sum()))))
    print("routes", shape, np.dtype(dtype).name, nan, sorted(routes.items()))
    assert covered == set(routes) and {r for r, _ in covered} >= {_lib.ROUTE_TWO_PASS, _lib.ROUTE_DIRECT, _lib.ROUTE_COPY}


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_disk_filters(gpu_device, dtype, nan):
    """erosion, dilation and opening by the ring and the direct kernel, radius 2, 17 and (finite rasters, where the fast
    restatement serves) 64"""
    from oracle import smrf_oracle as orc
    for shape in PF_SHAPES:
        Z = pf_raster(shape, dtype, nan)
        for r in (2, 17) if nan else (2, 17, 64):
            if nan:
                e, d = orc.erosion(Z, orc.disk(r)), orc.dilation(Z, orc.disk(r))
                o = orc.dilation(e, orc.disk(r))
            else:
                e, d = mn.erosion(Z, r, "rows"), mn.dilation(Z, r, "rows")
                o = mn.dilation(e, r, "rows")
            for impl in (0, 1, 2):
                for fn, want in zip(DISK, (e, d, o)):
                    c = (shape, np.dtype(dtype).name, nan, r, impl, fn)
                    run_guarded(lambda Zt: F(fn)(Zt, radius=r, impl=impl), [Z], name=fn, ctx=c,
                                reference=lambda got: assert_exact(got, want, c))


# ------------------------------------------------------------------------------------------
# cloud to raster
# ------------------------------------------------------------------------------------------
def dem_match(got, want, ctx):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0], equal_nan=True), ctx
    assert tuple(got[1]) == tuple(want[1])[:6], ctx


@pytest.mark.parametrize("bin_type", ["min", "max"])
def test_create_dem_samp21(gpu_device, bin_type):
    from oracle import smrf_oracle as orc
    x, y, z, _ = load_sample("samp21")
    # edges inside the cloud, so the filter drops points; off the centi-unit lattice of the sample's coordinates, so none
    # lies on the last edge (such a point passes the filter and is then outside the raster: both sides raise)
    xe = np.arange(np.floor(x.min()) + 10.503, np.ceil(x.max()) - 9.5, 1.0)
    ye = np.arange(np.ceil(y.max()) - 7.503, np.floor(y.min()) + 8.5, -1.0)
    assert ((x < xe[0]) | (x > xe[-1])).any() and ((y > ye[0]) | (y < ye[-1])).any()
    for edges in (None, (xe, ye)):
        want = orc.create_dem(x, y, z, 1, bin_type, edges=edges)
        run_guarded(lambda a, b, c: F("create_dem")(a, b, c, 1, bin_type, edges=edges), [x, y, z], name="create_dem",
                    ctx=(bin_type, edges is not None), reference=lambda got: dem_match(got, want, (bin_type, edges is not None)))


def test_create_dem_second_trip(gpu_device):
    """8192 * 256 + 257 points, the bin loop's second trip, into 300 x 257 cells"""
    from oracle import smrf_oracle as orc
    n = 8192 * 256 + 257
    rng = np.random.default_rng(22)
    x, y = rng.uniform(0.1, 255.9, n), rng.uniform(0.1, 298.9, n)
    x[:2], y[:2] = (0.1, 255.9), (0.1, 298.9)
    z = np.round(rng.normal(-3.0, 40.0, n), 2)
    want = orc.create_dem(x, y, z, 1, 'min')
    assert want[0].shape == (300, 257)
    run_guarded(lambda a, b, c: F("create_dem")(a, b, c, 1, 'min'), [x, y, z], name="create_dem", ctx="second trip",
                reference=lambda got: dem_match(got, want, "second trip"))


def read_las_case():
    """run_guarded's arguments for read_las_xyz on the smallest golden file (shared with tests/test_gpu_streams.py)"""
    from test_las import CASES, LAS
    tag = min(CASES, key=lambda c: LAS[c + "_col_x"].size)

    def ref(got):
        for k, c in enumerate("xyz"):
            assert np.array_equal(got[k], LAS[tag + "_col_" + c]), (tag, c)          # bit-exact with the reference's floats
    return dict(fn=lambda: F("read_las_xyz")(os.path.join(GOLDEN, "las", tag + ".las"))[1:], inputs=[], name="read_las_xyz",
                ctx=tag, reference=ref)


def test_read_las_xyz(gpu_device):
    run_guarded(**read_las_case())


# ------------------------------------------------------------------------------------------
# inpainting
# ------------------------------------------------------------------------------------------
def holes(shape, dtype, share, seed):
    rng = np.random.default_rng(seed)
    X = (rng.normal(size=shape) * 5 + 100).astype(dtype)
    X[rng.random(shape) < share] = np.nan
    return X


@pytest.mark.parametrize("dtype", [F32, F64])
def test_inpaint_nearest(gpu_device, dtype):
    """fills in place: the finite cells keep their bits.  nearest_source's planes as tests/test_gpu_nearest.py reads them"""
    single = np.full((40, 70), np.nan, dtype)
    single[23, 5] = 7.5
    for X, ctx in ((holes((1, 70), dtype, .5, 1), "(1, 70)"), (holes((67, 131), dtype, .6, 2), "(67, 131)"),
                   (single, "one source")):
        nbytes = lib().smrf_nearest_workspace_bytes(X.shape[0], X.shape[1], X.dtype.itemsize)
        run_guarded(lambda Xt: F("inpaint_nearest")(Xt), [X], name="inpaint_nearest", ctx=ctx, after=exact_workspace(nbytes),
                    known=lambda i, a: np.isfinite(a),
                    reference=lambda got: nn.same_bits(got, nn.inpaint_nearest(X)) or pytest.fail("inpaint_nearest " + ctx))

        def ref(got):
            dist, rc = got
            index, dist2, _ = nn.feature_transform(np.ascontiguousarray(X))
            assert dist.dtype == np.float64 and rc.dtype == np.int64 and rc.shape == (2,) + X.shape, ctx
            assert np.array_equal(rc[0] * X.shape[1] + rc[1], index), ctx
            assert np.array_equal(dist, np.sqrt(dist2.astype(np.float64))), ctx
        run_guarded(lambda Xt: F("nearest_source")(Xt), [X], name="nearest_source", ctx=ctx, reference=ref)


@pytest.mark.parametrize("shape,seed,share", [((37, 53), 1, .5), ((300, 2049), 101, .1)])
def test_inpaint_springs(gpu_device, shape, seed, share):
    """through the public function, in place: tests/test_gpu_springs.py's rasters, stop and bar (1000 x how far the oracle's
    own answer moves when every sum is taken in another order, never above 1e-7); the known cells keep their bits"""
    run_guarded(**springs_case(shape, seed, share))


def springs_case(shape, seed, share):
    """run_guarded's arguments for test_inpaint_springs (shared with tests/test_gpu_streams.py)"""
    import neilpy_amd as na
    from oracle import smrf_oracle as orc
    from test_gpu_springs import oracle_run, raster as springs_raster
    key = (shape, seed, share)
    A = np.array(springs_raster(*key))
    want, istop, itn = oracle_run(orc, A, key)
    flip, istop_f, itn_f = oracle_run(orc, A, key, flipped=True)
    assert (istop_f, itn_f) == (istop, itn)
    hole = np.isnan(A)
    bar = min(1e-7, 1000.0 * float(np.abs(flip - want)[hole].max()))

    def fill(At):
        assert F("inpaint_nans_by_springs")(At, inplace=True) is None
        st = na.last_stats["inpaint"]
        assert (st["istop"], st["itn"], st["n_unknown"]) == (istop, itn, int(hole.sum())), st
        return At

    def ref(got):
        diff = float(np.abs(got - want)[hole].max())
        print("springs %s: device vs oracle %.3g, bar %.3g" % (shape, diff, bar))
        assert not np.isnan(got).any() and diff <= bar, (diff, bar)
    return dict(fn=fill, inputs=[A], name="inpaint_nans_by_springs", ctx=shape, known=lambda i, a: ~np.isnan(a), reference=ref,
                after=exact_workspace(lib().smrf_springs_workspace_bytes(*shape)))


def test_inpaint_fda(gpu_device):
    run_guarded(**fda_case())


def fda_case():
    """run_guarded's arguments for test_inpaint_fda (shared with tests/test_gpu_streams.py)"""
    import neilpy_amd as na
    from test_fda import CASES, G, RTOL, _close_stop
    tag = min((c for c in CASES if np.isnan(G[c + "_in"]).any() and not np.isnan(G[c + "_in"]).all()),
              key=lambda c: G[c + "_in"].size)
    A, want = G[tag + "_in"], G[tag + "_out"]

    def fill(At):
        assert F("inpaint_nans_by_fda")(At, inplace=True) is None
        st = na.last_stats["inpaint_fda"]
        assert _close_stop((st["istop"], st["itn"]), G[tag + "_lsqr"]), st
        return At

    def ref(got):
        scale = max(1.0, float(np.nanmax(np.abs(want))))
        assert got.dtype == np.float64 and np.max(np.abs(got - want)) <= RTOL * scale, tag
    return dict(fn=fill, inputs=[A], name="inpaint_nans_by_fda", ctx=tag, known=lambda i, a: ~np.isnan(a), reference=ref,
                after=exact_workspace(lib().smrf_fda_workspace_bytes(*A.shape)))


# ------------------------------------------------------------------------------------------
# points and voxels
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3])
def test_points(gpu_device, d):
    """clouds of 1, 257 and 1024 * 256 + 257 points (the bounds loop's second trip); the largest is searched by 257
    queries, which keeps the brute-force restatement small"""
    rng = np.random.default_rng(140 + d)
    q = rng.uniform(-1, 11, (257, d))
    for n in (1, 257, 1024 * 256 + 257):
        p = rng.uniform(0, 10, (n, d))
        wd, wi = pn.nearest_points(q, p)
        nbytes = lib().smrf_points_nn_workspace_bytes(n, d)

        def ref(got):
            assert got[0].dtype == np.float64 and got[1].dtype == np.int64
            bad = np.flatnonzero((got[1] != wi) | (got[0].view(np.uint64) != wd.view(np.uint64)))
            assert bad.size == 0, (n, d, bad.size, bad[:5])
        run_guarded(lambda qt, pt: F("nearest_points")(qt, pt), [q, p], name="nearest_points", ctx=(n, d), reference=ref,
                    after=exact_workspace(nbytes))
        want = pn.chamfer_distance(q, p)
        run_guarded(lambda qt, pt: F("chamfer_distance")(qt, pt), [q, p], name="chamfer_distance", ctx=(n, d),
                    reference=lambda got: chamfer_close(got, want, n + len(q)))


def chamfer_close(got, want, n):
    from test_gpu_points import _bound
    assert got.dtype == np.float64 and _bound(np.float64(got), want, n), (got, want, n)


@pytest.mark.parametrize("T", [F32, F64])
def test_voxelize(gpu_device, T):
    from test_gpu_voxel import COUNTS, RESOLUTIONS, cloud
    n, resolution = COUNTS[0], RESOLUTIONS[0]
    for (x, y, z), res, kw in ((cloud(n, 10 * n + resolution, T), resolution, dict(bottom_fill=True)),
                               (cloud(4000, 77, T), 32, dict(ve=33 / 8.0, bottom_fill=False, pad=3, threshold=2))):
        want = vn.voxelize(None, x, y, z, res, **kw)
        run_guarded(lambda a, b, c: F("voxelize")(None, a, b, c, res, **kw), [x, y, z], name="voxelize", ctx=(n, res, kw),
                    reference=lambda got: (got.dtype == bool and got.shape == want.shape and np.array_equal(got, want)) or
                    pytest.fail("voxelize %r" % (kw,)))


# ------------------------------------------------------------------------------------------
# smrf's tail
# ------------------------------------------------------------------------------------------
PSSM_SHAPES = ((2, 2), (2, 65), (65, 2), (67, 131))


def test_pssm(gpu_device):
    """classes and RGBA on rasters narrower than the goldens of tests/test_pssm.py, equal to the oracle in every cell"""
    from oracle import smrf_oracle as orc
    from test_pssm import G
    for shape in PSSM_SHAPES:
        Z = raster(shape, F64)
        run_guarded(lambda Zt: F("pssm")(Zt, 1.5, 2.3, False, False), [Z], name="pssm", ctx=(shape, "classes"),
                    reference=lambda got: (got.dtype == np.uint8 and np.array_equal(got, orc.pssm_classes(Z, 1.5, 2.3))) or
                    pytest.fail("pssm classes %r" % (shape,)))
        for reverse, lut in ((False, "lut_bone_r"), (True, "lut_bone")):
            run_guarded(lambda Zt: F("pssm")(Zt, 1.5, 2.3, reverse), [Z], name="pssm", ctx=(shape, "rgba", reverse),
                        reference=lambda got: (got.shape == shape + (4,) and np.array_equal(got, orc.pssm(Z, G[lut], 1.5, 2.3)))
                        or pytest.fail("pssm rgba %r" % (shape,)))


def test_pssm_nan_is_class_zero(gpu_device):
    """a cell whose gradient reads a NaN has a NaN slope, and the class of NaN is 0 (NumPy's cast of NaN to uint8 on the
    reference's platform); every other cell is the oracle's"""
    from oracle import smrf_oracle as orc
    Z = raster((67, 131), F64, nan=True, seed=3)
    gy, gx = np.gradient(Z, 1.5)
    bad = np.isnan(gx) | np.isnan(gy)
    assert bad.any() and not bad.all()
    with np.errstate(all='ignore'):
        want = orc.pssm_classes(Z, 1.5, 2.3)

    def ref(got):
        assert got.dtype == np.uint8 and (got[bad] == 0).all(), int((got[bad] != 0).sum())
        assert np.array_equal(got[~bad], want[~bad])
    run_guarded(lambda Zt: F("pssm")(Zt, 1.5, 2.3, False, False), [Z], name="pssm", ctx="nan", reference=ref)


@pytest.mark.parametrize("shape", [(4, 4), (9, 300), (300, 257)])
def test_spline(gpu_device, shape):
    """smrf_spline_solve_ws_f64 and smrf_spline_eval_f64 as smrf() calls them, the scratch plane poisoned, against SciPy
    with the bars of tests/test_gpu_parity.py's test_spline_matches_scipy.  (300, 257): two chunks on both axes and a last
    64-column tile one column wide."""
    run_guarded(**spline_case(shape))


def spline_case(shape):
    """run_guarded's arguments for test_spline (shared with tests/test_gpu_streams.py)"""
    import torch
    from scipy import interpolate
    from neilpy_amd import _lib, spline
    rows, cols = shape
    rng = np.random.default_rng(12)
    Z = rng.normal(100, 5, shape)
    f = interpolate.RectBivariateSpline(np.arange(.5, rows + .5), np.arange(.5, cols + .5), Z)
    pr, pc = rng.uniform(-1.0, rows + 1.0, 5000), rng.uniform(-1.0, cols + 1.0, 5000)
    pr[:4], pc[:4] = [0.5, rows - 0.5, 0.0, rows], [0.5, cols - 0.5, cols, 0.0]
    pr[4:4 + min(rows, 50)] = np.arange(.5, rows + .5)[:50]
    want = f.ev(pr, pc)
    (tx, lur), (ty, luc) = spline.axis_factors(rows), spline.axis_factors(cols)

    def call(coef, txd, tyd, lurd, lucd, prd, pcd):
        L = lib()                                       # at call time: tests/streamed.py records through what load() returns
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
        scratch = torch.empty_like(coef)
        _lib.check(L.smrf_spline_solve_ws_f64(p(coef), p(scratch), rows, cols, p(lurd), p(lucd), st))
        out = torch.empty(pr.size, dtype=torch.float64, device=coef.device)
        _lib.check(L.smrf_spline_eval_f64(p(coef), rows, cols, p(txd), p(tyd), p(prd), p(pcd), pr.size, p(out), st))
        return coef, out

    def ref(got):
        print("spline %s: coefficients %.3g (bar 1e-10), values %.3g (bar 1e-9)" % (
            shape, np.abs(got[0].ravel() - f.tck[2]).max(), np.abs(got[1] - want).max()))
        np.testing.assert_allclose(got[0].ravel(), f.tck[2], rtol=0, atol=1e-10)
        np.testing.assert_allclose(got[1], want, rtol=0, atol=1e-9)
    # the solve works in place on the coefficient plane: input 0 is exempt from "unchanged", the others are not
    return dict(fn=call, inputs=[Z, tx, ty, lur, luc, pr, pc], name="smrf_spline", ctx=shape, reference=ref,
                known=lambda i, a: np.zeros(a.shape, bool) if i == 0 else None)


# ------------------------------------------------------------------------------------------
# the whole pipeline
# ------------------------------------------------------------------------------------------
def test_smrf_samp21(gpu_device):
    """smrf() with tensor inputs: every intermediate plane of the pipeline behind guards at once; against the golden of
    tests/test_gpu_parity.py's test_smrf_samples_golden, through that file's check_smrf"""
    case, tails = smrf_case()
    run_guarded(**case)
    assert same_bits(tails[0]["elevation_values"], tails[1]["elevation_values"])
    assert same_bits(tails[0]["slope_values"], tails[1]["slope_values"])


def smrf_case():
    """run_guarded's arguments for test_smrf_samp21 and the list that gets each run's tail statistics (shared with
    tests/test_gpu_streams.py)"""
    import neilpy_amd as na
    from test_gpu_parity import META, check_smrf
    x, y, z, g = load_sample("samp21")
    gold = golden("smrf_samp21.npz")
    kw = META["smrf_kwargs"]
    tails = []

    def call(xt, yt, zt):
        out = F("smrf")(xt, yt, zt, return_extras=True, **kw)
        tail = na.last_stats["tail"]
        tails.append({k: tail[k] for k in ("elevation_values", "slope_values")})
        return out

    def ref(got):
        class Shim:
            last_stats = dict(na.last_stats, tail=tails[0])

            @staticmethod
            def smrf(*a, **k):
                return got
        pts = check_smrf(Shim, gold, x, y, z, kw, "samp21" in META["full_dtm"], META["stride"])
        assert abs(100.0 * (1.0 - np.mean(pts == g)) - META["anchors"]["samp21"]["total_error_pct"]) < 1e-9
    return dict(fn=call, inputs=[x, y, z], name="smrf", ctx="samp21", reference=ref), tails


# ------------------------------------------------------------------------------------------
# the sharded path
# ------------------------------------------------------------------------------------------
def test_sharded_bands_on_one_gpu(gpu_device):
    """tests/test_gpu_edges.py's test_sharded_driver_bands_on_one_gpu at its smallest parametrisation (2 ranks, 200 x 131,
    windows 2, 6, 1), every rank in turn in this process: band planes and halo buffers come from sharded.py"""
    run_guarded(**sharded_case())


def sharded_case():
    """run_guarded's arguments for test_sharded_bands_on_one_gpu (shared with tests/test_gpu_streams.py)"""
    import neilpy_amd as na
    from neilpy_amd import sharded
    from oracle import smrf_oracle as orc
    from sharded_one_gpu import run_bands
    world, shape, win = 2, (200, 131), np.asarray([2, 6, 1])
    Z = na.synth_dem(shape[1], seed=9, rows=shape[0]).astype(F32)
    want_m, want_w = orc.progressive_filter(Z, win, 1, .15, return_when_dropped=True)

    def call(Zt):
        mask, when, _ = run_bands(na, Zt, win, world, return_when_dropped=True, budget=None, ops=sharded.HipBandOps,
                                  overlap=lambda k: k % 2 == 0)
        return mask, when
    return dict(fn=call, inputs=[Z], name="sharded", ctx=shape,
                reference=lambda got: (np.array_equal(got[0], want_m) and np.array_equal(got[1], want_w)) or pytest.fail("sharded"))


# ------------------------------------------------------------------------------------------
# entry points with a caller-supplied workspace, straight through ctypes (smrf_focal_*: test_focal_tpi_workspace_exact)
# ------------------------------------------------------------------------------------------
def _g():
    import guarded
    return guarded._active[0]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_workspace_raster_stats(gpu_device, dtype):
    from neilpy_amd import _lib
    from neilpy_amd.relief import _ROW, STATS
    L = lib()
    what = _lib.STATS_MOMENTS | _lib.STATS_MEDIAN
    nbytes = int(L.smrf_raster_stats_workspace_bytes(np.dtype(dtype).itemsize, what))
    rng = np.random.default_rng(3)
    for X in ((rng.normal(size=(1, 257)) * 100).astype(dtype), (rng.normal(size=(500, 600)) * 30 + 400).astype(dtype)):
        def call(Xt):
            row = (C.c_double * _lib.STATS_ROW)()
            ws = _g().bytes_of(nbytes)
            _lib.check(getattr(L, "smrf_raster_stats_" + ("f32" if dtype == F32 else "f64"))(_p(Xt), Xt.numel(), what, row, _p(ws),
                                                                                             nbytes, _st()))
            out = {n: (int(row[_ROW[n]]) if n == 'count' else dtype(row[_ROW[n]]) if n in ('min', 'max', 'median')
                       else np.float64(row[_ROW[n]])) for n in STATS}
            out['has_nan'] = row[_lib.STATS_NAN] > 0
            return out
        run_guarded(call, [X], name="smrf_raster_stats", ctx=X.shape, reference=lambda got: stats_match(got, X, X.shape))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_workspace_nearest(gpu_device, dtype):
    import torch
    from neilpy_amd import _lib
    L = lib()
    X = holes((67, 131), dtype, .6, 2)
    rows, cols = X.shape
    nbytes = int(L.smrf_nearest_workspace_bytes(rows, cols, X.dtype.itemsize))

    def call(Xt):
        index = torch.empty((rows, cols), dtype=torch.int64, device=Xt.device)
        dist2 = torch.empty((rows, cols), dtype=torch.int32, device=Xt.device)
        ws = _g().bytes_of(nbytes)
        _lib.check(getattr(L, "smrf_nearest_" + ("f32" if dtype == F32 else "f64"))(_p(Xt), _p(Xt), _p(index), _p(dist2), rows,
                                                                                    cols, _p(ws), nbytes, _st()))
        return Xt, index, dist2

    def ref(got):
        index, dist2, _ = nn.feature_transform(X)
        assert nn.same_bits(got[0], nn.inpaint_nearest(X))
        assert np.array_equal(got[1], index) and np.array_equal(got[2].view(np.uint32), dist2)
    run_guarded(call, [X], name="smrf_nearest", ctx=X.shape, known=lambda i, a: np.isfinite(a), reference=ref)


@pytest.mark.parametrize("d", [2, 3])
def test_workspace_points_nn(gpu_device, d):
    import torch
    from neilpy_amd import _lib
    L = lib()
    rng = np.random.default_rng(150 + d)
    q, pts = rng.uniform(-1, 11, (257, d)), rng.uniform(0, 10, (1024 * 256 + 257, d))
    wd, wi = pn.nearest_points(q, pts)
    n = len(pts)
    small_bytes, nbytes = int(L.smrf_points_nn_workspace_bytes(1, d)), int(L.smrf_points_nn_workspace_bytes(n, d))

    def call(qt, pt):
        g = _g()
        small, ws = g.bytes_of(small_bytes), g.bytes_of(nbytes)
        box, bad = (C.c_double * 4)(), C.c_int64(0)
        _lib.check(L.smrf_points_nn_bounds_f64(_p(pt), n, d, box, C.byref(bad), _p(small), small_bytes, _st()))
        assert bad.value == 0
        _lib.check(L.smrf_points_nn_build_f64(_p(pt), n, d, box, _p(ws), nbytes, _st()))
        dist = torch.empty(len(q), dtype=torch.float64, device=qt.device)
        index = torch.empty(len(q), dtype=torch.int64, device=qt.device)
        _lib.check(L.smrf_points_nn_search_f64(_p(qt), len(q), _p(pt), n, d, box, _p(dist), _p(index), _p(ws), nbytes, _st()))
        total = torch.empty(1, dtype=torch.float64, device=qt.device)
        _lib.check(L.smrf_points_nn_sum_f64(_p(dist), len(q), _p(total), _p(small), small_bytes, _st()))
        return dist, index, total, np.array(list(box))

    def ref(got):
        assert np.array_equal(got[1], wi) and np.array_equal(got[0].view(np.uint64), wd.view(np.uint64))
        chamfer_close(np.float64(got[2][0]) / np.float64(len(q)), pn.chamfer_distance(q, pts, direction='x_to_y'), len(q))
    run_guarded(call, [q, pts], name="smrf_points_nn", ctx=d, reference=ref)


@pytest.mark.parametrize("T", [F32, F64])
def test_workspace_voxel(gpu_device, T):
    import torch
    from neilpy_amd import _lib, voxel
    from test_gpu_voxel import cloud
    L = lib()
    sfx = "f32" if T == F32 else "f64"
    x, y, z = cloud(4000, 77, T)
    for threshold, pad in ((1, 0), (2, 3)):                  # the bit set, and the integer counts with solid layers below
        want = vn.voxelize(None, x, y, z, 32, bottom_fill=True, threshold=threshold, ve=33 / 8.0, pad=pad)

        def call(xt, yt, zt):
            g = _g()
            n = xt.numel()
            small = g.bytes_of(voxel.BOUNDS_BYTES)
            box, bad = (C.c_double * 6)(), C.c_int64(0)
            _lib.check(getattr(L, "smrf_voxel_bounds_" + sfx)(_p(xt), _p(yt), _p(zt), n, box, C.byref(bad), _p(small),
                                                              voxel.BOUNDS_BYTES, _st()))
            assert bad.value == 0
            edges, mins = voxel.bin_edges(list(box), T, 32, 33 / 8.0)
            nx, ny, nz = (len(e) - 1 for e in edges)
            nbytes = int(L.smrf_voxel_workspace_bytes(nx, ny, nz, threshold))
            ws = g.bytes_of(nbytes)
            H = torch.empty((nx, ny, nz + pad), dtype=torch.bool, device=xt.device)
            de = [g.tensor(e) for e in edges]
            offsets = (C.c_double * 3)(*[float(m) for m in mins])
            _lib.check(getattr(L, "smrf_voxel_mark_" + sfx)(_p(xt), _p(yt), _p(zt), n, offsets, _p(de[0]), _p(de[1]), _p(de[2]),
                                                            nx, ny, nz, threshold, _p(ws), nbytes, _st()))
            _lib.check(L.smrf_voxel_expand(_p(ws), nbytes, nx, ny, nz, threshold, 1, pad, _p(H), _st()))
            return H
        run_guarded(call, [x, y, z], name="smrf_voxel", ctx=(sfx, threshold, pad),
                    reference=lambda got: (got.shape == want.shape and np.array_equal(got, want)) or pytest.fail("voxel"))


@pytest.mark.parametrize("export", ["springs", "fda"])
def test_workspace_lsqr(gpu_device, export):
    """smrf_springs_lsqr_f64 and smrf_fda_lsqr_f64 as tests/test_gpu_springs.py's device_solve calls them, to the natural
    stop: the rasters, stops and bars of test_inpaint_springs (the (37, 53) raster) and test_inpaint_fda"""
    from neilpy_amd import _lib
    from oracle import smrf_oracle as orc
    from test_fda import CASES, G, RTOL, _close_stop
    from test_gpu_springs import raster as springs_raster
    L = lib()
    if export == "springs":
        A = np.array(springs_raster((37, 53), 1, .5))
        want, istop, itn = orc.lsqr_springs(A)
        flip = orc.lsqr_springs(np.ascontiguousarray(A[::-1, ::-1]))[0][::-1, ::-1]
        bar = min(1e-7, 1000.0 * float(np.abs(flip - want)[np.isnan(A)].max()))
    else:
        tag = min((c for c in CASES if np.isnan(G[c + "_in"]).any() and not np.isnan(G[c + "_in"]).all()),
                  key=lambda c: G[c + "_in"].size)
        A, want, (istop, itn) = G[tag + "_in"], G[tag + "_out"], (int(v) for v in G[tag + "_lsqr"])
        bar = RTOL * max(1.0, float(np.nanmax(np.abs(want))))
    hole = np.isnan(A)
    m, n = A.shape
    nbytes = int(getattr(L, "smrf_%s_workspace_bytes" % export)(m, n))
    stops = []

    def call(At):
        ws = _g().bytes_of(nbytes)
        s, k, u = C.c_int(-1), C.c_int64(-1), C.c_int64(-1)
        _lib.check(getattr(L, "smrf_%s_lsqr_f64" % export)(_p(At), m, n, 1e-6, 1e-6, 1e8, -1, C.byref(s), C.byref(k), C.byref(u),
                                                          _p(ws), nbytes, _st()))
        stops.append((s.value, k.value, u.value))
        return At

    def ref(got):
        diff = float(np.abs(got - want)[hole].max())
        print("%s workspace: stop %s, oracle (%d, %d), device vs oracle %.3g, bar %.3g" % (export, stops[0], istop, itn, diff, bar))
        assert not np.isnan(got).any() and diff <= bar
    run_guarded(call, [A], name="smrf_" + export, ctx=A.shape, known=lambda i, a: ~np.isnan(a), reference=ref)
    assert stops[0] == stops[1] and stops[0][2] == int(hole.sum())
    assert stops[0][:2] == (istop, itn) if export == "springs" else _close_stop(stops[0][:2], (istop, itn))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_workspace_progressive_filter(gpu_device, dtype):
    """smrf_progressive_filter_* with windows that take the chains, the fused opening, ring passes and the incremental erosion"""
    import torch
    from neilpy_amd import _lib
    L = lib()
    shape = (203, 331)
    Z = pf_raster(shape, dtype, False)
    win = np.ascontiguousarray(np.array([1, 2, 3, 4, 7, 10, 20, 21], dtype=np.int32))
    thr = np.ascontiguousarray(.15 * (win * 1.0))
    want_m, want_w = mn.progressive_filter(Z, win, 1, .15, return_when_dropped=True)
    nbytes = int(L.smrf_progressive_filter_workspace_bytes(shape[0], shape[1], np.dtype(dtype).itemsize))

    def call(Zt):
        mask = torch.empty(shape, dtype=torch.uint8, device=Zt.device)
        when = torch.empty(shape, dtype=torch.uint8, device=Zt.device)
        ws = _g().bytes_of(nbytes)
        _lib.check(getattr(L, "smrf_progressive_filter_" + ("f32" if dtype == F32 else "f64"))(
            _p(Zt), shape[0], shape[1], win.ctypes.data_as(C.c_void_p), thr.ctypes.data_as(C.c_void_p), int(win.size), _p(mask),
            _p(when), _p(ws), nbytes, -1, 0, _st()))
        return mask, when
    run_guarded(call, [Z], name="smrf_progressive_filter", ctx=np.dtype(dtype).name,
                reference=lambda got: (np.array_equal(got[0].astype(bool), want_m) and np.array_equal(got[1], want_w)) or
                pytest.fail("progressive_filter through ctypes"))
