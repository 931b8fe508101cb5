"""The case table of the kernel families (a plain helper module, no test in it): what tests/test_gpu_guarded.py,
tests/test_gpu_streams.py, tests/test_gpu_views.py and tests/test_gpu_threads.py share.

The package's exports are classified here (tests/test_guarded_host.py compares the lists with neilpy_amd's namespace), and
every name of GUARDED has a *builder*: a generator ``builder(names, **selection)`` of case dicts

    name, fn, inputs, ctx, reference            and optionally      known, after, stream

which are ``run_guarded``'s keywords.  A builder yields, for the names asked for, the family's whole guarded sweep - every
shape, dtype, keyword set, impl and window list the guarded module runs - in the order that module runs it, and the
selection keywords are that module's test parameters.  The cases marked ``stream=True`` are the ones the stream module
runs, one shape each.  Several names share a builder where they share rasters and references.

A reference that several cases share, or that only some selection needs, is wrapped in ``once``: it is computed when the
first case that needs it compares its result, so walking a whole sweep to pick a few cases costs the inputs only.  Loop
variables reach the closures as default arguments (or a factory's arguments), never through the loop's scope: a case stays
what it was after the generator has moved on.

Each family's comparison and margins live in that family's own GPU test and are imported inside the builder.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import focal_numpy as fnp
import footprint_numpy as fpn
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

# ------------------------------------------------------------------------------------------
# the package's exports, classified
# ------------------------------------------------------------------------------------------
# has a builder below and is called under the harnesses
GUARDED = ("slope", "aspect", "hillshade", "multiple_illumination", "esri_slope", "curvature", "esri_curvature",
           "zevenbergen_and_thorne_curvature", "evans_curvature", "wilson_gallant_curvature",
           "focal_convolve", "std", "topographic_position_index", "reduce_peaks",
           "openness", "skyview_factor", "count_openness", "geomorphons", "ternary_pattern_from_openness",
           "scaled_morphometry", "vip_score", "ashift",
           "raster_stats", "normalize", "rmse", "colortable_shade", "swiss_shading", "brassel_atmospheric_perspective",
           "progressive_filter", "erosion", "dilation", "opening",
           "create_dem", "inpaint_nearest", "nearest_source", "inpaint_nans_by_springs", "inpaint_nans_by_fda",
           "nearest_points", "chamfer_distance", "voxelize", "pssm", "smrf", "read_las_xyz",
           "hungarian_algorithm", "bdr", "bdr_bootstrap",
           "grey_erosion", "grey_dilation", "grey_opening", "grey_closing", "white_tophat", "black_tophat",
           "morphological_gradient")
# launches a kernel and has no builder: name -> reason
LEFT_OUT = {}
# exported and launches nothing: host helpers, constants, views and table look-ups by torch indexing
NO_KERNEL = ("SmrfHipError", "load_library", "LIB_PATH", "Affine", "edges_from_IT", "from_origin", "write_worldfile", "disk",
             "last_stats", "distance_kernel", "read_las", "write_las", "triangle_height", "cutter", "z_factor", "synth_dem",
             "synth_points", "geomorphon_cmap", "get_lowest_equivalent", "int2base", "progressive_window",
             "terrain_code_to_geomorphon", "rectangle", "square", "diamond")

# Returned tensors that do not live in an arena: (function, path of the leaf in the result) -> the torch op that made it.
# Every entry names a torch op, not a kernel; an entry whose tensor IS owned fails too, so the table cannot go stale.
NOT_OWNED = {
    ("rmse", ""): "torch.tensor(float(v)): the 0-dim result is built from the host's statistics row",
    ("smrf", "[4]['above_ground_height']"): "zd - elev_d, a torch subtraction of two vectors the kernels wrote",
    ("smrf", "[4]['when_dropped']"): "drop[ri, ci], a torch gather from the kernels' drop raster",
    ("sharded", "[0]"): "mask.bool() in tests/sharded_one_gpu.py, after copy_ stitched the bands' masks together",
}

SURFACE = tuple(sorted(sn.FUNCS))
TERRAIN = ("openness", "skyview_factor", "count_openness", "geomorphons", "ternary_pattern_from_openness")
DISK = ("erosion", "dilation", "opening")
MORPHOLOGY = tuple(fpn.FUNCTIONS)

DEVICE = "cuda:0"
AUTO, TILED, DIRECT = IMPLS = 0, 1, 2         # every wrapper's default is AUTO: a call without impl= is the AUTO case
RUNS = 1                                      # grey morphology's name for impl 1 (2 is its taps path)
F32, F64 = np.float32, np.float64


def F(name):
    """a guarded export by name: as a literal name, or as F(fn) with fn drawn from SURFACE, TERRAIN, DISK or MORPHOLOGY -
    tests/test_guarded_host.py reads GUARDED against exactly these in this file's source"""
    import neilpy_amd
    assert name in GUARDED, name
    return getattr(neilpy_amd, name)


# ------------------------------------------------------------------------------------------
# result trees
# ------------------------------------------------------------------------------------------
def is_affine(v):
    return type(v).__name__ == "Affine"


def leaves(v, path=""):
    if is_affine(v):
        yield path, v
    elif isinstance(v, (tuple, list)):
        for i, e in enumerate(v):
            yield from leaves(e, "%s[%d]" % (path, i))
    elif isinstance(v, dict):
        for k, e in v.items():
            yield from leaves(e, "%s[%r]" % (path, k))
    else:
        yield path, v


def to_numpy(v):
    import torch
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    if is_affine(v):
        return np.array(tuple(v)[:6], dtype=np.float64)
    return v if v is None else np.asarray(v)


def rebuild(v, f):
    if is_affine(v):
        return f(v)
    if isinstance(v, (tuple, list)):
        return type(v)(rebuild(e, f) for e in v)
    if isinstance(v, dict):
        return {k: rebuild(e, f) for k, e in v.items()}
    return f(v)


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
TILE_SHAPES = ((1, 1), (1, 65), (65, 1), (9, 65), (67, 131))      # 64 x 8 tiles: one cell past a tile in both axes, several tiles
GRADIENT_SHAPES = ((2, 65), (65, 2), (9, 65), (67, 131))
NAN_SHAPE = (67, 131)
PF_SHAPES = ((70, 300), (203, 331))
PSSM_SHAPES = ((2, 2), (2, 65), (65, 2), (67, 131))
SPRINGS = (((37, 53), 1, .5), ((300, 2049), 101, .1))             # tests/test_gpu_springs.py's rasters
SPLINE_SHAPES = ((4, 4), (9, 300), (300, 257))


def lib():
    from neilpy_amd import _lib
    return _lib.load()


def exact_workspace(nbytes):
    """an ``after=`` that asserts the harness served a uint8 allocation of exactly ``nbytes`` bytes"""
    import torch

    def look(g):
        sizes = [a.nbytes for a in g.arenas if a.dtype == torch.uint8 and len(a.shape) == 1]
        assert int(nbytes) in sizes, (int(nbytes), sizes)
    return look


def raster(shape, dtype, nan=False, seed=0):
    from test_gpu_focal import _raster
    return _raster(np.random.default_rng(20261101 + seed + 1000 * shape[0] + shape[1]), shape, dtype, nan=nan)


def cases_of(shapes, dtypes=(F32, F64)):
    """every shape and dtype without NaN, and the largest shape once more with 2 % NaN cells: the stream module's raster"""
    for dtype in dtypes:
        for shape in shapes:
            yield raster(shape, dtype), (shape, np.dtype(dtype).name)
        yield raster(NAN_SHAPE, dtype, nan=True, seed=7), (NAN_SHAPE, np.dtype(dtype).name, "nan")


def golden_kw(npz, fn):
    """the keywords of the golden case of ``fn`` that sets the most of them (the first such case)"""
    cs = [c for c in json.loads(str(golden(npz)["cases"])) if c["fn"] == fn]
    return dict(max(cs, key=lambda c: len(c["kw"]))["kw"])


def focal_kernels():
    rng = np.random.default_rng(20261102)
    w7 = rng.normal(size=(7, 7))
    w7[rng.random((7, 7)) < 0.3] = 0.0                       # zero taps are skipped by the tap table
    assert (w7 == 0).any()
    return {"7x7 with zero taps": w7, "1x9": rng.normal(size=(1, 9)), "6x4": rng.normal(size=(6, 4))}


def holes(shape, dtype, share, seed):
    rng = np.random.default_rng(seed)
    X = (rng.normal(size=shape) * 5 + 100).astype(dtype)
    X[rng.random(shape) < share] = np.nan
    return X


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


@functools.lru_cache(maxsize=None)
def pf_routes(shape, dtype, nan):
    """{(route, incremental): (windows, impl)}: for every route the plan can return for this shape and dtype, the first
    candidate list (smallest radii) and impl (automatic, forced ring, forced direct) that takes it"""
    first = {}
    for win in pf_candidates():
        for impl in IMPLS:
            for key in pf_plan(np.dtype(dtype).itemsize, win, shape, nan, impl):
                first.setdefault(key, (tuple(win), impl))
    return first


# ------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------
def once(f):
    """``f()``, computed at the first call and kept for the later ones"""
    return functools.lru_cache(maxsize=None)(f)


def terrain_call(fn, Z, kw, impl):
    """tests/test_gpu_terrain.py's call(): count_openness takes its first three parameters by position"""
    kw = dict(kw)
    if fn == "count_openness":
        return F(fn)(Z, kw.pop("cellsize"), kw.pop("lookup_pixels"), kw.pop("threshold_angle"), **kw, impl=impl)
    return F(fn)(Z, **kw, impl=impl)


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


def dem_match(got, want, ctx):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0], equal_nan=True), ctx
    assert tuple(got[1]) == tuple(want[1])[:6], ctx


def chamfer_close(got, want, n):
    from test_gpu_points import _bound
    assert got.dtype == np.float64 and _bound(np.float64(got), want, n), (got, want, n)


# ------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------
BUILDERS = {}                    # name of GUARDED -> builder
EXTRA = {}                       # run under both harnesses outside GUARDED's names: case name -> builder


def builds(*names, table=BUILDERS):
    def register(f):
        for n in names:
            assert (n in GUARDED) == (table is BUILDERS) and n not in BUILDERS and n not in EXTRA, n
            table[n] = f
        return f
    return register


def case(name, fn, inputs, ctx, reference, stream=False, **more):
    return dict(name=name, fn=fn, inputs=inputs, ctx=ctx, reference=reference, stream=bool(stream), **more)


@builds(*SURFACE)
def surface(names):
    from test_gpu_surface import GRADIENT, compare
    for fn in names:
        kw = golden_kw("surface.npz", fn)
        for Z, ctx in cases_of(GRADIENT_SHAPES if fn in GRADIENT else TILE_SHAPES):
            yield case(fn, lambda Zt, fn=fn, kw=kw: F(fn)(Zt, **sn.decode_kw(kw)), [Z], (ctx, kw), stream="nan" in ctx,
                       reference=lambda got, fn=fn, kw=kw, Z=Z: compare(fn, Z, kw, got, sn.run(fn, Z, kw)))


@builds("focal_convolve", "std", "topographic_position_index", "reduce_peaks")
def focal(names, dtypes=(F32, F64)):
    """stream, on the NaN raster at impl AUTO: the 7x7 kernel with zero taps, TPI with radius 4 and the standardising sd,
    reduce_peaks"""
    from test_gpu_focal import assert_bits, check_tpi
    for Z, ctx in cases_of(TILE_SHAPES, dtypes):
        for kname, w in focal_kernels().items():
            pos = np.abs(w) + (w != 0) * 0.1
            want_c, want_s = once(lambda Z=Z, w=w: fnp.convolve(Z, w)), once(lambda Z=Z, pos=pos: fnp.std(Z, pos))
            for impl in IMPLS:
                c, s = (ctx, kname, impl), "nan" in ctx and kname == "7x7 with zero taps" and impl == AUTO
                if "focal_convolve" in names:
                    yield case("focal_convolve", lambda Zt, w=w, impl=impl: F("focal_convolve")(Zt, w, impl=impl), [Z], c, stream=s,
                               reference=lambda got, want=want_c, c=c: assert_bits(got, want(), c))
                if "std" in names:
                    yield case("std", lambda Zt, pos=pos, impl=impl: F("std")(Zt, pos, impl=impl), [Z], c, stream=s,
                               reference=lambda got, want=want_s, c=c: assert_bits(got, want(), c))
        if "topographic_position_index" in names:
            for kw in (dict(radius=1, standardize=True), dict(radius=4, standardize=True), dict(radius=4, standardize=False)):
                for impl in IMPLS:
                    c = (ctx, kw, impl)
                    yield case("topographic_position_index", lambda Zt, kw=kw, impl=impl: F("topographic_position_index")(
                        Zt, impl=impl, **kw), [Z], c, lambda got, Z=Z, kw=kw, c=c: check_tpi(Z, got, kw, c),
                               stream="nan" in ctx and kw == dict(radius=4, standardize=True) and impl == AUTO)
        if "reduce_peaks" in names:
            want = once(lambda Z=Z: fnp.reduce_peaks(Z, 3))
            for impl in IMPLS:
                c = (ctx, "reduce_peaks", impl)
                yield case("reduce_peaks", lambda Zt, impl=impl: F("reduce_peaks")(Zt, 3, impl=impl), [Z], c,
                           lambda got, want=want, c=c: assert_bits(got, want(), c), stream="nan" in ctx and impl == AUTO)


@builds(*TERRAIN)
def terrain(names, dtypes=(F32, F64)):
    """stream: cap + 1 without the fast variant, impl AUTO, on the NaN raster"""
    from neilpy_amd import _lib
    from test_gpu_terrain import compare
    for fn in names:
        base = golden_kw("terrain.npz", fn)
        for dtype in dtypes:
            cap = _lib.TERRAIN_HALO_CAP["f32" if dtype == F32 else "f64"]
            for Z, ctx in cases_of(TILE_SHAPES, (dtype,)):
                variants = [(L, {}) for L in (1, cap, cap + 1)]
                if fn in ("openness", "count_openness", "geomorphons"):
                    variants.append((cap + 1, dict(fast=True, how_fast=20)))
                for L, extra in variants:
                    kw = dict(base, lookup_pixels=L, **extra)
                    if fn == "geomorphons":
                        kw["enhance"] = True
                    kw.pop("neighbors", None)
                    want = once(lambda fn=fn, Z=Z, kw=kw: tn.run(fn, Z, kw))
                    for impl in IMPLS:
                        yield case(fn, lambda Zt, fn=fn, kw=kw, impl=impl: terrain_call(fn, Zt, kw, impl), [Z], (ctx, kw, impl),
                                   lambda got, fn=fn, Z=Z, kw=kw, want=want: compare(fn, Z, kw, got, want()),
                                   stream="nan" in ctx and L == cap + 1 and not extra and impl == AUTO)


@builds("scaled_morphometry", "vip_score", "ashift")
def morphometry(names, dtypes=(F32, F64)):
    """stream: each function's golden keywords on the NaN raster"""
    from test_gpu_morphometry import compare_morphometry
    kw_m, kw_v, kw_a = (golden_kw("morphometry.npz", f) for f in ("scaled_morphometry", "vip_score", "ashift"))
    for Z, ctx in cases_of(TILE_SHAPES, dtypes):
        if "scaled_morphometry" in names:
            for kw in (kw_m, dict(kw_m, lookup_pixels=64), dict(kw_m, lookup_pixels=65)):      # a wave's width and past it
                yield case("scaled_morphometry", lambda Zt, kw=kw: F("scaled_morphometry")(Zt, **kw), [Z], (ctx, kw),
                           lambda got, Z=Z, kw=kw, ctx=ctx: compare_morphometry(got, mnp.scaled_morphometry(Z, **kw), (ctx,)),
                           stream="nan" in ctx and kw is kw_m)
        if "vip_score" in names:
            yield case("vip_score", lambda Zt: F("vip_score")(Zt, **kw_v), [Z], ctx, stream="nan" in ctx,
                       reference=lambda got, Z=Z, ctx=ctx: assert_exact(got, mnp.vip_score(Z, **kw_v), ctx))
        if "ashift" in names:
            for kw in (kw_a, dict(direction=4, n=3), dict(direction=7, n=64)):
                yield case("ashift", lambda Zt, kw=kw: F("ashift")(Zt, **kw), [Z], (ctx, kw), stream="nan" in ctx and kw is kw_a,
                           reference=lambda got, Z=Z, kw=kw, ctx=ctx: assert_exact(got, mnp.ashift(Z, **kw), (ctx, kw)))


@builds("raster_stats", "rmse")
def statistics(names, dtypes=(F32, F64)):
    """stream: the (67, 131) NaN raster"""
    from neilpy_amd import _lib
    for dtype in dtypes:
        rng = np.random.default_rng(1)
        rasters = [((rng.normal(size=(1, n)) * 100).astype(dtype), n) for n in (1, 65, 257)]
        X = (rng.normal(size=(500, 600)) * 30 + 400).astype(dtype)
        rasters.append((X, "500x600"))
        Xn = X.copy()
        Xn[rng.random(X.shape) < 0.02] = np.nan
        rasters.append((Xn, "500x600, 2 % NaN"))
        rasters.append((raster(NAN_SHAPE, dtype, nan=True, seed=7), (NAN_SHAPE, np.dtype(dtype).name, "nan")))
        nbytes = lib().smrf_raster_stats_workspace_bytes(np.dtype(dtype).itemsize, _lib.STATS_MOMENTS | _lib.STATS_MEDIAN)
        for X, ctx in rasters:
            if "raster_stats" in names:
                yield case("raster_stats", lambda Xt: F("raster_stats")(Xt), [X], ctx, after=exact_workspace(nbytes),
                           reference=lambda got, X=X, ctx=ctx: stats_match(got, X, ctx), stream=X.shape == NAN_SHAPE)
            if "rmse" in names:
                yield case("rmse", lambda Xt: F("rmse")(Xt), [X], ctx, stream=X.shape == NAN_SHAPE,
                           reference=lambda got, X=X, ctx=ctx: (got.dtype == X.dtype and got == rn.rmse(X)) or pytest.fail(
                               "rmse %r" % (ctx,)))


@builds("normalize", "colortable_shade", "swiss_shading", "brassel_atmospheric_perspective")
def relief_images(names, dtypes=(F32, F64)):
    """stream, on the NaN raster: normalize, colortable_shade with lut_ghc, swiss_shading, brassel with the uint8 shade"""
    import neilpy_amd as na
    G = golden("relief.npz")
    xr, yr = ['min', 'median', 'max'], [-1, 0, 1]
    for Z, ctx in cases_of(GRADIENT_SHAPES, dtypes):
        if "normalize" in names:
            yield case("normalize", lambda Zt: F("normalize")(Zt, xr, yr), [Z], ctx, stream="nan" in ctx,
                       reference=lambda got, Z=Z, ctx=ctx: assert_exact(got, rn.normalize(Z, xr, yr), ctx))
        # the device's own shade (its own case is surface's), zi is NumPy's.  Launched from reference(), which both runners
        # call after their harness has closed: on the default stream, outside the guarded block and the side stream
        H = once(lambda Z=Z: na.hillshade(Z, 2))
        for fn, table, call in (("colortable_shade", "lut_ghc", lambda Zt, lt: F("colortable_shade")(Zt, lt, 2)),
                                ("colortable_shade", "lut_rand4", lambda Zt, lt: F("colortable_shade")(Zt, lt, 2)),
                                ("swiss_shading", "lut_swiss", lambda Zt, lt: F("swiss_shading")(Zt, 2, lut=lt))):
            def ref(got, fn=fn, table=table, Z=Z, ctx=ctx, H=H):
                # np.min / np.max of a raster with a NaN: every cell reads row 0 of the table
                want = rn.table3(G[table])[np.zeros(Z.shape, int) if "nan" in ctx else rn.table_index(Z), H()]
                assert got.dtype == np.uint8 and np.array_equal(got, want), "%s %r: %d cells differ" % (fn, ctx, int((got != want).sum()))
            if fn in names:
                yield case(fn, call, [Z, G[table]], (ctx, table), ref, stream="nan" in ctx and table != "lut_rand4")
        if "brassel_atmospheric_perspective" in names:
            h = np.random.default_rng(8).uniform(0, 1, size=Z.shape)
            for hkind, Hs in (("u8", np.round(255 * h).astype(np.uint8)), ("f32", h.astype(F32)), ("f64", h)):
                kw = dict(k=2.303, C2=0.41) if hkind != "f32" else dict(k=1.371, flat=200, reverse=True)
                yield case("brassel_atmospheric_perspective", lambda Ht, Zt, kw=kw: F("brassel_atmospheric_perspective")(Ht, Zt, **kw),
                           [Hs, Z], (ctx, hkind), brassel_reference(Hs, Z, kw, (ctx, hkind)), stream="nan" in ctx and hkind == "u8")


@builds("progressive_filter")
def progressive_filter(names, shapes=PF_SHAPES, dtypes=(F32, F64), nans=(False, True)):
    """one window list per route smrf_pf_plan reports.  Finite rasters against tests/morph_numpy.py, rasters with NaN
    against the oracle (SciPy's NaN rule), masks and when_dropped bit for bit as in tests/test_gpu_fuzz.py.
    stream: (70, 300), finite"""
    from oracle import smrf_oracle as orc
    for shape in shapes:
        for dtype in dtypes:
            nbytes = lib().smrf_progressive_filter_workspace_bytes(shape[0], shape[1], np.dtype(dtype).itemsize)
            for nan in nans:
                Z = pf_raster(shape, dtype, nan)
                refs = {}
                for win, impl in sorted(set(pf_routes(shape, dtype, nan).values())):
                    if win not in refs:
                        refs[win] = once(lambda Z=Z, win=win, nan=nan: (orc if nan else mn).progressive_filter(
                            Z, np.asarray(win), 1, .15, return_when_dropped=True))

                    def ref(got, win=win, impl=impl, want=refs[win]):
                        m, w = want()
                        assert np.array_equal(got[0], m) and np.array_equal(got[1], w), (
                            "progressive_filter %r impl %d: mask %d, when %d cells differ" % (
                                win, impl, int((got[0] != m).sum()), int((got[1] != w).sum())))
                    yield case("progressive_filter", lambda Zt, w=np.asarray(win), impl=impl: F("progressive_filter")(
                        Zt, w, 1, .15, return_when_dropped=True, impl=impl), [Z], (shape, np.dtype(dtype).name, nan, win, impl), ref,
                        after=exact_workspace(nbytes), stream=shape == PF_SHAPES[0] and not nan)


@builds(*DISK)
def disk(names, dtypes=(F32, F64), nans=(False, True)):
    """radius 2, 17 and (finite rasters, where the fast restatement serves) 64.  stream: (70, 300), finite, radius 17, AUTO"""
    from oracle import smrf_oracle as orc
    for dtype in dtypes:
        for nan in nans:
            for shape in PF_SHAPES:
                Z = pf_raster(shape, dtype, nan)
                for r in (2, 17) if nan else (2, 17, 64):
                    if nan:
                        e, d = once(lambda Z=Z, r=r: orc.erosion(Z, orc.disk(r))), once(lambda Z=Z, r=r: orc.dilation(Z, orc.disk(r)))
                        o = once(lambda e=e, r=r: orc.dilation(e(), orc.disk(r)))
                    else:
                        e, d = once(lambda Z=Z, r=r: mn.erosion(Z, r, "rows")), once(lambda Z=Z, r=r: mn.dilation(Z, r, "rows"))
                        o = once(lambda e=e, r=r: mn.dilation(e(), r, "rows"))
                    for impl in IMPLS:
                        for fn, want in zip(DISK, (e, d, o)):
                            c = (shape, np.dtype(dtype).name, nan, r, impl, fn)
                            if fn in names:
                                yield case(fn, lambda Zt, fn=fn, r=r, impl=impl: F(fn)(Zt, radius=r, impl=impl), [Z], c,
                                           lambda got, want=want, c=c: assert_exact(got, want(), c),
                                           stream=shape == PF_SHAPES[0] and not nan and r == 17 and impl == AUTO)


@builds("create_dem")
def create_dem(names, bin_types=("min", "max"), second_trip=True):
    """samp21 with and without edges; 8192 * 256 + 257 points, the bin loop's second trip, into 300 x 257 cells.
    stream: samp21, 'min', no edges"""
    from oracle import smrf_oracle as orc

    def one(x, y, z, bin_type, edges, ctx, shape=None):
        @once
        def want():
            dem = orc.create_dem(x, y, z, 1, bin_type, edges=edges)
            assert shape is None or dem[0].shape == shape, dem[0].shape
            return dem
        return case("create_dem", lambda a, b, c: F("create_dem")(a, b, c, 1, bin_type, edges=edges), [x, y, z], ctx,
                    lambda got: dem_match(got, want(), ctx), stream=ctx == ("min", False))
    if bin_types:
        x, y, z, _ = load_sample("samp21")
        # edges inside the cloud, so the filter drops points; off the centi-unit lattice of the sample's coordinates, so none
        # lies on the last edge (such a point passes the filter and is then outside the raster: both sides raise)
        xe = np.arange(np.floor(x.min()) + 10.503, np.ceil(x.max()) - 9.5, 1.0)
        ye = np.arange(np.ceil(y.max()) - 7.503, np.floor(y.min()) + 8.5, -1.0)
        assert ((x < xe[0]) | (x > xe[-1])).any() and ((y > ye[0]) | (y < ye[-1])).any()
        for bin_type in bin_types:
            for edges in (None, (xe, ye)):
                yield one(x, y, z, bin_type, edges, (bin_type, edges is not None))
    if second_trip:
        n = 8192 * 256 + 257
        rng = np.random.default_rng(22)
        x, y = rng.uniform(0.1, 255.9, n), rng.uniform(0.1, 298.9, n)
        x[:2], y[:2] = (0.1, 255.9), (0.1, 298.9)
        yield one(x, y, np.round(rng.normal(-3.0, 40.0, n), 2), 'min', None, "second trip", (300, 257))


@builds("read_las_xyz")
def read_las(names):
    """the smallest golden file"""
    from test_las import CASES, LAS
    tag = min(CASES, key=lambda c: LAS[c + "_col_x"].size)

    def ref(got):
        for k, c in enumerate("xyz"):
            assert np.array_equal(got[k], LAS[tag + "_col_" + c]), (tag, c)          # bit-exact with the reference's floats
    yield case("read_las_xyz", lambda: F("read_las_xyz")(os.path.join(GOLDEN, "las", tag + ".las"))[1:], [], tag, ref, stream=True)


@builds("inpaint_nearest", "nearest_source")
def nearest(names, dtypes=(F32, F64)):
    """inpaint_nearest fills in place: the finite cells keep their bits.  stream: (67, 131)"""
    for dtype in dtypes:
        single = np.full((40, 70), np.nan, dtype)
        single[23, 5] = 7.5
        for X, ctx in ((holes((1, 70), dtype, .5, 1), "(1, 70)"), (holes((67, 131), dtype, .6, 2), "(67, 131)"),
                       (single, "one source")):
            if "inpaint_nearest" in names:
                nbytes = lib().smrf_nearest_workspace_bytes(X.shape[0], X.shape[1], X.dtype.itemsize)
                yield case("inpaint_nearest", lambda Xt: F("inpaint_nearest")(Xt), [X], ctx, after=exact_workspace(nbytes),
                           known=lambda i, a: np.isfinite(a), stream=X.shape == (67, 131),
                           reference=lambda got, X=X, ctx=ctx: nn.same_bits(got, nn.inpaint_nearest(X)) or pytest.fail(
                               "inpaint_nearest " + ctx))

            def ref(got, X=X, ctx=ctx):
                dist, rc = got
                index, dist2, _ = nn.feature_transform(np.ascontiguousarray(X))
                assert dist.dtype == np.float64 and rc.dtype == np.int64 and rc.shape == (2,) + X.shape, ctx
                assert np.array_equal(rc[0] * X.shape[1] + rc[1], index), ctx
                assert np.array_equal(dist, np.sqrt(dist2.astype(np.float64))), ctx
            if "nearest_source" in names:
                yield case("nearest_source", lambda Xt: F("nearest_source")(Xt), [X], ctx, ref, stream=X.shape == (67, 131))


def springs_case(shape, seed, share):
    """through the public function, in place: tests/test_gpu_springs.py's rasters, stop and bar (1000 x how far the oracle's
    own answer moves when every sum is taken in another order, never above 1e-7); the known cells keep their bits"""
    import neilpy_amd as na
    from oracle import smrf_oracle as orc
    from test_gpu_springs import oracle_run, raster as springs_raster
    key = (shape, seed, share)
    A = np.array(springs_raster(*key))
    hole = np.isnan(A)

    @once
    def oracle():
        want, istop, itn = oracle_run(orc, A, key)
        flip, istop_f, itn_f = oracle_run(orc, A, key, flipped=True)
        assert (istop_f, itn_f) == (istop, itn)
        return want, istop, itn, min(1e-7, 1000.0 * float(np.abs(flip - want)[hole].max()))

    def fill(At):
        assert F("inpaint_nans_by_springs")(At, inplace=True) is None
        st = na.last_stats["inpaint"]
        assert (st["istop"], st["itn"], st["n_unknown"]) == oracle()[1:3] + (int(hole.sum()),), st
        return At

    def ref(got):
        want, _, _, bar = oracle()
        diff = float(np.abs(got - want)[hole].max())
        print("springs %s: device vs oracle %.3g, bar %.3g" % (shape, diff, bar))
        assert not np.isnan(got).any() and diff <= bar, (diff, bar)
    return case("inpaint_nans_by_springs", fill, [A], shape, ref, known=lambda i, a: ~np.isnan(a),
                after=exact_workspace(lib().smrf_springs_workspace_bytes(*shape)), stream=key == SPRINGS[0])


@builds("inpaint_nans_by_springs")
def springs(names, params=SPRINGS):
    for key in params:
        yield springs_case(*key)


@builds("inpaint_nans_by_fda")
def fda(names):
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
    yield case("inpaint_nans_by_fda", fill, [A], tag, ref, known=lambda i, a: ~np.isnan(a),
               after=exact_workspace(lib().smrf_fda_workspace_bytes(*A.shape)), stream=True)


@builds("nearest_points", "chamfer_distance")
def points(names, ds=(2, 3)):
    """clouds of 1, 257 and 1024 * 256 + 257 points (the bounds loop's second trip); the largest is searched by 257
    queries, which keeps the brute-force restatement small.  stream: d = 2, n = 257"""
    for d in ds:
        rng = np.random.default_rng(140 + d)
        q = rng.uniform(-1, 11, (257, d))
        for n in (1, 257, 1024 * 256 + 257):
            p = rng.uniform(0, 10, (n, d))

            def ref(got, n=n, d=d, want=once(lambda q=q, p=p: pn.nearest_points(q, p))):
                wd, wi = want()
                assert got[0].dtype == np.float64 and got[1].dtype == np.int64
                bad = np.flatnonzero((got[1] != wi) | (got[0].view(np.uint64) != wd.view(np.uint64)))
                assert bad.size == 0, (n, d, bad.size, bad[:5])
            if "nearest_points" in names:
                yield case("nearest_points", lambda qt, pt: F("nearest_points")(qt, pt), [q, p], (n, d), ref, stream=(d, n) == (2, 257),
                           after=exact_workspace(lib().smrf_points_nn_workspace_bytes(n, d)))
            if "chamfer_distance" in names:
                yield case("chamfer_distance", lambda qt, pt: F("chamfer_distance")(qt, pt), [q, p], (n, d), stream=(d, n) == (2, 257),
                           reference=lambda got, q=q, p=p, n=n: chamfer_close(got, pn.chamfer_distance(q, p), n + len(q)))


@builds("hungarian_algorithm", "bdr", "bdr_bootstrap")
def matching(names):
    """70 against 300 points of dimension 3 for the assignment, 65 pairs for the regression, 30 of 60 points under a
    7-row sample table for the bootstrap; every device-formed value has the bits of tests/assign_numpy.py.  stream: all three"""
    import assign_cases as ac
    import assign_numpy as an
    from test_gpu_assign import assert_bits
    x, a = ac.random_pair(70, 300, 3, 60)
    bx, ba = ac.random_pair(65, 65, 2, 61)
    sx, sa = ac.random_pair(30, 60, 2, 62)
    ba, sa = ba + 0.7 * bx, sa + 0.5 * np.vstack([sx, sx])
    table = np.stack([np.random.default_rng(63 + s).permutation(60)[:30] for s in range(7)]).astype(np.int64)
    if "hungarian_algorithm" in names:
        yield case("hungarian_algorithm", lambda xt, at: F("hungarian_algorithm")(xt, at), [x, a], (70, 300, 3), stream=True,
                   reference=lambda got: assert_bits(got, an.hungarian_algorithm(x, a), range(3), "hungarian_algorithm"))
    if "bdr" in names:
        yield case("bdr", lambda xt, at: F("bdr")(xt, at), [bx, ba], 65, stream=True,
                   reference=lambda got: assert_bits(got, an.bdr(bx, ba), an.SCALARS, "bdr"))
    if "bdr_bootstrap" in names:
        yield case("bdr_bootstrap", lambda xt, at, tt: F("bdr_bootstrap")(xt, at, samples=tt), [sx, sa, table], (30, 60, 7),
                   stream=True, reference=lambda got: assert_bits(got, an.bdr_bootstrap(sx, sa, table), range(2), "bdr_bootstrap"))


@builds(*MORPHOLOGY)
def morphology(names, dtypes=(F32, F64)):
    """three footprints of tests/test_gpu_footprint.py - rand4x7 (even-sized and not its own mirror image: the gradient takes
    two launches), diamond5 (one) and L7x4 - under 'reflect' on every raster, under 'nearest' once per name, every impl
    (a forced runs launch the plan refuses is left to that module).  stream: the NaN raster, rand4x7, 'reflect', AUTO"""
    from test_gpu_footprint import assert_same, footprints, reference, runs_refused
    fps = {tag: fp for tag, fp in footprints().items() if tag in ("rand4x7", "diamond5", "L7x4")}
    for Z, ctx in cases_of(TILE_SHAPES, dtypes):
        for tag, fp in fps.items():
            nearest_too = tag == "rand4x7" and ctx[0] == NAN_SHAPE and "nan" not in ctx
            for mode in ("reflect", "nearest") if nearest_too else ("reflect",):
                for fn in names:
                    want = once(lambda fn=fn, Z=Z, fp=fp, mode=mode: reference(fn, Z, fp, mode))
                    for impl in IMPLS if mode == "reflect" else (AUTO,):
                        if impl == RUNS and runs_refused(fn, fp, Z.dtype):
                            continue
                        c = (ctx, tag, mode, impl)
                        yield case(fn, lambda Zt, fn=fn, fp=fp, mode=mode, impl=impl: F(fn)(Zt, footprint=fp, mode=mode, impl=impl),
                                   [Z], c, lambda got, want=want, c=c: assert_same(got, want(), c),
                                   stream="nan" in ctx and (tag, mode, impl) == ("rand4x7", "reflect", AUTO))


@builds("voxelize")
def voxelize(names, dtypes=(F32, F64)):
    """stream: the 4000-point cloud with a vertical exaggeration, padding and a count threshold"""
    from test_gpu_voxel import COUNTS, RESOLUTIONS, cloud
    n, resolution = COUNTS[0], RESOLUTIONS[0]
    for T in dtypes:
        for (x, y, z), res, kw in ((cloud(n, 10 * n + resolution, T), resolution, dict(bottom_fill=True)),
                                   (cloud(4000, 77, T), 32, dict(ve=33 / 8.0, bottom_fill=False, pad=3, threshold=2))):
            def ref(got, x=x, y=y, z=z, res=res, kw=kw):
                want = vn.voxelize(None, x, y, z, res, **kw)
                assert got.dtype == bool and got.shape == want.shape and np.array_equal(got, want), "voxelize %r" % (kw,)
            yield case("voxelize", lambda a, b, c, res=res, kw=kw: F("voxelize")(None, a, b, c, res, **kw), [x, y, z], (n, res, kw), ref,
                       stream="pad" in kw)


@builds("pssm")
def pssm(names, parts=("shapes", "nan")):
    """shapes: classes and RGBA on rasters narrower than the goldens of tests/test_pssm.py, equal to the oracle in every
    cell.  nan: a cell whose gradient reads a NaN has a NaN slope, and the class of NaN is 0 (NumPy's cast of NaN to uint8
    on the reference's platform); every other cell is the oracle's.  stream: classes, and RGBA reversed, on (67, 131)"""
    from oracle import smrf_oracle as orc
    from test_pssm import G
    for shape in PSSM_SHAPES if "shapes" in parts else ():
        Z = raster(shape, F64)
        yield case("pssm", lambda Zt: F("pssm")(Zt, 1.5, 2.3, False, False), [Z], (shape, "classes"), stream=shape == NAN_SHAPE,
                   reference=lambda got, Z=Z: (got.dtype == np.uint8 and np.array_equal(got, orc.pssm_classes(Z, 1.5, 2.3))) or
                   pytest.fail("pssm classes %r" % (Z.shape,)))
        for reverse, lut in ((False, "lut_bone_r"), (True, "lut_bone")):
            yield case("pssm", lambda Zt, reverse=reverse: F("pssm")(Zt, 1.5, 2.3, reverse), [Z], (shape, "rgba", reverse),
                       lambda got, Z=Z, lut=lut: (got.shape == Z.shape + (4,) and np.array_equal(got, orc.pssm(Z, G[lut], 1.5, 2.3)))
                       or pytest.fail("pssm rgba %r" % (Z.shape,)), stream=shape == NAN_SHAPE and reverse)
    if "nan" in parts:
        Z = raster((67, 131), F64, nan=True, seed=3)
        gy, gx = np.gradient(Z, 1.5)
        bad = np.isnan(gx) | np.isnan(gy)
        assert bad.any() and not bad.all()

        def ref(got):
            with np.errstate(all='ignore'):
                want = orc.pssm_classes(Z, 1.5, 2.3)
            assert got.dtype == np.uint8 and (got[bad] == 0).all(), int((got[bad] != 0).sum())
            assert np.array_equal(got[~bad], want[~bad])
        yield case("pssm", lambda Zt: F("pssm")(Zt, 1.5, 2.3, False, False), [Z], "nan", ref)


@builds("smrf")
def smrf(names, tails=None):
    """smrf() with tensor inputs: every intermediate plane of the pipeline at once; against the golden of
    tests/test_gpu_parity.py's test_smrf_samples_golden, through that file's check_smrf.  ``tails`` gets each run's tail
    statistics"""
    import neilpy_amd as na
    from test_gpu_parity import META, check_smrf
    x, y, z, g = load_sample("samp21")
    gold = golden("smrf_samp21.npz")
    kw = META["smrf_kwargs"]
    tails = [] if tails is None else tails

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
    yield case("smrf", call, [x, y, z], "samp21", ref, stream=True)


def spline_case(shape):
    """smrf_spline_solve_ws_f64 and smrf_spline_eval_f64 as smrf() calls them, the scratch plane the harness's, against
    SciPy with the bars of tests/test_gpu_parity.py's test_spline_matches_scipy.  (300, 257): two chunks on both axes and a
    last 64-column tile one column wide."""
    import torch
    from scipy import interpolate
    from neilpy_amd import _lib, spline
    rows, cols = shape
    rng = np.random.default_rng(12)
    Z = rng.normal(100, 5, shape)
    pr, pc = rng.uniform(-1.0, rows + 1.0, 5000), rng.uniform(-1.0, cols + 1.0, 5000)
    pr[:4], pc[:4] = [0.5, rows - 0.5, 0.0, rows], [0.5, cols - 0.5, cols, 0.0]
    pr[4:4 + min(rows, 50)] = np.arange(.5, rows + .5)[:50]
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
        f = interpolate.RectBivariateSpline(np.arange(.5, rows + .5), np.arange(.5, cols + .5), Z)
        want = f.ev(pr, pc)
        print("spline %s: coefficients %.3g (bar 1e-10), values %.3g (bar 1e-9)" % (
            shape, np.abs(got[0].ravel() - f.tck[2]).max(), np.abs(got[1] - want).max()))
        np.testing.assert_allclose(got[0].ravel(), f.tck[2], rtol=0, atol=1e-10)
        np.testing.assert_allclose(got[1], want, rtol=0, atol=1e-9)
    # the solve works in place on the coefficient plane: input 0 is exempt from "unchanged", the others are not
    return case("smrf_spline", call, [Z, tx, ty, lur, luc, pr, pc], shape, ref, stream=shape == (9, 300),
                known=lambda i, a: np.zeros(a.shape, bool) if i == 0 else None)


@builds("smrf_spline", table=EXTRA)
def spline(names, shapes=SPLINE_SHAPES):
    for shape in shapes:
        yield spline_case(shape)


@builds("sharded", table=EXTRA)
def sharded(names):
    """tests/test_gpu_edges.py's test_sharded_driver_bands_on_one_gpu at its smallest parametrisation (2 ranks, 200 x 131,
    windows 2, 6, 1), every rank in turn in this process: band planes and halo buffers come from sharded.py"""
    import neilpy_amd as na
    from neilpy_amd import sharded as bands
    from oracle import smrf_oracle as orc
    from sharded_one_gpu import run_bands
    world, shape, win = 2, (200, 131), np.asarray([2, 6, 1])
    Z = na.synth_dem(shape[1], seed=9, rows=shape[0]).astype(F32)

    def call(Zt):
        mask, when, _ = run_bands(na, Zt, win, world, return_when_dropped=True, budget=None, ops=bands.HipBandOps,
                                  overlap=lambda k: k % 2 == 0)
        return mask, when

    def ref(got):
        want_m, want_w = orc.progressive_filter(Z, win, 1, .15, return_when_dropped=True)
        assert np.array_equal(got[0], want_m) and np.array_equal(got[1], want_w), "sharded"
    yield case("sharded", call, [Z], shape, ref, stream=True)
