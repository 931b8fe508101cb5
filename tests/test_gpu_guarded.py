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

The cases - inputs, calls, references - are tests/family_cases.py's, one builder per export; each test below runs the
part of a builder's sweep that its parameters select.

Workspaces.  The public wrappers of ``smrf_raster_stats_*``, ``smrf_nearest_*``, ``smrf_points_nn_*``, ``smrf_voxel_*``,
``smrf_springs_lsqr_f64``, ``smrf_fda_lsqr_f64`` and ``smrf_progressive_filter_*`` allocate ``*_workspace_bytes(...)`` bytes
as they are (``exact_workspace`` asserts that such an allocation was served); the TPI workspace of ``smrf_focal_*`` is
rounded by its wrapper.  The last section calls every one of these entry points once more straight through ctypes with
a workspace of exactly that many bytes carved by the harness, so that the tail guard sits on the first byte the library
did not ask for whatever a wrapper does.
"""
import ctypes as C

import numpy as np
import pytest

import family_cases as FC
import focal_numpy as fnp
import morph_numpy as mn
import nearest_numpy as nn
import points_numpy as pn
import voxel_numpy as vn
from family_cases import (DEVICE, DIRECT, DISK, F32, F64, NOT_OWNED, PF_SHAPES, SURFACE, TERRAIN, TILE_SHAPES, TILED, chamfer_close,
                          holes, leaves, lib, pf_raster, raster, rebuild, stats_match, to_numpy)
from guarded import POISONS, guarded, same_bits

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------
# run_guarded
# ------------------------------------------------------------------------------------------
def run_guarded(fn, inputs, kw=None, *, name, reference=None, known=None, ctx=None, after=None, stream=None):
    """``fn(*inputs as harness tensors, **kw)`` under both poisons with the five assertions of the module docstring.
    ``name`` keys NOT_OWNED; ``reference(result as NumPy)`` asserts against the restatement; ``known(i, array)`` is the
    mask of cells of input ``i`` that must keep their bits (default: all of them); ``after(g)`` looks at the harness;
    ``stream`` is the case table's mark for tests/test_gpu_streams.py and means nothing here.
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
        for path, v in leaves(res):                                                      # Ownership
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
        runs.append(rebuild(res, to_numpy))
        del g, tens, res
    a, b = (list(leaves(r)) for r in runs)                                               # Identity
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


def run_all(cases):
    for case in cases:
        run_guarded(**case)


# ------------------------------------------------------------------------------------------
# the families: every case of tests/family_cases.py's builders, split by the parameters below
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", SURFACE)
def test_surface(gpu_device, fn):
    run_all(FC.surface((fn,)))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_focal_convolve_and_std(gpu_device, dtype):
    run_all(FC.focal(("focal_convolve", "std"), (dtype,)))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_focal_tpi_and_reduce_peaks(gpu_device, dtype):
    """TPI: the partials workspace and the single-workgroup reduce behind the standardising sd"""
    run_all(FC.focal(("topographic_position_index", "reduce_peaks"), (dtype,)))


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
                g = _g()
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


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("fn", TERRAIN)
def test_terrain(gpu_device, fn, dtype):
    """lookup_pixels 1, the LDS tile's halo cap and cap + 1 (the taps past the halo come from global memory), every impl;
    geomorphons with enhance (both marches from one launch, L > 16) and, like openness and count_openness, once fast"""
    run_all(FC.terrain((fn,), (dtype,)))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_morphometry(gpu_device, dtype):
    run_all(FC.morphometry(("scaled_morphometry", "vip_score", "ashift"), (dtype,)))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_raster_stats(gpu_device, dtype):
    """n = 1, 65, 257 and 500 x 600, the grid-stride loop's second trip; moments and the radix select's workspace"""
    run_all(FC.statistics(("raster_stats", "rmse"), (dtype,)))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_relief_images(gpu_device, dtype):
    """normalize with a median knot, the colour gather against the device's own shade, brassel with uint8 and float shades"""
    run_all(FC.relief_images(("normalize", "colortable_shade", "swiss_shading", "brassel_atmospheric_perspective"), (dtype,)))


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("shape", PF_SHAPES)
def test_progressive_filter_routes(gpu_device, shape, dtype, nan):
    """one window list per route smrf_pf_plan reports: ring passes, chains, the fused opening, the incremental erosion,
    the direct kernel and the copy"""
    from neilpy_amd import _lib
    routes = FC.pf_routes(shape, dtype, nan)
    covered = set()
    for case in FC.progressive_filter(("progressive_filter",), (shape,), (dtype,), (nan,)):
        run_guarded(**case)
        win, impl = case["ctx"][3:]
        covered |= set(FC.pf_plan(np.dtype(dtype).itemsize, win, shape, nan, impl))
    print("routes", shape, np.dtype(dtype).name, nan, sorted(routes.items()))
    assert covered == set(routes) and {r for r, _ in covered} >= {_lib.ROUTE_TWO_PASS, _lib.ROUTE_DIRECT, _lib.ROUTE_COPY}


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_disk_filters(gpu_device, dtype, nan):
    """erosion, dilation and opening by the ring and the direct kernel"""
    run_all(FC.disk(DISK, (dtype,), (nan,)))


@pytest.mark.parametrize("bin_type", ["min", "max"])
def test_create_dem_samp21(gpu_device, bin_type):
    run_all(FC.create_dem(("create_dem",), (bin_type,), second_trip=False))


def test_create_dem_second_trip(gpu_device):
    """8192 * 256 + 257 points, the bin loop's second trip, into 300 x 257 cells"""
    run_all(FC.create_dem(("create_dem",), (), second_trip=True))


def test_read_las_xyz(gpu_device):
    run_all(FC.read_las(("read_las_xyz",)))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_inpaint_nearest(gpu_device, dtype):
    """fills in place: the finite cells keep their bits.  nearest_source's planes as tests/test_gpu_nearest.py reads them"""
    run_all(FC.nearest(("inpaint_nearest", "nearest_source"), (dtype,)))


@pytest.mark.parametrize("shape,seed,share", FC.SPRINGS)
def test_inpaint_springs(gpu_device, shape, seed, share):
    run_all(FC.springs(("inpaint_nans_by_springs",), ((shape, seed, share),)))


def test_inpaint_fda(gpu_device):
    run_all(FC.fda(("inpaint_nans_by_fda",)))


@pytest.mark.parametrize("d", [2, 3])
def test_points(gpu_device, d):
    run_all(FC.points(("nearest_points", "chamfer_distance"), (d,)))


@pytest.mark.parametrize("fn", ["hungarian_algorithm", "bdr", "bdr_bootstrap"])
def test_matching(gpu_device, fn):
    run_all(FC.matching((fn,)))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_morphology(gpu_device, dtype):
    """three footprints, both border modes, the runs and the taps path: one and two launches per function"""
    run_all(FC.morphology(FC.MORPHOLOGY, (dtype,)))


@pytest.mark.parametrize("T", [F32, F64])
def test_voxelize(gpu_device, T):
    run_all(FC.voxelize(("voxelize",), (T,)))


def test_pssm(gpu_device):
    """classes and RGBA on rasters narrower than the goldens of tests/test_pssm.py, equal to the oracle in every cell"""
    run_all(FC.pssm(("pssm",), ("shapes",)))


def test_pssm_nan_is_class_zero(gpu_device):
    run_all(FC.pssm(("pssm",), ("nan",)))


@pytest.mark.parametrize("shape", FC.SPLINE_SHAPES)
def test_spline(gpu_device, shape):
    run_all(FC.spline(("smrf_spline",), (shape,)))


def test_smrf_samp21(gpu_device):
    """smrf() with tensor inputs: every intermediate plane of the pipeline behind guards at once"""
    tails = []
    run_all(FC.smrf(("smrf",), tails))
    assert same_bits(tails[0]["elevation_values"], tails[1]["elevation_values"])
    assert same_bits(tails[0]["slope_values"], tails[1]["slope_values"])


def test_sharded_bands_on_one_gpu(gpu_device):
    run_all(FC.sharded(("sharded",)))


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
