"""Every kernel family on a side stream (tests/streamed.py: decoy inputs, a delay ahead of every poison fill, the stream
handle of every library call recorded).

First the harness proves itself with stand-ins, torch ops on the harness's own memory: a correct one passes; one that
computes under the default stream reads the decoy; one whose last copy runs on the default stream ends up as poison; one
whose library call carries stream 0 fails the handle check - each in 10 of 10 repetitions at the delay D and at D / 4.

Then one ``run_streamed`` case per name of tests/test_gpu_guarded.py's GUARDED (and per dtype where the function takes
both), built from what that module builds for the name: the same rasters, keywords, window lists and reference
comparisons, at a single shape each - (67, 131) with 2 % NaN for the rasters, (70, 300) with one window list per route of
``smrf_pf_plan`` for progressive_filter - plus the spline pair, the one-GPU band driver, two NumPy-in NumPy-out calls of
slope (the second through the pinned staging buffers) and two streams in one thread that share an input and the library's
cached device tables.  Shapes are the guarded module's job; this one varies the stream only.

Measured on an MI355X (the module prints these figures; D is a sensitivity setting, no tolerance - correct code passes at
any D):
    torch.cuda._sleep runs 2.39 M cycles per millisecond.  On each of four fresh streams, 10 repetitions per delay:
    stand-ins (a) and (b) were caught 10 of 10 from 4 ms down to 0.0625 ms, (a) 9 of 10 on one stream at 0.03125 ms, none at
    0.015625 ms; (c) and the correct stand-in were judged right at every delay.  The detection threshold is 0.0625 ms,
    which makes 0.25 ms the smallest D that is caught at D and at D / 4.  D is set to 1 ms = 2 386 775 cycles, four times
    that: test_standins repeats the proof at D / 4 in every run, and at D = 1 ms that repetition runs at 0.25 ms, fourfold
    above the threshold instead of on it (what sets the threshold is how fast the host enqueues, which a busier machine
    does more slowly).  Side stream: candidate 0 of 4 (all four qualified).  376 redirected allocations per module run,
    each behind one delay; the module takes 5.1 s (tests/test_gpu_threads.py: 5.1 s).
Mutants, run once on a scratch copy: with ``_raster._stream()`` returning handle 0 all 65 cases of the 26 names whose
scratch planes hold values only (surface, focal, terrain, morphometry, disk filters, progressive_filter) failed on the
handle check; the other families were not run under that mutant, since a poisoned index plane read by a kernel on the
wrong stream can become an address.  For the same reason the ``hipMemsetAsync`` of points.hip was not moved to stream 0:
the cell counts would be poisoned before they are counted and the scatter kernel's slots would lie far outside the
workspace.  In its place the first ``points_sum_kernel`` launch of ``smrf_points_nn_sum_f64`` went to stream 0, built as a
library of its own: chamfer_distance failed on data (0.474 for 0.858), nearest_points, which does not call it, passed.
"""
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
import streamed as S
import test_gpu_guarded as T
from conftest import golden, load_sample
from family_checks import assert_exact
from streamed import EXPECTED, Host, run_streamed, standin_verdict
from test_gpu_guarded import F, F32, F64, GUARDED

pytestmark = pytest.mark.gpu

STATS = {}                       # allocations served over the module's run (printed by the last test)
SHAPE = T.NAN_SHAPE
PF_SHAPE = T.PF_SHAPES[0]


def streamed(fn, inputs, **k):
    return run_streamed(fn, inputs, stats=STATS, **k)


# ------------------------------------------------------------------------------------------
# the harness on stand-ins
# ------------------------------------------------------------------------------------------
def test_delay_is_what_it_says(gpu_device):
    import torch
    sleep = S.delay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sleep()
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    print("delay: D = %g ms asked, %.3f ms measured, %d cycles (%.0f cycles per ms)" % (
        S.D_MS, ms, int(S.D_MS * S.cycles_per_ms()), S.cycles_per_ms()))
    assert 0.5 * S.D_MS <= ms <= 4.0 * S.D_MS + 1.0          # the calibration holds: neither no delay nor a far longer one


def test_a_side_stream_on_which_offenders_are_caught(gpu_device):
    side = S.side_stream()                                   # StreamHarnessError when none of the candidates qualifies
    print("side stream: candidate %d of %d, handle 0x%x" % (S.SIDE_INDEX, S.CANDIDATES, side.cuda_stream))
    assert side.cuda_stream != 0


@pytest.mark.parametrize("share", [1.0, 0.25], ids=["D", "D/4"])
@pytest.mark.parametrize("kind", S.STANDINS)
def test_standins(gpu_device, kind, share):
    """the correct stand-in passes and each offender fails for its stated reason, 10 times of 10, at D and at D / 4"""
    side = S.side_stream()
    verdicts = [standin_verdict(kind, side, share * S.D_MS) for _ in range(10)]
    print("stand-in %s at %g ms: %s" % (kind, share * S.D_MS, verdicts))
    assert verdicts == [EXPECTED[kind]] * 10, (kind, share * S.D_MS, verdicts)


# ------------------------------------------------------------------------------------------
# one case per guarded name
# ------------------------------------------------------------------------------------------
CASES = {}                       # name -> generator of run_streamed keyword dicts


def cases(*names):
    def register(f):
        for n in names:
            assert n in GUARDED and n not in CASES, n
            CASES[n] = (lambda n=n: f(n))
        return f
    return register


def nan_raster(dtype):
    """cases_of()'s last raster: (67, 131) with 2 % NaN cells"""
    return T.raster(SHAPE, dtype, nan=True, seed=7), (SHAPE, np.dtype(dtype).name, "nan")


def both(f):
    """f(name, dtype, Z, ctx) -> case dicts, for float32 and float64"""
    def g(name):
        for dtype in (F32, F64):
            Z, ctx = nan_raster(dtype)
            yield from f(name, dtype, Z, ctx)
    return g


@cases(*T.SURFACE)
@both
def surface(fn, dtype, Z, ctx):
    from test_gpu_surface import compare
    kw = T.golden_kw("surface.npz", fn)
    yield dict(fn=lambda Zt: F(fn)(Zt, **sn.decode_kw(kw)), inputs=[Z], ctx=(ctx, kw),
               reference=lambda got: compare(fn, Z, kw, got, sn.run(fn, Z, kw)))


@cases("focal_convolve", "std", "reduce_peaks", "topographic_position_index")
@both
def focal(fn, dtype, Z, ctx):
    from test_gpu_focal import assert_bits, check_tpi
    w = T.focal_kernels()["7x7 with zero taps"]
    pos = np.abs(w) + (w != 0) * 0.1
    if fn == "focal_convolve":
        want = fnp.convolve(Z, w)
        yield dict(fn=lambda Zt: F("focal_convolve")(Zt, w), inputs=[Z], ctx=ctx, reference=lambda got: assert_bits(got, want, ctx))
    elif fn == "std":
        want = fnp.std(Z, pos)
        yield dict(fn=lambda Zt: F("std")(Zt, pos), inputs=[Z], ctx=ctx, reference=lambda got: assert_bits(got, want, ctx))
    elif fn == "reduce_peaks":
        want = fnp.reduce_peaks(Z, 3)
        yield dict(fn=lambda Zt: F("reduce_peaks")(Zt, 3), inputs=[Z], ctx=ctx, reference=lambda got: assert_bits(got, want, ctx))
    else:
        kw = dict(radius=4, standardize=True)                # the partials workspace and the single-workgroup reduce
        yield dict(fn=lambda Zt: F("topographic_position_index")(Zt, **kw), inputs=[Z], ctx=(ctx, kw),
                   reference=lambda got: check_tpi(Z, got, kw, ctx))


@cases(*T.TERRAIN)
@both
def terrain(fn, dtype, Z, ctx):
    from neilpy_amd import _lib
    from test_gpu_terrain import compare
    kw = dict(T.golden_kw("terrain.npz", fn), lookup_pixels=_lib.TERRAIN_HALO_CAP["f32" if dtype == F32 else "f64"] + 1)
    if fn == "geomorphons":
        kw["enhance"] = True
    kw.pop("neighbors", None)
    want = tn.run(fn, Z, kw)
    yield dict(fn=lambda Zt: T.terrain_call(fn, Zt, kw, T.AUTO), inputs=[Z], ctx=(ctx, kw),
               reference=lambda got: compare(fn, Z, kw, got, want))


@cases("scaled_morphometry", "vip_score", "ashift")
@both
def morphometry(fn, dtype, Z, ctx):
    from test_gpu_morphometry import compare_morphometry
    kw = T.golden_kw("morphometry.npz", fn)
    if fn == "scaled_morphometry":
        ref = lambda got: compare_morphometry(got, mnp.scaled_morphometry(Z, **kw), (ctx,))      # noqa: E731
    else:
        ref = lambda got: assert_exact(got, getattr(mnp, fn)(Z, **kw), ctx)                     # noqa: E731
    yield dict(fn=lambda Zt: F(fn)(Zt, **kw), inputs=[Z], ctx=(ctx, kw), reference=ref)


@cases("raster_stats", "rmse", "normalize")
@both
def statistics(fn, dtype, Z, ctx):
    if fn == "raster_stats":
        yield dict(fn=lambda Zt: F("raster_stats")(Zt), inputs=[Z], ctx=ctx, reference=lambda got: T.stats_match(got, Z, ctx))
    elif fn == "rmse":
        yield dict(fn=lambda Zt: F("rmse")(Zt), inputs=[Z], ctx=ctx,
                   reference=lambda got: (got.dtype == Z.dtype and got == rn.rmse(Z)) or pytest.fail("rmse %r" % (ctx,)))
    else:
        xr, yr = ['min', 'median', 'max'], [-1, 0, 1]
        yield dict(fn=lambda Zt: F("normalize")(Zt, xr, yr), inputs=[Z], ctx=ctx,
                   reference=lambda got: assert_exact(got, rn.normalize(Z, xr, yr), ctx))


@cases("colortable_shade", "swiss_shading", "brassel_atmospheric_perspective")
@both
def relief(fn, dtype, Z, ctx):
    import neilpy_amd as na
    G = golden("relief.npz")
    if fn == "brassel_atmospheric_perspective":
        Hs = np.round(255 * np.random.default_rng(8).uniform(0, 1, size=Z.shape)).astype(np.uint8)
        kw = dict(k=2.303, C2=0.41)
        yield dict(fn=lambda Ht, Zt: F(fn)(Ht, Zt, **kw), inputs=[Hs, Z], ctx=(ctx, "u8"),
                   reference=T.brassel_reference(Hs, Z, kw, (ctx, "u8")))
        return
    H = na.hillshade(Z, 2)                                   # the device's own shade, made on the default stream beforehand
    table = "lut_ghc" if fn == "colortable_shade" else "lut_swiss"
    want = rn.table3(G[table])[np.zeros(Z.shape, int), H]    # np.min / np.max of a raster with a NaN
    call = (lambda Zt, lt: F("colortable_shade")(Zt, lt, 2)) if fn == "colortable_shade" else \
        (lambda Zt, lt: F("swiss_shading")(Zt, 2, lut=lt))
    yield dict(fn=call, inputs=[Z, G[table]], ctx=(ctx, table),
               reference=lambda got: (got.dtype == np.uint8 and np.array_equal(got, want)) or pytest.fail(
                   "%s %r: %d cells differ" % (fn, ctx, int((got != want).sum()))))


@cases("progressive_filter")
def progressive_filter(_):
    """(70, 300), finite: one window list per route the plan reports for it, as test_progressive_filter_routes draws them"""
    for dtype in (F32, F64):
        Z = T.pf_raster(PF_SHAPE, dtype, False)
        routes = T.pf_routes(PF_SHAPE, dtype, False)
        for win, impl in sorted(set(routes.values())):
            w = np.asarray(win)
            want_m, want_w = mn.progressive_filter(Z, w, 1, .15, return_when_dropped=True)
            yield dict(fn=lambda Zt, w=w, impl=impl: F("progressive_filter")(Zt, w, 1, .15, return_when_dropped=True, impl=impl),
                       inputs=[Z], ctx=(PF_SHAPE, np.dtype(dtype).name, win, impl),
                       reference=lambda got, m=want_m, n=want_w: (np.array_equal(got[0], m) and np.array_equal(got[1], n)) or
                       pytest.fail("progressive_filter: mask %d, when %d cells differ" % (
                           int((got[0] != m).sum()), int((got[1] != n).sum()))))


@cases(*T.DISK)
def disk(fn):
    for dtype in (F32, F64):
        Z = T.pf_raster(PF_SHAPE, dtype, False)
        r = 17
        want = {"erosion": lambda: mn.erosion(Z, r, "rows"), "dilation": lambda: mn.dilation(Z, r, "rows"),
                "opening": lambda: mn.dilation(mn.erosion(Z, r, "rows"), r, "rows")}[fn]()
        c = (PF_SHAPE, np.dtype(dtype).name, r, fn)
        yield dict(fn=lambda Zt: F(fn)(Zt, radius=r), inputs=[Z], ctx=c, reference=lambda got, w=want: assert_exact(got, w, c))


@cases("create_dem")
def create_dem(_):
    from oracle import smrf_oracle as orc
    x, y, z, _g = load_sample("samp21")
    want = orc.create_dem(x, y, z, 1, 'min')
    yield dict(fn=lambda a, b, c: F("create_dem")(a, b, c, 1, 'min'), inputs=[x, y, z], ctx="samp21",
               reference=lambda got: T.dem_match(got, want, "samp21"))


@cases("read_las_xyz")
def read_las(_):
    yield T.read_las_case()


@cases("inpaint_nearest", "nearest_source")
def nearest(fn):
    for dtype in (F32, F64):
        X = T.holes(SHAPE, dtype, .6, 2)
        ctx = (SHAPE, np.dtype(dtype).name)
        if fn == "inpaint_nearest":
            yield dict(fn=lambda Xt: F("inpaint_nearest")(Xt), inputs=[X], ctx=ctx,
                       reference=lambda got, X=X: nn.same_bits(got, nn.inpaint_nearest(X)) or pytest.fail("inpaint_nearest"))
        else:
            def ref(got, X=X):
                dist, rc = got
                index, dist2, _ = nn.feature_transform(np.ascontiguousarray(X))
                assert dist.dtype == np.float64 and rc.dtype == np.int64 and rc.shape == (2,) + X.shape, ctx
                assert np.array_equal(rc[0] * X.shape[1] + rc[1], index), ctx
                assert np.array_equal(dist, np.sqrt(dist2.astype(np.float64))), ctx
            yield dict(fn=lambda Xt: F("nearest_source")(Xt), inputs=[X], ctx=ctx, reference=ref)


@cases("inpaint_nans_by_springs")
def springs(_):
    yield T.springs_case((37, 53), 1, .5)


@cases("inpaint_nans_by_fda")
def fda(_):
    yield T.fda_case()


@cases("nearest_points", "chamfer_distance")
def points(fn):
    d, n = 2, 257
    rng = np.random.default_rng(140 + d)
    q = rng.uniform(-1, 11, (257, d))
    p = rng.uniform(0, 10, (n, d))
    if fn == "nearest_points":
        wd, wi = pn.nearest_points(q, p)

        def ref(got):
            assert got[0].dtype == np.float64 and got[1].dtype == np.int64
            bad = np.flatnonzero((got[1] != wi) | (got[0].view(np.uint64) != wd.view(np.uint64)))
            assert bad.size == 0, (n, d, bad.size, bad[:5])
        yield dict(fn=lambda qt, pt: F("nearest_points")(qt, pt), inputs=[q, p], ctx=(n, d), reference=ref)
    else:
        want = pn.chamfer_distance(q, p)
        yield dict(fn=lambda qt, pt: F("chamfer_distance")(qt, pt), inputs=[q, p], ctx=(n, d),
                   reference=lambda got: T.chamfer_close(got, want, n + len(q)))


@cases("voxelize")
def voxelize(_):
    from test_gpu_voxel import cloud
    for dtype in (F32, F64):
        x, y, z = cloud(4000, 77, dtype)
        kw = dict(ve=33 / 8.0, bottom_fill=False, pad=3, threshold=2)
        want = vn.voxelize(None, x, y, z, 32, **kw)
        yield dict(fn=lambda a, b, c: F("voxelize")(None, a, b, c, 32, **kw), inputs=[x, y, z], ctx=(np.dtype(dtype).name, kw),
                   reference=lambda got, w=want: (got.dtype == bool and got.shape == w.shape and np.array_equal(got, w)) or
                   pytest.fail("voxelize %r" % (kw,)))


@cases("pssm")
def pssm(_):
    from oracle import smrf_oracle as orc
    from test_pssm import G
    Z = T.raster(T.PSSM_SHAPES[-1], F64)
    yield dict(fn=lambda Zt: F("pssm")(Zt, 1.5, 2.3, False, False), inputs=[Z], ctx="classes",
               reference=lambda got: (got.dtype == np.uint8 and np.array_equal(got, orc.pssm_classes(Z, 1.5, 2.3))) or
               pytest.fail("pssm classes"))
    yield dict(fn=lambda Zt: F("pssm")(Zt, 1.5, 2.3, True), inputs=[Z], ctx="rgba",
               reference=lambda got: (got.shape == Z.shape + (4,) and np.array_equal(got, orc.pssm(Z, G["lut_bone"], 1.5, 2.3)))
               or pytest.fail("pssm rgba"))


@cases("smrf")
def smrf(_):
    yield T.smrf_case()[0]


# run outside GUARDED's names: (case builder, run_streamed options)
EXTRA = {
    "smrf_spline": (lambda: T.spline_case((9, 300)), {}),
    # the band driver posts its exchanges on a stream of its own making: those handles are its own business, the
    # wait_event / wait_stream wiring to the caller's stream is what the data check sees
    "sharded": (lambda: T.sharded_case(), dict(own_streams=True)),
}


def _run(case, **opts):
    return streamed(case["fn"], case["inputs"], name=case.get("name", "?"), ctx=case["ctx"], reference=case["reference"], **opts)


@pytest.mark.parametrize("name", GUARDED)
def test_family(gpu_device, name):
    n = 0
    for case in CASES[name]():
        _run(dict(case, name=name))
        n += 1
    assert n >= 1, name


@pytest.mark.parametrize("name", sorted(EXTRA))
def test_extra(gpu_device, name):
    build, opts = EXTRA[name]
    _run(build(), **opts)


# ------------------------------------------------------------------------------------------
# NumPy in, NumPy out
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPE, (1025, 1030)], ids=["67x131", "staged"])
def test_numpy_in_numpy_out(gpu_device, shape):
    """slope on host arrays with a side stream current: the second raster is just above _xfer.SMALL, so it travels through
    the pinned staging buffers both ways and their events are recorded on the side stream"""
    from neilpy_amd import _xfer
    from test_gpu_surface import compare
    Z = T.raster(shape, F32, nan=(shape == SHAPE), seed=7)
    assert (Z.nbytes >= _xfer.SMALL) == (shape != SHAPE) and Z.nbytes < _xfer.SMALL + (64 << 10)
    kw = T.golden_kw("surface.npz", "slope")

    def ref(got):
        assert isinstance(got, np.ndarray)
        compare("slope", Z, kw, got, sn.run("slope", Z, kw))
    streamed(lambda Zh: F("slope")(Zh, **sn.decode_kw(kw)), [Host(Z)], name="slope", ctx=("numpy", shape), reference=ref)


# ------------------------------------------------------------------------------------------
# two streams in one thread
# ------------------------------------------------------------------------------------------
def test_two_streams_share_an_input_and_the_cached_tables(gpu_device):
    """evans_curvature on stream A, then scaled_morphometry(lookup_pixels=1) on stream B on the same tensor; B waits only
    for an event recorded when the input was written.  Both equal their serial results bit for bit: the device tables and
    launch caches made under one stream serve the other."""
    import torch
    import neilpy_amd as na
    from guarded import same_bits
    Z, _ = nan_raster(F64)
    kw_e = T.golden_kw("surface.npz", "evans_curvature")
    kw_m = dict(T.golden_kw("morphometry.npz", "scaled_morphometry"), lookup_pixels=1)
    Zd = torch.from_numpy(Z).to(S.DEVICE)
    torch.cuda.synchronize()
    want_e = T._rebuild(na.evans_curvature(Zd, **sn.decode_kw(kw_e)), T._np)
    want_m = T._rebuild(na.scaled_morphometry(Zd, **kw_m), T._np)
    torch.cuda.synchronize()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    sleep = S.delay()
    buf = torch.from_numpy(S.decoy_of(Z)).to(S.DEVICE)
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        sleep()
        buf.copy_(Zd, non_blocking=True)
        written = torch.cuda.Event()
        written.record()
        got_e = na.evans_curvature(buf, **sn.decode_kw(kw_e))
    with torch.cuda.stream(B):
        B.wait_event(written)
        got_m = na.scaled_morphometry(buf, **kw_m)
    with torch.cuda.stream(A):
        got_e = T._rebuild(got_e, T._np)
    with torch.cuda.stream(B):
        got_m = T._rebuild(got_m, T._np)
    torch.cuda.synchronize()
    for tag, got, want in (("evans_curvature", got_e, want_e), ("scaled_morphometry", got_m, want_m)):
        a, b = list(T._leaves(got)), list(T._leaves(want))
        assert [p for p, _ in a] == [p for p, _ in b], tag
        for (path, u), (_, v) in zip(a, b):
            assert same_bits(u, v), (tag, path)


def test_report(gpu_device):
    """the figures the module docstring and the README quote"""
    print("streams: D = %g ms = %d cycles, side stream candidate %s of %d, %d redirected allocations" % (
        S.D_MS, int(S.D_MS * S.cycles_per_ms()), S.SIDE_INDEX, S.CANDIDATES, STATS.get("allocations", 0)))
