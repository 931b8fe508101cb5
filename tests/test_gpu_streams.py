"""Every kernel family on a side stream (tests/streamed.py: decoy inputs, a delay ahead of every poison fill, the stream
handle of every library call recorded).

First the harness proves itself with stand-ins, torch ops on the harness's own memory: a correct one passes; one that
computes under the default stream reads the decoy; one whose last copy runs on the default stream ends up as poison; one
whose library call carries stream 0 fails the handle check - each in 10 of 10 repetitions at the delay D and at D / 4.

Then, per name of tests/family_cases.py's GUARDED, the cases that name's builder marks ``stream=True``: cases of the
guarded module's own sweep, the very dicts ``run_guarded`` gets, at a single shape each (and per dtype where the function
takes both) - (67, 131) with 2 % NaN for the rasters, (70, 300) with one window list per route of ``smrf_pf_plan`` for
progressive_filter - plus the table's two extras (the spline pair and the one-GPU band driver), two NumPy-in NumPy-out calls
of slope (the second through the pinned staging buffers) and two streams in one thread that share an input and the
library's cached device tables.  No case is built here; shapes are the guarded module's job, this one varies the stream only.

Measured on an MI355X (the module prints these figures; D is a sensitivity setting, no tolerance - correct code passes at
any D):
    torch.cuda._sleep runs 2.39 M cycles per millisecond.  On each of four fresh streams, 10 repetitions per delay:
    stand-ins (a) and (b) were caught 10 of 10 from 4 ms down to 0.0625 ms, (a) 9 of 10 on one stream at 0.03125 ms, none at
    0.015625 ms; (c) and the correct stand-in were judged right at every delay.  The detection threshold is 0.0625 ms,
    which makes 0.25 ms the smallest D that is caught at D and at D / 4.  D is set to 1 ms = 2 401 742 cycles, four times
    that: test_standins repeats the proof at D / 4 in every run, and at D = 1 ms that repetition runs at 0.25 ms, fourfold
    above the threshold instead of on it (what sets the threshold is how fast the host enqueues, which a busier machine
    does more slowly).  Side stream: candidate 0 of 4 (all four qualified).  439 redirected allocations per module run,
    each behind one delay; the module takes 4.6 s (tests/test_gpu_threads.py: 5.1 s).
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

import family_cases as FC
import streamed as S
import surface_numpy as sn
from family_cases import F, F32, F64, GUARDED, NAN_SHAPE as SHAPE
from streamed import EXPECTED, Host, run_streamed, standin_verdict

pytestmark = pytest.mark.gpu

STATS = {}                       # allocations served over the module's run (printed by the last test)


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
# the stream-marked cases of tests/family_cases.py's table
# ------------------------------------------------------------------------------------------
# the band driver posts its exchanges on a stream of its own making: those handles are its own business, the
# wait_event / wait_stream wiring to the caller's stream is what the data check sees
OPTIONS = {"sharded": dict(own_streams=True)}


def run_marked(name, builder):
    """every ``stream=True`` case ``builder`` yields for ``name``, and at least one"""
    n = 0
    for case in builder((name,)):
        if case["stream"]:
            streamed(case["fn"], case["inputs"], name=name, ctx=case["ctx"], reference=case["reference"], **OPTIONS.get(name, {}))
            n += 1
    assert n >= 1, name


@pytest.mark.parametrize("name", GUARDED)
def test_family(gpu_device, name):
    run_marked(name, FC.BUILDERS[name])


@pytest.mark.parametrize("name", sorted(FC.EXTRA))
def test_extra(gpu_device, name):
    run_marked(name, FC.EXTRA[name])


# ------------------------------------------------------------------------------------------
# NumPy in, NumPy out
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPE, (1025, 1030)], ids=["67x131", "staged"])
def test_numpy_in_numpy_out(gpu_device, shape):
    """slope on host arrays with a side stream current: the second raster is just above _xfer.SMALL, so it travels through
    the pinned staging buffers both ways and their events are recorded on the side stream"""
    from neilpy_amd import _xfer
    from test_gpu_surface import compare
    Z = FC.raster(shape, F32, nan=(shape == SHAPE), seed=7)
    assert (Z.nbytes >= _xfer.SMALL) == (shape != SHAPE) and Z.nbytes < _xfer.SMALL + (64 << 10)
    kw = FC.golden_kw("surface.npz", "slope")

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
    Z = FC.raster(SHAPE, F64, nan=True, seed=7)
    kw_e = FC.golden_kw("surface.npz", "evans_curvature")
    kw_m = dict(FC.golden_kw("morphometry.npz", "scaled_morphometry"), lookup_pixels=1)
    Zd = torch.from_numpy(Z).to(S.DEVICE)
    torch.cuda.synchronize()
    want_e = FC.rebuild(na.evans_curvature(Zd, **sn.decode_kw(kw_e)), FC.to_numpy)
    want_m = FC.rebuild(na.scaled_morphometry(Zd, **kw_m), FC.to_numpy)
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
        got_e = FC.rebuild(got_e, FC.to_numpy)
    with torch.cuda.stream(B):
        got_m = FC.rebuild(got_m, FC.to_numpy)
    torch.cuda.synchronize()
    for tag, got, want in (("evans_curvature", got_e, want_e), ("scaled_morphometry", got_m, want_m)):
        a, b = list(FC.leaves(got)), list(FC.leaves(want))
        assert [p for p, _ in a] == [p for p, _ in b], tag
        for (path, u), (_, v) in zip(a, b):
            assert same_bits(u, v), (tag, path)


def test_report(gpu_device):
    """the figures the module docstring and the README quote"""
    print("streams: D = %g ms = %d cycles, side stream candidate %s of %d, %d redirected allocations" % (
        S.D_MS, int(S.D_MS * S.cycles_per_ms()), S.SIDE_INDEX, S.CANDIDATES, STATS.get("allocations", 0)))
