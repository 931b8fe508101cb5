"""Every kernel family on offset, strided and host-order views of its inputs (tests/viewed.py; its own proof is
tests/test_viewed_host.py).

Per name of tests/family_cases.py's GUARDED and EXTRA, the cases that name's builder marks ``stream=True`` (and one more
of topographic_position_index, see ALSO) - the very
dicts ``run_guarded`` gets, one shape per function and dtype: (67, 131) with 2 % NaN for the rasters, (70, 300) with one
window list per route for progressive_filter, samp21 for create_dem and smrf - go through ``run_viewed``: the plain call on
contiguous tensors, checked against the family's restatement or oracle, then the same call with every array input as a
view inside a poisoned buffer of its own, in up to six layouts and under both poisons.  Every result is the plain call's
bit for bit, no byte around a view changes, the inputs keep their bits (the in-place fills arrive in the caller's view)
and no result lives in a caller's buffer.  No case is built here and there is no tolerance; this module varies where and
how the caller's arrays lie in memory, nothing else.

``offset`` hands every entry point a data pointer that is aligned to its element and to nothing wider, which is the
contract DESIGN.md section 1 and include/smrf_hip.h state; ``smrf_voxel_expand``, the one entry point that asks for more
(of ``d_out``), refuses such a pointer with SMRF_E_ARG (test_an_entry_point_that_needs_more_refuses).

Measured on an MI355X (the module prints these figures): 113 cases, 1310 calls under a layout (every layout under both
poisons, after the plain call: 12 for a raster or (n, d) cloud case, 10 for one that fills its argument, 8 for the vector
clouds of create_dem, voxelize and smrf), 2.9 s from the first case to the last (tests/test_gpu_streams.py: 4.6 s).  The layouts
found one wrong read: the band driver counted a strided band's NaNs through its data pointer
(test_a_strided_band_counts_its_own_nans).
Mutants, run once on a scratch copy, each layout of each case judged on its own:
* ``_raster._to_device`` returning ``t`` without ``.contiguous()``, for the 32 names whose planes hold values only (surface,
  focal, terrain, morphometry, relief, disk filters, progressive_filter; 79 cases): ``strided`` failed on Identity in 75 and
  ``transposed`` in 73, ``offset`` and ``reversed`` passed in all 79.  The runs that passed are the ones whose result does
  not depend on where a cell lies: the standardised topographic_position_index of the NaN raster (2 cases; NaN throughout,
  which is why ALSO adds the unstandardised case - that one failed), progressive_filter with the window list (0,) (2; the
  copy route's mask is empty whatever the raster) and, under ``transposed`` only, raster_stats and rmse of the float32
  raster (the same cells in another order, and the float64 sums of float32 cells came out the same).  With the layouts of
  tests/viewed.py the mutant's reads stay inside the harness's buffers; the other families were not run under it, since an
  index plane read from the wrong cells can become an address.
* ``api._inpaint`` without its ``A.copy_(work)``: inpaint_nans_by_springs and inpaint_nans_by_fda failed on Inputs ("the
  fill did not arrive in the view") under ``strided`` and ``transposed`` and passed under ``offset`` (filled where it lies)
  and ``reversed`` (the NumPy path).
* ``sharded.progressive_filter_sharded`` asking ``has_nan(Z_band)`` again: test_a_strided_band_counts_its_own_nans failed on
  Identity under ``strided`` with poison 0x5A, 2 of 26 200 mask bytes.
"""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import family_cases as FC
from conftest import ROOT
from family_cases import F32, GUARDED
from viewed import DEVICE_LAYOUTS, HOST_LAYOUTS, LAYOUTS, run_viewed

pytestmark = pytest.mark.gpu

STATS = {}                       # cases, calls under a layout and the first case's start (printed by the last test)

# name -> {layout that is not run: why}
VIEW_LEFT_OUT = {
    "read_las_xyz": {lay: "takes a file name: there is no array input to lay out" for lay in LAYOUTS},
    "smrf_spline": {lay: "the case calls smrf_spline_solve_ws_f64 / smrf_spline_eval_f64 through ctypes with data_ptr(): "
                         "the C ABI takes contiguous device planes" for lay in LAYOUTS if lay != "offset"},
    "sharded": {lay: "tests/sharded_one_gpu.py plays the neighbours with tensor ops on the raster: it takes a device "
                     "tensor (the band driver itself copies any view of a band, so the device layouts run)"
                for lay in HOST_LAYOUTS},
}
# what the table may hold at the most
MAY_LEAVE_OUT = {"read_las_xyz": set(LAYOUTS), "smrf_spline": set(LAYOUTS) - {"offset"}, "sharded": set(LAYOUTS) - {"offset"}}


# The stream-marked case of topographic_position_index standardises the NaN raster: its sd is NaN and so is every cell
# of the result, which any layout reproduces.  The table's unstandardised case on the same raster (radius 4, impl AUTO) is
# run as well: name -> which further cases of that name's sweep
ALSO = {"topographic_position_index": lambda case: "nan" in case["ctx"][0] and case["ctx"][1:] == (
    dict(radius=4, standardize=False), FC.AUTO)}


def marked(name, builder):
    """the cases of ``name`` this module runs: the ones ``builder`` marks ``stream=True``, and those ALSO selects"""
    for case in builder((name,)):
        if case["stream"] or ALSO.get(name, lambda case: False)(case):
            yield case


def tells(plain):
    """whether a result can differ between layouts at all: some leaf that is not NaN throughout"""
    return any(v is not None and not (np.asarray(v).dtype.kind == "f" and np.isnan(v).all()) for _, v in FC.leaves(plain))


def run_marked(name, builder):
    """every case of ``marked``, and at least one, in every layout that is not left out"""
    layouts = [lay for lay in LAYOUTS if lay not in VIEW_LEFT_OUT.get(name, {})]
    n = telling = 0
    STATS.setdefault("t0", time.perf_counter())
    for case in marked(name, builder):
        before = STATS.get("runs", 0)
        plain, ran = run_viewed(**case, layouts=layouts, stats=STATS)
        n += 1
        telling += tells(plain)
        STATS["cases"] = STATS.get("cases", 0) + 1
        arrays = [a for a in case["inputs"] if isinstance(a, np.ndarray)]
        fills = case.get("known") is not None
        need = {"offset", "strided"} if arrays else set()
        if any(a.ndim == 2 for a in arrays):
            need = set(LAYOUTS) - ({"readonly"} if fills else set())
        need -= set(VIEW_LEFT_OUT.get(name, {}))
        assert need <= set(ran), (name, case["ctx"], sorted(need - set(ran)))
        assert STATS.get("runs", 0) - before == 2 * len(ran)
    assert n >= 1 and telling >= 1, (name, n, telling)


@pytest.mark.parametrize("name", GUARDED)
def test_family(gpu_device, name):
    run_marked(name, FC.BUILDERS[name])


@pytest.mark.parametrize("name", sorted(FC.EXTRA))
def test_extra(gpu_device, name):
    run_marked(name, FC.EXTRA[name])


def test_the_table_of_layouts_left_out_cannot_grow_quietly():
    assert set(VIEW_LEFT_OUT) <= set(MAY_LEAVE_OUT) == {"read_las_xyz", "smrf_spline", "sharded"}
    assert set(VIEW_LEFT_OUT) <= set(GUARDED) | set(FC.EXTRA)
    for name, table in VIEW_LEFT_OUT.items():
        assert set(table) <= MAY_LEAVE_OUT[name], (name, sorted(set(table) - MAY_LEAVE_OUT[name]))
        assert all(isinstance(r, str) and r for r in table.values()), name


# ------------------------------------------------------------------------------------------
# what the layouts found, pinned
# ------------------------------------------------------------------------------------------
def test_a_strided_band_counts_its_own_nans(gpu_device):
    """the band driver asks ``smrf_count_nan_*`` whether its band holds a NaN and picks the kernels' NaN rule by the answer.
    It used to pass the caller's band by its data pointer and cell count: of a strided band that reads the cells around the
    view and misses the band's last rows.  Here both bands' only NaNs lie in their last row (tests/family_cases.py's sharded
    case otherwise); with finite surroundings (poison 0x5A) the old count was 0 and the masks were not the plain call's."""
    import neilpy_amd as na
    from neilpy_amd import sharded as bands
    from oracle import smrf_oracle as orc
    from sharded_one_gpu import run_bands
    world, shape, win = 2, (200, 131), np.asarray([2, 6, 1])
    Z = na.synth_dem(shape[1], seed=9, rows=shape[0]).astype(F32)
    for k in range(world):
        Z[bands.band_rows(shape[0], world, k)[1] - 1, 5:40] = np.nan

    def call(Zt):
        mask, when, _ = run_bands(na, Zt, win, world, return_when_dropped=True, budget=None, ops=bands.HipBandOps,
                                  overlap=lambda k: k % 2 == 0)
        return mask, when

    def ref(got):
        want_m, want_w = orc.progressive_filter(Z, win, 1, .15, return_when_dropped=True)
        assert np.array_equal(got[0], want_m) and np.array_equal(got[1], want_w), "sharded, NaN in the bands' last rows"
    _, ran = run_viewed(call, [Z], name="sharded", ctx="nan", reference=ref, layouts=DEVICE_LAYOUTS, stats=STATS)
    assert ran == list(DEVICE_LAYOUTS)


def test_an_entry_point_that_needs_more_refuses(gpu_device):
    """every caller's data pointer needs its element's alignment only; smrf_voxel_expand writes ``d_out`` in dwords and
    says so: SMRF_E_ARG for a bool plane one byte into a buffer, before anything is launched"""
    import torch
    from neilpy_amd import _lib
    L = FC.lib()
    e_arg = int(re.search(r"#define SMRF_E_ARG \((-\d+)\)", open(os.path.join(ROOT, "include", "smrf_hip.h")).read()).group(1))
    nx, ny, nz = 3, 5, 7
    nbytes = int(L.smrf_voxel_workspace_bytes(nx, ny, nz, 1))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=FC.DEVICE)
    buf = torch.full((nx * ny * nz + 8,), 0x5A, dtype=torch.uint8, device=FC.DEVICE)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in (1, 2, 3):
        out = buf[k:k + nx * ny * nz]
        assert out.data_ptr() % 4 == k
        rc = L.smrf_voxel_expand(C.c_void_p(ws.data_ptr()), nbytes, nx, ny, nz, 1, 1, 0, C.c_void_p(out.data_ptr()), st)
        assert rc == e_arg, (k, rc)
        with pytest.raises(_lib.SmrfHipError, match="4-byte aligned"):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())                         # refused: nothing was written
    _lib.check(L.smrf_voxel_expand(C.c_void_p(ws.data_ptr()), nbytes, nx, ny, nz, 1, 1, 0, C.c_void_p(buf[4:].data_ptr()), st))
    torch.cuda.synchronize()
    n = nx * ny * nz
    assert bool((buf[4:4 + n] == 0).all()) and bool((buf[:4] == 0x5A).all()) and bool((buf[4 + n:] == 0x5A).all())


def test_report(gpu_device):
    """the figures the module docstring and the README quote"""
    print("views: %d cases, %d calls under a layout (every layout under two poisons), %.1f s since the first case began" % (
        STATS.get("cases", 0), STATS.get("runs", 0), time.perf_counter() - STATS.get("t0", time.perf_counter())))
