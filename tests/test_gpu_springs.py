"""inpaint_nans_by_springs on the device (csrc/springs.hip) against the NumPy oracle (oracle.lsqr_springs) at the
smallest rasters on which a workgroup of the plane kernels walks MORE than one row, under -m gpu.

lsqr_grid2d launches ceil(cols / 256) column tiles by min(rows, 2048 / tiles) row phases; only with more rows than
phases does a workgroup stride r += gridDim.y, and that stride carries state in atu_kernel, atuxw_kernel and av2_kernel:
the hole bytes of the next row of the walk are fetched a step ahead and handed on, and rv decides which rows have a
vertical spring below them.  The cases below reach a second and a third step, a last tile one column wide, 97 tiles and
the 512-cell plane pitch of 24576 columns and more.  Three kinds of test:

* the natural stop: (istop, itn) and the filled cells against the oracle;
* a solve cut after exactly K iterations, odd and even, on and off the host's polls (after 4 and after 12 iterations),
  with the workspace filled with 0xFF bytes first: x is written every second iteration and the scatter owes the pending
  step at an odd stop (lsqr_core.h, lsqr_x_pending);
* degenerate systems.

Every bar comes from the oracle alone: `moved` is how far the oracle's own answer moves when the same system is solved
with every sum taken in another order (the raster flipped in both axes and the result flipped back).
"""
import ctypes as C

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


def make_raster(m, n, s, f):
    nan = np.nan
    rng = np.random.default_rng(s)
    A = rng.normal(0, 1, (m, n)).cumsum(0).cumsum(1) * 0.01 + 100
    A[rng.random((m, n)) < f] = nan
    A[m // 3: m // 3 + min(12, m // 2), n // 2: n // 2 + min(40, n // 2)] = nan   # a block hole
    A[0, 0] = A[0, -1] = A[-1, 0] = A[-1, -1] = nan                                # the four corners
    A[-1, :n // 2] = nan
    A[:m // 2, -1] = nan
    A[(2 * m) // 3, :] = nan                                                       # a whole row
    A[:, n // 4] = nan                                                             # a whole column
    return A


_RASTERS = {}
_RUNS = {}


def raster(shape, seed, share):
    key = (shape, seed, share)
    if key not in _RASTERS:
        A = make_raster(shape[0], shape[1], seed, share)
        A.setflags(write=False)
        _RASTERS[key] = A
    return _RASTERS[key]


def oracle_run(orc, A, key, K=None, flipped=False):
    """(filled raster, istop, itn) of the oracle, computed once per (raster, K, orientation) and left unchanged;
    K = None is the natural stop, any other K a solve cut after exactly K iterations (all tolerances 0)."""
    k = (key, K, flipped)
    if k not in _RUNS:
        src = np.ascontiguousarray(A[::-1, ::-1]) if flipped else A
        B, istop, itn = orc.lsqr_springs(src) if K is None else orc.lsqr_springs(src, 0, 0, 0, K)
        if flipped:
            B = np.ascontiguousarray(B[::-1, ::-1])
        B.setflags(write=False)
        _RUNS[k] = B, int(istop), int(itn)
    return _RUNS[k]


def device_solve(nz, gpu_device, A, atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=-1):
    """smrf_springs_lsqr_f64 on a copy of A with a workspace of 0xFF bytes: the set-up leaves w, x off the holes and the
    pad cells of every plane unwritten, so a kernel that reads one of them shows a NaN and not a leftover."""
    import torch
    from neilpy_amd import _lib
    lib = _lib.load()
    m, n = A.shape
    A_d = torch.from_numpy(np.array(A, dtype=np.float64, order="C")).to(gpu_device)
    nbytes = lib.smrf_springs_workspace_bytes(m, n)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=gpu_device)
    istop, itn, nunk = C.c_int(-1), C.c_int64(-1), C.c_int64(-1)
    _lib.check(lib.smrf_springs_lsqr_f64(C.c_void_p(A_d.data_ptr()), m, n, atol, btol, conlim, iter_lim, C.byref(istop),
                                         C.byref(itn), C.byref(nunk), C.c_void_p(ws.data_ptr()), nbytes,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return A_d.cpu().numpy(), istop.value, itn.value, nunk.value


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# shape, seed, share: what the walk reaches
WALKS = [((2100, 40), 100, .3),      # one column tile, 2048 row phases, 52 rows take a second step
         ((300, 2049), 101, .1),     # 9 tiles, the last one column wide, 227 phases, two steps, pitch 2080
         ((700, 777), 102, .5),      # 4 tiles, 512 phases, 188 rows in the second step
         ((45, 24577), 103, .2),     # 97 tiles, 21 phases, three steps (21, 21, 3), the 512-cell pitch
         ((2051, 257), 104, .1)]     # 2 tiles, 1024 phases, three steps, second tile one column wide


@pytest.mark.parametrize("shape,seed,share", WALKS)
def test_strided_walk_natural_stop_vs_oracle(nz, orc, gpu_device, shape, seed, share):
    """The bar on the filled cells is 1000 x `moved`, the factor covering the device's fixed reduction trees, and never
    above the project's 1e-7; the flipped oracle run must stop where the plain one does, or `moved` would compare two
    different iterates."""
    key = (shape, seed, share)
    A = raster(*key)
    want, istop, itn = oracle_run(orc, A, key)
    flip, istop_f, itn_f = oracle_run(orc, A, key, flipped=True)
    assert (istop_f, itn_f) == (istop, itn)
    hole = np.isnan(A)
    moved = float(np.abs(flip - want)[hole].max())
    bar = min(1e-7, 1000.0 * moved)
    got, g_istop, g_itn, g_nunk = device_solve(nz, gpu_device, A)
    diff = float(np.abs(got - want)[hole].max())
    print("springs %s: stop (%d, %d), device (%d, %d); moved %.3g, device vs oracle %.3g, bar %.3g"
          % (shape, istop, itn, g_istop, g_itn, moved, diff, bar))
    assert (g_istop, g_itn, g_nunk) == (istop, itn, int(hole.sum()))
    assert same_bits(got[~hole], A[~hole])                       # known cells untouched
    assert not np.isnan(got).any()
    assert diff <= bar


FIXED = [((37, 53), 1, .5), ((2100, 40), 100, .3), ((300, 2049), 101, .1)]


@pytest.mark.parametrize("K", (1, 2, 3, 4, 5, 12, 13))
@pytest.mark.parametrize("shape,seed,share", FIXED)
def test_pending_x_at_fixed_iteration(nz, orc, gpu_device, shape, seed, share, K):
    """The springs' form of test_fda.test_hip_pending_x_at_fixed_iteration.  Relative to max |x| over the holes the bar
    is max(1e-13, 100 x moved_K); the oracle's last step (K against K - 1) is at least 1000 x the bar, so a dropped or
    doubled pending step cannot pass."""
    key = (shape, seed, share)
    A = raster(*key)
    hole = np.isnan(A)
    want, istop, itn = oracle_run(orc, A, key, K)
    assert (istop, itn) == (7, K)
    xmax = float(np.abs(want[hole]).max())
    moved = float(np.abs(oracle_run(orc, A, key, K, flipped=True)[0] - want)[hole].max()) / xmax
    tol = max(1e-13, 100.0 * moved)
    step = float(np.abs(want - oracle_run(orc, A, key, K - 1)[0])[hole].max()) / xmax
    assert step >= 1000.0 * tol
    got, g_istop, g_itn, g_nunk = device_solve(nz, gpu_device, A, 0.0, 0.0, 0.0, K)
    diff = float(np.abs(got - want)[hole].max()) / xmax              # a NaN from the 0xFF workspace fails the bar below
    print("springs fixed K=%d %s: moved %.3g, device vs oracle %.3g, bar %.3g, oracle's last step %.3g"
          % (K, shape, moved, diff, tol, step))
    assert (g_istop, g_itn, g_nunk) == (7, K, int(hole.sum()))
    assert same_bits(got[~hole], A[~hole])
    assert diff <= tol


def _known(shape, seed):
    return np.random.default_rng(seed).normal(100.0, 5.0, shape)


def _degenerate():
    cases = {}
    cases["all_nan_3x300"] = np.full((3, 300), np.nan)
    cases["all_nan_300x3"] = np.full((300, 3), np.nan)
    cases["no_nan_70x300"] = _known((70, 300), 1)
    A = np.full((300, 3), np.nan)
    A[117, 1] = 42.5
    cases["one_known_300x3"] = A
    for shape in ((2, 2), (1, 257), (257, 1)):
        corners = sorted({(r, c) for r in (0, shape[0] - 1) for c in (0, shape[1] - 1)})
        for r, c in corners:
            A = _known(shape, 10 + shape[1])
            A[r, c] = np.nan
            cases["corner_%dx%d_at_%d_%d" % (shape + (r, c))] = A
    return cases


DEGENERATE = _degenerate()


@pytest.mark.parametrize("tag", sorted(DEGENERATE))
def test_degenerate_systems_vs_oracle(nz, orc, gpu_device, tag):
    """b = 0 (no iteration, zeros written), nothing to solve (untouched, itn 0), one known cell, and one unknown in each
    corner of the smallest rasters.  Same stop as the oracle; filled cells within 1000 x `moved` as above, with the
    fixed-iteration tests' floor of 1e-13 relative to the largest known value where the flipped system moves nothing
    (one unknown: every sum has one or two terms), and never above 1e-7."""
    A = DEGENERATE[tag]
    hole = np.isnan(A)
    want, istop, itn = orc.lsqr_springs(A)
    flip, istop_f, itn_f = orc.lsqr_springs(np.ascontiguousarray(A[::-1, ::-1]))
    assert (istop_f, itn_f) == (istop, itn)
    got, g_istop, g_itn, g_nunk = device_solve(nz, gpu_device, A)
    assert (g_istop, g_itn, g_nunk) == (istop, itn, int(hole.sum()))
    assert same_bits(got[~hole], A[~hole])
    if not hole.any():
        return
    if hole.all():
        assert itn == 0 and np.array_equal(want, np.zeros(A.shape))
        assert same_bits(got, want)                              # +0.0 in every cell
        return
    moved = float(np.abs(flip[::-1, ::-1] - want)[hole].max())
    bar = min(1e-7, max(1000.0 * moved, 1e-13 * float(np.abs(A[~hole]).max())))
    diff = float(np.abs(got - want)[hole].max())
    print("springs %s: stop (%d, %d); moved %.3g, device vs oracle %.3g, bar %.3g" % (tag, istop, itn, moved, diff, bar))
    assert diff <= bar
