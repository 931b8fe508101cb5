"""Grey morphology with flat footprints, everything that needs no GPU: the NumPy restatement (tests/footprint_numpy.py)
against scipy.ndimage, the host plan of neilpy_amd.morphology, the public interface's argument rules, the host helpers
and the C ABI's new exports."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import footprint_numpy as fpn
from conftest import ROOT

NAMES = tuple(fpn.FUNCTIONS)
MODES = ("reflect", "nearest")


def same(got, want, ctx):
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=True), ctx


def random_footprint(rng, shape, hole=False):
    fp = rng.random(shape) < 0.6
    if not fp.any():
        fp[rng.integers(shape[0]), rng.integers(shape[1])] = True
    if hole:                                        # a NaN raster is compared with SciPy through its footprint filter only
        if fp.all() and fp.size == 1:
            return None
        if fp.all():
            fp[rng.integers(shape[0]), rng.integers(shape[1])] = False
    return fp


# ------------------------------------------------------------------------------------------
# the restatement against SciPy
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_equals_scipy(dtype):
    rng = np.random.default_rng(20261101)
    n = 0
    for case in range(260):
        rows, cols = (int(v) for v in rng.integers(1, 10, size=2))
        kind = case % 5
        kshape = ((int(rng.integers(1, 6)), int(rng.integers(1, 6))), (1, int(rng.integers(1, 8))),
                  (int(rng.integers(1, 8)), 1), (2 * int(rng.integers(1, 4)), 2 * int(rng.integers(1, 4))),
                  (rows + int(rng.integers(1, 6)), cols + int(rng.integers(1, 6))))[kind]
        nan = case % 3 == 0
        fp = random_footprint(rng, kshape, hole=nan)
        if fp is None or not fpn.scipy_comparable(fp, (rows, cols)):
            continue
        X = np.round(rng.normal(size=(rows, cols)) * 8).astype(dtype)
        X[X == 0] = 0.0                                                  # one sign of zero
        if nan:
            X[rng.random(X.shape) < 0.3] = np.nan
        if case % 7 == 0:
            X[rng.random(X.shape) < 0.2] = np.inf
            X[rng.random(X.shape) < 0.1] = -np.inf
        for mode in MODES:
            for name in NAMES:
                with np.errstate(invalid="ignore"):
                    want = getattr(ndi, name)(X, footprint=fp, mode=mode)
                same(fpn.FUNCTIONS[name](X, fp, mode), want, (name, mode, X.shape, fp.astype(int).tolist(), nan))
                n += 1
    assert n > 2000


def test_all_ones_footprints_on_nan_free_rasters_and_size():
    """SciPy sends an all-ones footprint (and size=) through its separable filters: the same values without NaN"""
    rng = np.random.default_rng(20261102)
    for kshape in ((1, 1), (3, 3), (2, 5), (4, 4), (1, 6), (7, 2)):
        X = rng.normal(size=(int(rng.integers(1, 10)), int(rng.integers(1, 10))))
        for mode in MODES:
            for name in NAMES:
                same(fpn.FUNCTIONS[name](X, np.ones(kshape), mode), getattr(ndi, name)(X, size=kshape, mode=mode),
                     (name, mode, kshape))


def test_all_ones_nan_deviation_exists():
    """DESIGN.md section 19, deviations: for an all-ones footprint SciPy's separable filters follow their line buffer,
    not the first-visited rule that this package applies to every footprint.  One pinned case: the first visited member
    of the last cell of a 1 x 3 dilation is its left neighbour, a NaN, so the rule gives NaN; SciPy gives the
    maximum of the finite samples."""
    X = np.array([[-3.0, np.nan, -1.0]])
    ones = np.ones((1, 3))
    mine = fpn.grey_dilation(X, ones)
    scipy_ones = ndi.grey_dilation(X, footprint=ones)
    assert np.array_equal(mine, [[-3.0, -1.0, np.nan]], equal_nan=True)
    assert np.array_equal(scipy_ones, [[-3.0, -1.0, -1.0]])
    # the same members with zeros around them go through SciPy's footprint filter and follow the rule
    holed = np.zeros((1, 5), dtype=int)
    holed[0, 1:4] = 1                                                     # offsets -1, 0, 1 as the 1 x 3 ones
    same(fpn.grey_dilation(X, holed), ndi.grey_dilation(X, footprint=holed), "holed")
    same(fpn.grey_dilation(X, holed), mine, "the rule does not depend on the zeros around the members")


def test_restatement_beyond_scipys_reach():
    """a footprint whose half-extent is 2 * min(rows, cols) or more: the restatement against the periodic definition
    written once more with Python loops"""
    rng = np.random.default_rng(20261103)
    X = rng.normal(size=(3, 2))
    fp = rng.random((9, 14)) < 0.5
    assert not fpn.scipy_comparable(fp, X.shape)
    for mode in MODES:
        E = np.empty_like(X)
        D = np.empty_like(X)
        for i in range(3):
            for j in range(2):
                e, d = [], []
                for s in range(9):
                    for t in range(14):
                        if fp[s, t]:
                            e.append(X[fpn.index(i + s - 4, 3, mode), fpn.index(j + t - 7, 2, mode)])
                            d.append(X[fpn.index(i - (s - 4), 3, mode), fpn.index(j - (t - 7), 2, mode)])
                E[i, j], D[i, j] = min(e), max(d)
        same(fpn.grey_erosion(X, fp, mode), E, mode)
        same(fpn.grey_dilation(X, fp, mode), D, mode)


# ------------------------------------------------------------------------------------------
# the host plan
# ------------------------------------------------------------------------------------------
def plan_footprints():
    from neilpy_amd import disk
    from neilpy_amd.morphology import diamond, square
    rng = np.random.default_rng(20261104)
    L = np.zeros((7, 4), dtype=np.uint8)
    L[:, 0] = 1
    L[6, :] = 1
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 0, 0]])
    out = [np.ones((1, 1)), np.ones((1, 2)), np.ones((2, 1)), np.ones((3, 3)), cross, L, np.ones((1, 65)), diamond(5),
           square(31), disk(10), np.ones((4, 6))]
    out += [random_footprint(rng, (int(rng.integers(1, 9)), int(rng.integers(1, 12)))) for _ in range(30)]
    return out


def test_plan_runs_offsets_and_levels():
    from neilpy_amd import morphology as mo
    for fp in plan_footprints():
        fp = np.asarray(fp) != 0
        kh, kw = fp.shape
        for dilate in (False, True):
            P = mo.plan(fp, dilate)
            dr, dc = fpn.members(fp)
            if dilate:
                dr, dc = -dr[::-1], -dc[::-1]
            want = list(zip(dr.tolist(), dc.tolist()))
            assert [tuple(o) for o in P.offsets.tolist()] == want                # the visiting order, first member first
            cells = [(d, c0 + k) for d, c0, L in P.runs for k in range(L)]
            assert sorted(cells) == sorted(want) and len(cells) == len(set(cells))   # the runs' union, each member once
            member = set(want)
            for d, c0, L in P.runs:                                              # maximal: no member on either side
                assert (d, c0 - 1) not in member and (d, c0 + L) not in member
            assert P.levels == tuple(sorted({int(np.floor(np.log2(L))) for _, _, L in P.runs}))
            r_lo, c_lo, bh, bw = P.box
            assert (r_lo, c_lo) == (min(dr), min(dc)) and (bh, bw) == (max(dr) - r_lo + 1, max(dc) - c_lo + 1)
            assert P.tile == (mo.TY + bh - 1, mo.TX + bw - 1) and P.halo == (bh - 1, bw - 1)
            # the slots: a level is never built into its source's plane nor into the plane of a lower level runs read
            assert len(P.slots) == P.levels[-1] + 1 and max(P.slots) + 1 == P.nplanes
            for k in range(1, len(P.slots)):
                assert P.slots[k] != P.slots[k - 1]
            for lv in P.levels:
                assert all(P.slots[k] != P.slots[lv] for k in range(lv + 1, len(P.slots)))
            # the packed arrays
            assert P.head.dtype == np.int32 and P.head.tolist()[:8] == [len(want), len(P.runs), r_lo, c_lo, bh, bw,
                                                                        P.levels[-1], P.nplanes]
            assert P.table.dtype == np.int32 and len(P.table) == 2 * len(want) + 4 * len(P.runs)
            recs = P.table[2 * len(want):].reshape(-1, 4)
            for (d, c0, L), (trow, tcol, tcol2, slot) in zip(P.runs, recs.tolist()):
                k = L.bit_length() - 1
                assert (trow, tcol, tcol2, slot) == (d - r_lo, c0 - c_lo, c0 - c_lo + L - 2 ** k, P.slots[k])
                assert 0 <= trow < bh and 0 <= tcol <= tcol2 and tcol2 + 2 ** k <= bw


def test_plan_known_shapes():
    from neilpy_amd import disk, morphology as mo
    square = mo.square
    P = mo.plan(square(31))
    assert len(P.runs) == 31 and P.levels == (4,) and P.nplanes == 2 and len(P.offsets) == 961
    assert P.lds_bytes == 2 * 38 * 94 * 4 and P.path == "runs"
    P = mo.plan(disk(10), itemsize=4)
    assert len(P.runs) == 21 and P.nplanes == len(P.levels)
    assert mo.plan(np.ones((1, 65))).levels == (6,)
    assert mo.plan(np.ones((3, 3))).path == "runs" and mo.plan(np.ones((2, 4))).path == "taps"     # fewer than 9 members


def test_plan_path_follows_the_cap_and_the_library():
    """past the LDS cap the automatic path is taps and a forced runs launch is refused; the library's own decision
    (smrf_footprint_path, host logic) is the plan's for every footprint, dtype, epilogue and impl"""
    import ctypes as C
    from neilpy_amd import _lib, morphology as mo
    square = mo.square
    lib = _lib.load()
    cap = lib.smrf_footprint_tile_bytes()
    assert cap == mo.TILE_BYTES
    header = open(os.path.join(ROOT, "include", "smrf_hip.h")).read()
    for c_name, value in (("SMRF_FOOTPRINT_RUNS_MIN_TAPS", mo.RUNS_MIN_TAPS), ("SMRF_FOOTPRINT_TILE_BYTES", mo.TILE_BYTES),
                          ("SMRF_FOOTPRINT_IMPL_AUTO", mo.IMPL_AUTO), ("SMRF_FOOTPRINT_IMPL_RUNS", mo.IMPL_RUNS),
                          ("SMRF_FOOTPRINT_IMPL_TAPS", mo.IMPL_TAPS), ("SMRF_FOOTPRINT_REFLECT", mo.REFLECT),
                          ("SMRF_FOOTPRINT_NEAREST", mo.NEAREST), ("SMRF_FOOTPRINT_STORE", mo.STORE),
                          ("SMRF_FOOTPRINT_SUB_MINUS", mo.SUB_MINUS), ("SMRF_FOOTPRINT_MINUS_SUB", mo.MINUS_SUB),
                          ("SMRF_FOOTPRINT_GRADIENT", mo.GRADIENT), ("SMRF_FOCAL_TILE_BYTES", mo.TILE_BYTES)):   # one cap
        assert int(re.search(r"#define %s (\d+)" % c_name, header).group(1)) == value, c_name
    for itemsize in (4, 8):
        w = 1
        while mo.plan(square(w + 1), itemsize=itemsize, cap=cap).lds_bytes <= cap:
            w += 1
        assert w > 8
        assert mo.plan(square(w), itemsize=itemsize, cap=cap).path == "runs"
        assert mo.plan(square(w + 1), itemsize=itemsize, cap=cap).path == "taps"
        assert mo.plan(square(w + 1), itemsize=itemsize, impl=mo.IMPL_RUNS, cap=cap).path == "refused"
        assert mo.plan(square(w), itemsize=itemsize, impl=mo.IMPL_TAPS, cap=cap).path == "taps"
    assert mo.plan(square(9), cap=1000).path == "taps"
    code = {"taps": 0, "runs": 1, "refused": -5}
    fps = plan_footprints() + [square(w) for w in (40, 47, 48, 60, 90)] + [np.ones((3, 400)), np.ones((200, 3))]
    for fp in fps:
        for dilate in (False, True):
            for itemsize in (4, 8):
                for grad in (False, True):
                    for impl in (0, 1, 2):
                        P = mo.plan(fp, dilate, itemsize=itemsize, gradient=grad, impl=impl)
                        got = lib.smrf_footprint_path(P.head.ctypes.data_as(C.c_void_p), itemsize, 3 if grad else 0, impl)
                        assert got == code[P.path], (np.shape(fp), dilate, itemsize, grad, impl, got, P.path)
    bad = mo.plan(square(3)).head.copy()
    bad[7] = 0                                                                  # no plane
    assert lib.smrf_footprint_path(bad.ctypes.data_as(C.c_void_p), 4, 0, 0) == -1


# ------------------------------------------------------------------------------------------
# the interface
# ------------------------------------------------------------------------------------------
def test_signatures_are_scipys_plus_keyword_only():
    import neilpy_amd
    mo = neilpy_amd.morphology                              # the package imports the module
    assert set(NAMES) | {"rectangle", "square", "diamond", "plan"} == set(mo.__all__)
    assert all(getattr(neilpy_amd, n) is getattr(mo, n) for n in mo.__all__ if n != "plan") and not hasattr(neilpy_amd, "plan")
    for name in NAMES:
        positional = lambda f: [(p.name, p.kind, p.default) for p in inspect.signature(f).parameters.values()
                                if p.kind is not inspect.Parameter.KEYWORD_ONLY]
        mine = positional(getattr(mo, name))
        assert mine == positional(getattr(ndi, name)), name
        assert [m[0] for m in mine] == ["input", "size", "footprint", "structure", "output", "mode", "cval", "origin"]
        extra = [p for p in inspect.signature(getattr(mo, name)).parameters.values()
                 if p.kind is inspect.Parameter.KEYWORD_ONLY]
        assert [p.name for p in extra] == ["impl"] and extra[0].default == 0


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_come_from_the_host(name):
    """every refusal is decided before the device is touched: it is the same with and without a GPU"""
    from neilpy_amd import morphology as mo
    f = getattr(mo, name)
    X = np.zeros((4, 5), np.float32)
    with pytest.raises(ValueError):
        f(X)                                                   # neither size nor footprint
    with pytest.raises(ValueError):
        f(X, footprint=np.ones((2, 2, 2)))
    with pytest.raises(ValueError):
        f(X, footprint=np.ones(3))
    with pytest.raises(ValueError):
        f(X, footprint=np.zeros((3, 3)))                       # no member
    with pytest.raises(ValueError):
        f(X, size=0)
    with pytest.raises(ValueError):
        f(X, size=(1, 2, 3))
    with pytest.raises(ValueError):
        f(np.zeros((2, 3, 4)), size=3)                         # not a 2-D raster
    with pytest.raises(ValueError):
        f(np.zeros(5), size=3)
    for mode in ("constant", "mirror", "wrap", "grid-wrap"):
        with pytest.raises(NotImplementedError):
            f(X, size=3, mode=mode)
    with pytest.raises(NotImplementedError):
        f(X, size=3, structure=np.zeros((3, 3)))
    with pytest.raises(NotImplementedError):
        f(X, size=3, output=np.empty_like(X))
    with pytest.raises(NotImplementedError):
        f(X, size=3, origin=1)
    with pytest.raises(NotImplementedError):
        f(X, size=3, origin=(0, -1))
    with pytest.raises(ValueError):
        f(X, size=3, impl=3)


def test_valid_call_without_a_gpu_raises():
    import torch
    import neilpy_amd
    if torch.cuda.is_available():
        return                                                 # tests/test_gpu_footprint.py runs the valid calls
    for name in NAMES:
        with pytest.raises(neilpy_amd.SmrfHipError):
            getattr(neilpy_amd.morphology, name)(np.zeros((4, 5), np.float32), size=(2, 3), cval=7.0, origin=0)
        with pytest.raises(neilpy_amd.SmrfHipError):
            getattr(neilpy_amd.morphology, name)(np.zeros((4, 5)), footprint=[[0, 1, 1]], mode="nearest")


def test_disk_only_functions_still_refuse_other_footprints():
    import neilpy_amd
    for f in (neilpy_amd.erosion, neilpy_amd.dilation, neilpy_amd.opening):
        with pytest.raises(NotImplementedError, match="only skimage disk"):
            f(np.zeros((4, 4), np.float32), neilpy_amd.morphology.square(3))


# ------------------------------------------------------------------------------------------
# helpers, the case table and the ABI
# ------------------------------------------------------------------------------------------
def test_helpers():
    from neilpy_amd import disk
    from neilpy_amd.morphology import diamond, rectangle, square
    r = rectangle(3, 5)
    assert r.dtype == np.uint8 and r.shape == (3, 5) and r.all()
    s = square(4)
    assert s.dtype == np.uint8 and s.shape == (4, 4) and s.all()
    for rad in range(0, 6):
        d = diamond(rad)
        assert d.dtype == np.uint8 and d.shape == (2 * rad + 1, 2 * rad + 1)
        for y in range(-rad, rad + 1):
            for x in range(-rad, rad + 1):
                assert d[y + rad, x + rad] == (abs(y) + abs(x) <= rad)
    assert np.array_equal(diamond(1), disk(1))


def test_the_case_table_holds_inputs_the_references_accept():
    """tests/family_cases.py's morphology cases, walked without a GPU: each case's reference (SciPy where it is the
    oracle) passes on the restatement's result for that raster, footprint and mode, and every name and dtype has a case for
    the stream and view runs"""
    import family_cases as FC
    from test_gpu_footprint import footprints
    fps, restated, marked = footprints(), {}, set()
    for case in FC.morphology(NAMES):
        (X,), (ctx, tag, mode, impl) = case["inputs"], case["ctx"]
        key = (case["name"], ctx, tag, mode)
        if key not in restated:
            restated[key] = fpn.FUNCTIONS[case["name"]](X, fps[tag], mode)
        case["reference"](restated[key])
        marked |= {(case["name"], X.dtype.type)} if case["stream"] else set()
    assert marked == {(n, t) for n in NAMES for t in (np.float32, np.float64)}
    assert {k[2:] for k in restated} == {(t, "reflect") for t in ("rand4x7", "diamond5", "L7x4")} | {("rand4x7", "nearest")}


def test_kernels_compile_without_scratch(tmp_path):
    """csrc/footprint.hip for gfx950: dtype x path x border mode x {min, max, both}, every kernel in registers"""
    import family_checks as fc
    text, kernels = fc.device_asm("footprint", tmp_path)
    assert len(kernels) == 24 and sum("footprint_runs_kernel" in k for k in kernels) == 12
    fc.assert_no_scratch(text, kernels)


def test_abi_argument_errors():
    """refusals by status code, before any launch and so without a GPU"""
    import ctypes as C
    import streamed as S
    from neilpy_amd import _lib, morphology as mo
    lib = _lib.load()
    assert {n for n in S.declarations() if n.startswith("smrf_footprint_")} == {"smrf_footprint_" + n for n in (
        "tile_bytes", "path", "filter_f32", "filter_f64")}
    p, null = C.c_void_p(4096), C.c_void_p(0)                        # never dereferenced: every call is refused first
    head = mo.plan(np.ones((3, 3))).head
    h = head.ctypes.data_as(C.c_void_p)
    f = lib.smrf_footprint_filter_f32
    E_ARG, E_UNSUPPORTED = -1, -5
    assert f(p, null, p, -1, 5, p, h, 0, 0, 0, 0, 0, null) == E_ARG
    assert f(p, null, p, 5, 5, p, null, 0, 0, 0, 0, 0, null) == E_ARG              # no plan head
    assert f(p, null, p, 5, 5, p, h, 0, 2, 0, 0, 0, null) == E_ARG                 # unknown mode
    assert f(p, null, p, 5, 5, p, h, 0, 0, 0, 3, 0, null) == E_ARG                 # unknown impl
    assert f(p, null, p, 5, 5, p, h, 0, 0, 0, 0, 4, null) == E_ARG                 # unknown epilogue
    assert f(null, null, p, 5, 5, p, h, 0, 0, 0, 0, 0, null) == E_ARG
    assert f(p, null, p, 5, 5, null, h, 0, 0, 0, 0, 0, null) == E_ARG
    assert f(p, null, p, 5, 5, p, h, 1, 0, 0, 0, 1, null) == E_ARG                 # a subtraction without d_sub
    assert f(p, null, p, (1 << 30) + 1, 5, p, h, 0, 0, 0, 0, 0, null) == E_UNSUPPORTED
    big = mo.plan(np.ones((90, 90)), impl=mo.IMPL_RUNS)
    assert big.path == "refused"
    assert f(p, null, p, 5, 5, p, big.head.ctypes.data_as(C.c_void_p), 0, 0, 0, mo.IMPL_RUNS, 0, null) == E_UNSUPPORTED
    assert f(p, null, p, 0, 5, p, h, 0, 0, 0, 0, 0, null) == 0                     # an empty raster: nothing launched
    for k, v in ((0, 0), (1, 0), (1, 10), (4, 0), (5, (1 << 20) + 1), (6, 16), (6, 2), (7, 17), (8, 5)):
        bad = head.copy()
        bad[k] = v
        assert f(p, null, p, 5, 5, p, bad.ctypes.data_as(C.c_void_p), 0, 0, 0, 0, 0, null) == E_ARG, (k, v)
