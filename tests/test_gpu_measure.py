"""Per-label measurements on the MI355X (neilpy_amd/measure.py, csrc/measure.hip).  The oracle is
the restatement tests/measure_numpy.py, bit for bit for every output, the sums included, on shapes up to 200 x 190 (above
that its Python-integer sums get slow); SciPy, within the bounds of tests/test_measure_host.py, at 513 x 577 and
1025 x 1030.  Zeros are compared by ``==``."""
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import scipy.ndimage as ndi

import label_numpy as lbn
import measure_numpy as mn
from conftest import ROOT

pytestmark = pytest.mark.gpu

# a wave takes 64 cells: one cell, one row and one column, a column short of, at and past a wave, several workgroups
SHAPES = ((1, 1), (1, 130), (130, 1), (17, 63), (17, 64), (17, 65), (65, 129), (200, 190))
LARGE = ((513, 577), (1025, 1030))
ALL = mn.STATS + ("flags",)
NAMES = ("sum_labels", "mean", "variance", "standard_deviation", "minimum", "maximum", "extrema", "minimum_position",
         "maximum_position")


def _ms():
    from neilpy_amd import measure
    return measure


def table(X, L, n, what=ALL):
    """the kernels' table with the flags, as NumPy arrays"""
    ms = _ms()
    T = ms._Table(X, L, n, ms.LABELS_AS_GIVEN, ms.mask_of(what))
    return {name: T.out(name) for name in what}


def assert_same(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype, got.shape, want.shape)
    ok = (got == want) | ((got != got) & (want != want))
    assert ok.all(), (ctx, int((~ok).sum()), np.flatnonzero(~ok.ravel())[:5], got.ravel()[~ok.ravel()][:5], want.ravel()[~ok.ravel()][:5])


def assert_table(got, want, ctx):
    for name in got:
        assert_same(got[name], want[name], (ctx, name))


# ------------------------------------------------------------------------------------------
# label rasters and values
# ------------------------------------------------------------------------------------------
def label_rasters(shape):
    """name -> (labels int32, n)"""
    out = {}
    for name in ("blobs", "rings", "maze"):
        L, n = ndi.label(lbn.GENERATORS[name](shape, 5))
        out[name] = (L, n)
    out["one label"] = (np.ones(shape, np.int32), 1)                   # every cell on one entry: the most contention
    C = mn.checker_labels(shape)
    out["checkerboard"] = (C, int(C.max()))                            # every stretch has length 1
    return out


def special_labels(L, n):
    """the six largest labels, largest first (fewer where the raster has fewer): the ones `special` gives its roles to"""
    sizes = np.bincount(L.ravel().clip(0), minlength=n + 1)[1:n + 1]
    return [int(k) + 1 for k in np.argsort(-sizes, kind="stable")[:6]]


def special(shape, L, n, seed=7):
    """a terrain in which, of `special_labels`, the first holds a NaN, the second is all NaN, the third holds +inf, the
    fourth both infinities, the fifth is all subnormal and the sixth lies near 1e308"""
    X = mn.dtm(shape, seed)
    flat, lab = X.ravel(), L.ravel()
    roles = special_labels(L, n)
    cells = lambda r: np.flatnonzero(lab == roles[r]) if r < len(roles) else np.zeros(0, np.int64)          # noqa: E731
    c = cells(0)
    flat[c[c.size // 2:c.size // 2 + 1]] = np.nan
    flat[cells(1)] = np.nan
    flat[cells(2)[:1]] = np.inf
    flat[cells(3)[-1:]] = np.inf
    flat[cells(3)[:1]] = -np.inf
    c5, c6 = cells(4), cells(5)
    flat[c5] = (np.arange(c5.size) % 97 - 40) * 5e-324
    flat[c6] = 1e308 * (0.5 + 0.49 * np.cos(np.arange(c6.size)))
    return X


def _to_float32(X):
    with np.errstate(over="ignore"):
        return X.astype(np.float32)                       # 1e308 becomes an infinity, the subnormals zero


def value_rasters(shape, L, n):
    """name -> values"""
    rng = np.random.default_rng([20270306] + list(shape))
    zeros = np.where(rng.random(shape) < 0.5, 0.0, -0.0)
    zeros[rng.random(shape) < 0.05] = 3.5
    cells = shape[0] * shape[1]
    return {
        "dtm": mn.dtm(shape, 1),
        "dtm float32": mn.dtm(shape, 1, np.float32),
        "1000 +- 1e-3": mn.cancelling(shape, 1),
        "40 decades": mn.decades(shape, 1),
        "all equal": np.full(shape, 271.25),
        "both zeros": zeros,
        "special": special(shape, L, n),
        "special float32": _to_float32(special(shape, L, n)),
        "subnormal": (rng.integers(-2000, 2000, shape) * 5e-324),
        "near 1e308": 1e308 * rng.uniform(-1.0, 1.7, shape),
        "uint8": (np.arange(cells).reshape(shape) * 37 % 256).astype(np.uint8),
        "int32": (mn.distinct(shape, 2) * 100003 % 2 ** 31 - 2 ** 30).astype(np.int32),
    }


@functools.lru_cache(maxsize=None)
def cases(shape):
    """[(context, values, labels, n, the restatement's table)]: every pair on the small shapes, each label raster with a
    rotating third (a quarter at 200 x 190) of the value rasters on the two large ones - every value raster still meets
    some label raster there"""
    out = []
    small = shape[0] * shape[1] <= 1200
    for j, (lname, (L, n)) in enumerate(label_rasters(shape).items()):
        for i, (vname, X) in enumerate(value_rasters(shape, L, n).items()):
            if small or (i + j) % (4 if shape[0] * shape[1] > 20000 else 3) == 0 or (vname == "special" and lname == "blobs"):
                with np.errstate(all="ignore"):
                    out.append(((shape, lname, vname), X, L, n, mn.region_stats(X, L, n)))
    return out


# ------------------------------------------------------------------------------------------
# the table, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_table_equals_the_restatement(gpu_device, shape):
    seen = set()
    for ctx, X, L, n, want in cases(shape):
        keep = X.copy(), L.copy()
        assert_table(table(X, L, n), want, ctx)
        assert keep[0].tobytes() == X.tobytes() and keep[1].tobytes() == L.tobytes(), ctx
        seen.add(ctx[2])
    assert len(seen) == 12                                               # every value raster was measured on this shape


def test_special_values_are_what_the_contract_says(gpu_device):
    """the rows of the non-finite, subnormal and huge labels spelt out, not only compared"""
    shape = (65, 129)
    L, n = label_rasters(shape)["blobs"]
    roles = special_labels(L, n)
    assert len(roles) == 6
    X = special(shape, L, n)
    T = table(X, L, n)
    k = roles
    assert T["flags"][k].tolist() == [1, 1, 2, 6, 0, 0]
    assert np.isnan(T["sum"][[k[0], k[1], k[3]]]).all() and T["sum"][k[2]] == np.inf and np.isnan(T["variance"][k[:4]]).all()
    assert np.isfinite(T["min"][k[0]]) and np.isnan(T["max"][k[0]]) and np.isnan(T["min"][k[1]]) and np.isnan(T["max"][k[1]])
    assert T["max"][k[2]] == np.inf and T["min"][k[3]] == -np.inf and T["max"][k[3]] == np.inf
    lab = L.ravel()
    assert T["min_index"][k[1]] == np.flatnonzero(lab == k[1])[0]
    assert T["max_index"][k[0]] == np.flatnonzero((lab == k[0]) & np.isnan(X.ravel()))[0]
    c5 = X.ravel()[lab == k[4]]
    assert 0 < np.abs(c5).max() < 2.3e-308
    assert T["sum"][k[4]] == float(np.sum(np.round(c5 / 5e-324))) * 5e-324       # whole multiples of 2**-1074: exact in integers
    assert T["min"][k[4]] == c5.min() and T["max"][k[4]] == c5.max() and T["variance"][k[4]] >= 0
    c6 = X.ravel()[lab == k[5]]
    exact = mn.exact_sum(c6)
    assert exact >= Fraction(2) ** 1024 and T["sum"][k[5]] == np.inf         # the sum itself leaves the range: +inf
    assert T["variance"][k[5]] == np.inf
    with np.errstate(all="ignore"):
        assert ndi.sum_labels(X, L, [k[5]])[0] == np.inf and ndi.variance(X, L, [k[5]])[0] == np.inf


@pytest.mark.parametrize("what", [(w,) for w in mn.STATS] + [mn.STATS, ("max", "count"), ("mean", "min_index")],
                         ids=lambda w: "+".join(w) if len(w) < 8 else "all")
def test_region_stats_computes_what_is_asked(gpu_device, what):
    """each single measurement, pairs and all of them: the same bits whatever else is computed beside them, NumPy in ->
    NumPy out with n given and with the raster's maximum"""
    ms = _ms()
    ctx, X, L, n, want = next(c for c in cases((65, 129)) if c[0][1:] == ("blobs", "special"))
    for given in (None, n, n + 3, 2):
        got = ms.region_stats(X, L, given, what)
        assert list(got) == [w for w in mn.STATS if w in what] and all(isinstance(v, np.ndarray) for v in got.values())
        m = n if given is None else given
        for name, v in got.items():
            ref = want[name][:m + 1]
            if m > n:                                                    # labels that do not occur
                pad = {"count": 0, "sum": 0.0, "mean": np.nan, "variance": np.nan, "min": 0, "max": 0, "min_index": -1, "max_index": -1}
                ref = np.concatenate([ref, np.full(m - n, pad[name], dtype=ref.dtype)])
            assert_same(v, ref, (what, given, name))
    assert np.array_equal(ms.region_stats(X, L, n, ("count",))["count"], np.bincount(L.ravel(), minlength=n + 1))


def test_hand_made_labels(gpu_device):
    """gaps in the numbering, negative labels and labels above n, alone and tiled over several waves; label dtypes"""
    ms = _ms()
    for H in (lbn.HAND, np.tile(lbn.HAND, (13, 19))):
        X = mn.dtm(H.shape, 3)
        for n in (0, 1, 7, 9, 45):
            with np.errstate(all="ignore"):
                want = mn.region_stats(X, H, n)
            assert_table(table(X, H, n), want, (H.shape, n))
        got = ms.region_stats(X, H)                                     # the raster's maximum: 40
        assert got["count"].shape == (41,) and got["count"][40] == np.sum(H == 40) and got["count"][3] == 0
        assert got["min_index"][3] == -1 and got["sum"][6] == 0 and np.isnan(got["mean"][6])
        for dtype in (np.int8, np.int16, np.int64):
            assert_table(ms.region_stats(X, H.astype(dtype), 9), ms.region_stats(X, H, 9), dtype)
        assert_table(ms.region_stats(X, (H == 1), 1), ms.region_stats(X, (H == 1).astype(np.int32), 1), "bool")


# ------------------------------------------------------------------------------------------
# scipy.ndimage's wrappers
# ------------------------------------------------------------------------------------------
def forms(L, n):
    return (("labels=None", None, None), ("index=None", L, None), ("scalar", L, min(2, n)), ("scalar missing", L, n + 2),
            ("array", L, [n, 1, 0, 1, n + 5, -2, max(n - 1, 1)]))


def assert_result(got, want, ctx):
    if isinstance(want, tuple) and len(want) == 4:                                                    # extrema
        assert isinstance(got, tuple) and len(got) == 4, ctx
        assert_same(got[0], want[0], ctx), assert_same(got[1], want[1], ctx)
        assert_result(got[2], want[2], ctx), assert_result(got[3], want[3], ctx)
    elif isinstance(want, (tuple, list)):                                                             # positions
        assert type(got) is type(want) and got == want, (ctx, got, want)
        flat = [v for p in (got if isinstance(got, list) else [got]) for v in p]
        assert all(type(v) is int for v in flat), ctx
    else:
        assert_same(got, want, ctx)


def _host(v):
    import torch
    if isinstance(v, torch.Tensor):
        return v.cpu().numpy()
    return tuple(_host(e) for e in v) if isinstance(v, tuple) and v and isinstance(v[0], torch.Tensor) else v


@pytest.mark.parametrize("vname", ["special", "special float32", "uint8", "int32", "all equal"])
def test_wrappers_under_every_form(gpu_device, vname):
    """every SciPy-named function under labels=None, index=None, a scalar index and an unsorted array index with repeats,
    0, a missing and a negative label: NumPy in gives the restatement's value bit for bit, a tensor in gives the same on its
    device"""
    import torch
    ms = _ms()
    shape = (65, 129)
    rasters = [label_rasters(shape)["blobs"], (np.tile(lbn.HAND, (13, 19))[:, :129], 7)]
    for L, n in rasters:
        L = np.ascontiguousarray(L)
        X = value_rasters(shape, L, n)[vname]
        Xt, Lt = torch.from_numpy(X).to(gpu_device), torch.from_numpy(L).to(gpu_device)
        for fname, lab, index in forms(L, n):
            for name in NAMES:
                with np.errstate(all="ignore"):
                    want = getattr(mn, name)(X, lab, index)
                got = getattr(ms, name)(X, lab, index)
                assert_result(got, want, (vname, fname, name))
                if "position" not in name and name != "extrema":
                    assert isinstance(got, (np.ndarray, np.generic)), (name, type(got))
                tgot = getattr(ms, name)(Xt, None if lab is None else Lt, index)
                first = tgot[0] if name == "extrema" else tgot
                if "position" not in name:
                    assert isinstance(first, torch.Tensor) and first.device == Xt.device, (name, type(first))
                    assert first.dim() == (1 if fname == "array" else 0)
                if name == "extrema":
                    tgot = (_host(tgot[0]), _host(tgot[1]), tgot[2], tgot[3])
                assert_result(_host(tgot), want if not isinstance(want, np.generic) else np.asarray(want), (vname, fname, name, "tensor"))
        assert Xt.cpu().numpy().tobytes() == X.tobytes() and Lt.cpu().numpy().tobytes() == L.tobytes()      # unchanged


def test_views_tensors_and_index_kinds(gpu_device):
    """transposed and strided views of values and labels give the contiguous call's bits; the inputs are unchanged; index as
    a list, an array, a tensor; labels on the device with values from the host"""
    import torch
    ms = _ms()
    shape = (65, 129)
    L, n = label_rasters(shape)["rings"]
    for X in (mn.dtm(shape, 9), mn.dtm(shape, 9, np.float32), value_rasters(shape, L, n)["int32"]):
        want = ms.region_stats(X, L, n)
        Xt, Lt = torch.from_numpy(X).to(gpu_device), torch.from_numpy(L).to(gpu_device)
        got = ms.region_stats(Xt, Lt, n)
        assert all(isinstance(v, torch.Tensor) and v.device == Xt.device for v in got.values())
        assert got["count"].dtype == torch.int64 and got["sum"].dtype == torch.float64 and got["min"].dtype == Xt.dtype
        assert got["min_index"].dtype == torch.int64
        assert_table({k: v.cpu().numpy() for k, v in got.items()}, want, "tensor")
        XT = torch.from_numpy(np.ascontiguousarray(X.T)).to(gpu_device).T
        LT = torch.from_numpy(np.ascontiguousarray(L.T)).to(gpu_device).T
        assert not XT.is_contiguous()
        assert_table({k: v.cpu().numpy() for k, v in ms.region_stats(XT, LT, n).items()}, want, "transposed")
        wide = torch.zeros((shape[0] + 3, 2 * shape[1] + 5), dtype=Xt.dtype, device=gpu_device)
        view = wide[2:2 + shape[0], 3:3 + 2 * shape[1]:2]
        view.copy_(Xt)
        before = wide.clone()
        assert_table({k: v.cpu().numpy() for k, v in ms.region_stats(view, Lt, n).items()}, want, "strided")
        assert torch.equal(wide, before) and Xt.cpu().numpy().tobytes() == X.tobytes()
        assert_table(ms.region_stats(np.asfortranarray(X), np.asfortranarray(L), n), want, "host order")
        index = [n, 1, 0, 2]
        ref = ms.sum_labels(X, L, index)
        for kind in (np.array(index), np.array(index, dtype=np.uint8 if n < 256 else np.int64), torch.tensor(index), tuple(index)):
            assert_same(ms.sum_labels(X, L, kind), ref, type(kind))
        assert_same(ms.sum_labels(Xt, Lt, index).cpu().numpy(), ref, "tensor")
        assert_same(ms.maximum(Xt, Lt, index).cpu().numpy(), ms.maximum(X, L, index), "tensor maximum")
    Z = mn.dtm(shape, 9)
    assert_table(ms.region_stats(Z.tolist(), L.tolist(), n), ms.region_stats(Z, L, n), "lists")


def test_the_same_on_every_run(gpu_device):
    """three runs of the 200 x 190 cases with the most atomics on one entry, bit for bit"""
    import torch
    ms = _ms()
    for ctx, X, L, n, want in cases((200, 190)):
        if ctx[1] not in ("one label", "blobs"):
            continue
        Xt, Lt = torch.from_numpy(X).to(gpu_device), torch.from_numpy(L).to(gpu_device)
        runs = [ms.region_stats(Xt, Lt, n) for _ in range(3)]
        for name in runs[0]:
            a, b, c = (r[name].view(torch.uint8) if r[name].dtype != torch.int64 else r[name] for r in runs)
            assert torch.equal(a, b) and torch.equal(a, c), (ctx, name)


# ------------------------------------------------------------------------------------------
# above the restatement's reach: SciPy within the host test's bounds
# ------------------------------------------------------------------------------------------
def _groups(L, n):
    lab = L.ravel()
    order = np.argsort(lab, kind="stable")
    start = np.searchsorted(lab[order], np.arange(n + 2))
    return [order[start[k]:start[k + 1]] for k in range(n + 1)]


@pytest.mark.parametrize("shape", LARGE, ids=lambda s: "%dx%d" % s)
def test_large_rasters_against_scipy(gpu_device, shape):
    """counts, extrema and positions exactly; a sum within ulp / 2 + n 2**(E - 93) of the exact sum, SciPy's within
    n 2**-52 sum |t| of it, the exact sum by math.fsum (half an ulp of its own); the variance against the exact sum of its own
    terms, taken from the mean the device gives"""
    ms = _ms()
    L, n = ndi.label(lbn.blobs(shape, 11))
    index = np.arange(n + 1)
    for X in (mn.dtm(shape, 11), mn.cancelling(shape, 11).astype(np.float64), mn.dtm(shape, 12, np.float32)):
        T = ms.region_stats(X, L, n)
        assert np.array_equal(T["count"], np.bincount(L.ravel(), minlength=n + 1))
        assert_same(T["min"], ndi.minimum(X, L, index), "min"), assert_same(T["max"], ndi.maximum(X, L, index), "max")
        theirs = ndi.sum_labels(X, L, index)
        x = X.astype(np.float64).ravel()
        for k, cells in enumerate(_groups(L, n)):
            t = x[cells]
            cnt = t.size
            assert cnt == T["count"][k] > 0
            s, absum = math.fsum(t), math.fsum(np.abs(t))
            half = mn.ulp(s) / 2
            E = mn.exponent_of(float(np.abs(t).max()))
            assert abs(Fraction(float(T["sum"][k])) - Fraction(s)) <= mn.ulp(T["sum"][k]) / 2 + cnt * Fraction(2) ** (E - 93) + half, k
            assert abs(Fraction(float(theirs[k])) - Fraction(s)) <= cnt * Fraction(2) ** -52 * Fraction(absum) + half, k
            assert T["mean"][k] == T["sum"][k] / np.float64(cnt)
            d = t - T["mean"][k]
            sq = d * d
            v = math.fsum(sq)
            bound = (mn.ulp(T["variance"][k] * cnt) / 2 + cnt * Fraction(2) ** (2 * E + 3 - 93) + mn.ulp(v) / 2) / cnt + mn.ulp(T["variance"][k])
            assert abs(Fraction(float(T["variance"][k])) - Fraction(v) / cnt) <= bound, k
    D = mn.distinct(shape, 11)
    cols = shape[1]
    T = ms.region_stats(D, L, n, ("min_index", "max_index"))
    assert [divmod(int(i), cols) for i in T["min_index"]] == [tuple(p) for p in ndi.minimum_position(D, L, index)]
    assert [divmod(int(i), cols) for i in T["max_index"]] == [tuple(p) for p in ndi.maximum_position(D, L, index)]
    assert ms.maximum_position(D, L, [1, n]) == [tuple(int(v) for v in p) for p in ndi.maximum_position(D, L, [1, n])]
    one = np.ones(shape, np.int32)                                       # one object: every wave on one entry
    X = mn.dtm(shape, 13)
    got, s = ms.sum_labels(X, one, 1), math.fsum(X.ravel())
    assert abs(Fraction(float(got)) - Fraction(s)) <= mn.ulp(got) / 2 + X.size * Fraction(2) ** (mn.exponent_of(float(X.max())) - 93) + mn.ulp(s) / 2
    assert got == ms.sum_labels(X) == ms.sum_labels(X, one) and ms.minimum_position(X) == tuple(int(v) for v in ndi.minimum_position(X))


# ------------------------------------------------------------------------------------------
# guarded memory and a side stream, on cases built here
# ------------------------------------------------------------------------------------------
def harness_cases():
    """region_stats with everything on a float32 terrain with NaN (the three passes and both table kernels), and three
    measurements on float64 with labels that do not occur, on a shape with ragged waves"""
    ms = _ms()
    shape = (67, 131)
    L, n = ndi.label(lbn.blobs(shape, 13))
    X = _to_float32(special(shape, L, n))
    with np.errstate(all="ignore"):
        want = mn.region_stats(X, L, n)

    def stats_ref(got):
        assert sorted(got) == sorted(mn.STATS)
        assert_table(got, want, "region_stats")
    yield dict(name="region_stats", fn=lambda Xt, Lt: ms.region_stats(Xt, Lt, n), inputs=[X, L], ctx=("region_stats", "float32"),
               reference=stats_ref)
    Y = mn.cancelling(shape, 13)
    some = ("count", "variance", "max_index")
    with np.errstate(all="ignore"):
        want64 = mn.region_stats(Y, L, n + 2)

    def some_ref(got):
        assert sorted(got) == sorted(some)
        assert_table(got, want64, "region_stats of three")
    yield dict(name="region_stats", fn=lambda Yt, Lt: ms.region_stats(Yt, Lt, n + 2, some), inputs=[Y, L],
               ctx=("region_stats of three", "float64"), reference=some_ref)


def wrapper_case():
    """variance under an array index: the gather by torch behind the kernels (its result is torch's own allocation, so this
    case is for the side stream only)"""
    ms = _ms()
    shape = (67, 131)
    L, n = ndi.label(lbn.blobs(shape, 13))
    Y = mn.cancelling(shape, 13)
    index = [n, 2, 0, 2, n + 3, -1]
    with np.errstate(all="ignore"):
        var = mn.variance(Y, L, index)
    return dict(name="variance", fn=lambda Yt, Lt: ms.variance(Yt, Lt, index), inputs=[Y, L], ctx=("variance", "float64"),
                reference=lambda got: assert_same(got, var, "variance"))


def test_on_guarded_memory(gpu_device):
    from test_gpu_guarded import run_guarded
    for case in harness_cases():
        run_guarded(**case)


def test_on_a_side_stream(gpu_device):
    """every launch carries the current stream: the handles of smrf_measure_* are recorded beside the shared header's"""
    import streamed as S
    from test_gpu_streams import streamed
    slots = dict(S.stream_slots(), **S.stream_slots(open(os.path.join(ROOT, "include", "smrf_measure.h")).read()))
    assert (slots["smrf_measure_f32"], slots["smrf_measure_f64"], slots["smrf_measure_workspace_bytes"]) == (10, 10, None)
    for case in list(harness_cases()) + [wrapper_case()]:
        streamed(case["fn"], case["inputs"], name=case["name"], ctx=case["ctx"], reference=case["reference"], slots=slots)
