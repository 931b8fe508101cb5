"""Connected components on the MI355X (neilpy_amd/label.py, csrc/label.hip): label under all 16
structures against scipy.ndimage.label on shapes that straddle every tile edge, on random masks near and far from the
percolation thresholds and on constructed masks; the input kinds; region_sizes, bounding_boxes, find_objects and
remove_small_objects against np.bincount, scipy.ndimage.find_objects and the NumPy expression over SciPy's labels;
repeatability; a drawn table of structured masks (blobs, strokes, rings, mazes) and the constructed chains at 17 x 17
tiles; guarded memory and a side stream.  The oracle is SciPy on this machine and every comparison is exact."""
import functools
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

import label_numpy as lbn
from conftest import ROOT

pytestmark = pytest.mark.gpu

# 64 x 64 tiles: one cell, one row and one column, a column short of, at and past a tile, several tiles with ragged edges
SHAPES = ((1, 1), (1, 130), (130, 1), (17, 63), (17, 64), (17, 65), (65, 129), (200, 190))
ALL_STRUCTURES_ON = ((65, 129), (200, 190))
MID = (2048, 2047)
DENSITIES = (0.1, 0.41, 0.59, 0.95)
USUAL = (lbn.FOUR, lbn.EIGHT)


def _lb():
    from neilpy_amd import label
    return label


def assert_labels(got, want, ctx):
    (L, n), (W, m) = got, want
    assert isinstance(n, int) and n == m, (ctx, n, m)
    assert L.dtype == W.dtype == np.int32 and L.shape == W.shape, (ctx, L.dtype, L.shape)
    assert np.array_equal(L, W), (ctx, int(np.sum(L != W)))


@functools.lru_cache(maxsize=None)
def mid_case():
    """the mid-size mask at the 4-connected percolation threshold and SciPy's labels of it, computed once"""
    mask = lbn.random_mask(MID, 0.59, 7)
    L, n = ndi.label(mask)
    return mask, L, n


# ------------------------------------------------------------------------------------------
# label
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_random_masks_against_scipy(gpu_device, shape):
    lb = _lb()
    for p in DENSITIES:
        mask = lbn.random_mask(shape, p, 3)
        for k in (range(16) if shape in ALL_STRUCTURES_ON else USUAL):
            assert_labels(lb.label(mask, lbn.STRUCTURES[k]), ndi.label(mask, lbn.STRUCTURES[k]), (shape, p, k))
    assert_labels(lb.label(mask), ndi.label(mask), (shape, "default structure"))


def test_mid_size_against_scipy(gpu_device):
    lb = _lb()
    mask, L, n = mid_case()
    assert_labels(lb.label(mask), (L, n), (MID, 0.59, "4"))
    for p, k in ((0.41, lbn.EIGHT), (0.1, lbn.FOUR), (0.95, lbn.EIGHT)):
        m = lbn.random_mask(MID, p, 7)
        assert_labels(lb.label(m, lbn.STRUCTURES[k]), ndi.label(m, lbn.STRUCTURES[k]), (MID, p, k))


@pytest.mark.parametrize("shape", [(130, 130), (257, 257)], ids=lambda s: "%dx%d" % s)
def test_constructed_masks_against_scipy(gpu_device, shape):
    lb = _lb()
    counts = {}
    for name, mask in lbn.constructed(shape).items():
        for k in USUAL + (lbn.SE, lbn.SW, 0):
            got = lb.label(mask, lbn.STRUCTURES[k])
            assert_labels(got, ndi.label(mask, lbn.STRUCTURES[k]), (shape, name, k))
            counts[name, k] = got[1]
    cells = shape[0] * shape[1]
    assert counts["zeros", lbn.FOUR] == 0 and counts["ones", lbn.FOUR] == counts["ones", lbn.EIGHT] == 1
    assert counts["ones", 0] == cells                                           # no link: every cell its own object
    assert counts["checkerboard", lbn.FOUR] == (cells + 1) // 2 and counts["checkerboard", lbn.EIGHT] == 1
    assert counts["serpentine", lbn.FOUR] == counts["spiral", lbn.FOUR] == counts["comb", lbn.FOUR] == counts["frame", lbn.FOUR] == 1
    assert counts["stripes se", lbn.SE] < counts["stripes se", lbn.SW] == counts["stripes se", 0]
    assert counts["stripes sw", lbn.SW] < counts["stripes sw", lbn.SE] == counts["stripes sw", 0]
    L, n = lb.label(lbn.u_and_speck(shape))
    assert n == 2 and L[0, shape[1] - 3] == L[2, 2] == L[-1, shape[1] // 2] == 1 and L[1, shape[1] // 2] == 2


def test_input_kinds(gpu_device):
    """bool, uint8, int32, float32 with NaN and -0.0, float64: the same labels; tensor in, tensor out; views; the input
    unchanged; empty rasters"""
    import torch
    lb = _lb()
    shape = (65, 129)
    mask = lbn.random_mask(shape, 0.59, 11)
    want = ndi.label(mask)
    rng = np.random.default_rng(20270102)
    f32 = np.where(mask, rng.normal(size=shape), 0.0).astype(np.float32)
    f32[mask & (rng.random(shape) < 0.2)] = np.nan
    f32[~mask & (rng.random(shape) < 0.5)] = -0.0
    assert np.isnan(f32).any() and np.signbit(f32[f32 == 0]).any()
    kinds = {"bool": mask, "uint8": mask.astype(np.uint8) * 200, "int32": np.where(mask, -5, 0).astype(np.int32), "float32": f32,
             "float64": f32.astype(np.float64), "int64": mask.astype(np.int64) << 40, "uint16": mask.astype(np.uint16)}
    for name, X in kinds.items():
        assert np.array_equal(X != 0, mask)
        assert_labels(ndi.label(X), want, ("scipy", name))
        keep = X.copy()
        assert_labels(lb.label(X), want, name)
        assert keep.tobytes() == X.tobytes(), name
        if name == "uint16":
            continue
        Xt = torch.from_numpy(X).to(gpu_device)
        before = Xt.clone()
        L, n = lb.label(Xt, output=np.int32)
        assert isinstance(L, torch.Tensor) and L.device == Xt.device and L.dtype == torch.int32 and isinstance(n, int)
        assert_labels((L.cpu().numpy(), n), want, (name, "tensor"))
        assert torch.equal(Xt.view(torch.uint8), before.view(torch.uint8)), name
        # a transposed and an offset-strided view: the contiguous call's bits
        base = torch.from_numpy(np.ascontiguousarray(X.T)).to(gpu_device)
        assert_labels(tuple(map(_host, lb.label(base.T))), want, (name, "transposed"))
        wide = torch.ones((shape[0] + 3, 2 * shape[1] + 5), dtype=Xt.dtype, device=gpu_device)
        view = wide[2:2 + shape[0], 3:3 + 2 * shape[1]:2]
        view.copy_(Xt)
        assert not view.is_contiguous()
        assert_labels(tuple(map(_host, lb.label(view, lbn.STRUCTURES[lbn.FOUR]))), want, (name, "strided"))
    assert_labels(lb.label(np.asfortranarray(f32)), want, "host order")
    assert_labels(lb.label(mask.tolist()), want, "a list")
    for empty in ((0, 5), (4, 0), (0, 0)):
        L, n = lb.label(torch.zeros(empty, dtype=torch.float32, device=gpu_device))
        assert isinstance(L, torch.Tensor) and L.is_cuda and tuple(L.shape) == empty and L.dtype == torch.int32 and n == 0
        L, n = lb.label(np.zeros(empty, bool))
        assert isinstance(L, np.ndarray) and L.shape == empty and L.dtype == np.int32 and n == 0


def _host(v):
    return v if isinstance(v, int) else v.cpu().numpy()


def test_the_same_on_every_run(gpu_device):
    """three calls on the mid-size mask: the order in which atomics land does not reach the numbering"""
    import torch
    lb = _lb()
    mask, L, n = mid_case()
    Mt = torch.from_numpy(mask).to(gpu_device)
    runs = [lb.label(Mt) for _ in range(3)]
    assert [r[1] for r in runs] == [n] * 3
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], runs[2][0])
    assert np.array_equal(runs[0][0].cpu().numpy(), L)


# ------------------------------------------------------------------------------------------
# sizes, boxes, find_objects, remove_small_objects
# ------------------------------------------------------------------------------------------
def boxes_of(slices, n):
    out = np.zeros((n, 4), dtype=np.int32)
    for k, s in enumerate(slices):
        if s is not None:
            out[k] = (s[0].start, s[0].stop, s[1].start, s[1].stop)
    return out


def label_rasters():
    yield "mid", mid_case()[1], mid_case()[2]
    for shape, p, k in (((200, 190), 0.41, lbn.EIGHT), ((65, 129), 0.1, lbn.FOUR), ((1, 130), 0.59, lbn.FOUR), ((130, 1), 0.95, lbn.FOUR)):
        L, n = ndi.label(lbn.random_mask(shape, p, 3), lbn.STRUCTURES[k])
        yield (shape, p, k), L, n
    for name in ("serpentine", "checkerboard", "zeros", "frame", "stripes se"):
        L, n = ndi.label(lbn.constructed((130, 130))[name])
        yield name, L, n


def test_regions_against_numpy_and_scipy(gpu_device):
    import torch
    lb = _lb()
    for ctx, L, n in label_rasters():
        want_size = np.bincount(L.ravel(), minlength=n + 1).astype(np.int64)
        want_find = ndi.find_objects(L)
        want_box = boxes_of(want_find, n)
        for given in (None, n):
            size, box = lb.region_sizes(L, given), lb.bounding_boxes(L, given)
            assert size.dtype == np.int64 and np.array_equal(size, want_size), (ctx, given)
            assert box.dtype == np.int32 and box.shape == (n, 4) and np.array_equal(box, want_box), (ctx, given)
        assert lb.find_objects(L) == want_find, ctx
        if ctx == "mid":
            continue                      # some 120 000 objects: the variants below are run on the smaller rasters
        assert lb.find_objects(L, n + 3) == ndi.find_objects(L, n + 3), ctx
        if n > 2:
            assert lb.find_objects(L, n // 2) == ndi.find_objects(L, n // 2), ctx
            assert np.array_equal(lb.region_sizes(L, n // 2), want_size[:n // 2 + 1]), ctx
        Lt = torch.from_numpy(L).to(gpu_device)
        size, box = lb.region_sizes(Lt), lb.bounding_boxes(Lt, n)
        assert size.is_cuda and size.dtype == torch.int64 and np.array_equal(size.cpu().numpy(), want_size), ctx
        assert box.is_cuda and box.dtype == torch.int32 and np.array_equal(box.cpu().numpy(), want_box), ctx
        assert lb.find_objects(Lt) == want_find, ctx
        assert lb.find_objects(Lt.to(torch.int64)) == lb.find_objects(L.astype(np.uint8 if n < 256 else np.int64)) == want_find, ctx


def test_regions_on_the_hand_made_labels(gpu_device):
    """gaps, a label above max_label and negative cells"""
    import torch
    lb = _lb()
    H = lbn.HAND
    for max_label in (0, 1, 5, 7, 9, 45):
        assert lb.find_objects(H, max_label) == ndi.find_objects(H, max_label), max_label
        assert lb.find_objects(torch.from_numpy(H).to(gpu_device), max_label) == ndi.find_objects(H, max_label), max_label
    for dtype in (np.int8, np.int16, np.int64):
        assert lb.find_objects(H.astype(dtype), 9) == ndi.find_objects(H, 9), dtype
    for n in (7, 9, 45, None):
        m = 40 if n is None else n
        assert np.array_equal(lb.region_sizes(H, n), lbn.region_sizes(H, m)), n
        assert np.array_equal(lb.bounding_boxes(H, n), lbn.bounding_boxes(H, m)), n
        assert np.array_equal(lb.bounding_boxes(H, n), boxes_of(ndi.find_objects(H, m), m)), n
    pos = np.where((H >= 0) & (H <= 7), H, 0)
    assert np.array_equal(lb.region_sizes(H, 7)[1:], np.bincount(pos.ravel(), minlength=8)[1:])
    assert lb.region_sizes(H, 0).tolist() == [int(np.count_nonzero(H == 0))] and lb.bounding_boxes(H, 0).shape == (0, 4)
    Z = np.zeros((3, 4), np.int32)
    assert lb.find_objects(Z) == ndi.find_objects(Z) == [] and lb.region_sizes(Z).tolist() == [12]
    far = np.array([[0, 2 ** 40, -2 ** 40, 1]], dtype=np.int64)
    assert lb.find_objects(far, 2) == ndi.find_objects(far, 2)


@pytest.mark.parametrize("connectivity", [1, 2])
def test_remove_small_objects(gpu_device, connectivity):
    import torch
    lb = _lb()
    structure = lbn.STRUCTURES[lbn.FOUR if connectivity == 1 else lbn.EIGHT]
    masks = [((200, 190), lbn.random_mask((200, 190), p, 5)) for p in (0.1, 0.41, 0.59)]
    masks += [(MID, mid_case()[0]), ("checkerboard", lbn.checkerboard((65, 129))), ("zeros", np.zeros((17, 65), bool))]
    for ctx, mask in masks:
        L, n = (mid_case()[1:] if ctx == MID and connectivity == 1 else ndi.label(mask, structure))
        sizes = np.bincount(L.ravel(), minlength=n + 1)
        for min_size in (1, 2, int(np.median(sizes[1:])) if n else 5):
            want = lbn.kept(L, sizes, min_size)          # np.isin(L, np.flatnonzero(sizes >= min_size)[1:]), see there
            got = lb.remove_small_objects(mask, min_size, connectivity)
            assert got.dtype == bool and np.array_equal(got, want), (ctx, min_size)
        t = lb.remove_small_objects(torch.from_numpy(mask).to(gpu_device), connectivity=connectivity)
        assert t.is_cuda and t.dtype == torch.bool
        assert np.array_equal(t.cpu().numpy(), lbn.kept(L, sizes, 64)), ctx
    # any input is the mask `!= 0`: an integer raster is not taken as labels
    ints = np.where(masks[1][1], 3, 0).astype(np.int32)
    assert np.array_equal(lb.remove_small_objects(ints, 5, connectivity), lb.remove_small_objects(masks[1][1], 5, connectivity))


# ------------------------------------------------------------------------------------------
# structured masks: solid objects across many seams, objects inside holes, long winding chains
# ------------------------------------------------------------------------------------------
# Generator (tests/label_numpy.py), shape (rows and columns from 1, 2, 63..65, 127..129, 191..193, 513, 577), seed and
# structure.  Each of the four structures with both the E and the S link - where the seam pass skips pairs that jobs next
# to it join - three times on blobs, every other structure once.  Drawn once from numpy's default_rng(20270207) and kept as
# a literal, so a failure names its case and replays alone.
DRAWS = [
    # id, generator, shape, seed, structure
    (600, 'blobs', (2, 513), 93, 3),
    (601, 'blobs', (577, 129), 14, 3),
    (602, 'blobs', (193, 65), 60, 3),
    (603, 'blobs', (193, 63), 39, 7),
    (604, 'blobs', (192, 191), 27, 7),
    (605, 'blobs', (192, 127), 92, 7),
    (606, 'blobs', (2, 63), 86, 11),
    (607, 'blobs', (192, 577), 94, 11),
    (608, 'blobs', (64, 63), 90, 11),
    (609, 'blobs', (193, 63), 76, 15),
    (610, 'blobs', (192, 191), 87, 15),
    (611, 'blobs', (577, 192), 64, 15),
    (612, 'strokes', (513, 2), 12, 0),
    (613, 'rings', (191, 193), 54, 1),
    (614, 'maze', (65, 1), 21, 2),
    (615, 'strokes', (129, 64), 15, 4),
    (616, 'rings', (63, 192), 68, 5),
    (617, 'maze', (129, 577), 36, 6),
    (618, 'strokes', (192, 191), 84, 8),
    (619, 'rings', (65, 129), 2, 9),
    (620, 'maze', (513, 63), 75, 10),
    (621, 'strokes', (128, 64), 88, 12),
    (622, 'rings', (577, 129), 8, 13),
    (623, 'maze', (128, 64), 86, 14),
]
DRAW_AXIS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 513, 577)
LARGE = (1025, 1030)                      # 17 x 17 tiles


def test_the_draws_cover_every_structure():
    assert len(DRAWS) >= 24 and len({c[0] for c in DRAWS}) == len(DRAWS)
    assert all(c[2][0] in DRAW_AXIS and c[2][1] in DRAW_AXIS and c[1] in lbn.GENERATORS for c in DRAWS)
    assert {c[4] for c in DRAWS} == set(range(16))
    assert {c[1] for c in DRAWS} == set(lbn.GENERATORS)
    for k in range(16):
        if k & lbn.E and k & lbn.S:
            assert sum(c[1] == "blobs" and c[4] == k for c in DRAWS) >= 3, k


@pytest.mark.parametrize("case", DRAWS, ids=lambda c: str(c[0]))
def test_structured_masks_against_scipy(gpu_device, case):
    """label against SciPy, then sizes, boxes and find_objects on those labels and remove_small_objects on the mask"""
    lb = _lb()
    cid, name, shape, seed, k = case
    mask = lbn.GENERATORS[name](shape, seed)
    L, n = ndi.label(mask, lbn.STRUCTURES[k])
    got = lb.label(mask, lbn.STRUCTURES[k])
    assert_labels(got, (L, n), case)
    sizes = np.bincount(L.ravel(), minlength=n + 1).astype(np.int64)
    found = ndi.find_objects(L)
    assert np.array_equal(lb.region_sizes(got[0], n), sizes), case
    assert np.array_equal(lb.bounding_boxes(got[0], n), boxes_of(found, n)), case
    assert lb.find_objects(got[0]) == found, case
    connectivity = 2 if k & (lbn.SE | lbn.SW) else 1
    if k not in USUAL:                                      # remove_small_objects knows the two usual structures only
        L, n = ndi.label(mask, lbn.STRUCTURES[USUAL[connectivity - 1]])
        sizes = np.bincount(L.ravel(), minlength=n + 1)
    for min_size in (2, int(np.median(sizes[1:])) if n else 5, 64):
        keep = lb.remove_small_objects(mask, min_size, connectivity)
        assert keep.dtype == bool and np.array_equal(keep, lbn.kept(L, sizes, min_size)), (case, min_size)


def large_masks():
    """name -> mask at 17 x 17 tiles: the constructed chains, their transposes (chains along columns cross the other
    seam) and the maze"""
    out = {}
    for name, make in (("serpentine", lbn.serpentine), ("spiral", lbn.spiral), ("comb", lbn.comb)):
        out[name] = make(LARGE)
        out[name + " transposed"] = np.ascontiguousarray(make(LARGE[::-1]).T)
    out["maze"] = lbn.maze(LARGE, 1)
    return out


def _timed(lb, Mt, structure, repeats=5):
    """the labels of a mask on the device and the median wall time of the call, which ends with the read of the count"""
    import time
    import torch
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L, n = lb.label(Mt, structure)
        times.append(time.perf_counter() - t0)
    return (L.cpu().numpy(), n), sorted(times)[repeats // 2]


def test_large_constructed_masks_against_scipy(gpu_device, capsys):
    """1025 x 1030 under the 4- and the 8-neighbourhood; the checkerboard under the 4-neighbourhood, some 528 000
    objects, so the scan runs over many blocks; the maze three times, bit for bit.  The find-root walks have no path
    compression, so each mask's wall time is printed beside a Bernoulli mask's of the same size (DESIGN.md section 21
    keeps the figures; nothing is asserted of them)."""
    import torch
    lb = _lb()
    noise = torch.from_numpy(lbn.random_mask(LARGE, 0.59, 7)).to(gpu_device)
    lb.label(noise)                                                          # the first call loads the kernels
    times = {}
    for k in USUAL:
        times["random p=0.59", k] = _timed(lb, noise, lbn.STRUCTURES[k])[1]
    for name, mask in large_masks().items():
        Mt = torch.from_numpy(mask).to(gpu_device)
        for k in USUAL:
            got, times[name, k] = _timed(lb, Mt, lbn.STRUCTURES[k])
            want = ndi.label(mask, lbn.STRUCTURES[k])
            assert_labels(got, want, (name, k))
        if name == "maze":
            again = [lb.label(Mt) for _ in range(3)]
            assert [r[1] for r in again] == [1] * 3
            assert torch.equal(again[0][0], again[1][0]) and torch.equal(again[0][0], again[2][0])
            assert np.array_equal(again[0][0].cpu().numpy(), ndi.label(mask)[0])
    board = lbn.checkerboard(LARGE)
    got, times["checkerboard", lbn.FOUR] = _timed(lb, torch.from_numpy(board).to(gpu_device), lbn.STRUCTURES[lbn.FOUR])
    assert_labels(got, ndi.label(board), "checkerboard")
    assert got[1] == (LARGE[0] * LARGE[1] + 1) // 2 > 500000
    with capsys.disabled():
        for (name, k), t in times.items():
            print("\nlabel %s %d x %d, structure %d: %.2f ms (%.1f x random)" % ((name,) + LARGE + (k, 1e3 * t, t / times["random p=0.59", k])), end="")


# ------------------------------------------------------------------------------------------
# guarded memory and a side stream, on cases built here
# ------------------------------------------------------------------------------------------
def harness_cases():
    """label of a float32 raster with NaN under the 8-neighbourhood (the byte mask by torch, then the six launches), and
    remove_small_objects of a bool mask (label, sizes, keep), on shapes with ragged tiles"""
    lb = _lb()
    mask = lbn.random_mask((67, 131), 0.41, 13)
    X = np.where(mask, np.float32(np.nan), np.float32(0))
    want = ndi.label(mask, lbn.STRUCTURES[lbn.EIGHT])

    def label_ref(got):
        assert_labels((got[0], int(got[1])), want, "label")
    yield dict(name="label", fn=lambda Xt: lb.label(Xt, lbn.STRUCTURES[lbn.EIGHT]), inputs=[X], ctx=("label", "float32"),
               reference=label_ref)
    M = lbn.random_mask((130, 67), 0.59, 14)
    L, n = ndi.label(M)
    keep = lbn.kept(L, np.bincount(L.ravel(), minlength=n + 1), 6)

    def keep_ref(got):
        assert got.dtype == bool and np.array_equal(got, keep), "remove_small_objects"
    yield dict(name="remove_small_objects", fn=lambda Mt: lb.remove_small_objects(Mt, 6), inputs=[M], ctx=("keep", "bool"),
               reference=keep_ref)


def test_on_guarded_memory(gpu_device):
    from test_gpu_guarded import run_guarded
    for case in harness_cases():
        run_guarded(**case)


def test_on_a_side_stream(gpu_device):
    """every launch carries the current stream: the handles of smrf_label_* are recorded beside the shared header's"""
    import streamed as S
    from test_gpu_streams import streamed
    slots = dict(S.stream_slots(), **S.stream_slots(open(os.path.join(ROOT, "include", "smrf_label.h")).read()))
    assert (slots["smrf_label_u8"], slots["smrf_label_regions"], slots["smrf_label_keep"]) == (8, 6, 5)
    for case in harness_cases():
        streamed(case["fn"], case["inputs"], name=case["name"], ctx=case["ctx"], reference=case["reference"], slots=slots)
