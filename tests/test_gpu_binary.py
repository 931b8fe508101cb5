"""Binary morphology on the MI355X (neilpy_amd/binary.py, csrc/binary.hip, csrc/binary_bits.h):
erosion, dilation, opening, closing and hit-or-miss against scipy.ndimage on shapes of one word, at the word edge on both
sides and with ragged tails; the batch boundary of iterations < 1; propagation and fill_holes under all 16 symmetric
structures, through the components of the mask and by steps, on random and constructed masks; the input kinds;
repeatability; guarded memory and a side stream.  The oracle is SciPy on this machine and every comparison is exact.

SciPy is kept alive as in tests/test_binary_host.py: no origin outside the accepted range reaches it, and where a
structure is longer than the raster along an axis and SciPy iterates it is called with brute_force=True."""
import functools
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

import binary_numpy as bn
import label_numpy as lbn
from conftest import ROOT

pytestmark = pytest.mark.gpu

# one word, the word edge on both sides, ragged tails, several words and rows
SHAPES = ((1, 1), (1, 130), (130, 1), (17, 63), (17, 64), (17, 65), (65, 129), (200, 190))
LARGEST = ((65, 129), (200, 190))
MID = (2048, 2047)
DENSITIES = (0.1, 0.5, 0.9)


def _bm():
    from neilpy_amd import binary
    return binary


def drawn(shape, origin, seed):
    """a drawn structure of this shape, about 60 % members, with its centre at `origin` a member"""
    s = np.random.default_rng([20270311, seed] + list(shape)).random(shape) < 0.6
    s[shape[0] // 2 + origin[0], shape[1] // 2 + origin[1]] = True
    return s


# (structure, origin): the cross, 3 x 3 ones, 2 x 2, 4 x 3 at (-2, 1), 1 x 5 at (0, 2), 3 x 70 at (0, -20)
STRUCTURES = ((None, (0, 0)), (np.ones((3, 3), bool), (0, 0)), (np.ones((2, 2), bool), (0, 0)), (drawn((4, 3), (-2, 1), 1), (-2, 1)),
              (drawn((1, 5), (0, 2), 1), (0, 2)), (drawn((3, 70), (0, -20), 1), (0, -20)))
NINE = (drawn((9, 9), (0, 0), 1), (0, 0))


def brute(structure, shape, iterations):
    """whether SciPy has to take its brute-force path (module docstring)"""
    return structure is not None and iterations != 1 and (structure.shape[0] > shape[0] or structure.shape[1] > shape[1])


def assert_bits(got, want, ctx):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype == bool and got.shape == want.shape, (ctx, got.dtype, got.shape)
    assert np.array_equal(got, want), (ctx, int(np.sum(got != want)))


def check_erosion_and_dilation(shape, structures):
    bm = _bm()
    for p in DENSITIES:
        X, M = lbn.random_mask(shape, p, 21), lbn.random_mask(shape, 0.7, 22)
        for s, origin in structures:
            for border in (0, 1):
                for mask in (None, M):
                    for it in (1, 3, -1):
                        b = brute(s, shape, it)
                        ctx = (shape, p, None if s is None else s.shape, origin, border, mask is not None, it)
                        assert_bits(bm.binary_erosion(X, s, it, mask, None, border, origin),
                                    ndi.binary_erosion(X, s, it, mask, None, border, origin, b), ("erosion",) + ctx)
                        assert_bits(bm.binary_dilation(X, s, it, mask, None, border, origin),
                                    ndi.binary_dilation(X, s, it, mask, None, border, origin, b), ("dilation",) + ctx)


# ------------------------------------------------------------------------------------------
# erosion, dilation, opening, closing, hit or miss
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_erosion_and_dilation_against_scipy(gpu_device, shape):
    check_erosion_and_dilation(shape, STRUCTURES)


@pytest.mark.parametrize("shape", [(5, 7), (65, 129)], ids=lambda s: "%dx%d" % s)
def test_a_9_by_9_structure_against_scipy(gpu_device, shape):
    """larger than the 5 x 7 raster along both axes"""
    check_erosion_and_dilation(shape, (NINE,))


@pytest.mark.parametrize("shape", LARGEST, ids=lambda s: "%dx%d" % s)
def test_opening_and_closing_against_scipy(gpu_device, shape):
    bm = _bm()
    M = lbn.random_mask(shape, 0.7, 22)
    for p in DENSITIES:
        X = lbn.random_mask(shape, p, 23)
        for s, origin in STRUCTURES + (NINE,):
            for it in (1, 2):
                for border, mask in ((0, None), (1, None), (0, M), (1, M)):
                    ctx = (shape, p, None if s is None else s.shape, it, border, mask is not None)
                    b = brute(s, shape, it)
                    assert_bits(bm.binary_opening(X, s, it, None, origin, mask, border),
                                ndi.binary_opening(X, s, it, None, origin, mask, border, b), ("opening",) + ctx)
                    assert_bits(bm.binary_closing(X, s, it, None, origin, mask, border),
                                ndi.binary_closing(X, s, it, None, origin, mask, border, b), ("closing",) + ctx)
    assert_bits(bm.binary_opening(X), ndi.binary_opening(X), "defaults")
    assert_bits(bm.binary_closing(X), ndi.binary_closing(X), "defaults")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_hit_or_miss_against_scipy(gpu_device, shape):
    bm = _bm()
    two_three, four_one = drawn((2, 3), (0, 0), 2), drawn((4, 1), (-1, 0), 2)
    corner = np.array([[0, 1, 0], [1, 1, 0], [0, 0, 0]], bool)
    for p in DENSITIES:
        X = lbn.random_mask(shape, p, 24)
        assert_bits(bm.binary_hit_or_miss(X), ndi.binary_hit_or_miss(X), (shape, p, "defaults"))
        assert_bits(bm.binary_hit_or_miss(X, corner), ndi.binary_hit_or_miss(X, corner), (shape, p, "structure2 defaulted"))
        assert_bits(bm.binary_hit_or_miss(X, corner, origin1=(1, -1)), ndi.binary_hit_or_miss(X, corner, origin1=(1, -1)),
                    (shape, p, "origin2 defaulted"))
        miss = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1]], bool)
        assert_bits(bm.binary_hit_or_miss(X, corner, miss), ndi.binary_hit_or_miss(X, corner, miss), (shape, p, "structure2 given"))
        assert_bits(bm.binary_hit_or_miss(X, corner, miss, None, (0, 1), (-1, 0)),
                    ndi.binary_hit_or_miss(X, corner, miss, None, (0, 1), (-1, 0)), (shape, p, "both origins"))
        assert_bits(bm.binary_hit_or_miss(X, two_three, four_one, None, (-1, 1), (1, 0)),
                    ndi.binary_hit_or_miss(X, two_three, four_one, None, (-1, 1), (1, 0)), (shape, p, "2 x 3 against 4 x 1"))
        wide = drawn((3, 70), (0, -20), 1)
        assert_bits(bm.binary_hit_or_miss(X, wide & (np.arange(70) % 9 == 0), ~wide & (np.arange(70) % 11 == 0), None, (0, -20), (1, 30)),
                    ndi.binary_hit_or_miss(X, wide & (np.arange(70) % 9 == 0), ~wide & (np.arange(70) % 11 == 0), None, (0, -20), (1, 30)),
                    (shape, p, "3 x 70"))


def test_the_batch_boundary(gpu_device):
    """iterations=-1 on a full n x n square under 3 x 3 ones and border 0: a step peels one layer, so the steps end with
    the ceil(n / 2) + 1-th, the first that changes nothing.  n is chosen so that this is the last step of a batch, the
    step before it and the first of the next batch"""
    bm = _bm()
    every = bm.CHECK_EVERY
    ones = np.ones((3, 3), bool)
    for steps in (every - 1, every, every + 1, 2 * every, 2 * every + 1):
        for n in (2 * (steps - 1), 2 * (steps - 1) - 1):
            X = np.ones((n, n), bool)
            assert not bn.binary_erosion(X, ones, steps - 1).any() and bn.binary_erosion(X, ones, steps - 2).any()
            assert_bits(bm.binary_erosion(X, ones, -1), ndi.binary_erosion(X, ones, -1), (steps, n))
            Y = np.pad(X, 3)                                         # the square survives nowhere either way; a dilation back
            assert_bits(bm.binary_dilation(~Y, ones, -1, Y), ndi.binary_dilation(~Y, ones, -1, Y), (steps, n, "masked dilation"))
            for it in (steps - 2, steps - 1, steps, 5 * every):       # counted steps over the batch size, with early ends
                assert_bits(bm.binary_erosion(X, ones, it), ndi.binary_erosion(X, ones, it), (steps, n, it))


# ------------------------------------------------------------------------------------------
# propagation and fill_holes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LARGEST, ids=lambda s: "%dx%d" % s)
def test_propagation_and_fill_holes_against_scipy(gpu_device, shape):
    """all 16 structures, masks near the two percolation thresholds, sparse seeds inside and outside the mask, both
    border values; both routes"""
    bm = _bm()
    for p in (0.41, 0.59):
        M = lbn.random_mask(shape, p, 25)
        X = lbn.random_mask(shape, 0.001, 26)
        X[tuple(np.argwhere(~M)[3])] = True
        assert (X & ~M).any() and (X & M).any()
        for k in range(16):
            s = lbn.STRUCTURES[k]
            for border in (0, 1):
                want = ndi.binary_propagation(X, s, M, None, border)
                assert_bits(bm.binary_propagation(X, s, M, None, border), want, (shape, p, k, border))
                assert_bits(bm.binary_propagation(X, s, M, None, border, impl="labels"), want, (shape, p, k, border, "labels"))
                if k in (0, lbn.FOUR, lbn.EIGHT, lbn.SE):
                    assert_bits(bm.binary_propagation(X, s, M, None, border, impl="iterate"), want, (shape, p, k, border, "iterate"))
            want = ndi.binary_fill_holes(M, s)
            assert_bits(bm.binary_fill_holes(M, s), want, (shape, p, k, "fill_holes"))
            if k in (0, lbn.FOUR, lbn.EIGHT, lbn.SW):
                assert_bits(bm.binary_fill_holes(M, s, impl="iterate"), want, (shape, p, k, "fill_holes", "iterate"))
        assert_bits(bm.binary_propagation(X, mask=M), ndi.binary_propagation(X, mask=M), (shape, p, "default structure"))
        assert_bits(bm.binary_propagation(X), ndi.binary_propagation(X), (shape, p, "no mask"))
        assert_bits(bm.binary_fill_holes(M), ndi.binary_fill_holes(M), (shape, p, "default structure"))


def seeds_of(shape):
    seed = np.zeros(shape, bool)
    seed[0, 0] = seed[shape[0] // 2, shape[1] // 2] = seed[-1, -2] = True
    return seed


ASYMMETRIC = np.array([[0, 1, 0], [1, 1, 0], [0, 0, 1]], bool)


def test_constructed_masks_through_the_labels(gpu_device):
    """257 x 257: a serpentine whose path is some 33 000 cells long, a spiral, a comb, a frame, a checkerboard - the label
    route does not iterate"""
    bm = _bm()
    shape = (257, 257)
    seed = seeds_of(shape)
    for name, mask in lbn.constructed(shape).items():
        for k in (lbn.FOUR, lbn.EIGHT):
            s = lbn.STRUCTURES[k]
            for border in (0, 1):
                assert_bits(bm.binary_propagation(seed, s, mask, None, border, impl="labels"),
                            ndi.binary_propagation(seed, s, mask, None, border), (name, k, border))
            assert_bits(bm.binary_fill_holes(mask, s, impl="labels"), ndi.binary_fill_holes(mask, s), (name, k, "fill_holes"))
        assert_bits(bm.binary_propagation(seed, lbn.STRUCTURES[lbn.EIGHT], mask), ndi.binary_propagation(seed, lbn.STRUCTURES[lbn.EIGHT], mask),
                    (name, "impl=None"))


def test_constructed_masks_by_steps(gpu_device):
    """21 x 26: the same masks by steps in batches, and an asymmetric structure, which impl=None sends there"""
    bm = _bm()
    shape = (21, 26)
    seed = seeds_of(shape)
    for name, mask in lbn.constructed(shape).items():
        for s in (lbn.STRUCTURES[lbn.FOUR], lbn.STRUCTURES[lbn.EIGHT]):
            assert_bits(bm.binary_propagation(seed, s, mask, impl="iterate"), ndi.binary_propagation(seed, s, mask), (name, "iterate"))
            assert_bits(bm.binary_fill_holes(mask, s, impl="iterate"), ndi.binary_fill_holes(mask, s), (name, "fill_holes", "iterate"))
        assert_bits(bm.binary_propagation(seed, lbn.STRUCTURES[lbn.EIGHT], mask), ndi.binary_propagation(seed, lbn.STRUCTURES[lbn.EIGHT], mask),
                    (name, "8-connected"))
        assert_bits(bm.binary_propagation(seed, ASYMMETRIC, mask), ndi.binary_propagation(seed, ASYMMETRIC, mask), (name, "asymmetric"))
        assert_bits(bm.binary_fill_holes(mask, ASYMMETRIC), ndi.binary_fill_holes(mask, ASYMMETRIC), (name, "asymmetric", "fill_holes"))
        assert_bits(bm.binary_propagation(seed, lbn.STRUCTURES[lbn.FOUR], mask, origin=(0, 1)),
                    ndi.binary_propagation(seed, lbn.STRUCTURES[lbn.FOUR], mask, origin=(0, 1)), (name, "origin"))


@functools.lru_cache(maxsize=None)
def mid_case():
    """the mid-size mask at the 4-connected percolation threshold and SciPy's results on it, computed once"""
    mask = lbn.random_mask(MID, 0.59, 7)
    zeros = np.zeros(MID, bool)
    return (mask, ndi.binary_fill_holes(mask), ndi.binary_propagation(zeros, None, mask, None, 1),
            ndi.binary_opening(mask, None, 2))


def test_mid_size_against_scipy(gpu_device):
    bm = _bm()
    mask, filled, from_border, opened = mid_case()
    assert_bits(bm.binary_fill_holes(mask), filled, (MID, "fill_holes"))
    assert_bits(bm.binary_propagation(np.zeros(MID, bool), None, mask, None, 1), from_border, (MID, "propagation from the border"))
    assert_bits(bm.binary_opening(mask, None, 2), opened, (MID, "opening"))
    assert filled.sum() > mask.sum() and 0 < from_border.sum() < mask.sum() and 0 < opened.sum() < mask.sum()


# ------------------------------------------------------------------------------------------
# input kinds, repeatability
# ------------------------------------------------------------------------------------------
def _host(v):
    return v if isinstance(v, np.ndarray) else v.cpu().numpy()


def test_input_kinds(gpu_device):
    """bool, uint8, int32, float32 with NaN and -0.0, float64: the same bits; tensor in, tensor out; views; the input
    unchanged; empty rasters"""
    import torch
    bm = _bm()
    shape = (65, 129)
    mask = lbn.random_mask(shape, 0.59, 11)
    M = lbn.random_mask(shape, 0.7, 12)
    s = drawn((4, 3), (-2, 1), 1)
    calls = {"dilation": (lambda X, Mk: bm.binary_dilation(X, s, 2, Mk, None, 1, (-2, 1)), ndi.binary_dilation(mask, s, 2, M, None, 1, (-2, 1))),
             "fill_holes": (lambda X, Mk: bm.binary_fill_holes(X), ndi.binary_fill_holes(mask)),
             "propagation": (lambda X, Mk: bm.binary_propagation(Mk, None, X), ndi.binary_propagation(M, None, mask)),
             "hit_or_miss": (lambda X, Mk: bm.binary_hit_or_miss(X, s, None, None, (-2, 1)), ndi.binary_hit_or_miss(mask, s, None, None, (-2, 1)))}
    rng = np.random.default_rng(20270312)
    f32 = np.where(mask, rng.normal(size=shape), 0.0).astype(np.float32)
    f32[mask & (rng.random(shape) < 0.2)] = np.nan
    f32[~mask & (rng.random(shape) < 0.5)] = -0.0
    assert np.isnan(f32).any() and np.signbit(f32[f32 == 0]).any()
    kinds = {"bool": mask, "uint8": mask.astype(np.uint8) * 200, "int32": np.where(mask, -5, 0).astype(np.int32), "float32": f32,
             "float64": f32.astype(np.float64), "int64": mask.astype(np.int64) << 40, "uint16": mask.astype(np.uint16)}
    for name, X in kinds.items():
        assert np.array_equal(X != 0, mask)
        for what, (call, want) in calls.items():
            keep = X.copy()
            assert_bits(call(X, M), want, (what, name))
            assert keep.tobytes() == X.tobytes(), (what, name)
            if name == "uint16":
                continue
            Xt, Mt = torch.from_numpy(X).to(gpu_device), torch.from_numpy(M).to(gpu_device)
            before = Xt.clone()
            got = call(Xt, Mt)
            assert isinstance(got, torch.Tensor) and got.device == Xt.device and got.dtype == torch.bool, (what, name)
            assert_bits(_host(got), want, (what, name, "tensor"))
            assert torch.equal(Xt.view(torch.uint8), before.view(torch.uint8)), (what, name)
            assert_bits(_host(call(X, Mt)), want, (what, name, "a host raster with a device mask"))
            # a transposed and an offset-strided view: the contiguous call's bits
            base = torch.from_numpy(np.ascontiguousarray(X.T)).to(gpu_device)
            assert_bits(_host(call(base.T, Mt)), want, (what, name, "transposed"))
            wide = torch.ones((shape[0] + 3, 2 * shape[1] + 5), dtype=Xt.dtype, device=gpu_device)
            view = wide[2:2 + shape[0], 3:3 + 2 * shape[1]:2]
            view.copy_(Xt)
            assert not view.is_contiguous()
            assert_bits(_host(call(view, Mt)), want, (what, name, "strided"))
            rows = torch.ones((shape[0] + 3, shape[1]), dtype=Xt.dtype, device=gpu_device)[3:]      # contiguous at an odd address
            rows.copy_(Xt)
            assert rows.is_contiguous() and (rows.data_ptr() % 4 != 0 or Xt.element_size() > 1)
            assert_bits(_host(call(rows, Mt)), want, (what, name, "offset"))
    assert_bits(bm.binary_dilation(np.asfortranarray(f32), s, 2, M, None, 1, (-2, 1)), calls["dilation"][1], "host order")
    assert_bits(bm.binary_fill_holes(mask.tolist()), calls["fill_holes"][1], "a list")
    for empty in ((0, 5), (4, 0), (0, 0)):
        for name in bm.__all__:
            got = getattr(bm, name)(torch.zeros(empty, dtype=torch.float32, device=gpu_device))
            assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == empty and got.dtype == torch.bool
            got = getattr(bm, name)(np.zeros(empty, bool))
            assert isinstance(got, np.ndarray) and got.shape == empty and got.dtype == bool


def test_the_same_on_every_run(gpu_device):
    """three calls each: the order in which the mark pass's stores and the flag's atomics land does not reach the bits"""
    import torch
    bm = _bm()
    mask, filled, from_border, opened = mid_case()
    Mt = torch.from_numpy(mask).to(gpu_device)
    Zt = torch.zeros(MID, dtype=torch.bool, device=gpu_device)
    small = torch.from_numpy(lbn.random_mask((200, 190), 0.59, 25)).to(gpu_device)
    for call, want in ((lambda: bm.binary_fill_holes(Mt), filled), (lambda: bm.binary_propagation(Zt, None, Mt, None, 1), from_border),
                       (lambda: bm.binary_opening(Mt, None, 2), opened),
                       (lambda: bm.binary_fill_holes(small, impl="iterate"), ndi.binary_fill_holes(small.cpu().numpy()))):
        runs = [call() for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
        assert np.array_equal(runs[0].cpu().numpy(), want)


# ------------------------------------------------------------------------------------------
# guarded memory and a side stream, on cases built here
# ------------------------------------------------------------------------------------------
def harness_cases():
    """a masked dilation of a float32 raster with NaN under a 4 x 3 structure, iterated until nothing changes (the byte
    masks by torch, two packs, the steps in batches with their flags, unpack), and fill_holes of a bool mask (the
    complement by torch, then smrf_binary_propagate), on shapes with ragged words"""
    bm = _bm()
    s, origin = drawn((4, 3), (-2, 1), 1), (-2, 1)
    seeds, M = lbn.random_mask((67, 131), 0.02, 13), lbn.random_mask((67, 131), 0.7, 14)
    X = np.where(seeds, np.float32(np.nan), np.float32(0))
    want = ndi.binary_dilation(seeds, s, -1, M, None, 0, origin)

    def dilation_ref(got):
        assert_bits(got, want, "masked dilation")
    yield dict(name="binary_dilation", fn=lambda Xt, Mt: bm.binary_dilation(Xt, s, -1, Mt, None, 0, origin), inputs=[X, M],
               ctx=("dilation", "float32"), reference=dilation_ref)
    H = lbn.random_mask((130, 67), 0.59, 15)
    filled = ndi.binary_fill_holes(H)

    def fill_ref(got):
        assert_bits(got, filled, "fill_holes")
    yield dict(name="binary_fill_holes", fn=lambda Ht: bm.binary_fill_holes(Ht), inputs=[H], ctx=("fill_holes", "bool"),
               reference=fill_ref)


def test_on_guarded_memory(gpu_device):
    from test_gpu_guarded import run_guarded
    for case in harness_cases():
        run_guarded(**case)


def test_on_a_side_stream(gpu_device):
    """every launch carries the current stream: the handles of smrf_binary_* are recorded beside the shared header's"""
    import streamed as S
    from test_gpu_streams import streamed
    slots = dict(S.stream_slots(), **S.stream_slots(open(os.path.join(ROOT, "include", "smrf_binary.h")).read()))
    assert (slots["smrf_binary_pack"], slots["smrf_binary_unpack"], slots["smrf_binary_step"], slots["smrf_binary_hit_or_miss"],
            slots["smrf_binary_propagate"]) == (5, 5, 10, 8, 10)
    for case in harness_cases():
        streamed(case["fn"], case["inputs"], name=case["name"], ctx=case["ctx"], reference=case["reference"], slots=slots)
