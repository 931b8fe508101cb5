"""Connected components without a GPU (neilpy_amd/label.py, csrc/label.hip, csrc/label_runs.h): the
restatement tests/label_numpy.py against scipy.ndimage.label, np.bincount and scipy.ndimage.find_objects, the host logic
behind the C ABI of include/smrf_label.h, the bit logic and the union-find of label_runs.h compiled with g++ under the
address and undefined-behaviour sanitizers, and the argument refusals.  Every comparison is exact."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.ndimage as ndi

import label_numpy as lbn
from conftest import ROOT

E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -5
NAMES = ("label", "region_sizes", "bounding_boxes", "find_objects", "remove_small_objects")
SMALL_SHAPES = ((1, 1), (1, 9), (9, 1), (5, 7), (12, 13))
DENSITIES = (0.1, 0.41, 0.59, 0.95)


def _lb():
    from neilpy_amd import label
    return label


def cases():
    """(name, mask, structures to run it under)"""
    for shape in SMALL_SHAPES:
        for p in DENSITIES:
            yield ("random p=%g" % p, shape), lbn.random_mask(shape, p, 1), range(16)
    for shape in ((9, 11), (21, 26)):
        for name, mask in lbn.constructed(shape).items():
            yield (name, shape), mask, (lbn.FOUR, lbn.EIGHT, lbn.SE, lbn.SW | lbn.E)


# ------------------------------------------------------------------------------------------
# the restatement against SciPy
# ------------------------------------------------------------------------------------------
def test_restatement_equals_scipy():
    compared = 0
    for ctx, mask, structures in cases():
        for k in structures:
            want, n = ndi.label(mask, lbn.STRUCTURES[k])
            got, m = lbn.label(mask, lbn.STRUCTURES[k])
            assert m == n and got.dtype == want.dtype == np.int32 and np.array_equal(got, want), (ctx, k)
            assert np.array_equal(lbn.region_sizes(got, n), np.bincount(want.ravel(), minlength=n + 1)), (ctx, k)
            assert lbn.find_objects(got) == ndi.find_objects(want), (ctx, k)
            boxes = lbn.bounding_boxes(got, n)
            assert boxes.shape == (n, 4) and [tuple(b) for b in boxes] == [
                (s[0].start, s[0].stop, s[1].start, s[1].stop) for s in ndi.find_objects(want)], (ctx, k)
            compared += 1
    assert compared >= 400, compared
    # the default structure is the 4-neighbourhood, and the numbering case is what its docstring says
    U = lbn.u_and_speck((9, 11))
    assert np.array_equal(lbn.label(U)[0], ndi.label(U)[0])
    L, n = lbn.label(U)
    assert n == 2 and L[0, 8] == L[2, 2] == 1 and L[1, 5] == 2


def test_restatement_equals_scipy_on_the_structured_masks():
    """blobs, strokes, rings and the maze: a row, a column and a raster each, and what their docstrings promise"""
    compared = 0
    for name, make in lbn.GENERATORS.items():
        for shape in ((1, 1), (1, 37), (41, 1), (2, 2), (23, 38)):
            for seed in (1, 2):
                mask = make(shape, seed)
                assert mask.dtype == bool and mask.shape == shape, (name, shape)
                assert np.array_equal(mask, make(shape, seed)), (name, shape, "the same mask from the same seed")
                for k in (lbn.FOUR, lbn.EIGHT, lbn.E | lbn.S | lbn.SE, lbn.S | lbn.SW, 0):
                    want, n = ndi.label(mask, lbn.STRUCTURES[k])
                    got, m = lbn.label(mask, lbn.STRUCTURES[k])
                    assert m == n and np.array_equal(got, want), (name, shape, seed, k)
                    compared += 1
    assert compared == 200
    for seed in (1, 2, 3):
        M = lbn.maze((65, 130), seed)
        assert ndi.label(M)[1] == 1 and M[::2, ::2].all() and not M[1::2, 1::2].any()
        assert M.sum() == 2 * 33 * 65 - 1                                  # a tree: one passage less than cells
        B = lbn.blobs((65, 130), seed)
        holes = ndi.label(~B)[1]
        assert 0.4 < B.mean() < 0.6 and 2 <= ndi.label(B)[1] < 200 and holes >= 2
        R = lbn.rings((65, 130), seed)
        assert ndi.label(R, lbn.STRUCTURES[lbn.EIGHT])[1] >= 3
        assert 0.02 < lbn.strokes((65, 130), seed).mean() < 0.9


def test_restatement_on_the_hand_made_labels():
    H = lbn.HAND
    for max_label in (0, 1, 5, 7, 9, 45):
        assert lbn.find_objects(H, max_label) == ndi.find_objects(H, max_label), max_label
    assert lbn.find_objects(np.zeros((3, 4), np.int32)) == ndi.find_objects(np.zeros((3, 4), np.int32)) == []
    pos = np.where((H >= 0) & (H <= 7), H, 0)
    assert np.array_equal(lbn.region_sizes(H, 7)[1:], np.bincount(pos.ravel(), minlength=8)[1:])
    assert lbn.region_sizes(H, 7)[0] == np.count_nonzero(H == 0)


def test_restatement_of_remove_small_objects():
    for ctx, mask, _ in cases():
        for connectivity, k in ((1, lbn.FOUR), (2, lbn.EIGHT)):
            L, n = ndi.label(mask, lbn.STRUCTURES[k])
            sizes = np.bincount(L.ravel(), minlength=n + 1)
            for min_size in (1, 2, int(np.median(sizes[1:])) if n else 3):
                want = np.isin(L, np.flatnonzero(sizes[1:] >= min_size) + 1)
                assert np.array_equal(want, lbn.kept(L, sizes, min_size))
                if sizes[0] >= min_size:
                    assert np.array_equal(want, np.isin(L, np.flatnonzero(sizes >= min_size)[1:]))
                assert np.array_equal(lbn.remove_small_objects(mask, min_size, connectivity), want), (ctx, connectivity, min_size)


# ------------------------------------------------------------------------------------------
# the C ABI, host side
# ------------------------------------------------------------------------------------------
def _scipy_refusal(structure):
    """the exception type scipy.ndimage.label raises for this structure on a 2-D raster, or None"""
    try:
        ndi.label(np.ones((2, 2), np.uint8), structure)
    except Exception as e:                                  # noqa: BLE001: the type is what is asked for
        return type(e)
    return None


def test_links_accepts_exactly_what_scipy_accepts():
    lib = _lb()._library()
    accepted = 0
    for bits in range(512):
        s = np.array([(bits >> k) & 1 for k in range(9)], dtype=np.uint8)
        got = lib.smrf_label_links(s.ctypes.data_as(C.c_void_p))
        refused = _scipy_refusal(s.reshape(3, 3))
        if refused is None:
            accepted += 1
            assert got == lbn.links_of(s.reshape(3, 3)), (bits, got)
            # the link mask names the same structure up to the centre, which SciPy ignores as well
            want = lbn.structure_of(got)
            want[1, 1] = s[4]
            assert np.array_equal(want, s.reshape(3, 3).astype(bool)), bits
        else:
            assert got == E_ARG, (bits, got)
    assert accepted == 32                                   # 16 structures, with and without the centre
    big = (np.arange(9) % 2 * 200).astype(np.uint8)         # any non-zero byte is a member
    assert lib.smrf_label_links(big.ctypes.data_as(C.c_void_p)) == lbn.FOUR
    assert lib.smrf_label_links(C.c_void_p(0)) == E_ARG
    centre = np.ones((3, 3), bool)
    centre[1, 1] = False
    assert np.array_equal(ndi.label(lbn.random_mask((9, 9), 0.5, 3), centre)[0],
                          ndi.label(lbn.random_mask((9, 9), 0.5, 3), np.ones((3, 3)))[0])


def test_workspace_bytes_is_the_documented_formula():
    lb = _lb()
    lib = lb._library()
    up = lambda b: (b + 255) // 256 * 256                   # noqa: E731
    for rows, cols in ((1, 1), (1, 63), (64, 64), (65, 129), (2048, 2047), (2048, 1), (1, 2049), (16384, 16384), (46340, 46340),
                       (1, 2 ** 31 - 1)):
        cells = rows * cols
        want = up(4 * cells) + up(4 * -(-cells // lb.SCAN_BLOCK))
        assert lib.smrf_label_workspace_bytes(rows, cols) == lb.workspace_bytes(rows, cols) == want, (rows, cols)
        assert want <= 4 * cells + 4 * (cells // lb.SCAN_BLOCK + 1) + 510           # one int32 plane plus the block sums
    for rows, cols in ((0, 5), (5, 0), (0, 0)):
        assert lib.smrf_label_workspace_bytes(rows, cols) == lb.workspace_bytes(rows, cols) == 0
    assert lib.smrf_label_workspace_bytes(-1, 5) == E_ARG
    assert lib.smrf_label_workspace_bytes(46341, 46341) == E_UNSUPPORTED
    assert lib.smrf_label_workspace_bytes(1, 2 ** 31 - 1) > 0 and lib.smrf_label_workspace_bytes(2, 2 ** 30) == E_UNSUPPORTED


def test_header_library_and_bindings_agree():
    """every name include/smrf_label.h declares is exported and bound in label.py with the declaration's arity; nothing of
    it sits in the shared header, the shared signature table or the package's namespace"""
    import streamed as S
    import neilpy_amd
    from neilpy_amd import _lib
    lb = _lb()
    text = open(os.path.join(ROOT, "include", "smrf_label.h")).read()
    decl = S.declarations(text)
    assert set(decl) == set(lb.SIGNATURES) == {"smrf_label_" + n for n in ("links", "workspace_bytes", "u8", "regions", "keep")}
    lib = lb._library()
    for name, params in decl.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(params) == len(lb.SIGNATURES[name][1]), name
    slots = S.stream_slots(text)
    assert slots == {"smrf_label_links": None, "smrf_label_workspace_bytes": None, "smrf_label_u8": 8,
                     "smrf_label_regions": 6, "smrf_label_keep": 5}
    for name, slot in slots.items():
        if slot is not None:
            assert slot == len(decl[name]) - 1 and lb.SIGNATURES[name][1][slot] is C.c_void_p
    assert not [n for n in _lib.SIGNATURES if "label" in n] and not [n for n in S.declarations() if "label" in n]
    assert inspect.ismodule(neilpy_amd.label) and not set(NAMES[1:]) & set(dir(neilpy_amd)), "the family is not re-exported"
    macro = lambda n: int(re.search(r"#define SMRF_LABEL_%s (\d+)" % n, text).group(1))          # noqa: E731
    assert (lb.LINK_E, lb.LINK_S, lb.LINK_SE, lb.LINK_SW) == tuple(macro(n) for n in ("E", "S", "SE", "SW")) == (
        lbn.E, lbn.S, lbn.SE, lbn.SW)
    assert (lb.TILE_ROWS, lb.TILE_COLS, lb.SCAN_BLOCK) == (macro("TILE_ROWS"), macro("TILE_COLS"), macro("SCAN_BLOCK"))
    runs = open(os.path.join(ROOT, "neilpy_amd", "csrc", "label_runs.h")).read()
    assert re.search(r"SMRF_LINK_E = 1, SMRF_LINK_S = 2, SMRF_LINK_SE = 4, SMRF_LINK_SW = 8", runs)


def test_abi_argument_errors():
    """refusals by status code, before any launch and so without a GPU"""
    lib = _lb()._library()
    p, null = C.c_void_p(4096), C.c_void_p(0)                        # never dereferenced: every call is refused first
    big = 1 << 40
    assert lib.smrf_label_u8(p, p, -1, 5, 3, p, big, p, null) == E_ARG
    assert lib.smrf_label_u8(p, p, 46341, 46341, 3, p, big, p, null) == E_UNSUPPORTED
    for links in (-1, 16):
        assert lib.smrf_label_u8(p, p, 5, 5, links, p, big, p, null) == E_ARG
    assert lib.smrf_label_u8(p, p, 5, 5, 3, p, big, null, null) == E_ARG
    assert lib.smrf_label_u8(null, p, 5, 5, 3, p, big, p, null) == E_ARG
    assert lib.smrf_label_u8(p, null, 5, 5, 3, p, big, p, null) == E_ARG
    assert lib.smrf_label_u8(p, p, 5, 5, 3, null, big, p, null) == E_WORKSPACE
    assert lib.smrf_label_u8(p, p, 5, 5, 3, p, lib.smrf_label_workspace_bytes(5, 5) - 1, p, null) == E_WORKSPACE
    assert lib.smrf_label_regions(p, -1, 5, 3, p, p, null) == E_ARG
    assert lib.smrf_label_regions(p, 5, 5, -1, p, p, null) == E_ARG
    assert lib.smrf_label_regions(p, 5, 5, 3, null, null, null) == E_ARG
    assert lib.smrf_label_regions(null, 5, 5, 3, p, p, null) == E_ARG
    assert lib.smrf_label_regions(p, 2, 2 ** 30, 3, p, p, null) == E_UNSUPPORTED
    assert lib.smrf_label_keep(p, p, -1, 1, p, null) == E_ARG
    assert lib.smrf_label_keep(p, p, 0, 1, p, null) == 0                                # nothing launched
    for bad in ((null, p, p), (p, null, p), (p, p, null)):
        assert lib.smrf_label_keep(bad[0], bad[1], 5, 1, bad[2], null) == E_ARG


def test_kernels_compile_without_scratch(tmp_path):
    """csrc/label.hip for gfx950: the six phases of label, the three region kernels and the keep pass, all in registers"""
    import family_checks as fc
    text, kernels = fc.device_asm("label", tmp_path)
    for stem in ("label_tile", "label_seam", "label_flatten", "label_scan", "label_number", "label_relabel", "regions_clear",
                 "regions_kernel", "regions_close", "keep_kernel"):
        assert len([k for k in kernels if stem in k]) == 1, (stem, sorted(kernels))
    assert len(kernels) == 10
    fc.assert_no_scratch(text, kernels)


# ------------------------------------------------------------------------------------------
# csrc/label_runs.h on the CPU
# ------------------------------------------------------------------------------------------
_RUNS_CPP = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "label_runs.h"

// a tile of up to 64 x 64 cells labelled the way csrc/label.hip's tile pass does it, one "lane" after the other
static void label_tile(const std::vector<uint64_t>& rows, int cols, int links) {
  const int n = (int)rows.size();
  std::vector<int> par(n * 64, -7);                     // only a run's first cell is ever read
  auto load = [&](int i) { if (par[i] < 0) std::abort(); return par[i]; };
  auto lower = [&](int i, int v) { const int old = par[i]; if (v < old) par[i] = v; return old; };
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < cols; ++c)
      if (smrf_run_starts(rows[r], links) >> c & 1) par[r * 64 + c] = r * 64 + c;
  for (int r = 1; r < n; ++r)
    for (int c = 0; c < cols; ++c)
      if (rows[r] >> c & 1) {
        const int mine = r * 64 + smrf_run_start_of(smrf_run_starts(rows[r], links), c);
        const uint64_t up_starts = smrf_run_starts(rows[r - 1], links);
        smrf_row_links(rows[r - 1], rows[r], c, links, [&](int cu) {
          if (cu < 0 || cu >= cols) std::abort();
          smrf_unite_min(mine, (r - 1) * 64 + smrf_run_start_of(up_starts, cu), load, lower);
        });
      }
  for (int r = 0; r < n; ++r) {
    for (int c = 0; c < cols; ++c) {
      int v = -1;
      if (rows[r] >> c & 1) {
        const int root = smrf_find_root(r * 64 + smrf_run_start_of(smrf_run_starts(rows[r], links), c), load);
        v = (root / 64) * cols + root % 64;
      }
      std::printf("%d ", v);
    }
  }
  std::printf("\n");
}

// stdin: cases of "rows cols links" followed by one hexadecimal row mask per row; stdout: per case the root of every cell
int main() {
  int n, cols, links;
  while (std::scanf("%d %d %d", &n, &cols, &links) == 3) {
    std::vector<uint64_t> rows(n);
    for (auto& m : rows) {
      unsigned long long v;
      if (std::scanf("%llx", &v) != 1) return 2;
      m = v;
    }
    label_tile(rows, cols, links);
  }
  unsigned char s[9] = {1, 0, 0, 0, 0, 0, 0, 0, 1}, t[9] = {1, 0, 0, 0, 1, 0, 0, 0, 0};
  std::printf("%d %d\n", smrf_links_of(s), smrf_links_of(t));
  return 0;
}
'''


def test_label_runs_header_on_the_cpu(tmp_path):
    """csrc/label_runs.h compiled with g++ -fsanitize=address,undefined into a stand-alone program that labels tiles with
    the tile pass's own text - run starts, the links between adjacent rows, the union-find to the minimum - on random and
    constructed masks up to 64 x 64 under all 16 structures: every root is its object's first cell, and the roots
    numbered by rank are scipy.ndimage.label's labels"""
    src = tmp_path / "runs.cpp"
    src.write_text(_RUNS_CPP)
    exe = tmp_path / "runs"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "neilpy_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    masks = []
    for shape in ((1, 1), (1, 64), (64, 1), (7, 63), (17, 64), (64, 64), (33, 20)):
        for p in DENSITIES:
            masks.append(lbn.random_mask(shape, p, 2))
    for shape in ((64, 64), (31, 64), (20, 17)):
        masks.extend(lbn.constructed(shape).values())
    todo, lines = [], []
    for mask in masks:
        for links in range(16):
            todo.append((mask, links))
            lines.append("%d %d %d" % (mask.shape[0], mask.shape[1], links))
            lines.extend("%x" % sum(1 << c for c in np.flatnonzero(row)) for row in mask)
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    got = out.stdout.strip().split("\n")
    assert len(got) == len(todo) + 1 and got[-1].split() == [str(lbn.SE), "-1"]
    for (mask, links), line in zip(todo, got):
        root = np.array(line.split(), dtype=np.int64).reshape(mask.shape)
        want, n = ndi.label(mask, lbn.STRUCTURES[links])
        L, m = lbn.number(root)
        assert m == n and np.array_equal(L, want), (mask.shape, links)
        assert np.array_equal(root, lbn.roots(mask, links)), (mask.shape, links)


# ------------------------------------------------------------------------------------------
# the interface
# ------------------------------------------------------------------------------------------
def test_signatures_are_scipys():
    lb = _lb()
    for name in ("label", "find_objects"):
        want = list(inspect.signature(getattr(ndi, name)).parameters.values())
        got = list(inspect.signature(getattr(lb, name)).parameters.values())
        assert [(g.name, g.kind, g.default) for g in got] == [(w.name, w.kind, w.default) for w in want], name
    assert [(p.name, p.default) for p in inspect.signature(lb.remove_small_objects).parameters.values()] == [
        ("mask", inspect.Parameter.empty), ("min_size", 64), ("connectivity", 1)]
    for name in ("region_sizes", "bounding_boxes"):
        assert [(p.name, p.default) for p in inspect.signature(getattr(lb, name)).parameters.values()] == [
            ("labels", inspect.Parameter.empty), ("num_features", None)]
    assert sorted(lb.__all__) == sorted(NAMES)


def test_argument_errors_come_from_the_host():
    """every refusal is decided before the device is touched: it is the same with and without a GPU.  The exception types of
    label are scipy.ndimage.label's own, taken from it here"""
    lb = _lb()
    X = np.zeros((4, 5), np.uint8)
    asym = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]])
    for bad in (asym, np.ones((3, 3, 3)), np.ones(3), np.ones((3, 5)), np.ones((2, 2)), np.ones((5, 5)),
                np.array([[0, 1, 0], [1, 1, 0], [0, 1, 0]])):
        want = _scipy_refusal(bad)
        assert want is not None
        with pytest.raises(want) as info:
            lb.label(X, bad)
        assert info.type is want, (bad, info.type, want)
    with pytest.raises(type(_complex_refusal())):
        lb.label(np.zeros((4, 5), np.complex64))
    for output in (np.int64, np.uint8, "float32", np.empty((4, 5), np.int32), 7):
        with pytest.raises(NotImplementedError):
            lb.label(X, output=output)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(2 ** 16, 2 ** 15), strides=(0, 0))
    for name, lead in (("label", ()), ("region_sizes", ()), ("bounding_boxes", ()), ("find_objects", ()), ("remove_small_objects", ())):
        f = getattr(lb, name)
        for Y in (np.zeros((2, 3, 4), np.uint8), np.zeros(5, np.uint8), np.uint8(1)):
            with pytest.raises(NotImplementedError):
                f(Y, *lead)                                                 # not a 2-D raster
        with pytest.raises(NotImplementedError):
            f(big)                                                          # 2**31 cells
    for name in ("region_sizes", "bounding_boxes", "find_objects"):
        for Y in (np.zeros((4, 5)), np.zeros((4, 5), np.float32)):
            with pytest.raises(TypeError):
                getattr(lb, name)(Y)
    with pytest.raises(TypeError):
        ndi.find_objects(np.zeros((4, 5)))                                  # as SciPy
    for name in ("region_sizes", "bounding_boxes"):
        with pytest.raises(ValueError):
            getattr(lb, name)(X, -1)
        with pytest.raises(TypeError):
            getattr(lb, name)(X, 2.5)
    with pytest.raises(TypeError):
        lb.find_objects(X, 2.5)
    with pytest.raises(ValueError):
        lb.find_objects(np.zeros((0, 5), np.int32))                         # SciPy: no maximum of an empty raster
    with pytest.raises(ValueError):
        ndi.find_objects(np.zeros((0, 5), np.int32))
    for kw in (dict(min_size=-1), dict(connectivity=0), dict(connectivity=3)):
        with pytest.raises(ValueError):
            lb.remove_small_objects(X, **kw)
    with pytest.raises(TypeError):
        lb.remove_small_objects(X, min_size=2.5)


def _complex_refusal():
    try:
        ndi.label(np.zeros((4, 5), np.complex64))
    except Exception as e:                                  # noqa: BLE001
        return e
    raise AssertionError("SciPy labels complex input")


def test_empty_rasters_need_no_device():
    lb = _lb()
    for shape in ((0, 5), (4, 0), (0, 0)):
        L, n = lb.label(np.zeros(shape, np.float32))
        want, m = ndi.label(np.zeros(shape, np.float32))
        assert n == m == 0 and L.shape == want.shape == shape and L.dtype == want.dtype == np.int32
        assert lb.region_sizes(L).tolist() == [0] and lb.region_sizes(L).dtype == np.int64
        assert lb.region_sizes(L, 2).tolist() == [0, 0, 0]
        assert lb.bounding_boxes(L).shape == (0, 4) and lb.bounding_boxes(L, 2).tolist() == [[0, 0, 0, 0]] * 2
        assert lb.find_objects(L, 2) == ndi.find_objects(want, 2) == [None, None]
        keep = lb.remove_small_objects(np.zeros(shape, bool))
        assert keep.shape == shape and keep.dtype == bool


def test_valid_call_without_a_gpu_raises():
    import torch
    import neilpy_amd
    lb = _lb()
    if torch.cuda.is_available():
        return                                                 # tests/test_gpu_label.py runs the valid calls
    X = np.ones((4, 5), np.uint8)
    for call in (lambda: lb.label(X), lambda: lb.label(X.astype(np.float64), np.ones((3, 3))), lambda: lb.region_sizes(X),
                 lambda: lb.bounding_boxes(X, 1), lambda: lb.find_objects(X), lambda: lb.remove_small_objects(X, 2, 2)):
        with pytest.raises(neilpy_amd.SmrfHipError):
            call()
