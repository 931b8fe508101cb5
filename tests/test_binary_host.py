"""Binary morphology without a GPU (neilpy_amd/binary.py, csrc/binary.hip, csrc/binary_bits.h): the
restatement tests/binary_numpy.py against scipy.ndimage's binary_* functions, the propagation identity against
binary_propagation and binary_fill_holes, the host logic behind the C ABI of include/smrf_binary.h, the step of
binary_bits.h compiled with g++ under the address and undefined-behaviour sanitizers, and the argument refusals.  Every
comparison is exact.

Two rules keep SciPy itself alive here.  No origin outside -(n // 2) <= origin <= (n - 1) // 2 is ever handed to it: it
reads out of bounds there.  And where a structure is longer than the raster along an axis, SciPy is called with
brute_force=True whenever it iterates: its other path (the coordinate list of NI_BinaryErosion2) corrupts the heap on
such structures in SciPy 1.15 - a masked binary_dilation of a 6 x 6, 3 x 70 or 9 x 9 structure on a 5 x 7 raster with
iterations=2 ends in "double free or corruption" - and gives other bits than its own brute-force path, which is the loop
of steps SciPy documents.  Where the structure fits the raster both paths are compared."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.ndimage as ndi

import binary_numpy as bn
import label_numpy as lbn
from conftest import ROOT

E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -5
NAMES = ("binary_erosion", "binary_dilation", "binary_opening", "binary_closing", "binary_hit_or_miss", "binary_propagation",
         "binary_fill_holes")
RASTER = (5, 7)
STRUCTURE_SHAPES = ((3, 3), (2, 2), (4, 3), (1, 5), (5, 2), (2, 7), (6, 6), (3, 70), (9, 9))
ITERATIONS = (1, 2, 3, 7, 0, -1)


def _bm():
    from neilpy_amd import binary
    return binary


def fits(structure, shape):
    s = np.shape(structure)
    return s[0] <= shape[0] and s[1] <= shape[1]


def brute_choices(structure, shape):
    """the brute_force values SciPy may be called with (module docstring)"""
    return (False, True) if structure is None or fits(structure, shape) else (True,)


def structure_of(shape, seed):
    """a drawn structure of this shape, about 60 % members, never without one"""
    s = np.random.default_rng([20270301, seed] + list(shape)).random(shape) < 0.6
    s[0, 0] = True
    return s


# ------------------------------------------------------------------------------------------
# the restatement against SciPy
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sshape", STRUCTURE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_scipy(sshape):
    """every function, every accepted origin, both border values, with and without a mask, every iteration count"""
    rng = np.random.default_rng([20270302] + list(sshape))
    compared = 0
    for k, origin in enumerate(bn.origins_of(sshape)):
        s = structure_of(sshape, k % 3)
        monotone = bn.centre_is_member(s, origin)
        X, M = rng.random(RASTER) < 0.5, rng.random(RASTER) < 0.7
        for brute in brute_choices(s, RASTER):
            for border in (0, 1):
                for mask in (None, M):
                    for it in ITERATIONS:
                        if it < 1 and not monotone:
                            with pytest.raises(NotImplementedError):
                                bn.binary_erosion(X, s, it, mask, border, origin)
                            continue                      # SciPy may never return here
                        ctx = (sshape, origin, border, mask is not None, it, brute)
                        assert np.array_equal(bn.binary_erosion(X, s, it, mask, border, origin),
                                              ndi.binary_erosion(X, s, it, mask, None, border, origin, brute)), ("erosion", ctx)
                        assert np.array_equal(bn.binary_dilation(X, s, it, mask, border, origin),
                                              ndi.binary_dilation(X, s, it, mask, None, border, origin, brute)), ("dilation", ctx)
                        assert np.array_equal(bn.binary_opening(X, s, it, origin, mask, border),
                                              ndi.binary_opening(X, s, it, None, origin, mask, border, brute)), ("opening", ctx)
                        assert np.array_equal(bn.binary_closing(X, s, it, origin, mask, border),
                                              ndi.binary_closing(X, s, it, None, origin, mask, border, brute)), ("closing", ctx)
                        compared += 4
                    if monotone and fits(s, RASTER):       # binary_propagation has no brute_force to pass on
                        assert np.array_equal(bn.binary_propagation(X, s, mask, border, origin),
                                              ndi.binary_propagation(X, s, mask, None, border, origin)), (sshape, origin, border)
                        compared += 1
        if monotone and fits(s, RASTER):
            assert np.array_equal(bn.binary_fill_holes(X, s, origin), ndi.binary_fill_holes(X, s, None, origin)), (sshape, origin)
        assert np.array_equal(bn.binary_hit_or_miss(X, s, None, origin), ndi.binary_hit_or_miss(X, s, None, None, origin)), (sshape, origin)
        for origin2 in bn.origins_of(sshape)[::7]:
            s2 = structure_of(sshape, 5) & ~s
            assert np.array_equal(bn.binary_hit_or_miss(X, s, s2, origin, origin2),
                                  ndi.binary_hit_or_miss(X, s, s2, None, origin, origin2)), (sshape, origin, origin2)
            compared += 1
    assert compared >= 40 * len(bn.origins_of(sshape)), compared


def test_restatement_defaults_and_edge_structures():
    """structure=None is the cross; a structure without members gives all ones for erosion and all zeros for dilation;
    foreground is `!= 0` with NaN foreground and -0.0 background"""
    X = lbn.random_mask((9, 11), 0.5, 4)
    for name in NAMES[:4]:
        assert np.array_equal(getattr(bn, name)(X), getattr(ndi, name)(X)), name
        assert np.array_equal(getattr(bn, name)(X, np.zeros((3, 3))), getattr(ndi, name)(X, np.zeros((3, 3)))), name
    assert bn.binary_erosion(X, np.zeros((2, 3))).all() and not bn.binary_dilation(X, np.zeros((2, 3))).any()
    assert np.array_equal(bn.binary_hit_or_miss(X), ndi.binary_hit_or_miss(X))
    assert np.array_equal(bn.binary_propagation(X, mask=lbn.random_mask((9, 11), 0.8, 5)),
                          ndi.binary_propagation(X, mask=lbn.random_mask((9, 11), 0.8, 5)))
    assert np.array_equal(bn.binary_fill_holes(X), ndi.binary_fill_holes(X))
    F = np.array([[np.nan, -0.0, 0.0, 2.5, -1.0]])
    assert np.array_equal(bn.binary_dilation(F, np.ones((1, 1))), [[True, False, False, True, True]])
    assert np.array_equal(ndi.binary_dilation(F, np.ones((1, 1))), [[True, False, False, True, True]])
    with pytest.raises(ValueError):
        bn.members(np.ones((3, 3)), (0, 2))
    with pytest.raises(ValueError):
        bn.members(np.ones((2, 2)), (0, -2))


def test_propagation_identity_equals_scipy():
    """the converged masked dilation read off the components of the mask, for all 16 structures, both border values, seeds
    inside and outside the mask; fill_holes likewise"""
    compared = 0
    for shape in ((1, 1), (1, 9), (9, 1), (5, 7), (12, 13), (40, 130)):
        for p in (0.41, 0.59, 0.9):
            M = lbn.random_mask(shape, p, 6)
            X = lbn.random_mask(shape, 0.05, 7)
            assert shape[0] * shape[1] < 50 or (X & ~M).any()
            for k in range(16):
                s = lbn.STRUCTURES[k]
                for border in (0, 1):
                    for mask in (M, None):
                        want = ndi.binary_propagation(X, s, mask, None, border)
                        assert np.array_equal(bn.propagation_by_labels(X, s, mask, border, ndi.label), want), (shape, p, k, border)
                        compared += 1
                assert np.array_equal(bn.fill_holes_by_labels(M, s, ndi.label), ndi.binary_fill_holes(M, s)), (shape, p, k)
                if shape[0] * shape[1] <= 35:
                    assert np.array_equal(bn.propagation_by_labels(X, s, M, 1, lbn.label), ndi.binary_propagation(X, s, M, None, 1))
    assert compared == 6 * 3 * 16 * 4
    for name, mask in lbn.constructed((21, 26)).items():
        seed = np.zeros(mask.shape, bool)
        seed[0, 0] = seed[10, 13] = True
        for k in (lbn.FOUR, lbn.EIGHT):
            s = lbn.STRUCTURES[k]
            assert np.array_equal(bn.propagation_by_labels(seed, s, mask, 0, ndi.label), ndi.binary_propagation(seed, s, mask)), name
            assert np.array_equal(bn.fill_holes_by_labels(mask, s, ndi.label), ndi.binary_fill_holes(mask, s)), name


# ------------------------------------------------------------------------------------------
# the C ABI, host side
# ------------------------------------------------------------------------------------------
ENTRIES = ("offsets", "plane_bytes", "pack", "unpack", "step", "hit_or_miss", "propagate_workspace_bytes", "propagate")


def test_header_library_and_bindings_agree():
    """every name include/smrf_binary.h declares is exported and bound in binary.py with the declaration's arity; the stream
    is every launching entry's last argument; nothing of it sits in the shared header, the shared signature table or the
    package's namespace, and no export carries another family's name"""
    import streamed as S
    import neilpy_amd
    from neilpy_amd import _lib
    bm = _bm()
    text = open(os.path.join(ROOT, "include", "smrf_binary.h")).read()
    decl = S.declarations(text)
    assert set(decl) == set(bm.SIGNATURES) == {"smrf_binary_" + n for n in ENTRIES}
    lib = bm._library()
    for name, params in decl.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(params) == len(bm.SIGNATURES[name][1]), name
        assert not re.search("label|rank|measure", name), name
    slots = S.stream_slots(text)
    assert slots == {"smrf_binary_offsets": None, "smrf_binary_plane_bytes": None, "smrf_binary_pack": 5, "smrf_binary_unpack": 5,
                     "smrf_binary_step": 10, "smrf_binary_hit_or_miss": 8, "smrf_binary_propagate_workspace_bytes": None,
                     "smrf_binary_propagate": 10}
    for name, slot in slots.items():
        if slot is not None:
            assert slot == len(decl[name]) - 1 and bm.SIGNATURES[name][1][slot] is C.c_void_p
    assert not [n for n in _lib.SIGNATURES if "binary" in n] and not [n for n in S.declarations() if "binary" in n]
    assert inspect.ismodule(neilpy_amd.binary) and not set(NAMES) & set(dir(neilpy_amd)), "the family is not re-exported"
    macro = lambda n: int(re.search(r"#define SMRF_BINARY_%s (\d+)" % n, text).group(1))          # noqa: E731
    assert (bm.ERODE, bm.DILATE) == (macro("ERODE"), macro("DILATE")) == (0, 1)
    bits = open(os.path.join(ROOT, "neilpy_amd", "csrc", "binary_bits.h")).read()
    assert re.search(r"SMRF_BITS_AND = 0, SMRF_BITS_OR = 1", bits)
    assert isinstance(bm.CHECK_EVERY, int) and bm.CHECK_EVERY >= 2


def test_offsets_are_the_restatements_members():
    """smrf_binary_offsets against binary_numpy.members for every accepted origin, plain and reflected; SMRF_E_ARG for
    the origins next to the range"""
    lib = _bm()._library()
    for sshape in STRUCTURE_SHAPES + ((1, 1), (1, 139)):
        s = structure_of(sshape, 1)
        flat = np.ascontiguousarray(s, dtype=np.uint8) * 7
        out = np.zeros((s.size, 2), np.int32)
        call = lambda o, reflect, buf: lib.smrf_binary_offsets(flat.ctypes.data_as(C.c_void_p), sshape[0], sshape[1], o[0], o[1],  # noqa: E731
                                                               reflect, buf)
        for origin in bn.origins_of(sshape):
            want = bn.members(s, origin)
            n = call(origin, 0, out.ctypes.data_as(C.c_void_p))
            assert n == len(want) == call(origin, 0, C.c_void_p(0)) and [tuple(p) for p in out[:n]] == want == sorted(want), (sshape, origin)
            n = call(origin, 1, out.ctypes.data_as(C.c_void_p))
            assert n == len(want) and [tuple(p) for p in out[:n]] == sorted((-a, -b) for a, b in want), (sshape, origin)
        rr, cc = bn.origin_range(sshape[0]), bn.origin_range(sshape[1])
        for bad in ((rr[0] - 1, 0), (rr[-1] + 1, 0), (0, cc[0] - 1), (0, cc[-1] + 1)):
            assert call(bad, 0, C.c_void_p(0)) == E_ARG, (sshape, bad)
    empty = np.zeros(6, np.uint8)
    assert lib.smrf_binary_offsets(empty.ctypes.data_as(C.c_void_p), 2, 3, 0, 0, 0, C.c_void_p(0)) == 0
    assert lib.smrf_binary_offsets(C.c_void_p(0), 2, 3, 0, 0, 0, C.c_void_p(0)) == E_ARG
    assert lib.smrf_binary_offsets(empty.ctypes.data_as(C.c_void_p), -1, 3, 0, 0, 0, C.c_void_p(0)) == E_ARG


def test_workspace_bytes_is_the_documented_formula():
    bm = _bm()
    from neilpy_amd import label as lb
    lib = bm._library()
    up = lambda b: (b + 255) // 256 * 256                   # noqa: E731
    for rows, cols in ((1, 1), (1, 63), (64, 64), (65, 129), (2048, 2047), (2048, 1), (1, 2049), (16384, 16384), (46340, 46340),
                       (1, 2 ** 31 - 1)):
        cells, plane = rows * cols, 8 * rows * -(-cols // 64)
        assert lib.smrf_binary_plane_bytes(rows, cols) == bm.plane_bytes(rows, cols) == plane, (rows, cols)
        want = up(4 * cells) + lb.workspace_bytes(rows, cols) + up(cells + 1) + 3 * up(plane) + 256
        assert lib.smrf_binary_propagate_workspace_bytes(rows, cols) == bm.propagate_workspace_bytes(rows, cols) == want, (rows, cols)
    for rows, cols in ((0, 5), (5, 0), (0, 0)):
        assert lib.smrf_binary_propagate_workspace_bytes(rows, cols) == bm.propagate_workspace_bytes(rows, cols) == 0
        assert lib.smrf_binary_plane_bytes(rows, cols) == 0
    for fn in (lib.smrf_binary_propagate_workspace_bytes, lib.smrf_binary_plane_bytes):
        assert fn(-1, 5) == E_ARG and fn(5, -1) == E_ARG
        assert fn(46341, 46341) == E_UNSUPPORTED and fn(2, 2 ** 30) == E_UNSUPPORTED and fn(1, 2 ** 31 - 1) > 0


def test_abi_argument_errors():
    """refusals by status code, before any launch and so without a GPU"""
    lib = _bm()._library()
    p, q, null = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(0)      # never dereferenced: every call is refused first
    big = 1 << 40
    for fn in (lib.smrf_binary_pack, lib.smrf_binary_unpack):
        assert fn(p, q, -1, 5, 0, null) == E_ARG and fn(p, q, 5, -1, 0, null) == E_ARG
        assert fn(p, q, 46341, 46341, 0, null) == E_UNSUPPORTED
        assert fn(null, q, 5, 5, 0, null) == E_ARG and fn(p, null, 5, 5, 0, null) == E_ARG
        assert fn(null, null, 0, 5, 0, null) == 0                       # an empty raster: nothing launched
    assert lib.smrf_binary_unpack(p, C.c_void_p(8196), 5, 5, 0, null) == E_ARG            # 8-byte stores
    step = lib.smrf_binary_step
    assert step(p, q, -1, 5, null, p, 3, 0, 0, null, null) == E_ARG
    assert step(p, q, 2, 2 ** 30, null, p, 3, 0, 0, null, null) == E_UNSUPPORTED
    assert step(p, q, 5, 5, null, p, -1, 0, 0, null, null) == E_ARG
    for op in (-1, 2):
        assert step(p, q, 5, 5, null, p, 3, op, 0, null, null) == E_ARG
    assert step(null, q, 5, 5, null, p, 3, 0, 0, null, null) == E_ARG
    assert step(p, null, 5, 5, null, p, 3, 0, 0, null, null) == E_ARG
    assert step(p, q, 5, 5, null, null, 3, 0, 0, null, null) == E_ARG
    assert step(p, p, 5, 5, null, p, 3, 0, 0, null, null) == E_ARG                          # in place
    assert step(null, null, 0, 5, null, null, 0, 1, 0, null, null) == 0
    hom = lib.smrf_binary_hit_or_miss
    assert hom(p, q, 5, -1, p, 2, p, 2, null) == E_ARG and hom(p, q, 46341, 46341, p, 2, p, 2, null) == E_UNSUPPORTED
    assert hom(p, q, 5, 5, p, -1, p, 2, null) == E_ARG and hom(p, q, 5, 5, p, 2, p, -1, null) == E_ARG
    assert hom(null, q, 5, 5, p, 2, p, 2, null) == E_ARG and hom(p, null, 5, 5, p, 2, p, 2, null) == E_ARG
    assert hom(p, q, 5, 5, null, 2, p, 2, null) == E_ARG and hom(p, q, 5, 5, p, 2, null, 2, null) == E_ARG
    assert hom(p, p, 5, 5, p, 2, p, 2, null) == E_ARG
    prop = lib.smrf_binary_propagate
    w = C.c_void_p(1 << 20)
    assert prop(p, p, q, -1, 5, 3, 0, 0, w, big, null) == E_ARG
    assert prop(p, p, q, 46341, 46341, 3, 0, 0, w, big, null) == E_UNSUPPORTED
    for links in (-1, 16):
        assert prop(p, p, q, 5, 5, links, 0, 0, w, big, null) == E_ARG
    assert prop(p, null, q, 5, 5, 3, 0, 0, w, big, null) == E_ARG
    assert prop(p, p, null, 5, 5, 3, 0, 0, w, big, null) == E_ARG
    assert prop(p, p, C.c_void_p(8194), 5, 5, 3, 0, 0, w, big, null) == E_ARG             # dword stores
    assert prop(p, p, q, 5, 5, 3, 0, 0, null, big, null) == E_WORKSPACE
    assert prop(p, p, q, 5, 5, 3, 0, 0, w, lib.smrf_binary_propagate_workspace_bytes(5, 5) - 1, null) == E_WORKSPACE
    assert prop(p, p, q, 5, 5, 3, 0, 0, C.c_void_p((1 << 20) + 8), big, null) == E_ARG    # the workspace's alignment
    assert prop(null, null, null, 0, 5, 3, 0, 0, null, 0, null) == 0


def test_kernels_compile_without_scratch(tmp_path):
    """csrc/binary.hip for gfx950: pack, unpack, the step, the 3 x 3 member table, mark and select, all in registers"""
    import family_checks as fc
    text, kernels = fc.device_asm("binary", tmp_path)
    for stem in ("binary_pack", "binary_unpack", "binary_step", "binary_link_table", "binary_mark", "binary_select"):
        assert len([k for k in kernels if stem in k]) == 1, (stem, sorted(kernels))
    assert len(kernels) == 6
    fc.assert_no_scratch(text, kernels)


# ------------------------------------------------------------------------------------------
# csrc/binary_bits.h on the CPU
# ------------------------------------------------------------------------------------------
_BITS_CPP = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "binary_bits.h"

struct Structure {
  int rows, cols, o_r, o_c;
  std::vector<unsigned char> s;
  std::vector<int> table;      // exactly 2 n ints: a read past the members is a heap overflow the sanitizer sees
};

static bool read_structure(FILE* f, int reflect, Structure& t) {
  if (std::fscanf(f, "%d %d %d %d", &t.rows, &t.cols, &t.o_r, &t.o_c) != 4) return false;
  t.s.resize((size_t)t.rows * t.cols);
  for (auto& b : t.s) {
    int v;
    if (std::fscanf(f, "%d", &v) != 1) return false;
    b = (unsigned char)v;
  }
  const int n = smrf_bits_offsets(t.s.data(), t.rows, t.cols, t.o_r, t.o_c, reflect, nullptr);
  if (n < 0) return false;
  t.table.assign(2 * (size_t)n, 0);
  return smrf_bits_offsets(t.s.data(), t.rows, t.cols, t.o_r, t.o_c, reflect, t.table.data()) == n;
}

static bool read_plane(FILE* f, size_t words, std::vector<uint64_t>& p) {
  p.resize(words);
  for (auto& w : p) {
    unsigned long long v;
    if (std::fscanf(f, "%llx", &v) != 1) return false;
    w = v;
  }
  return true;
}

// argv[1]: cases of "rows cols op border has_mask hit_or_miss", one structure (two for hit-or-miss) as "srows scols
// origin_r origin_c" and its bytes, the input plane and the mask plane in hexadecimal words.  stdout, per case: the
// table, then every output word of the step made "lane by lane" with the kernel's own text, then the changed flag.
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int rows, cols, op, border, has_mask, hom;
  while (std::fscanf(f, "%d %d %d %d %d %d", &rows, &cols, &op, &border, &has_mask, &hom) == 6) {
    Structure a, b;
    if (!read_structure(f, op == SMRF_BITS_OR && !hom, a)) return 3;
    if (hom && !read_structure(f, 0, b)) return 3;
    const int W = smrf_bits_words(cols);
    std::vector<uint64_t> in, mask;
    if (!read_plane(f, (size_t)rows * W, in)) return 4;
    if (has_mask && !read_plane(f, (size_t)rows * W, mask)) return 4;
    auto load = [&](int r, int j) {
      if (r < 0 || r >= rows || j < 0 || j >= W) std::abort();       // only words of the raster are ever loaded
      return in.at((size_t)r * W + j);
    };
    std::printf("%d", (int)a.table.size() / 2);
    for (int v : a.table) std::printf(" %d", v);
    std::printf("\n");
    bool any = false;
    for (int r = 0; r < rows; ++r)
      for (int w = 0; w < W; ++w) {
        int first, last;
        for (size_t k = 0; k < a.table.size(); k += 2) {
          smrf_bits_span(w, a.table[k + 1], &first, &last);
          if (first * 64ll > 64ll * w + a.table[k + 1] || last * 64ll + 63 < 64ll * w + 63 + a.table[k + 1]) std::abort();
        }
        bool changed;
        const uint64_t v = smrf_bits_step_word(load, rows, cols, r, w, a.table.data(), (int)a.table.size() / 2, op, border,
                                               hom ? b.table.data() : nullptr, hom ? (int)b.table.size() / 2 : -1, has_mask != 0,
                                               has_mask ? mask[(size_t)r * W + w] : 0, &changed);
        if (v & ~smrf_bits_valid(cols, w)) std::abort();               // the bits past cols are written as zeros
        any |= changed;
        std::printf("%llx ", (unsigned long long)v);
      }
    std::printf("\n%d\n", (int)any);
  }
  std::fclose(f);
  return 0;
}
'''


def _words(mask, rng):
    """a bool raster as rows of hexadecimal words; the bits past the last column are drawn at random: nobody trusts them"""
    rows, cols = mask.shape
    W = -(-cols // 64)
    out = []
    for r in range(rows):
        bits = sum(1 << int(c) for c in np.flatnonzero(mask[r]))
        junk = int(rng.integers(0, 2 ** 63)) << cols & (1 << 64 * W) - 1
        bits |= junk
        out.append(" ".join("%x" % (bits >> 64 * w & (1 << 64) - 1) for w in range(W)))
    return out


def _cells(words, shape):
    rows, cols = shape
    W = -(-cols // 64)
    v = np.array([int(t, 16) for t in words], dtype=np.uint64).reshape(rows, W)
    bits = (v[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(rows, 64 * W)[:, :cols].astype(bool)


def _bits_cases():
    """(shape, op, border, mask?, hit-or-miss?, structure, origin, second structure, its origin)"""
    wide = np.zeros((1, 139), bool)
    wide[0, [0, 1, 5, 64, 69, 70, 133, 138]] = True                    # dc from -69 to +69 about the centre
    wide3 = np.zeros((3, 139), bool)
    wide3[[0, 1, 1, 2], [0, 69, 138, 75]] = True
    tall = structure_of((9, 3), 2)                                      # taller than the rasters of 4 rows
    structures = [(wide, (0, 0)), (wide3, (1, 0)), (tall, (0, 0)), (tall, (-4, 1)), (np.ones((3, 3), bool), (0, 0)),
                  (structure_of((4, 3), 1), (-2, 1)), (structure_of((2, 2), 1), (-1, 0)), (np.zeros((2, 3), bool), (0, 0)),
                  (structure_of((3, 70), 1), (0, -20)), (structure_of((3, 70), 1), (1, 34))]
    for cols in (1, 63, 64, 65, 129, 190):
        for rows in (4, 1):
            for s, origin in structures:
                for op in (0, 1):
                    for border in (0, 1):
                        for masked in (False, True):
                            if rows == 1 and (masked or border):
                                continue
                            yield (rows, cols), op, border, masked, False, s, origin, None, None
            yield (rows, cols), 0, 0, False, True, structure_of((2, 3), 3), (0, 0), structure_of((4, 1), 3), (-1, 0)
            yield (rows, cols), 0, 0, False, True, wide, (0, 0), wide3 & ~np.pad(wide, ((1, 1), (0, 0))), (-1, 0)
            yield (rows, cols), 0, 0, False, True, np.ones((3, 3), bool), (0, 0), None, None


def test_binary_bits_header_on_the_cpu(tmp_path):
    """csrc/binary_bits.h compiled with g++ -fsanitize=address,undefined into a stand-alone program that makes every
    output word of a step with the step kernel's own text: member tables from smrf_bits_offsets, spans of shifted words,
    the window of two adjacent words, tails, borders, masks and the second table of hit-or-miss, on rasters whose last
    words end 1, 63, 64, 1 and 62 cells in, with members up to 69 columns away and structures taller than the raster.
    Compared with scipy.ndimage at iterations=1 and with the restatement."""
    src = tmp_path / "bits.cpp"
    src.write_text(_BITS_CPP)
    exe = tmp_path / "bits"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "neilpy_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(20270303)
    todo, lines = [], []
    for shape, op, border, masked, hom, s, origin, s2, origin2 in _bits_cases():
        X = rng.random(shape) < (0.8 if op == 0 else 0.2)
        M = rng.random(shape) < 0.6 if masked else None
        if hom and s2 is None:
            s2, origin2 = ~s, origin
        todo.append((shape, op, border, M, hom, s, origin, s2, origin2, X))
        lines.append("%d %d %d %d %d %d" % (shape + (op, border, int(masked), int(hom))))
        for t, o in ((s, origin), (s2, origin2)):
            if t is not None:
                lines.append("%d %d %d %d" % (t.shape + tuple(o)))
                lines.append(" ".join(str(int(v) * 3) for v in t.ravel()))
        lines.extend(_words(X, rng))
        if masked:
            lines.extend(_words(M, rng))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    got = out.stdout.strip("\n").split("\n")
    assert len(got) == 3 * len(todo) >= 600
    for k, (shape, op, border, M, hom, s, origin, s2, origin2, X) in enumerate(todo):
        ctx = (shape, op, border, M is not None, hom, s.shape, origin)
        table = [int(v) for v in got[3 * k].split()]
        want_table = bn.members(s, origin)
        if op == 1 and not hom:
            want_table = sorted((-a, -b) for a, b in want_table)
        assert table[0] == len(want_table) and list(zip(table[1::2], table[2::2])) == want_table, ctx
        cells = _cells(got[3 * k + 1].split(), shape)
        if hom:
            want = ndi.binary_hit_or_miss(X, s, s2, None, origin, origin2)
            assert np.array_equal(want, bn.binary_hit_or_miss(X, s, s2, origin, origin2)), ctx
        else:
            name = ("binary_erosion", "binary_dilation")[op]
            want = getattr(ndi, name)(X, s, 1, M, None, border, origin)
            assert np.array_equal(want, getattr(bn, name)(X, s, 1, M, border, origin)), ctx
        assert np.array_equal(cells, want), (ctx, int(np.sum(cells != want)))
        assert int(got[3 * k + 2]) == int(not np.array_equal(want, X)), ctx


# ------------------------------------------------------------------------------------------
# the interface
# ------------------------------------------------------------------------------------------
def test_signatures_are_scipys():
    bm = _bm()
    for name in NAMES:
        want = list(inspect.signature(getattr(ndi, name)).parameters.values())
        got = list(inspect.signature(getattr(bm, name)).parameters.values())
        extra = got[len(want):]
        assert [(g.name, g.kind, g.default) for g in got[:len(want)]] == [(w.name, w.kind, w.default) for w in want], name
        if name in ("binary_propagation", "binary_fill_holes"):
            assert [(g.name, g.kind, g.default) for g in extra] == [("impl", inspect.Parameter.KEYWORD_ONLY, None)], name
        else:
            assert not extra, name
    assert sorted(bm.__all__) == sorted(NAMES)


def _refusal(call):
    """the exception type SciPy raises for this call"""
    try:
        call()
    except Exception as e:                                  # noqa: BLE001: the type is what is asked for
        return type(e)
    raise AssertionError("SciPy accepts the call")


def test_argument_errors_come_from_the_host():
    """every refusal is decided before the device is touched: it is the same with and without a GPU.  SciPy's own refusals
    keep SciPy's exception types, taken from it here; an origin outside the accepted range is never handed to SciPy"""
    bm = _bm()
    X = np.zeros((4, 5), np.uint8)
    ones = np.ones((3, 3))
    for name in NAMES:
        f, g = getattr(bm, name), getattr(ndi, name)
        for Y in (np.zeros((2, 3, 4), np.uint8), np.zeros(5, np.uint8), np.uint8(1)):
            with pytest.raises(NotImplementedError):
                f(Y)                                                        # not a 2-D raster
        big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), shape=(2 ** 16, 2 ** 15), strides=(0, 0))
        with pytest.raises(NotImplementedError):
            f(big)                                                          # 2**31 cells
        if name != "binary_fill_holes":                                     # SciPy fills the holes of a complex raster
            want = _refusal(lambda: g(np.zeros((4, 5), np.complex64)))
            with pytest.raises(want) as info:
                f(np.zeros((4, 5), np.complex64))
            assert info.type is want, name
        for bad in (np.ones((3, 3, 3)), np.ones(3)):
            want = _refusal(lambda: g(X, bad))
            with pytest.raises(want) as info:
                f(X, bad)
            assert info.type is want, (name, bad.shape)
        for output in (np.int64, np.uint8, "float32", np.empty((4, 5), bool), 7):
            with pytest.raises(NotImplementedError):
                f(X, output=output)
        for axes in ((0,), (1,), 0, (1, 0), (0, 1, 2)):
            with pytest.raises(NotImplementedError):
                f(X, axes=axes)
    for name in NAMES[:4]:
        f, g = getattr(bm, name), getattr(ndi, name)
        want = _refusal(lambda: g(X, ones, 1.5))
        with pytest.raises(want) as info:
            f(X, ones, 1.5)
        assert info.type is want, name
        want = _refusal(lambda: g(X, ones, mask=np.ones((4, 6))))
        with pytest.raises(want) as info:
            f(X, ones, mask=np.ones((4, 6)))
        assert info.type is want, name
        # the deviations: origins outside the range (ValueError, never SciPy's), iterations < 1 without the centre
        for s, origin in ((ones, (0, 2)), (np.ones((2, 2)), (0, -2)), (np.ones((1, 5)), (-1, -2)), (np.ones((5, 2)), (3, 0)),
                          (ones, 2), (ones, -2), (np.ones((2, 2)), 1)):
            with pytest.raises(ValueError):
                f(X, s, origin=origin)
        off = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]])
        for it in (0, -1):
            with pytest.raises(NotImplementedError):
                f(X, off, it)
            with pytest.raises(NotImplementedError):
                f(X, np.array([[1, 1, 0]]), it, origin=(0, 1))              # the centre moves onto a cell that is no member
    want = _refusal(lambda: ndi.binary_propagation(X, ones, np.ones((4, 6))))
    with pytest.raises(want):
        bm.binary_propagation(X, ones, np.ones((4, 6)))
    off = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]])
    for call in (lambda: bm.binary_propagation(X, off), lambda: bm.binary_fill_holes(X, off),
                 lambda: bm.binary_propagation(X, np.array([[1, 1, 0]]), origin=(0, 1))):
        with pytest.raises(NotImplementedError):
            call()
    for call in (lambda: bm.binary_propagation(X, ones, origin=(0, 2)), lambda: bm.binary_fill_holes(X, ones, origin=-2),
                 lambda: bm.binary_hit_or_miss(X, ones, origin1=(2, 0)), lambda: bm.binary_hit_or_miss(X, ones, ones, origin2=(0, -2)),
                 lambda: bm.binary_propagation(X, impl="fast"), lambda: bm.binary_fill_holes(X, impl="fast"),
                 lambda: bm.binary_propagation(X, np.ones((5, 5)), impl="labels"),
                 lambda: bm.binary_fill_holes(X, np.array([[1, 1, 0], [0, 1, 0], [0, 0, 0]]), impl="labels")):
        with pytest.raises(ValueError):
            call()


def test_empty_rasters_need_no_device():
    bm = _bm()
    for shape in ((0, 5), (4, 0), (0, 0)):
        for name in NAMES:
            got = getattr(bm, name)(np.zeros(shape, np.float32))
            want = getattr(ndi, name)(np.zeros(shape, np.float32))
            assert got.shape == want.shape == shape and got.dtype == want.dtype == bool, (name, shape)


def test_valid_call_without_a_gpu_raises():
    import torch
    import neilpy_amd
    bm = _bm()
    if torch.cuda.is_available():
        return                                                 # tests/test_gpu_binary.py runs the valid calls
    X = np.ones((4, 5), np.uint8)
    for name in NAMES:
        with pytest.raises(neilpy_amd.SmrfHipError):
            getattr(bm, name)(X)
    with pytest.raises(neilpy_amd.SmrfHipError):
        bm.binary_fill_holes(X, impl="iterate")
