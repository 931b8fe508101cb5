"""Per-label measurements without a GPU (neilpy_amd/measure.py, csrc/measure.hip, csrc/measure_fixed.h; DESIGN.md section
22): the restatement tests/measure_numpy.py against scipy.ndimage under every form of ``labels`` and ``index`` - extrema and
positions exactly, sums within bounds computed from the data - the fixed-point split and the 128-bit rounding of
measure_fixed.h compiled with g++ under the address and undefined-behaviour sanitizers, the host logic behind the C ABI of
include/smrf_measure.h, and the argument refusals."""
import ctypes as C
import inspect
import math
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import scipy.ndimage as ndi

import label_numpy as lbn
import measure_numpy as mn
from conftest import ROOT

E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -5
NAMES = ("sum_labels", "mean", "variance", "standard_deviation", "minimum", "maximum", "extrema", "minimum_position",
         "maximum_position")
SHAPE = (23, 38)


def _ms():
    from neilpy_amd import measure
    return measure


def labels_of(shape=SHAPE, seed=1):
    return ndi.label(lbn.blobs(shape, seed))


def forms(n):
    """the five forms of (labels given?, index): an unsorted array index that repeats labels and includes 0, a label that
    does not occur and a negative one"""
    return (("labels=None", False, None), ("index=None", True, None), ("scalar", True, min(2, n)),
            ("array", True, [n, 1, 0, 1, n + 5, -2, max(n - 1, 1)]))


# ------------------------------------------------------------------------------------------
# the restatement against SciPy
# ------------------------------------------------------------------------------------------
def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def test_extrema_and_positions_equal_scipy():
    L, n = labels_of()
    assert n >= 3
    compared = 0
    for dtype in (np.float64, np.float32, np.int32, np.uint8):
        X = mn.distinct(SHAPE, 3, np.float64)
        X = (X % 251).astype(dtype) if dtype == np.uint8 else X.astype(dtype)
        for ctx, with_labels, index in forms(n):
            lab = L if with_labels else None
            for name in ("minimum", "maximum"):
                got, want = getattr(mn, name)(X, lab, index), getattr(ndi, name)(X, lab, index)
                assert same(got, want), (dtype, ctx, name, got, want)
                compared += 1
            if dtype == np.uint8:
                continue                         # values repeat: the positions are a matter of ties
            for name in ("minimum_position", "maximum_position"):
                got, want = getattr(mn, name)(X, lab, index), getattr(ndi, name)(X, lab, index)
                assert _positions(got) == _positions(want), (dtype, ctx, name, got, want)
            got, want = mn.extrema(X, lab, index), ndi.extrema(X, lab, index)
            assert same(got[0], want[0]) and same(got[1], want[1]), (dtype, ctx)
            assert _positions(got[2]) == _positions(want[2]) and _positions(got[3]) == _positions(want[3]), (dtype, ctx)
    assert compared == 32


def _positions(p):
    return [tuple(int(v) for v in q) for q in p] if isinstance(p, list) else tuple(int(v) for v in p)


def test_non_finite_and_missing_rows_equal_scipy():
    """NaN, the infinities and labels that do not occur, exactly: with an array index NaN sorts last (the minimum skips it,
    the maximum is it), with one selection np.min and np.max give NaN; a missing label gives 0.0, NaN, 0 and (0, 0)"""
    L, n = labels_of()
    X = mn.dtm(SHAPE, 4)
    cells = {k: np.flatnonzero(L.ravel() == k) for k in range(1, n + 1)}
    X.ravel()[cells[1][1]] = np.nan                        # label 1: one NaN
    X.ravel()[cells[2]] = np.nan                           # label 2: all NaN
    X.ravel()[cells[3][0]] = np.inf                        # label 3: +inf
    index = [3, 1, 2, n + 4, -1, 0]
    with np.errstate(all="ignore"):
        for name in ("sum_labels", "mean", "variance", "standard_deviation", "minimum", "maximum"):
            got, want = getattr(mn, name)(X, L, index), getattr(ndi, name)(X, L, index)
            rows = [0, 1, 2, 3, 4] if name in ("minimum", "maximum") else [1, 2, 3, 4]      # the non-finite and missing rows
            if name in ("sum_labels", "mean"):
                rows.append(0)                                                             # the infinity itself
            assert np.array_equal(np.asarray(got)[rows], np.asarray(want)[rows], equal_nan=True), (name, got, want)
        assert np.isnan(mn.maximum(X, L, index)[1]) and np.isfinite(mn.minimum(X, L, index)[1])
        assert np.isnan(mn.minimum(X, L, index)[2])
        for name in ("minimum", "maximum"):
            for lab, idx in ((None, None), (L, None), (L, 1), (L, 2)):
                got, want = getattr(mn, name)(X, lab, idx), getattr(ndi, name)(X, lab, idx)
                assert np.isnan(got) and np.isnan(want), (name, idx)
        both = X.copy()
        both.ravel()[cells[3][1]] = -np.inf
        assert np.isnan(mn.sum_labels(both, L, [3])[0]) and np.isnan(ndi.sum_labels(both, L, [3])[0])
        assert mn.sum_labels(X, L, 3) == ndi.sum_labels(X, L, 3) == np.inf
    Y = mn.distinct(SHAPE, 5)
    for name in ("minimum_position", "maximum_position"):
        assert getattr(mn, name)(Y, L, [n + 4, -1]) == [(0, 0), (0, 0)]
        assert _positions(getattr(ndi, name)(Y, L, [n + 4, -1])) == [(0, 0), (0, 0)]
    zeros = np.array([[0.0, -0.0, 5.0], [-0.0, 0.0, -5.0]])
    assert mn.minimum(zeros, zeros == 0, 1) == ndi.minimum(zeros, zeros == 0, 1) == 0
    assert mn.minimum_position(zeros, zeros == 0, 1) == (0, 1)                # -0.0 orders before +0.0
    assert mn.maximum_position(zeros, zeros == 0, 1) == (0, 0)


def value_rasters():
    yield "dtm", mn.dtm(SHAPE, 1)
    yield "dtm float32", mn.dtm(SHAPE, 1, np.float32)
    yield "1000 +- 1e-3", mn.cancelling(SHAPE, 1)
    yield "40 decades", mn.decades(SHAPE, 1)
    yield "1e-300", mn.dtm(SHAPE, 2) * 1e-300
    yield "1e300", mn.dtm(SHAPE, 2) * 1e300
    yield "uint8", (mn.distinct(SHAPE, 2) % 251).astype(np.uint8)
    yield "int32", (mn.distinct(SHAPE, 2) * 1000003).astype(np.int32)


def _selections(L, n):
    """(form, labels, index, [flat boolean masks of its groups])"""
    lab = L.ravel()
    for ctx, with_labels, index in forms(n):
        if not with_labels:
            yield ctx, None, index, [np.ones(lab.size, bool)]
        elif index is None:
            yield ctx, L, index, [lab > 0]
        elif np.ndim(index) == 0:
            yield ctx, L, index, [lab == index]
        else:
            yield ctx, L, index, [lab == k for k in index]


def test_sums_against_scipy_within_computed_bounds():
    """|restatement - exact| <= ulp / 2 + n 2**(E - 93) and |SciPy - exact| <= n 2**-52 sum |t|, the exact sum by Fraction;
    the mean is one division of each"""
    L, n = labels_of()
    checked = 0
    worst = Fraction(0)
    for vname, X in value_rasters():
        x = X.astype(np.float64).ravel()
        for ctx, lab, index, groups in _selections(L, n):
            ours, theirs = np.atleast_1d(mn.sum_labels(X, lab, index)), np.atleast_1d(ndi.sum_labels(X, lab, index))
            ours_mean = np.atleast_1d(mn.mean(X, lab, index))
            assert ours.dtype == np.float64 and ours.shape == theirs.shape == (len(groups),)
            for g, a, b, m in zip(groups, ours, theirs, ours_mean):
                t = x[g]
                if t.size == 0:
                    assert a == 0.0 and b == 0 and np.isnan(m), (vname, ctx)
                    continue
                exact = mn.exact_sum(t)
                M = float(np.abs(t).max())
                if M == 0:
                    assert a == 0.0 and b == 0
                    continue
                assert abs(Fraction(float(a)) - exact) <= mn.contract_bound(t, mn.exponent_of(M), a), (vname, ctx)
                assert m == np.float64(a) / np.float64(t.size)
                checked += 1
                if X.dtype == np.float32 and ctx != "array":
                    continue                   # SciPy adds one selection of float32 in float32: another quantity
                bound = mn.sequential_bound(t)
                err = abs(Fraction(float(b)) - exact)
                assert err <= bound, (vname, ctx, float(err), float(bound))
                if bound:
                    worst = max(worst, err / bound)
    assert checked >= 8 * 8
    assert 0 < worst <= 1, float(worst)        # SciPy compared, and inside its own bound: the derivation holds here


def test_variance_against_scipy_within_computed_bounds():
    """Each side against the exact sum of its own terms t = fl(fl(x - mean)**2), and the two exact sums apart by no more
    than the means' difference allows: with delta the largest |d - d'| over the cells, sum |d'^2 - d^2| <=
    2 delta sum |d| + n delta**2, and a rounded square is within 2**-53 of its own value of the exact one."""
    L, n = labels_of()
    checked = 0
    for vname, X in value_rasters():
        if vname == "1e300":
            continue                           # squares overflow: the rows of infinities are compared below
        x = X.astype(np.float64).ravel()
        for ctx, lab, index, groups in _selections(L, n):
            with np.errstate(all="ignore"):      # 0 / 0 for the labels that do not occur
                ours, theirs = np.atleast_1d(mn.variance(X, lab, index)), np.atleast_1d(ndi.variance(X, lab, index))
            means = np.atleast_1d(mn.mean(X, lab, index))
            their_sums = np.atleast_1d(ndi.sum_labels(X, lab, index))
            std = np.atleast_1d(mn.standard_deviation(X, lab, index))
            for g, a, b, m_o, s_s, sd in zip(groups, ours, theirs, means, their_sums, std):
                t = x[g]
                cnt = t.size
                if cnt == 0:
                    assert np.isnan(a) and np.isnan(b) and np.isnan(sd), (vname, ctx)
                    continue
                assert sd == np.sqrt(a)
                M = float(np.abs(t).max())
                if M == 0:
                    assert a == 0 and b == 0
                    continue
                # SciPy's mean: its sum over the count with an array index, np.mean of the selection otherwise
                m_s = np.float64(s_s) / np.float64(cnt) if ctx == "array" else X.ravel()[g].mean()
                d_o, d_s = t - m_o, t - np.float64(m_s)
                t_o, t_s = d_o * d_o, d_s * d_s
                Ev = 2 * mn.exponent_of(M) + 3
                total = mn.contract_sum(t_o, Ev)
                ex_o, ex_s = mn.exact_sum(t_o), mn.exact_sum(t_s)
                assert abs(Fraction(total) - ex_o) <= mn.contract_bound(t_o, Ev, total), (vname, ctx)
                assert a == np.float64(total) / np.float64(cnt)
                if X.dtype == np.float32 and ctx != "array":
                    continue                   # SciPy works in float32 there: another quantity
                delta = Fraction(float(np.abs(d_o - d_s).max()))
                bridge = 2 * delta * mn.exact_sum(np.abs(d_s)) + cnt * delta * delta + Fraction(2) ** -52 * (ex_o + ex_s)
                assert abs(ex_o - ex_s) <= bridge
                slack = (mn.contract_bound(t_o, Ev, total) + mn.sequential_bound(t_s) + bridge) / cnt + mn.ulp(a) + mn.ulp(b)
                assert abs(Fraction(float(a)) - Fraction(float(b))) <= slack, (vname, ctx, float(a), float(b))
                checked += 1
    assert checked >= 6 * 8
    big = mn.dtm(SHAPE, 2) * 1e300
    with np.errstate(all="ignore"):
        assert np.array_equal(mn.variance(big, L, [1, 2]), ndi.variance(big, L, [1, 2])) and mn.variance(big, L, 1) == np.inf


def test_region_stats_restatement_is_the_wrappers_table():
    L, n = labels_of()
    X = mn.dtm(SHAPE, 6)
    T = mn.region_stats(X, L, n + 2)
    assert np.array_equal(T["count"], np.bincount(L.ravel(), minlength=n + 3))
    assert T["count"][n + 1] == 0 and T["min_index"][n + 1] == -1 and T["sum"][n + 1] == 0 and np.isnan(T["mean"][n + 1])
    index = list(range(n + 1))
    assert np.array_equal(T["sum"][:n + 1], mn.sum_labels(X, L, index))
    assert np.array_equal(T["min"][:n + 1], ndi.minimum(X, L, index)) and np.array_equal(T["max"][:n + 1], ndi.maximum(X, L, index))
    assert [divmod(int(i), SHAPE[1]) for i in T["max_index"][:n + 1]] == _positions(ndi.maximum_position(X, L, index))
    H = lbn.HAND
    T = mn.region_stats(mn.dtm(H.shape, 1), H, 9)
    assert T["count"].tolist() == [int(np.sum(H == k)) for k in range(10)]          # negative cells and 40 are ignored


# ------------------------------------------------------------------------------------------
# csrc/measure_fixed.h on the CPU
# ------------------------------------------------------------------------------------------
_FIXED_CPP = r'''
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "measure_fixed.h"

static __int128 read128(const char* s) {                  // a decimal integer of any sign
  bool neg = *s == '-';
  if (neg) ++s;
  unsigned __int128 v = 0;
  for (; *s; ++s) v = v * 10 + (unsigned)(*s - '0');
  return neg ? -(__int128)v : (__int128)v;
}

// argv[1]: a file of cases with the values expected of them.
//   E <abs bits hex> <E>                              smrf_fixed_exponent
//   S <bits hex> <E> <p0> <p1> <p2>                   smrf_fixed_split
//   R <a0> <a1> <a2> <e2> <bits hex>                  smrf_fixed_round(smrf_fixed_total(a), e2)
//   T <total decimal> <e2> <bits hex>                 smrf_fixed_round(total, e2)
// Prints every case that differs and returns their number (at most 100).
int main(int argc, char** argv) {
  if (argc != 2) return 101;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 102;
  char kind[4], big[64];
  int bad = 0, seen = 0;
  while (std::fscanf(f, "%3s", kind) == 1) {
    ++seen;
    if (kind[0] == 'E') {
      unsigned long long b; int want;
      if (std::fscanf(f, "%llx %d", &b, &want) != 2) return 103;
      const int got = smrf_fixed_exponent(b);
      if (got != want) { std::printf("E %llx: %d, expected %d\n", b, got, want); ++bad; }
    } else if (kind[0] == 'S') {
      unsigned long long b; int E; long long w[3];
      if (std::fscanf(f, "%llx %d %lld %lld %lld", &b, &E, &w[0], &w[1], &w[2]) != 5) return 103;
      int64_t p[3];
      smrf_fixed_split(smrf_f64_of(b), E, p);
      if (p[0] != w[0] || p[1] != w[1] || p[2] != w[2]) {
        std::printf("S %llx %d: %lld %lld %lld\n", b, E, (long long)p[0], (long long)p[1], (long long)p[2]);
        ++bad;
      }
    } else if (kind[0] == 'R') {
      long long a[3]; int e2; unsigned long long want;
      if (std::fscanf(f, "%lld %lld %lld %d %llx", &a[0], &a[1], &a[2], &e2, &want) != 5) return 103;
      const int64_t acc[3] = {a[0], a[1], a[2]};
      const unsigned long long got = smrf_f64_bits(smrf_fixed_round(smrf_fixed_total(acc), e2));
      if (got != want) { std::printf("R %lld %lld %lld %d: %llx, expected %llx\n", a[0], a[1], a[2], e2, got, want); ++bad; }
    } else if (kind[0] == 'T') {
      int e2; unsigned long long want;
      if (std::fscanf(f, "%63s %d %llx", big, &e2, &want) != 3) return 103;
      const unsigned long long got = smrf_f64_bits(smrf_fixed_round(read128(big), e2));
      if (got != want) { std::printf("T %s %d: %llx, expected %llx\n", big, e2, got, want); ++bad; }
    } else {
      return 104;
    }
  }
  std::fclose(f);
  std::printf("cases %d\n", seen);
  return bad > 100 ? 100 : bad;
}
'''


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _rounded_bits(total, e2):
    """float(Fraction(total) * 2**e2) as bits; beyond the largest float the infinity"""
    try:
        return _bits(float(Fraction(total) * Fraction(2) ** e2))
    except OverflowError:
        return _bits(math.inf if total > 0 else -math.inf)


def _pieces(q):
    s = -1 if q < 0 else 1
    a = abs(q)
    return s * (a & (2 ** 31 - 1)), s * ((a >> 31) & (2 ** 31 - 1)), s * (a >> 62)


def fixed_cases():
    rng = np.random.default_rng(20270305)
    tiny, huge = 5e-324, 1.7976931348623157e308
    lines = []
    # exponents: powers of two and their neighbours, subnormals, the ends of the range
    mags = [tiny, 2 * tiny, 3 * tiny, 2.2250738585072014e-308, 2.225073858507201e-308, 1.0, 1.5, 2.0, 1e308, huge, 1000.001]
    for e in (-1074, -1073, -1050, -1023, -1022, -1021, -1, 0, 1, 52, 53, 1022, 1023):
        p = math.ldexp(1.0, e)
        mags += [p, np.nextafter(p, 0.0), np.nextafter(p, np.inf)]
    mags = [float(m) for m in mags if 0 < m < np.inf]
    for m in mags:
        lines.append("E %x %d" % (_bits(m), math.frexp(m)[1]))
    # splits: every magnitude as M, against terms at and far below it, both signs, and the squares' exponent 2 E + 3
    for M in mags:
        E = math.frexp(M)[1]
        terms = [M, -M, M / 3, -M / 7, M * 2.0 ** -40, M * 2.0 ** -93, -M * 2.0 ** -94, M * 2.0 ** -120, 0.0, -0.0, tiny, -tiny]
        terms += list(M * rng.uniform(-1, 1, 6))
        for t in terms:
            t = float(t)
            if abs(t) > M:
                continue
            for EE, t in ((E, t), (2 * E + 3, (2 * t) * (2 * t))):      # a value, and the square of a difference of two
                if not math.isfinite(t):
                    continue
                q = mn.quantum(t, EE)
                assert abs(q) < 2 ** 93
                assert q == int(Fraction(t) * Fraction(2) ** (93 - EE))          # int() cuts towards zero
                lines.append("S %x %d %d %d %d" % ((_bits(t), EE) + _pieces(q)))
    # roundings of accumulator triples: random, negative, near 2**62 per accumulator, into subnormals and past the top
    for _ in range(300):
        a = [int(rng.integers(-2 ** 62 + 1, 2 ** 62)) >> int(rng.integers(0, 62)) for _ in range(3)]
        e2 = int(rng.choice([-2236, -1200, -1167, -1166, -1150, -1100, -1074, -1000, -93, -60, 0, 500, 900, 931, 940, 1000]))
        total = a[2] * 2 ** 62 + a[1] * 2 ** 31 + a[0]
        lines.append("R %d %d %d %d %x" % (a[0], a[1], a[2], e2, _rounded_bits(total, e2)))
    # exact ties, one below and one above them, at 54 to 120 bits, to even and to odd neighbours, both signs; carries into
    # the next power of two; ties at the subnormal boundary
    for nbits in (54, 55, 64, 65, 93, 120, 124):
        drop = nbits - 53
        for kept in (2 ** 52, 2 ** 52 + 1, 2 ** 53 - 2, 2 ** 53 - 1, 2 ** 52 + 12345):
            for rem in (2 ** (drop - 1), 2 ** (drop - 1) - 1, 2 ** (drop - 1) + 1, 0, 2 ** drop - 1):
                if drop == 1 and rem > 1:
                    continue
                for sign in (1, -1):
                    total = sign * ((kept << drop) + rem)
                    for e2 in (-93, -1100 - drop, 931 - drop + 40, -1074 - drop - 30):
                        lines.append("T %d %d %x" % (total, e2, _rounded_bits(total, e2)))
    for total in (1, -1, 2, 3, 5, 2 ** 52, 2 ** 53 + 1, 2 ** 70 + 2 ** 17, -(2 ** 70 + 2 ** 17)):
        for e2 in (-1076, -1075, -1074, -1073, -1127, -1128, -1200, -2236, 0, 971, 1023 - total.bit_length() + 1, 1024):
            lines.append("T %d %d %x" % (total, e2, _rounded_bits(total, e2)))
    lines.append("T 0 5 0")
    return lines


def test_measure_fixed_header_on_the_cpu(tmp_path):
    """csrc/measure_fixed.h compiled with g++ -fsanitize=address,undefined into a stand-alone program: the pieces of a value
    recombine to trunc(x * 2**(93 - E)) exactly and are the three 31-bit pieces of it, and the 128-bit rounding equals
    float(Fraction(...)) - at 2**E boundaries, on subnormals, near 1e308, on negative totals and on exact ties.  The cases
    and what is expected of them are written here, as a file the program reads."""
    src = tmp_path / "fixed.cpp"
    src.write_text(_FIXED_CPP)
    exe = tmp_path / "fixed"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "neilpy_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = fixed_cases()
    kinds = {k: sum(1 for line in lines if line[0] == k) for k in "ESRT"}
    assert kinds["E"] >= 40 and kinds["S"] >= 1000 and kinds["R"] == 300 and kinds["T"] >= 1000, kinds
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.strip().split("\n")[-1] == "cases %d" % len(lines)
    # the pieces recombine: checked here on the expected values themselves
    for line in lines:
        if line[0] == "S":
            _, b, E, p0, p1, p2 = line.split()
            t = struct.unpack("<d", struct.pack("<Q", int(b, 16)))[0]
            assert int(p2) * 2 ** 62 + int(p1) * 2 ** 31 + int(p0) == mn.quantum(t, int(E))


# ------------------------------------------------------------------------------------------
# the C ABI, host side
# ------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    """every name include/smrf_measure.h declares is exported and bound in measure.py with the declaration's arity; nothing
    of it sits in the shared header, the shared signature table or the package's namespace"""
    import streamed as S
    import neilpy_amd
    from neilpy_amd import _lib
    ms = _ms()
    text = open(os.path.join(ROOT, "include", "smrf_measure.h")).read()
    decl = S.declarations(text)
    assert set(decl) == set(ms.SIGNATURES) == {"smrf_measure_" + n for n in ("workspace_bytes", "f32", "f64")}
    lib = ms._library()
    for name, params in decl.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(params) == len(ms.SIGNATURES[name][1]), name
    slots = S.stream_slots(text)
    assert slots == {"smrf_measure_workspace_bytes": None, "smrf_measure_f32": 10, "smrf_measure_f64": 10}
    for name in ("smrf_measure_f32", "smrf_measure_f64"):
        assert slots[name] == len(decl[name]) - 1 and ms.SIGNATURES[name][1][10] is C.c_void_p
    assert not [n for n in _lib.SIGNATURES if "measure" in n] and not [n for n in S.declarations() if "measure" in n]
    macro = lambda n: int(re.search(r"#define SMRF_MEASURE_%s (\d+)" % n, text).group(1))          # noqa: E731
    for name, bit in ms.WHAT.items():
        assert macro(name.upper()) == bit, name
    assert list(ms.WHAT.values()) == [1 << k for k in range(9)] and macro("ALL") == ms.WHAT_ALL == 511
    assert (macro("HAS_NAN"), macro("HAS_POS_INF"), macro("HAS_NEG_INF")) == (ms.HAS_NAN, ms.HAS_POS_INF, ms.HAS_NEG_INF) == (1, 2, 4)
    assert (macro("LABELS_AS_GIVEN"), macro("LABELS_POSITIVE")) == (ms.LABELS_AS_GIVEN, ms.LABELS_POSITIVE) == (0, 1)
    # the result structure: one pointer per measurement, in the order of the mask's bits
    body = re.search(r"typedef struct smrf_measure_out \{(.*?)\} smrf_measure_out;", text, re.S).group(1)
    fields = re.findall(r"\*\s*(\w+);", body)
    assert fields == [f[0] for f in ms.Out._fields_] == list(ms.WHAT) and C.sizeof(ms.Out) == 9 * C.sizeof(C.c_void_p)
    fixed = open(os.path.join(ROOT, "neilpy_amd", "csrc", "measure_fixed.h")).read()
    assert re.search(r"SMRF_FIXED_BITS = 93;", fixed) and re.search(r"SMRF_FIXED_PIECE = 31;", fixed) and mn.BITS == 93


def test_the_measure_names_stay_out_of_the_package_namespace():
    import neilpy_amd
    ms = _ms()
    assert inspect.ismodule(neilpy_amd.measure)
    assert not set(ms.__all__) & set(vars(neilpy_amd)), sorted(set(ms.__all__) & set(vars(neilpy_amd)))
    assert not set(ms.__all__) & set(getattr(neilpy_amd, "__all__", ()))
    assert sorted(ms.__all__) == sorted(NAMES + ("region_stats",))


def test_workspace_bytes_is_the_documented_formula():
    ms = _ms()
    lib = ms._library()
    up = lambda b: (b + 255) // 256 * 256                   # noqa: E731
    W = ms.WHAT
    for n in (0, 1, 2, 31, 32, 63, 64, 1000, 123457, 2 ** 20, 2 ** 31 - 2):
        L = n + 1
        base = 4 * up(8 * L) + up(4 * L)
        sums, index, var = up(24 * L) + up(8 * L), up(16 * L), up(24 * L)
        want = {W["count"]: base, W["min"] | W["max"]: base, W["flags"]: base, W["sum"]: base + sums, W["mean"]: base + sums,
                W["min_index"]: base + index, W["max_index"] | W["count"]: base + index, W["variance"]: base + sums + var,
                W["sum"] | W["min_index"]: base + sums + index, ms.WHAT_ALL: base + sums + index + var}
        for what, size in want.items():
            assert lib.smrf_measure_workspace_bytes(n, what) == ms.workspace_bytes(n, what) == size, (n, what)
    assert ms.workspace_bytes(0, ms.WHAT_ALL) == 9 * 256                      # nine parts of one granule each
    assert lib.smrf_measure_workspace_bytes(-1, 1) == E_ARG
    for what in (0, -1, 512, 1024 + 1):
        assert lib.smrf_measure_workspace_bytes(5, what) == E_ARG
    assert lib.smrf_measure_workspace_bytes(2 ** 31 - 1, 1) == E_UNSUPPORTED
    assert [ms.passes_of(ms.mask_of(w)) for w in (("count",), ("min", "max"), ("sum",), ("mean", "count"), ("min_index",),
                                                    ("max_index", "max"), ("variance",), ms.STATS)] == [1, 1, 2, 2, 2, 2, 3, 3]


def test_abi_argument_errors():
    """refusals by status code, before any launch and so without a GPU"""
    ms = _ms()
    lib = ms._library()
    p, null = C.c_void_p(4096), C.c_void_p(0)                        # never dereferenced: every call is refused first
    big = 1 << 40
    full = ms.Out(**{name: 4096 for name in ms.WHAT})
    out = C.cast(C.pointer(full), C.c_void_p)
    for fn in (lib.smrf_measure_f32, lib.smrf_measure_f64):
        assert fn(p, p, -1, 5, 3, 0, 511, out, p, big, null) == E_ARG
        assert fn(p, p, 5, -1, 3, 0, 511, out, p, big, null) == E_ARG
        assert fn(p, p, 46341, 46341, 3, 0, 511, out, p, big, null) == E_UNSUPPORTED
        assert fn(p, p, 2, 2 ** 30, 3, 0, 511, out, p, big, null) == E_UNSUPPORTED
        assert fn(p, p, 5, 5, -1, 0, 511, out, p, big, null) == E_ARG
        assert fn(p, p, 5, 5, 2 ** 31 - 1, 0, 1, out, p, big, null) == E_UNSUPPORTED
        for mode in (-1, 2):
            assert fn(p, p, 5, 5, 3, mode, 511, out, p, big, null) == E_ARG
        for what in (0, -1, 512):
            assert fn(p, p, 5, 5, 3, 0, what, out, p, big, null) == E_ARG
        assert fn(p, p, 5, 5, 3, 0, 511, null, p, big, null) == E_ARG
        assert fn(null, p, 5, 5, 3, 0, 511, out, p, big, null) == E_ARG
        for name, bit in ms.WHAT.items():                            # a measurement asked for without a place for it
            part = ms.Out(**{k: (0 if k == name else 4096) for k in ms.WHAT})
            assert fn(p, p, 5, 5, 3, 0, bit, C.cast(C.pointer(part), C.c_void_p), p, big, null) == E_ARG, name
        assert fn(p, p, 5, 5, 3, 0, 511, out, null, big, null) == E_WORKSPACE
        assert fn(p, p, 5, 5, 3, 0, 511, out, p, lib.smrf_measure_workspace_bytes(3, 511) - 1, null) == E_WORKSPACE
        assert fn(p, p, 5, 5, 3, 0, 1, out, p, lib.smrf_measure_workspace_bytes(3, 1) - 1, null) == E_WORKSPACE


def test_kernels_compile_without_scratch(tmp_path):
    """csrc/measure.hip for gfx950: clear, the three passes and the finalize kernel for float32 and float64, and the
    variance kernel, all in registers - the 128-bit rounding included"""
    import family_checks as fc
    text, kernels = fc.device_asm("measure", tmp_path)
    for stem, count in (("measure_clear", 1), ("measure_pass1", 2), ("measure_pass2", 2), ("measure_pass3", 2),
                        ("measure_finalize", 2), ("measure_variance", 1)):
        assert len([k for k in kernels if stem in k]) == count, (stem, sorted(kernels))
    assert len(kernels) == 10
    fc.assert_no_scratch(text, kernels)
    # integer atomics only: no float atomic instruction in the unit
    assert not re.search(r"atomic_(add|min|max|pk_add)_b?f(16|32|64)", text)
    assert re.search(r"global_atomic_add_x2", text) and re.search(r"global_atomic_umin_x2", text)


# ------------------------------------------------------------------------------------------
# the interface
# ------------------------------------------------------------------------------------------
def test_signatures_are_scipys():
    ms = _ms()
    for name in NAMES:
        want = list(inspect.signature(getattr(ndi, name)).parameters.values())
        got = list(inspect.signature(getattr(ms, name)).parameters.values())
        assert [(g.name, g.kind, g.default) for g in got] == [(w.name, w.kind, w.default) for w in want], name
    assert [(p.name, p.default) for p in inspect.signature(ms.region_stats).parameters.values()] == [
        ("input", inspect.Parameter.empty), ("labels", inspect.Parameter.empty), ("num_features", None),
        ("what", ("count", "sum", "mean", "variance", "min", "max", "min_index", "max_index"))]


def test_argument_errors_come_from_the_host():
    """every refusal is decided before the device is touched: it is the same with and without a GPU"""
    ms = _ms()
    X = np.zeros((4, 5), np.float32)
    L = np.zeros((4, 5), np.int32)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(2 ** 16, 2 ** 15), strides=(0, 0))
    for name in NAMES + ("region_stats",):
        f = getattr(ms, name)
        lead = (L,) if name == "region_stats" else ()
        for Y in (np.zeros((2, 3, 4), np.float32), np.zeros(5, np.float32), np.float32(1)):
            with pytest.raises(NotImplementedError):
                f(Y, *lead)                                                 # not a 2-D raster
        with pytest.raises(NotImplementedError):
            f(big, *lead)                                                   # 2**31 cells
        for dtype in (np.int64, np.uint64):
            with pytest.raises(NotImplementedError):
                f(np.zeros((4, 5), dtype), *lead)
        for dtype in (np.complex64, np.complex128):
            with pytest.raises(TypeError):
                f(np.zeros((4, 5), dtype), *lead)
        for bad in (np.zeros((4, 5)), np.zeros((4, 5), np.float32)):
            with pytest.raises(TypeError):
                f(X, bad)                                                   # labels must be integers
        for bad in (np.zeros((5, 4), np.int32), np.zeros((4, 6), np.int32), np.zeros((1, 5), np.int32)):
            with pytest.raises(ValueError):
                f(X, bad)                                                   # no broadcasting: the labels have the input's shape
        with pytest.raises(NotImplementedError):
            f(X, np.zeros((4, 5, 1), np.int32))
    for name in NAMES:
        f = getattr(ms, name)
        for bad in ([1.5, 2.0], 2.5, "a", [[1.0]]):
            with pytest.raises(TypeError):
                f(X, L, bad)
    with pytest.raises(TypeError):
        ms.region_stats(X, None)
    with pytest.raises(ValueError):
        ms.region_stats(X, L, -1)
    with pytest.raises(TypeError):
        ms.region_stats(X, L, 2.5)
    for bad in (("median",), ("count", "flags"), (), "sums"):
        with pytest.raises(ValueError):
            ms.region_stats(X, L, 3, bad)


def _scipy_outcome(name, X, lab, index):
    try:
        with np.errstate(all="ignore"):
            return getattr(ndi, name)(X, lab, index)
    except Exception as e:                                  # noqa: BLE001: the type is what is asked for
        return type(e)


def test_empty_rasters_need_no_device():
    """what SciPy gives for a raster without cells, or what it raises, under every form; the table of region_stats"""
    import warnings
    ms = _ms()
    compared = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for shape in ((0, 5), (4, 0), (0, 0)):
            X, L = np.zeros(shape, np.float32), np.zeros(shape, np.int32)
            for name in NAMES:
                for lab, index in ((None, None), (L, None), (L, 2), (L, [1, 2, 0])):
                    want = _scipy_outcome(name, X, lab, index)
                    if isinstance(want, type):
                        with pytest.raises(want):
                            getattr(ms, name)(X, lab, index)
                    else:
                        got = getattr(ms, name)(X, lab, index)
                        assert np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), equal_nan=True), (
                            shape, name, index, got, want)
                    compared += 1
            T = ms.region_stats(X, L)
            assert sorted(T) == sorted(ms.STATS) and all(isinstance(v, np.ndarray) and v.shape == (1,) for v in T.values())
            T = ms.region_stats(X, L, 2, ("count", "sum", "mean", "min", "max_index"))
            assert T["count"].tolist() == [0, 0, 0] and T["count"].dtype == np.int64 and T["sum"].tolist() == [0.0] * 3
            assert np.isnan(T["mean"]).all() and T["min"].dtype == np.float32 and T["min"].tolist() == [0] * 3
            assert T["max_index"].tolist() == [-1] * 3 and T["max_index"].dtype == np.int64
    assert compared == 3 * 9 * 4


def test_valid_call_without_a_gpu_raises():
    import torch
    import neilpy_amd
    ms = _ms()
    if torch.cuda.is_available():
        return                                                 # tests/test_gpu_measure.py runs the valid calls
    X = np.ones((4, 5), np.float32)
    L = np.ones((4, 5), np.int32)
    calls = [lambda f=getattr(ms, name): f(X, L, [1]) for name in NAMES]
    calls += [lambda: ms.sum_labels(X), lambda: ms.minimum(X.astype(np.uint8), L), lambda: ms.region_stats(X, L, 1, ("count",))]
    for call in calls:
        with pytest.raises(neilpy_amd.SmrfHipError):
            call()
