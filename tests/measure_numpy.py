"""The contract of neilpy_amd/measure.py restated in plain Python (a helper module, no test in it).

The sums are made with Python integers and ``fractions.Fraction``: every term becomes the integer
``trunc(t * 2**(93 - E))``, the integers are added, and the total times ``2**(E - 93)`` is rounded once by ``float``.  The
extrema are the ends of ``np.sort``, the positions ``np.flatnonzero(...)[0]`` on the order-preserving keys, and the
``labels`` / ``index`` forms are SciPy's.  Slow, and meant to be: nothing here is shared with the kernels.
"""
import math
from fractions import Fraction

import numpy as np

BITS = 93
STATS = ("count", "sum", "mean", "variance", "min", "max", "min_index", "max_index")


def exponent_of(M):
    """E with 2**(E - 1) <= M < 2**E"""
    return math.frexp(M)[1]


def quantum(t, E):
    """trunc(t * 2**(93 - E)) of a finite float, exactly"""
    num, den = float(t).as_integer_ratio()                  # den is a power of two
    shift = BITS - E - (den.bit_length() - 1)
    q = abs(num) << shift if shift >= 0 else abs(num) >> -shift
    return -q if num < 0 else q


def round_scaled(total, E):
    """total * 2**(E - 93) as the nearest float, ties to even; beyond the largest float the infinity"""
    try:
        return float(Fraction(total) * Fraction(2) ** (E - BITS))
    except OverflowError:
        return math.inf if total > 0 else -math.inf


def contract_sum(terms, E):
    """the sum of fp64 terms under the contract; ``E`` None: no finite magnitude above zero"""
    terms = [float(t) for t in terms]
    if any(math.isnan(t) for t in terms) or (math.inf in terms and -math.inf in terms):
        return math.nan
    if math.inf in terms:
        return math.inf
    if -math.inf in terms:
        return -math.inf
    if E is None or not terms:
        return 0.0
    return round_scaled(sum(quantum(t, E) for t in terms), E)


def keys(x):
    """order-preserving uint64 keys of float64 values, every NaN last: np.sort's order, -0.0 before +0.0"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    sign = np.uint64(1 << 63)
    k = np.where(b & sign != 0, ~b, b | sign)
    return np.where(np.isnan(x), np.uint64(2 ** 64 - 1), k)


def group_stats(values, positions):
    """every measurement of one group: its values in C order, in the input's dtype, and their linear indices"""
    x = values.astype(np.float64)
    count = x.size
    out = {"count": count, "flags": (1 if np.isnan(x).any() else 0) | (2 if (x == np.inf).any() else 0) | (4 if (x == -np.inf).any() else 0)}
    fin = np.abs(x[np.isfinite(x)])
    M = float(fin.max()) if fin.size else 0.0
    E = exponent_of(M) if M > 0 else None
    with np.errstate(all="ignore"):
        total = np.float64(contract_sum(x, E))
        mean = total / np.float64(count)
        d = x - mean
        sq = d * d
        var = np.float64(contract_sum(sq, None if E is None else 2 * E + 3)) / np.float64(count)
    out.update(sum=total, mean=mean, variance=var)
    if count == 0:
        out.update(min=values.dtype.type(0), max=values.dtype.type(0), min_index=-1, max_index=-1)
        return out
    s = np.sort(values)
    k = keys(x)
    out.update(min=s[0], max=s[-1], min_index=int(positions[np.flatnonzero(k == k.min())[0]]),
               max_index=int(positions[np.flatnonzero(k == k.max())[0]]))
    return out


def region_stats(X, L, n):
    """{name: array of n + 1} over labels 0..n; cells below 0 or above n are ignored"""
    X, L = np.asarray(X), np.asarray(L)
    flat, lab = X.ravel(), L.ravel()
    order = np.argsort(lab, kind="stable")                  # the cells of each label together, in C order
    start = np.searchsorted(lab[order], np.arange(n + 2))
    rows = [group_stats(flat[order[start[k]:start[k + 1]]], order[start[k]:start[k + 1]]) for k in range(n + 1)]
    dtypes = dict(count=np.int64, sum=np.float64, mean=np.float64, variance=np.float64, min=X.dtype, max=X.dtype,
                  min_index=np.int64, max_index=np.int64, flags=np.int32)
    return {name: np.array([r[name] for r in rows], dtype=dt) for name, dt in dtypes.items()}


# ------------------------------------------------------------------------------------------
# scipy.ndimage's forms
# ------------------------------------------------------------------------------------------
def _groups(input, labels, index):
    """(scalar?, one selection, [boolean masks over the flat raster])"""
    X = np.asarray(input)
    if labels is None:
        return True, True, [np.ones(X.size, bool)]
    lab = np.asarray(labels).ravel()
    if index is None:
        return True, True, [lab > 0]
    if np.ndim(index) == 0:
        return True, True, [(lab == index) & (lab >= 0)]
    return False, False, [(lab == k) & (lab >= 0) for k in np.asarray(index).ravel()]


def _measure(input, labels, index, name):
    X = np.asarray(input)
    scalar, single, masks = _groups(input, labels, index)
    flat = X.ravel()
    res = []
    for m in masks:
        g = group_stats(flat[m], np.flatnonzero(m))
        v = g[name]
        if single and name in ("min", "max") and g["flags"] & 1:
            v = X.dtype.type(np.nan)                         # np.min / np.max of the selection
        res.append(v)
    if name in ("min_index", "max_index"):
        cols = max(X.shape[1], 1)
        res = [(max(v, 0) // cols, max(v, 0) % cols) for v in res]
        return res[0] if scalar else res
    dt = X.dtype if name in ("min", "max") else np.float64
    return np.dtype(dt).type(res[0]) if scalar else np.array(res, dtype=dt)


def sum_labels(input, labels=None, index=None):
    return _measure(input, labels, index, "sum")


def mean(input, labels=None, index=None):
    return _measure(input, labels, index, "mean")


def variance(input, labels=None, index=None):
    return _measure(input, labels, index, "variance")


def standard_deviation(input, labels=None, index=None):
    with np.errstate(all="ignore"):
        return np.sqrt(variance(input, labels, index))


def minimum(input, labels=None, index=None):
    return _measure(input, labels, index, "min")


def maximum(input, labels=None, index=None):
    return _measure(input, labels, index, "max")


def minimum_position(input, labels=None, index=None):
    return _measure(input, labels, index, "min_index")


def maximum_position(input, labels=None, index=None):
    return _measure(input, labels, index, "max_index")


def extrema(input, labels=None, index=None):
    return (minimum(input, labels, index), maximum(input, labels, index), minimum_position(input, labels, index),
            maximum_position(input, labels, index))


# ------------------------------------------------------------------------------------------
# the error bounds of DESIGN.md section 22, computed from the data
# ------------------------------------------------------------------------------------------
def exact_sum(terms):
    return sum((Fraction(float(t)) for t in terms), Fraction(0))


def ulp(v):
    return Fraction(float(np.spacing(np.abs(np.float64(v))))) if np.isfinite(v) else Fraction(0)


def contract_bound(terms, E, result):
    """|contract sum - exact| <= ulp(result) / 2 + n 2**(E - 93)"""
    return ulp(result) / 2 + len(terms) * Fraction(2) ** (E - BITS)


def sequential_bound(terms):
    """|a sequential (or pairwise) fp64 sum - exact| <= n 2**-52 sum |t_i|: (1 + 2**-53)**(n - 1) - 1 < n 2**-52 for the
    n of a raster"""
    return len(terms) * Fraction(2) ** -52 * sum((abs(Fraction(float(t))) for t in terms), Fraction(0))


# ------------------------------------------------------------------------------------------
# values and label rasters the tests share
# ------------------------------------------------------------------------------------------
def dtm(shape, seed, dtype=np.float64):
    """a synthetic terrain: a tilted plane, two waves and noise, some hundreds of metres up"""
    rng = np.random.default_rng([20270301, seed] + list(shape))
    r, c = np.indices(shape)
    z = 312.5 + 0.31 * r - 0.17 * c + 9.0 * np.sin(r / 7.0) * np.cos(c / 11.0) + rng.normal(0.0, 0.4, shape)
    return z.astype(dtype)


def distinct(shape, seed, dtype=np.float64):
    """values that are all different, in a shuffled order: every extremum has one position"""
    rng = np.random.default_rng([20270302, seed] + list(shape))
    n = shape[0] * shape[1]
    return (rng.permutation(n).reshape(shape) - n // 3).astype(dtype)


def cancelling(shape, seed):
    """1000 +- 1e-3: the variance under cancellation"""
    rng = np.random.default_rng([20270303, seed] + list(shape))
    return 1000.0 + rng.uniform(-1e-3, 1e-3, shape)


def decades(shape, seed, lo=-20, hi=20):
    """magnitudes mixed over the decades lo..hi, both signs"""
    rng = np.random.default_rng([20270304, seed] + list(shape))
    return rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 10.0, shape) * 10.0 ** rng.integers(lo, hi + 1, shape)


def checker_labels(shape):
    """a checkerboard of distinct labels: every stretch of equal labels has length 1 (0 between them)"""
    r, c = np.indices(shape)
    on = (r + c) % 2 == 0
    return np.where(on, np.cumsum(on.ravel()).reshape(shape), 0).astype(np.int32)
