"""Brute-force NumPy restatement of the nearest-source contract: all pairs, small rasters only.

A hole is a cell where ``np.isfinite`` is false, a source any other cell.  The distance of two cells is the integer
``(r - r')**2 + (c - c')**2``.  Every hole takes the bits of the source at the minimal distance; among several the lowest
flat index (lowest row, then lowest column) wins.  Sources keep their value, and a raster without a source is unchanged
(index -1, squared distance 2**32 - 1, as the library reports it).
"""
import numpy as np

NO_SOURCE_DIST2 = 2 ** 32 - 1


def feature_transform(X, chunk=512):
    """``(index, dist2, n_ties)`` of a 2-D raster: the flat int64 index of every cell's nearest source (its own for a
    source), the exact squared distance (int64) and the number of sources at that distance"""
    X = np.asarray(X)
    rows, cols = X.shape
    finite = np.isfinite(X)
    src = np.flatnonzero(finite.ravel())                    # ascending flat index
    index = np.full(rows * cols, -1, dtype=np.int64)
    dist2 = np.full(rows * cols, NO_SOURCE_DIST2, dtype=np.int64)
    nties = np.zeros(rows * cols, dtype=np.int64)
    if src.size:
        sr, sc = np.divmod(src, cols)
        for lo in range(0, rows * cols, chunk):
            cell = np.arange(lo, min(lo + chunk, rows * cols))
            r, c = np.divmod(cell, cols)
            d = (r[:, None] - sr[None, :]) ** 2 + (c[:, None] - sc[None, :]) ** 2
            k = np.argmin(d, axis=1)                        # the first minimum: the lowest flat index
            index[cell] = src[k]
            dist2[cell] = d[np.arange(cell.size), k]
            nties[cell] = (d == dist2[cell][:, None]).sum(axis=1)
    return index.reshape(rows, cols), dist2.reshape(rows, cols), nties.reshape(rows, cols)


def inpaint_nearest(X):
    """a filled copy of ``X`` (the library fills in place; the rule is the same)"""
    X = np.asarray(X)
    index, _, _ = feature_transform(X)
    out = X.copy()
    if (index >= 0).all():
        out = X.ravel()[index.ravel()].reshape(X.shape).copy()
    return out


def candidates(X, dist2):
    """for every hole the set of values a valid nearest-source fill may give: yields ``(r, c, values)``"""
    X = np.asarray(X)
    finite = np.isfinite(X)
    sr, sc = np.nonzero(finite)
    for r, c in zip(*np.nonzero(~finite)):
        d = (sr - r) ** 2 + (sc - c) ** 2
        yield r, c, X[sr[d == dist2[r, c]], sc[d == dist2[r, c]]]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(a.view(u), b.view(u))
