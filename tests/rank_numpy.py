"""Rank filters with an arbitrary flat footprint in plain NumPy - TEST INFRASTRUCTURE, the restatement of the contract of
DESIGN.md section 20 that the GPU tests compare against where SciPy cannot serve (NaN rasters, footprints so large that
SciPy's reflect table reads out of bounds).  tests/test_rank_host.py pins it to SciPy.  It does not import the package.

With ``ch, cw = KH // 2, KW // 2`` and ``idx`` the period-2n reflect (``morph_numpy.fold``) for 'reflect' and the clamp
for 'nearest', the samples of cell (i, j) are ``X[idx(i + s - ch, R), idx(j + t - cw, C)]`` over the members (s, t), and

    out[i, j] = np.sort(samples)[rank]

np.sort puts NaN last, whatever its sign, and -0.0 and +0.0 compare equal: comparisons are by value.  The rank is
SciPy's (``resolve``).
"""
import operator

import numpy as np

from footprint_numpy import index, members


def resolve(kind, n, value=None):
    """scipy.ndimage._filters._rank_filter's rank of a footprint of n members"""
    if kind == "median":
        rank = n // 2
    elif kind == "minimum":
        rank = 0
    elif kind == "maximum":
        rank = n - 1
    elif kind == "percentile":
        p = value
        if p < 0.0:
            p += 100.0
        if p < 0 or p > 100:
            raise RuntimeError('invalid percentile')
        rank = n - 1 if p == 100.0 else int(float(n) * p / 100.0)
    else:
        rank = operator.index(value)
    if rank < 0:
        rank += n
    if rank < 0 or rank >= n:
        raise RuntimeError('rank not within filter footprint size')
    return rank


def samples(X, footprint, mode="reflect"):
    """(rows, cols, n): every cell's samples, the members in row-major order"""
    X = np.asarray(X)
    rows, cols = X.shape
    dr, dc = members(footprint)
    i, j = np.arange(rows), np.arange(cols)
    out = np.empty((rows, cols, len(dr)), dtype=X.dtype)
    for k, (a, b) in enumerate(zip(dr, dc)):
        out[:, :, k] = X[index(i + a, rows, mode)][:, index(j + b, cols, mode)]
    return out


def rank_filter(X, rank, footprint, mode="reflect"):
    X = np.asarray(X)
    if X.size == 0:
        return X.copy()
    S = samples(X, footprint, mode)
    return np.sort(S, axis=-1)[..., resolve("rank", S.shape[-1], rank)]


def _named(kind):
    def f(X, footprint, mode="reflect", value=None):
        n = int(np.count_nonzero(np.asarray(footprint)))
        return rank_filter(X, resolve(kind, n, value), footprint, mode)
    f.__name__ = kind + "_filter"
    return f


median_filter, minimum_filter, maximum_filter = _named("median"), _named("minimum"), _named("maximum")


def percentile_filter(X, percentile, footprint, mode="reflect"):
    return _named("percentile")(X, footprint, mode, percentile)


def masked_count_rule(X, rank, footprint, mode="reflect"):
    """the NaN rule stated on its own: NaN iff fewer than rank + 1 samples are not NaN, else the rank-th of the others"""
    S = samples(np.asarray(X), footprint, mode)
    rank = resolve("rank", S.shape[-1], rank)
    out = np.empty(S.shape[:2], dtype=S.dtype)
    for i in range(S.shape[0]):
        for j in range(S.shape[1]):
            v = S[i, j][~np.isnan(S[i, j])]
            out[i, j] = np.sort(v)[rank] if len(v) >= rank + 1 else np.nan
    return out
