"""Grey morphology with an arbitrary flat footprint in plain NumPy - TEST INFRASTRUCTURE, the restatement of the contract
of DESIGN.md section 19 that the GPU tests compare against where SciPy cannot serve (all-ones footprints on NaN rasters,
footprints so large that SciPy's reflect table reads out of bounds).

With ``ch, cw = KH // 2, KW // 2`` and ``idx`` the period-2n reflect (``morph_numpy.fold``) for 'reflect' and the clamp
for 'nearest':

    E[i, j] = min over members (s, t) of X[idx(i + s - ch, R), idx(j + t - cw, C)]
    D[i, j] = max over members (s, t) of X[idx(i - (s - ch), R), idx(j - (t - cw), C)]

NaN: the result is NaN iff the first visited member's sample is NaN, every other NaN is ignored.  The first visited
member is the first in row-major order for the erosion and the last (at its mirrored offset) for the dilation - the loop
of ndimage's footprint filter, ``res = first; for the others: if v < res: res = v``.  Written here exactly so: one
gather per member, valid for any footprint size.  min / max do not order -0.0 against +0.0: comparisons are by value.
"""
import numpy as np

from morph_numpy import fold


def index(i, n, mode):
    if mode == "reflect":
        return fold(i, n)
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    raise NotImplementedError(mode)


def members(footprint):
    fp = np.asarray(footprint) != 0
    assert fp.ndim == 2 and fp.any()
    s, t = np.nonzero(fp)                      # row-major
    return s - fp.shape[0] // 2, t - fp.shape[1] // 2


def _filter(X, footprint, mode, dilate):
    X = np.asarray(X)
    rows, cols = X.shape
    dr, dc = members(footprint)
    if dilate:
        dr, dc = -dr[::-1], -dc[::-1]
    if X.size == 0:
        return X.copy()
    i, j = np.arange(rows), np.arange(cols)
    res = None
    for a, b in zip(dr, dc):
        v = X[index(i + a, rows, mode)][:, index(j + b, cols, mode)]
        if res is None:
            res = v.copy()
        else:
            take = v > res if dilate else v < res          # False wherever either is NaN
            res[take] = v[take]
    return res


def grey_erosion(X, footprint, mode="reflect"):
    return _filter(X, footprint, mode, False)


def grey_dilation(X, footprint, mode="reflect"):
    return _filter(X, footprint, mode, True)


def grey_opening(X, footprint, mode="reflect"):
    return grey_dilation(grey_erosion(X, footprint, mode), footprint, mode)


def grey_closing(X, footprint, mode="reflect"):
    return grey_erosion(grey_dilation(X, footprint, mode), footprint, mode)


def _minus(a, b):
    with np.errstate(invalid="ignore", over="ignore"):      # inf - inf
        return a - b


def white_tophat(X, footprint, mode="reflect"):
    return _minus(np.asarray(X), grey_opening(X, footprint, mode))


def black_tophat(X, footprint, mode="reflect"):
    return _minus(grey_closing(X, footprint, mode), np.asarray(X))


def morphological_gradient(X, footprint, mode="reflect"):
    return _minus(grey_dilation(X, footprint, mode), grey_erosion(X, footprint, mode))


FUNCTIONS = {f.__name__: f for f in (grey_erosion, grey_dilation, grey_opening, grey_closing, white_tophat, black_tophat,
                                     morphological_gradient)}


def scipy_comparable(footprint, shape):
    """SciPy's reflect table reads out of bounds for very large footprints: it is the oracle only
    with a half-extent below 2 * min(rows, cols)"""
    return max(np.shape(footprint)) // 2 < 2 * min(shape)
