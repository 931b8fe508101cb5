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

``runs_from_plan`` is a model of the device's runs path instead: it computes from the packed plan of
``morphology.plan``, as footprint_runs_kernel does, so that tests/test_footprint_draws_host.py can tell a wrong plan
from a wrong kernel.
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


TX, TY = 64, 8                 # the workgroup's cells (csrc/footprint.hip)


def runs_from_plan(X, head, table, mode, op, nan_aware=None):
    """What footprint_runs_kernel computes from the packed ``head`` and ``table`` of ``morphology.plan``, workgroup by
    workgroup of 64 x 8 cells: the TH x LW tile staged through ``index``; level k built from level k - 1 into the plane
    ``slots[k]`` with the kernel's ``pair`` rule (a cell whose partner lies past the plane keeps its value); then, from
    the planes as the last level left them, every run record read at ``tcol`` and ``tcol2`` of its slot and reduced.
    ``op`` is 'min', 'max' or 'both' (a second set of planes; the result is max - min); fmin / fmax ignore a NaN, and
    with ``nan_aware`` (default: X holds a NaN) a NaN first visited sample makes the result NaN.  A plane nothing wrote
    is None here, so a plan that reads one fails loudly."""
    X = np.asarray(X)
    rows, cols = X.shape
    head, table = np.asarray(head), np.asarray(table)
    ntaps, nruns, r_lo, c_lo, bh, bw, maxlevel, nplanes = (int(v) for v in head[:8])
    slots = [int(v) for v in head[8:9 + maxlevel]]
    taps, runs = table[:2 * ntaps].reshape(ntaps, 2), table[2 * ntaps:].reshape(nruns, 4).tolist()
    TH, LW = TY + bh - 1, TX + bw - 1
    fs = {"min": (np.fmin,), "max": (np.fmax,), "both": (np.fmin, np.fmax)}[op]
    out = [np.empty_like(X) for _ in fs]
    for r0 in range(0, rows, TY):
        for c0 in range(0, cols, TX):
            tile = X[index(r0 + r_lo + np.arange(TH), rows, mode)][:, index(c0 + c_lo + np.arange(LW), cols, mode)]
            for f, res in zip(fs, out):
                planes = [None] * nplanes
                planes[slots[0]] = tile.copy()
                for k in range(1, maxlevel + 1):
                    half = 1 << (k - 1)
                    src = planes[slots[k - 1]]
                    dst = src.copy()
                    dst[:, :LW - half] = f(src[:, :LW - half], src[:, half:])
                    assert slots[k] != slots[k - 1]
                    planes[slots[k]] = dst
                acc = None
                for trow, tcol, tcol2, slot in runs:
                    p = planes[slot]
                    v = p[trow:trow + TY, tcol:tcol + TX]
                    if tcol2 != tcol:
                        v = f(v, p[trow:trow + TY, tcol2:tcol2 + TX])
                    assert v.shape == (TY, TX), (trow, tcol, tcol2, slot)
                    acc = v if acc is None else f(acc, v)
                res[r0:r0 + TY, c0:c0 + TX] = acc[:rows - r0, :cols - c0]
    if np.isnan(X).any() if nan_aware is None else nan_aware:
        i, j = np.arange(rows), np.arange(cols)
        first = X[index(i + int(taps[0, 0]), rows, mode)][:, index(j + int(taps[0, 1]), cols, mode)]
        for res in out:
            res[np.isnan(first)] = np.nan
    return _minus(out[1], out[0]) if op == "both" else out[0]


def scipy_comparable(footprint, shape):
    """SciPy's reflect table reads out of bounds for very large footprints: it is the oracle only
    with a half-extent below 2 * min(rows, cols)"""
    return max(np.shape(footprint)) // 2 < 2 * min(shape)
