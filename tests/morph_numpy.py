"""Disk erosion / dilation and progressive_filter in plain NumPy - TEST INFRASTRUCTURE, the fast reference of the GPU tests.

Written from the contract in DESIGN.md sections 2 and 4, not from kernel code:

    E[y, x] = min over (dy, dx) with dx^2 + dy^2 <= r^2 of Z[fold(y + dy, rows), fold(x + dx, cols)]
            = min over |dy| <= r of min over |dx| <= w(dy) of the same cells,  w(dy) = isqrt(r^2 - dy^2)

with `fold` the period-2n reflect (... 1 0 | 0 1 ... n-1 | n-1 n-2 ...), dilation the same with max, and the reference's
loop and flag rule around them (neilpy.py:1659-1680).  Both lines are written out, in the input's dtype:
* form="cells": the reflected padding is gathered once, then one running np.minimum / np.maximum per disk cell over a
  shifted slice - pi r^2 array operations; about ten times faster than SciPy's grey_erosion on large disks;
* form="rows" (what progressive_filter uses): the same padding, the running minimum over |dx| <= w grown one column pair at
  a time, and every row offset dy takes it at w = w(dy) - 4 r + 1 array operations, the same minimum over the same cells
  (min and max are exact, so the grouping changes no bit).
tests/test_morph_numpy.py pins BOTH to oracle/smrf_oracle.py (SciPy) and to each other, bit for bit.  Unlike SciPy's reflect
table they are valid for any radius (SciPy reads out of bounds from r >= 4 min(rows, cols)).

min / max do not order -0.0 against +0.0 (neither does SciPy): a raster compared through this module holds one sign of
zero only, and comparisons are by value (np.array_equal).  NaN is not handled (SciPy's NaN rule is the oracle's business).
"""
from math import isqrt

import numpy as np


def fold(i, n):
    """index i of an axis of n cells under the period-2n reflect"""
    p = np.mod(i, 2 * n)
    return np.where(p < n, p, 2 * n - 1 - p)


def disk_offsets(r):
    """every (dy, dx) of the digital disk of radius r"""
    r = int(r)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def _padded(Z, r):
    rows, cols = Z.shape
    return np.ascontiguousarray(Z[fold(np.arange(-r, rows + r), rows)][:, fold(np.arange(-r, cols + r), cols)])


def _by_cells(Z, r, op):
    rows, cols = Z.shape
    P = _padded(Z, r)
    wp = cols + 2 * r
    flat = P.ravel()
    n = (rows - 1) * wp + cols                            # the outputs as ONE contiguous run of the padded raster (the
    buf = np.empty(rows * wp, dtype=Z.dtype)              # 2 r cells between two rows' outputs are computed and dropped)
    out = buf[:n]
    out[...] = flat[r * wp + r:r * wp + r + n]
    for dy, dx in disk_offsets(r):
        at = (r + dy) * wp + r + dx
        op(out, flat[at:at + n], out=out)
    return buf.reshape(rows, wp)[:, :cols].copy()


def _by_rows(Z, r, op):
    rows, cols = Z.shape
    P = _padded(Z, r)
    H = P[:, r:r + cols].copy()                           # running op over |dx| <= w, for every padded row
    out = None
    for w in range(r + 1):
        if w:
            op(H, P[:, r - w:r - w + cols], out=H)
            op(H, P[:, r + w:r + w + cols], out=H)
        for dy in range(-r, r + 1):
            if isqrt(r * r - dy * dy) == w:
                out = H[r + dy:r + dy + rows].copy() if out is None else op(out, H[r + dy:r + dy + rows], out=out)
    return out


def _disk_op(Z, r, op, form):
    Z = np.asarray(Z)
    if form not in ("cells", "rows"):
        raise ValueError("form is 'cells' or 'rows'")
    return (_by_cells if form == "cells" else _by_rows)(Z, int(r), op)


def erosion(Z, r, form="cells"):
    return _disk_op(Z, r, np.minimum, form)


def dilation(Z, r, form="cells"):
    return _disk_op(Z, r, np.maximum, form)               # the disk is its own reflection


def progressive_filter(Z, windows, cellsize=1, slope_threshold=.15, return_when_dropped=False, return_surfaces=False,
                       form="rows"):
    """the oracle's loop (oracle/smrf_oracle.py progressive_filter) on the erosion / dilation above.  With
    return_surfaces also the eroded and the opened surface of every window, as two lists."""
    Z = np.asarray(Z)
    windows = np.asarray(windows)
    last_surface = Z.copy()
    elevation_thresholds = slope_threshold * (windows * cellsize)
    is_object_cell = np.zeros(Z.shape, dtype=bool)
    when_dropped = np.zeros(Z.shape, dtype=np.uint8)
    eroded, opened = [], []
    for i, window in enumerate(windows):
        e = erosion(last_surface, window, form)
        this_surface = dilation(e, window, form)
        with np.errstate(invalid="ignore", over="ignore"):              # inf - inf: NaN, never an object
            new_obj = last_surface - this_surface > elevation_thresholds[i]
        is_object_cell = is_object_cell | new_obj
        when_dropped[new_obj] = i
        eroded.append(e)
        opened.append(this_surface)
        if len(windows) > 1:
            last_surface = this_surface
    out = (is_object_cell,)
    if return_when_dropped:
        out += (when_dropped,)
    if return_surfaces:
        out += (eroded, opened)
    return out[0] if len(out) == 1 else out
