"""create_dem's device steps, once: the extent of a cloud and the clear -> bin -> finalize of a band of raster rows
(csrc/grid.hip).  ``api`` grids the whole raster with them, ``sharded`` one rank's band; DESIGN.md, the create_dem section.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._raster import _ptr, _stream, _torch

EXTENT_PARTS = 1024      # most partial rows of four doubles the extent reduction writes (csrc/cloud_reduce.h)


def extent(xd, yd):
    """``(xmin, xmax, ymin, ymax)`` of the float64 device arrays as Python floats: four NaN if a coordinate is NaN, as
    np.min / np.max answer; ``(inf, -inf, inf, -inf)`` for no points"""
    if xd.numel() == 0:
        return (np.inf, -np.inf, np.inf, -np.inf)
    ws = _torch().empty(4 * EXTENT_PARTS, dtype=_torch().float64, device=xd.device)
    ext = (C.c_double * 4)()
    _lib.check(_lib.load().smrf_points_extent_f64(_ptr(xd), _ptr(yd), xd.numel(), ext, _ptr(ws), ws.numel() * 8, _stream()))
    return tuple(float(v) for v in ext)


def grid_rows(xd, yd, zd, inv, grid_shape, row0, rows_local, bin_type, h_filter=None):
    """Rows ``[row0, row0 + rows_local)`` of the ``(ny, nx)`` raster whose inverse transform is ``inv`` (a, b, c, d, e, f):
    ``(float64 grid, uint8 empty mask, points outside the whole raster)``.  Points of other rows are passed over;
    ``h_filter`` = (xedges[0], xedges[-1], yedges[-1], yedges[0]) drops the points outside given edges first
    (neilpy.py:1128).  Any ``bin_type`` but 'max' bins the minimum: the caller refuses the others."""
    torch = _torch()
    lib = _lib.load()
    ny, nx = grid_shape
    keys = torch.empty((rows_local, nx), dtype=torch.int64, device=xd.device)
    n_out = torch.zeros(1, dtype=torch.int64, device=xd.device)
    grid = torch.empty((rows_local, nx), dtype=torch.float64, device=xd.device)
    empty = torch.empty((rows_local, nx), dtype=torch.uint8, device=xd.device)
    h_inv = (C.c_double * 6)(*[float(v) for v in inv])
    if h_filter is not None:
        h_filter = (C.c_double * 4)(*[float(v) for v in h_filter])
    is_max = 1 if bin_type == 'max' else 0
    _lib.check(lib.smrf_grid_clear_u64(_ptr(keys), keys.numel(), _stream()))
    _lib.check(lib.smrf_grid_bin_f64(_ptr(xd), _ptr(yd), _ptr(zd), xd.numel(), h_inv, h_filter, _ptr(keys), ny, nx, row0,
                                     rows_local, is_max, _ptr(n_out), _stream()))
    _lib.check(lib.smrf_grid_finalize_f64(_ptr(keys), _ptr(grid), _ptr(empty), keys.numel(), is_max, _stream()))
    return grid, empty, int(n_out.item())
