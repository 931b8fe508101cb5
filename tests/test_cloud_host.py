"""create_dem's one gridding path (neilpy_amd/_cloud.py) without a GPU: who may name the four ABI calls it owns, and
that every caller reaches ``_cloud.grid_rows`` with its own band and filter."""
import glob
import os

import numpy as np
import pytest

from conftest import ROOT

OWNED = ("smrf_grid_bin_f64", "smrf_grid_clear_u64", "smrf_grid_finalize_f64", "smrf_points_extent_f64")


def test_cloud_owns_its_abi_calls():
    """the clear / bin / finalize calls and the extent call are named in _cloud.py only (and in _lib.py's signatures)"""
    users = {name: set() for name in OWNED}
    for path in glob.glob(os.path.join(ROOT, "neilpy_amd", "*.py")):
        text = open(path).read()
        for name in OWNED:
            if name in text:
                users[name].add(os.path.basename(path))
    for name in OWNED:
        assert users[name] - {"_lib.py"} == {"_cloud.py"}, (name, users[name])
        assert "_lib.py" in users[name], name


class Points:
    """stand-in for a device array of n coordinates"""

    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


def test_every_caller_reaches_grid_rows(monkeypatch):
    from neilpy_amd import _cloud, _lib, api, sharded
    calls = []

    def recorder(xd, yd, zd, inv, grid_shape, row0, rows_local, bin_type, h_filter=None):
        assert len(tuple(inv)) == 6
        calls.append((tuple(grid_shape), row0, rows_local, bin_type, h_filter is None))
        nx = grid_shape[1]
        return np.zeros((rows_local, nx)), np.ones((rows_local, nx), np.uint8), 0

    monkeypatch.setattr(_cloud, "grid_rows", recorder)
    monkeypatch.setattr(_cloud, "extent", lambda xd, yd: (0.0, 9.0, 0.0, 99.0))
    monkeypatch.setattr(_lib, "load", lambda: None)
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    xd = yd = zd = Points(5)
    inv = (1.0, 0.0, 0.5, 0.0, -1.0, 99.5)

    # the replicated-points band of rank 7 of 16: rows 46..51 of 100
    assert sharded.band_rows(100, 16, 7) == (46, 52)
    grid, empty, n_out = sharded.create_dem_band(xd, yd, zd, inv, (100, 10), rank=7, world_size=16, bin_type='min')
    assert calls.pop() == ((100, 10), 46, 6, 'min', True)
    assert grid.shape == (6, 10) and empty.shape == (6, 10) and n_out == 0

    # the sharded-points band: what the driver hands over goes through as it is
    grid, empty, n_out = sharded.HipPointOps().bin_band(xd, yd, zd, inv, (100, 10), 46, 6, 'max')
    assert calls.pop() == ((100, 10), 46, 6, 'max', True)
    assert grid.shape == (6, 10) and n_out == 0
    assert sharded.HipPointOps().extent(xd, yd) == (0.0, 9.0, 0.0, 99.0)

    # the whole raster: from the extent (no filter), and inside given edges (a filter)
    grid, empty, t = api._create_dem_device(xd, yd, zd, 1, 'min', None)
    xedges, yedges = api._edges_from_extent(np.float64(0.0), np.float64(9.0), np.float64(0.0), np.float64(99.0), 1)
    ny, nx = len(yedges) - 1, len(xedges) - 1
    assert calls.pop() == ((ny, nx), 0, ny, 'min', True)
    assert grid.shape == (ny, nx) and tuple(t)[:6] == (1.0, 0.0, xedges[0], 0.0, -1.0, yedges[0])
    grid, empty, t = api._create_dem_device(xd, yd, zd, 1, 'max', (xedges, yedges))
    assert calls.pop() == ((ny, nx), 0, ny, 'max', False)
    assert not calls

    # the order of the two errors: a point outside the raster is reported before an unknown bin type
    monkeypatch.setattr(_cloud, "grid_rows", lambda *a, **k: (None, None, 3))
    for bin_type in ('median', 'max'):
        with pytest.raises(ValueError, match="^invalid entry in coordinates array$"):
            api._create_dem_device(xd, yd, zd, 1, bin_type, None)
    monkeypatch.setattr(_cloud, "grid_rows", lambda *a, **k: (None, None, 0))
    with pytest.raises(ValueError, match="^This type not supported.$"):
        api._create_dem_device(xd, yd, zd, 1, 'median', None)
