"""NumPy restatement of the voxelize contract, written from the contract and held to the reference's
goldens (tests/golden/voxel.npz) bit for bit by tests/test_voxel_host.py.  It decides the device tests.

Nothing here calls ``np.histogramdd``: the bin rule is spelled out (``bins_of``), so that the kernel's walk along the
edges has something independent to be compared with."""
import operator

import numpy as np


def cloud_dtype(x, y, z):
    """float32 when all three arrays are, float64 otherwise (mixed dtypes are widened first: a deviation)"""
    return np.float32 if all(np.asarray(a).dtype == np.float32 for a in (x, y, z)) else np.float64


def edges_of(x, y, z, resolution, ve):
    """((xbins, ybins, zbins) as float64, (min_x, min_y, min_z), (dx, dy, dz)): the reference's expressions (neilpy.py:224
    to :238) on arrays of the cloud's dtype, ``resolution`` and ``ve`` as Python numbers"""
    T = cloud_dtype(x, y, z)
    resolution, ve = operator.index(resolution), float(ve)
    x, y, z = (np.asarray(a, dtype=T) for a in (x, y, z))
    mins = (np.min(x), np.min(y), np.min(z))
    d = (x - mins[0], y - mins[1], z - mins[2])
    max_x, max_y, max_z = np.max(d[0]), np.max(d[1]), np.max(d[2])
    if max_x > max_y:
        interval = np.ceil(max_x) / resolution
    else:
        interval = np.ceil(max_y) / resolution
    xbins = np.arange(0, np.ceil(max_x) + interval, interval)
    ybins = np.arange(0, np.ceil(max_y) + interval, interval)
    zbins = np.arange(0, np.ceil(max_z) + interval / ve, interval / ve)
    return tuple(np.asarray(b, dtype=np.float64) for b in (xbins, ybins, zbins)), mins, d


def bins_of(edges, d):
    """np.histogramdd's bin of every sample on one axis, -1 for a dropped one: searchsorted(side='right') - 1 in float64,
    a sample equal to the last edge in the last bin, a sample below the first edge or above the last dropped"""
    edges, d = np.asarray(edges, dtype=np.float64), np.asarray(d, dtype=np.float64)
    nb = len(edges) - 1
    i = np.searchsorted(edges, d, side='right') - 1
    i[d == edges[-1]] = nb - 1
    i[(d < edges[0]) | (d > edges[-1]) | (i >= nb)] = -1
    return i


def counts_of(edges, d):
    """int64 counts (nx, ny, nz) of the samples d = (dx, dy, dz) between the three edge arrays"""
    shape = tuple(len(e) - 1 for e in edges)
    idx = [bins_of(e, v) for e, v in zip(edges, d)]
    keep = (idx[0] >= 0) & (idx[1] >= 0) & (idx[2] >= 0)
    out = np.zeros(shape, dtype=np.int64)
    if out.size:
        np.add.at(out, tuple(i[keep] for i in idx), 1)
    return out


def solid(counts, threshold=1, bottom_fill=True, pad=0):
    """counts -> the boolean model: threshold, fill below the lowest occupied voxel of each column, pad layers beneath"""
    H = counts >= threshold
    nx, ny, nz = H.shape
    if bottom_fill and nz:
        has = H.any(axis=2)
        low = np.where(has, H.argmax(axis=2), 0)                 # the lowest occupied level; 0 fills nothing
        H = H | (np.arange(nz)[None, None, :] < low[:, :, None])
    if pad > 0:
        H = np.concatenate([np.ones((nx, ny, pad), dtype=bool), H], axis=2)
    return np.ascontiguousarray(H)


def voxelize(filename, x, y, z, resolution, bottom_fill=True, threshold=1, material=0, ve=1, pad=0, *,
             return_edges=False):
    assert filename is None
    edges, mins, d = edges_of(x, y, z, resolution, ve)
    H = solid(counts_of(edges, d), operator.index(threshold), bottom_fill, operator.index(pad))
    if return_edges:
        return H, edges, mins
    return H
