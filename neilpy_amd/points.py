"""One point cloud against another: exact nearest points and the Chamfer distance (MI355X only).

``chamfer_distance`` mirrors the reference function of that name (neilpy/neilpy.py:2679 of the reference checkout), which
asks scikit-learn's KD-tree for every point's nearest neighbour in the other cloud and averages the distances.
``nearest_points`` returns what the kernels compute on the way, the distance to that neighbour and its row; it plays the
part ``nearest_source`` plays for rasters.

Both run the counting sort into a uniform cell grid and the ring search of ``csrc/points.hip`` (``smrf_points_nn_*``); the
contract - float64 distances formed in a fixed order without FMA, ties to the lowest row, the three rules that make the
search exact - is DESIGN.md section 14.  NumPy in -> NumPy out; CUDA tensors in -> CUDA tensors out on their device, with
no host copy of the clouds.  float32 and integer coordinates are widened to float64, as scikit-learn widens them.  There
is no CPU fallback: without the library or a GPU both raise :class:`neilpy_amd.SmrfHipError`.

Deviations from the reference, all ``ValueError`` and all raised before a cloud is touched except
the last: a ``metric`` other than ``'l2'`` / ``'euclidean'`` (the reference passes any scikit-learn metric on); clouds
that are not ``(n, 2)`` or ``(n, 3)`` or differ in dimension; an empty cloud; an unknown ``direction``; a NaN or infinite
coordinate (one device reduction per cloud).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._xfer import to_host as _d2h
from ._raster import _ptr, _stream, _to_device, _torch

__all__ = ["nearest_points", "chamfer_distance"]

_METRICS = ("l2", "euclidean")
_DIRECTIONS = ("y_to_x", "x_to_y", "bi")


def _shape_check(a, name):
    """(n, d) of a cloud, from its shape alone: nothing is copied or launched"""
    shape = tuple(a.shape) if _is_tensor(a) else np.shape(a)
    if len(shape) != 2:
        raise ValueError("%s: expected an (n, d) array of points, got shape %s" % (name, (shape,)))
    n, d = shape
    if d not in (2, 3):
        raise ValueError("%s: points of dimension %d, expected 2 or 3" % (name, d))
    if n == 0:
        raise ValueError("%s: empty cloud" % name)
    return n, d


def _pair_check(a, aname, b, bname):
    (_, da), (_, db) = _shape_check(a, aname), _shape_check(b, bname)
    if da != db:
        raise ValueError("%s has dimension %d, %s has %d" % (aname, da, bname, db))


class _Cloud:
    """a cloud on the device: contiguous float64 (n, d), checked finite, with its planar box; its grid is built when it
    is first searched"""

    def __init__(self, a, name):
        torch = _torch()
        self.t = _to_device(a, torch.float64)
        self.n, self.d = self.t.shape
        lib = _lib.load()
        self.nbytes = lib.smrf_points_nn_workspace_bytes(self.n, self.d)
        if self.nbytes == 0:
            raise ValueError("%s: %d points are more than one search takes (2**30)" % (name, self.n))
        # the bounds and the sum only use the partials at the head of a workspace: one point's workspace holds them
        self.small = torch.empty(lib.smrf_points_nn_workspace_bytes(1, self.d), dtype=torch.uint8, device=self.t.device)
        self.box = (C.c_double * 4)()
        bad = C.c_int64(0)
        _lib.check(lib.smrf_points_nn_bounds_f64(_ptr(self.t), self.n, self.d, self.box, C.byref(bad), _ptr(self.small),
                                                 self.small.numel(), _stream()))
        if bad.value:
            raise ValueError("%s: %d coordinates are NaN or infinite" % (name, bad.value))
        self.ws = None

    def build(self):
        if self.ws is None:
            ws = _torch().empty(self.nbytes, dtype=_torch().uint8, device=self.t.device)
            _lib.check(_lib.load().smrf_points_nn_build_f64(_ptr(self.t), self.n, self.d, self.box, _ptr(ws),
                                                            self.nbytes, _stream()))
            self.ws = ws

    def search(self, query, want_dist, want_index):
        """nearest point of this cloud for every point of the cloud ``query``: (dist float64, index int64), None where
        not asked for"""
        torch = _torch()
        self.build()
        dist = torch.empty(query.n, dtype=torch.float64, device=self.t.device) if want_dist else None
        index = torch.empty(query.n, dtype=torch.int64, device=self.t.device) if want_index else None
        _lib.check(_lib.load().smrf_points_nn_search_f64(_ptr(query.t), query.n, _ptr(self.t), self.n, self.d, self.box,
                                                         _ptr(dist), _ptr(index), _ptr(self.ws), self.nbytes, _stream()))
        return dist, index

    def mean_nearest(self, query):
        """mean over ``query`` of the distance to this cloud's nearest point: the ordered device sum over its count"""
        torch = _torch()
        dist, _ = self.search(query, True, False)
        total = torch.empty(1, dtype=torch.float64, device=self.t.device)
        _lib.check(_lib.load().smrf_points_nn_sum_f64(_ptr(dist), query.n, _ptr(total), _ptr(self.small),
                                                      self.small.numel(), _stream()))
        return np.float64(total.item()) / np.float64(query.n)


@_device_scoped
def nearest_points(query, points):
    """For every row of ``query`` (nq, d) the nearest row of ``points`` (np, d), d 2 or 3: ``(dist, index)`` with ``dist``
    float64 (nq,), ``sqrt((q0-p0)*(q0-p0) + (q1-p1)*(q1-p1) [+ (q2-p2)*(q2-p2)])`` in float64 in that order, and ``index``
    int64 (nq,), that point's row - the lowest row among equally near points.  NumPy in -> NumPy out; when ``query`` is a
    CUDA tensor both results are CUDA tensors on its device."""
    _pair_check(query, "query", points, "points")
    q, p = _Cloud(query, "query"), _Cloud(points, "points")
    dist, index = p.search(q, True, True)
    if _is_tensor(query):
        return dist, index
    return _d2h(dist), _d2h(index)


@_device_scoped
def chamfer_distance(x, y, metric='l2', direction='bi'):
    """Chamfer distance between the clouds ``x`` (nx, d) and ``y`` (ny, d); same arguments and result as
    neilpy.chamfer_distance.  ``'y_to_x'``: the mean over ``y`` of the distance to the nearest point of ``x``;
    ``'x_to_y'``: the converse; ``'bi'``: their sum.  Returns ``numpy.float64``, also for tensor input."""
    if metric not in _METRICS:
        raise ValueError("metric %r: only the Euclidean metric ('l2', 'euclidean') runs on the device" % (metric,))
    if direction not in _DIRECTIONS:
        raise ValueError("Invalid direction type. Supported types: 'y_to_x', 'x_to_y', 'bi'")
    _pair_check(x, "x", y, "y")
    cx, cy = _Cloud(x, "x"), _Cloud(y, "y")
    if direction == 'y_to_x':
        return cx.mean_nearest(cy)
    if direction == 'x_to_y':
        return cy.mean_nearest(cx)
    return cx.mean_nearest(cy) + cy.mean_nearest(cx)
