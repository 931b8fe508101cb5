"""Point-set matching: the assignment problem, bidimensional regression and its bootstrap (MI355X only).

``hungarian_algorithm``, ``bdr`` and ``bdr_bootstrap`` mirror the reference functions of those names (neilpy/neilpy.py:2724,
:2642 and :2735 of the reference checkout).  The reference forms ``cdist`` and hands it to SciPy's
``linear_sum_assignment``; here one wave64 solves one problem out of LDS by shortest augmenting paths with float64 duals
and, for ``bdr_bootstrap``, regresses the matched points straight away, all ``k`` samples in one launch
(``csrc/assign.hip``, ``smrf_assign_*`` of ``include/smrf_hip.h``).  The contract - the cost bits, the tie rule, the summation order, the limit on
the number of points - is DESIGN.md section 18.  NumPy in -> NumPy out; CUDA tensors in -> CUDA tensors out on their
device.  float32 and integer coordinates are widened to float64.  There is no CPU fallback: without the library or a GPU
every function raises :class:`neilpy_amd.SmrfHipError`.

Deviations from the reference: where several assignments are optimal the one returned follows the
stated tie rule, not SciPy's; ``bdr`` with fewer than 3 points is a ``ValueError`` (the reference divides by zero at 2);
``P`` is the closed form ``(1 - rsquare) ** (n - 2)`` of the F tail with two numerator degrees of freedom, not
``1 - scipy.stats.f.cdf``; clouds that are not ``(n, 2)`` / ``(n, 3)``, an empty cloud, a NaN or infinite coordinate
and more than ``assignment_limit()`` points on a side are ``ValueError``.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._xfer import to_device as _h2d, to_host as _d2h
from ._raster import _ptr, _stream, _torch
from .points import _Cloud, _pair_check, _shape_check

__all__ = ["hungarian_algorithm", "bdr", "bdr_bootstrap", "assignment_limit", "assignment_route"]

_SCALARS = ("beta1", "beta2", "alpha1", "alpha2", "rsquare", "D", "Dmax", "DI", "F")


def assignment_limit():
    """The most points either side of one assignment problem may have (what fits one workgroup's LDS)."""
    return int(_lib.load().smrf_assign_limit())


def assignment_route(nr, nc, d=2):
    """How an ``nr x nc`` problem of dimension ``d`` runs: ``register_columns`` (columns from there on keep their state
    in LDS), ``cached`` (the cost matrix is kept in LDS, not recomputed), ``waves`` per workgroup, ``lds_bytes`` per
    wave and ``cached_square``, the largest ``n`` whose ``n x n`` problem is cached."""
    r = (C.c_int * 5)()
    _lib.check(_lib.load().smrf_assign_route(int(nr), int(nc), int(d), r))
    return dict(register_columns=r[0], cached=bool(r[1]), waves=r[2], lds_bytes=r[3], cached_square=r[4])


def _limit_check(n, what):
    lim = assignment_limit()
    if n > lim:
        raise ValueError("%s: %d points are more than one assignment takes, the limit is %d" % (what, n, lim))


def _workspace(device, nr, nc, d):
    return _torch().empty(_lib.load().smrf_assign_workspace_bytes(nr, nc, d), dtype=_torch().uint8, device=device)


def _status(ws):
    st = int(ws[8:12].view(_torch().int32).item())
    if st & 2:
        raise ValueError("samples: an entry is not a row of AB")
    if st & 1:
        raise ValueError("a cost overflowed: no finite assignment")


@_device_scoped
def hungarian_algorithm(XY, AB):
    """The minimum-cost assignment between the rows of ``XY`` (nr, d) and ``AB`` (nc, d), d 2 or 3, under the Euclidean
    distance; same arguments and result as neilpy.hungarian_algorithm: ``(row_indices, col_indices, min_costs)`` of
    length ``min(nr, nc)``, int64 ascending, int64 and float64.  ``min_costs`` holds ``cdist``'s bits.  Where the
    optimum is unique this is SciPy's assignment; otherwise an optimal one chosen by the tie rule of DESIGN.md
    section 18.  ``XY`` alone decides the kind of result: CUDA tensors on its device when it is one, NumPy arrays when it
    is not, whatever ``AB`` is (``bdr`` and ``bdr_bootstrap`` follow the same rule)."""
    _pair_check(XY, "XY", AB, "AB")
    (nr, d), (nc, _) = _shape_check(XY, "XY"), _shape_check(AB, "AB")
    _limit_check(nr, "XY")
    _limit_check(nc, "AB")
    x, a = _Cloud(XY, "XY"), _Cloud(AB, "AB")
    torch = _torch()
    n = min(nr, nc)
    rows = torch.empty(n, dtype=torch.int64, device=x.t.device)
    cols = torch.empty(n, dtype=torch.int64, device=x.t.device)
    costs = torch.empty(n, dtype=torch.float64, device=x.t.device)
    ws = _workspace(x.t.device, nr, nc, d)
    _lib.check(_lib.load().smrf_assign_solve_f64(_ptr(x.t), nr, _ptr(a.t), nc, d, _ptr(rows), _ptr(cols), _ptr(costs),
                                                  _ptr(ws), ws.numel(), _stream()))
    _status(ws)
    if _is_tensor(XY):
        return rows, cols, costs
    return _d2h(rows), _d2h(cols), _d2h(costs)


def _plane_check(a, name):
    n, d = _shape_check(a, name)
    if d != 2:
        raise ValueError("%s: points of dimension %d, bidimensional regression takes 2" % (name, d))
    return n


def _regress(x, a, samples, k, solve, full):
    """k regressions in one launch: (scalars (k, 9), aPrime, bPrime) when ``full``, else (rsquare, DI)"""
    torch = _torch()
    dev, n = x.t.device, x.n
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    scal = ap = bp = rsq = di = None
    if full:
        scal, ap, bp = new(k, 9), new(k, n), new(k, n)
    else:
        rsq, di = new(k), new(k)
    ws = _workspace(dev, 1, 1, 2)
    _lib.check(_lib.load().smrf_assign_bdr_f64(_ptr(x.t), n, _ptr(a.t), a.n, _ptr(samples), k, int(solve), _ptr(scal),
                                                _ptr(ap), _ptr(bp), _ptr(rsq), _ptr(di), _ptr(ws), ws.numel(), _stream()))
    if solve:
        _status(ws)
    return (scal, ap, bp) if full else (rsq, di)


@_device_scoped
def bdr(XY, AB):
    """Bidimensional regression of ``AB`` (n, 2) on ``XY`` (n, 2), row i on row i, n >= 3; same arguments and keys as
    neilpy.bdr: ``beta1 beta2 alpha1 alpha2 scale theta aPrime bPrime rsquare D Dmax DI F P``.  Scalars are
    ``numpy.float64``; ``aPrime`` / ``bPrime`` are float64 (n,), CUDA tensors when ``XY`` is one."""
    n, m = _plane_check(XY, "XY"), _plane_check(AB, "AB")
    if n != m:
        raise ValueError("XY has %d points, AB has %d: the regression pairs them row by row" % (n, m))
    if n < 3:
        raise ValueError("%d points: the regression needs at least 3" % n)
    x, a = _Cloud(XY, "XY"), _Cloud(AB, "AB")
    scal, ap, bp = _regress(x, a, None, 1, False, True)
    s = _d2h(scal)[0]
    out = {name: np.float64(v) for name, v in zip(_SCALARS, s)}
    beta1, beta2, rsquare = out["beta1"], out["beta2"], out["rsquare"]
    out["scale"] = (beta1**2 + beta2**2)**.5
    out["theta"] = np.rad2deg(np.arctan2(beta2, beta1))
    out["aPrime"], out["bPrime"] = (ap[0], bp[0]) if _is_tensor(XY) else (_d2h(ap)[0], _d2h(bp)[0])
    out["P"] = np.float64((1 - rsquare) ** (n - 2))
    return out


def _sample_table(samples, n, m, device):
    """(k, n) int64 on the device, every entry a row of AB (one reduction on the device)"""
    torch = _torch()
    shape = tuple(samples.shape) if _is_tensor(samples) else np.shape(samples)
    if len(shape) != 2 or shape[1] != n or shape[0] < 1:
        raise ValueError("samples: expected a (k, %d) table of rows of AB, got shape %s" % (n, (shape,)))
    if _is_tensor(samples):
        if samples.dtype.is_floating_point or samples.dtype == torch.bool:
            raise ValueError("samples: an integer table expected, got %s" % samples.dtype)
        t = samples.to(device=device, dtype=torch.int64).contiguous()
    else:
        arr = np.asarray(samples)
        if arr.dtype.kind not in "iu":
            raise ValueError("samples: an integer table expected, got %s" % arr.dtype)
        t = _h2d(np.ascontiguousarray(arr, dtype=np.int64))
    ws = _workspace(device, 1, 1, 2)
    bad = C.c_int64(0)
    _lib.check(_lib.load().smrf_assign_samples_check(_ptr(t), shape[0], n, m, C.byref(bad), _ptr(ws), ws.numel(),
                                                      _stream()))
    if bad.value:
        raise ValueError("samples: %d entries are not rows of AB (0 .. %d)" % (bad.value, m - 1))
    return t


@_device_scoped
def bdr_bootstrap(XY, AB, k=10000, *, samples=None):
    """``k`` times: draw ``len(XY)`` rows of ``AB`` (m, 2) without replacement, match them to ``XY`` (n, 2) at the least
    total distance, regress the matched points on ``XY``; same arguments and result as neilpy.bdr_bootstrap:
    ``(rsquare, DI)``, float64 (k,).  The draws are ``k`` calls of ``np.random.choice(len(AB), len(XY), replace=False)``
    on NumPy's global state, as the reference makes them, uploaded as one table; ``samples``, a (k, n) integer table of
    rows of ``AB``, replaces the draw (``k`` is then its first dimension; a row may repeat within a sample).  One kernel
    launch solves and regresses every sample."""
    n, m = _plane_check(XY, "XY"), _plane_check(AB, "AB")
    if n < 3:
        raise ValueError("%d points: the regression needs at least 3" % n)
    _limit_check(n, "XY")
    if samples is None and int(k) < 0:
        raise ValueError("k = %d: a count of samples expected" % int(k))
    x, a = _Cloud(XY, "XY"), _Cloud(AB, "AB")
    if samples is None and int(k) == 0:                # the reference's two empty arrays; nothing is drawn or launched
        if _is_tensor(XY):
            return tuple(_torch().zeros(0, dtype=_torch().float64, device=x.t.device) for _ in range(2))
        return np.zeros(0), np.zeros(0)
    if samples is None:                                # n > m: the first draw raises the reference's ValueError
        samples = np.stack([np.random.choice(m, n, replace=False) for _ in range(int(k))]).astype(np.int64, copy=False)
    table = _sample_table(samples, n, m, x.t.device)
    rsq, di = _regress(x, a, table, table.shape[0], True, False)
    if _is_tensor(XY):
        return rsq, di
    return _d2h(rsq), _d2h(di)
