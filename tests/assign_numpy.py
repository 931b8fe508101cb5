"""Restatement of the point-set matching contract; not a test.

Two restatements, each the bit-for-bit yardstick of its device code:

``hungarian_algorithm``   shortest augmenting paths with float64 duals in SciPy's arithmetic
                          (``r = minVal + c - u[i] - v[j]`` left to right, ``u += minVal - shortest``, ``v -= ...``) and the
                          stated tie rule: among the unreached columns at the lowest tentative distance an unassigned
                          one, among those the lowest index.  With more rows than columns the roles are swapped and the
                          pairs sorted by row, as SciPy does.
``bdr``                   the bidimensional regression with the device's summation order: element l, l + 64, ... on
                          lane l from +0.0, then ``p += p[lane ^ o]`` for o = 32 .. 1.

``costs`` is ``cdist``'s arithmetic: the squared differences added in axis order, then the root.
"""
import numpy as np

LANES = 64
SCALARS = ("beta1", "beta2", "alpha1", "alpha2", "rsquare", "D", "Dmax", "DI", "F")
DEVICE_FIELDS = SCALARS + ("aPrime", "bPrime")


def _f64(a):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] not in (2, 3) or a.shape[0] == 0:
        raise ValueError("expected a non-empty (n, 2) or (n, 3) array")
    return np.ascontiguousarray(a, dtype=np.float64)


def costs(XY, AB):
    x, a = _f64(XY), _f64(AB)
    t = x[:, 0, None] - a[None, :, 0]
    d2 = t * t
    for k in range(1, x.shape[1]):
        t = x[:, k, None] - a[None, :, k]
        d2 = d2 + t * t
    return np.sqrt(d2)


def solve(C, count=None):
    """col4row (nr,) of the nr <= nc cost matrix ``C``; ``count["steps"]`` is raised by one per scan step"""
    nr, nc = C.shape
    assert nr <= nc
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64)
    path = np.full(nc, -1, np.int64)
    for cur in range(nr):
        sh = np.full(nc, np.inf)
        sc = np.zeros(nc, bool)
        i, sink, minval = cur, -1, 0.0
        while sink < 0:
            if count is not None:
                count["steps"] = count.get("steps", 0) + 1
            free = ~sc
            r = ((minval + C[i]) - u[i]) - v
            upd = free & (r < sh)
            sh[upd] = r[upd]
            path[upd] = i
            low = np.where(free, sh, np.inf).min()
            if not low < np.inf:
                raise ValueError("no finite augmenting path")
            idx = np.flatnonzero(free & (sh == low))
            un = idx[row4col[idx] < 0]
            j = int(un[0]) if un.size else int(idx[0])
            minval = low
            sc[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
        u[cur] = u[cur] + minval
        reached = np.flatnonzero(sc)
        d = minval - sh[reached]
        v[reached] = v[reached] - d
        owned = row4col[reached] >= 0
        owners = row4col[reached][owned]
        u[owners] = u[owners] + d[owned]            # the owners of distinct columns are distinct rows
        j = sink
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, int(col4row[i])
            if i == cur:
                break
    return col4row


def hungarian_algorithm(XY, AB):
    """(row_indices int64 ascending, col_indices int64, min_costs float64), min(nr, nc) of each"""
    C = costs(XY, AB)
    nr, nc = C.shape
    if nr <= nc:
        rows, cols = np.arange(nr, dtype=np.int64), solve(C)
    else:
        rows = solve(np.ascontiguousarray(C.T))
        cols = np.arange(nc, dtype=np.int64)
        order = np.argsort(rows)
        rows, cols = rows[order], cols[order]
    return rows, cols, C[rows, cols]


def lane_sum(x):
    """the device's sum of a float64 vector"""
    x = np.asarray(x, np.float64)
    pad = (-x.size) % LANES
    rows = np.concatenate([x, np.zeros(pad)]).reshape(-1, LANES)
    p = np.zeros(LANES)
    for row in rows:
        p = p + row
    lane = np.arange(LANES)
    o = LANES // 2
    while o:
        p = p + p[lane ^ o]
        o //= 2
    return p[0]


def bdr(XY, AB):
    """the device-formed fields of bdr: SCALARS as numpy.float64, aPrime and bPrime"""
    xy, ab = _f64(XY), _f64(AB)
    if xy.shape != ab.shape or xy.shape[1] != 2 or xy.shape[0] < 3:
        raise ValueError("two (n, 2) arrays of n >= 3 points expected")
    n = xy.shape[0]
    X, Y, A, B = xy[:, 0], xy[:, 1], ab[:, 0], ab[:, 1]
    dn = np.float64(n)
    mx, my, ma, mb = lane_sum(X) / dn, lane_sum(Y) / dn, lane_sum(A) / dn, lane_sum(B) / dn
    cx, cy, ca, cb = X - mx, Y - my, A - ma, B - mb
    xa, yb, xb, ya = lane_sum(cx * ca), lane_sum(cy * cb), lane_sum(cx * cb), lane_sum(cy * ca)
    xx, yy, aa, bb = lane_sum(cx * cx), lane_sum(cy * cy), lane_sum(ca * ca), lane_sum(cb * cb)
    den = xx + yy
    beta1, beta2 = (xa + yb) / den, (xb - ya) / den
    alpha1 = (ma - beta1 * mx) + beta2 * my
    alpha2 = (mb - beta2 * mx) - beta1 * my
    aPrime = (alpha1 + beta1 * X) - beta2 * Y
    bPrime = (alpha2 + beta2 * X) + beta1 * Y
    ea, eb = A - aPrime, B - bPrime
    res = lane_sum(ea * ea + eb * eb)
    tot = aa + bb
    rsquare = np.float64(1.0) - res / tot
    om = np.float64(1.0) - rsquare
    out = dict(beta1=beta1, beta2=beta2, alpha1=alpha1, alpha2=alpha2, rsquare=rsquare, D=np.sqrt(res), Dmax=np.sqrt(tot),
               DI=np.sqrt(om), F=(np.float64(2 * n - 4) / np.float64(2.0)) * (rsquare / om))
    out = {k: np.float64(val) for k, val in out.items()}
    out["aPrime"], out["bPrime"] = aPrime, bPrime
    return out


def host_fields(r, n):
    """scale, theta and P as the package forms them on the host from the device's scalars"""
    return dict(scale=(r["beta1"]**2 + r["beta2"]**2)**.5, theta=np.rad2deg(np.arctan2(r["beta2"], r["beta1"])),
                P=np.float64((1 - r["rsquare"]) ** (n - 2)))


def bdr_bootstrap(XY, AB, samples):
    """(rsquare, DI) float64 (k,) of the (k, n) table ``samples`` of rows of AB"""
    xy, ab = _f64(XY), _f64(AB)
    samples = np.asarray(samples)
    rsq, di = np.empty(len(samples)), np.empty(len(samples))
    for s, idx in enumerate(samples):
        abs_ = ab[idx]
        _, cols, _ = hungarian_algorithm(xy, abs_)
        r = bdr(xy, abs_[cols])
        rsq[s], di[s] = r["rsquare"], r["DI"]
    return rsq, di


def draw(m, n, k):
    """the table bdr_bootstrap draws: k calls of np.random.choice(m, n, replace=False) on the global state"""
    return np.stack([np.random.choice(m, n, replace=False) for _ in range(k)]).astype(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def valid_assignment(rows, cols, nr, nc):
    n = min(nr, nc)
    return (rows.shape == cols.shape == (n,) and np.all(np.diff(rows) > 0) and rows.min() >= 0 and rows.max() < nr
            and np.unique(cols).size == n and cols.min() >= 0 and cols.max() < nc)
