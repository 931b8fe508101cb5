"""Brute-force restatement of the nearest-point contract; not a test.

All pairs, in blocks of query rows: the float64 distance ``sqrt((q0-p0)*(q0-p0) + (q1-p1)*(q1-p1) [+ (q2-p2)*(q2-p2)])``
with the squares added in axis order, and ``argmin``, which takes the lowest row among equal distances.  Exact by
construction, so it is the reference every point of every GPU test is compared with."""
import numpy as np

BLOCK_CELLS = 1 << 22        # distances held at once


def _f64(a):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] not in (2, 3) or a.shape[0] == 0:
        raise ValueError("expected a non-empty (n, 2) or (n, 3) array")
    return np.ascontiguousarray(a, dtype=np.float64)


def nearest_points(query, points):
    """(dist float64 (nq,), index int64 (nq,))"""
    q, p = _f64(query), _f64(points)
    if q.shape[1] != p.shape[1]:
        raise ValueError("dimensions differ")
    nq, d = q.shape
    dist = np.empty(nq, np.float64)
    index = np.empty(nq, np.int64)
    step = max(1, BLOCK_CELLS // p.shape[0])
    cols = [np.ascontiguousarray(p[:, k]) for k in range(d)]

    def block(a):
        b = min(nq, a + step)
        t = q[a:b, 0, None] - cols[0][None, :]
        d2 = np.multiply(t, t)
        for k in range(1, d):
            np.subtract(q[a:b, k, None], cols[k][None, :], out=t)
            np.multiply(t, t, out=t)
            np.add(d2, t, out=d2)
        D = np.sqrt(d2, out=d2)
        j = np.argmin(D, axis=1)
        index[a:b] = j
        dist[a:b] = D[np.arange(b - a), j]

    starts = range(0, nq, step)
    if len(starts) < 8:
        for a in starts:
            block(a)
    else:                                # NumPy releases the GIL in these loops: blocks side by side, same arithmetic
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=8) as ex:
            list(ex.map(block, starts))
    return dist, index


def chamfer_distance(x, y, metric='l2', direction='bi'):
    if direction == 'y_to_x':
        return np.mean(nearest_points(y, x)[0])
    if direction == 'x_to_y':
        return np.mean(nearest_points(x, y)[0])
    if direction == 'bi':
        return np.mean(nearest_points(y, x)[0]) + np.mean(nearest_points(x, y)[0])
    raise ValueError("Invalid direction type. Supported types: 'y_to_x', 'x_to_y', 'bi'")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
