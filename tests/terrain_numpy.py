"""Vectorised NumPy restatement of the terrain contract: test infrastructure only.

Each function marches the rays the way the kernels do - per direction the largest and smallest slope over the step
list, one arctan per direction and sign - so tests can (a) check the contract itself against the reference's goldens
and (b) check the GPU against the contract on inputs the reference was never run on.  The product never imports this.
"""
import numpy as np

DIRS = [(-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1)]
DLIST = np.array([np.sqrt(2), 1])

GEO = np.zeros((9, 9), dtype=np.uint8)
GEO[0, :] = [1, 1, 1, 8, 8, 9, 9, 9, 10]
GEO[1, :8] = [1, 1, 8, 8, 8, 9, 9, 9]
GEO[2, :7] = [1, 4, 6, 6, 7, 7, 9]
GEO[3, :6] = [4, 4, 6, 6, 6, 7]
GEO[4, :5] = [4, 4, 5, 6, 6]
GEO[5, :4] = [3, 3, 5, 5]
GEO[6, :3] = [3, 3, 3]
GEO[7, :2] = [3, 3]
GEO[8, :1] = [2]


def progressive_window(lo, hi, percent):
    out = [lo]
    v = lo
    while v < hi:
        v = int(np.ceil(v * (100 + percent) / 100))
        if v <= hi:
            out.append(v)
    return out


def steps_of(L, fast=False, how_fast=20):
    return progressive_window(1, L, how_fast) if fast else list(range(1, L + 1))


def _prep(Z):
    Z = np.asarray(Z)
    if Z.dtype not in (np.float32, np.float64):
        Z = Z.astype(np.float64)
    return Z


def _kin(shape, d):
    rows, cols = shape
    R, C = np.indices(shape)
    dr, dc = DIRS[d]
    k = np.full(shape, 1 << 30)
    if dr < 0:
        k = np.minimum(k, R)
    if dr > 0:
        k = np.minimum(k, rows - 1 - R)
    if dc < 0:
        k = np.minimum(k, C)
    if dc > 0:
        k = np.minimum(k, cols - 1 - C)
    return R, C, k


def slopes(Z, d, steps, cellsize, sky=False):
    """per step: t_k = fp64(Z[sample] - Z) / D(d, k), with the edge rule of openness (sample = cell) or sky-view
    (sample = last on-raster cell)"""
    Z = _prep(Z)
    R, C, kin = _kin(Z.shape, d)
    dr, dc = DIRS[d]
    for k in steps:
        m = np.minimum(k, kin) if sky else np.where(k <= kin, k, 0)
        diff = (Z[R + dr * m, C + dc * m] - Z).astype(np.float64)
        yield diff / ((cellsize * k) * DLIST[d % 2])


def extremes(Z, d, steps, cellsize, sky=False):
    """(max t, min t) over the steps, NaN ignored (NaN when no sample is a number)"""
    shape = np.shape(Z)
    tmax = np.full(shape, np.nan)
    tmin = np.full(shape, np.nan)
    for t in slopes(Z, d, steps, cellsize, sky):
        tmax = np.fmax(tmax, t)
        tmin = np.fmin(tmin, t)
    return tmax, tmin


def _angle(tmax):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(tmax), np.inf, np.pi / 2 - np.arctan(tmax))


def openness(Z, cellsize=1, lookup_pixels=1, neighbors=range(8), fast=False, how_fast=20):
    steps = steps_of(lookup_pixels, fast, how_fast)
    nb = list(np.asarray(neighbors).reshape(-1))
    a = {d: _angle(extremes(Z, d, steps, cellsize)[0]) for d in set(nb)}
    s = a[nb[0]].copy()
    for d in nb[1:]:
        s = s + a[d]
    return np.rad2deg(s / len(nb))


def skyview_factor(Z, cellsize=1, lookup_pixels=1):
    steps = list(range(1, lookup_pixels + 1))
    total = np.zeros(np.shape(Z))
    for d in range(8):
        tmax, _ = extremes(Z, d, steps, cellsize, sky=True)
        with np.errstate(invalid="ignore"):
            ang = np.where(np.isnan(tmax), 0.0, np.maximum(0.0, np.arctan(tmax)))
        total += np.sin(ang)
    return 1 - total / 8


def openness_differences(Z, cellsize, steps, use_negative=True, with_exact=False):
    """O_i = deg(openness(Z, [i])) - deg(openness(-Z, [i])) for i = 0..7 (or - 90 without the negative openness).
    ``with_exact``: also a mask of the O_i that are exactly 0 whatever the arctan (tmax == -tmin, or tmax == 0)"""
    out, exact = [], []
    for d in range(8):
        tmax, tmin = extremes(Z, d, steps, cellsize)
        with np.errstate(invalid="ignore"):
            pos = np.rad2deg(_angle(tmax))
            out.append(pos - np.rad2deg(_angle(-tmin)) if use_negative else pos - 90.0)
            exact.append(tmax == -tmin if use_negative else tmax == 0)
    return (np.stack(out), np.stack(exact)) if with_exact else np.stack(out)


def margin(O, thr, exact=None):
    """smallest distance of any |O_i| to the threshold (degrees): cells closer than this could flip a decision
    (an O_i in ``exact`` is the same on every arctan implementation and does not count)"""
    with np.errstate(invalid="ignore"):
        m = np.abs(np.abs(O) - thr)
    m = np.where(np.isnan(m), np.inf, m)
    if exact is not None:
        m = np.where(exact, np.inf, m)
    return np.min(m, axis=0)


def count_openness(Z, cellsize, lookup_pixels, threshold_angle, fast=False, how_fast=20, return_O=False):
    O = openness_differences(Z, cellsize, steps_of(lookup_pixels, fast, how_fast))
    with np.errstate(invalid="ignore"):
        pos = np.sum(O > threshold_angle, axis=0).astype(np.uint8)
        neg = np.sum(O < -threshold_angle, axis=0).astype(np.uint8)
    return (pos, neg, O) if return_O else (pos, neg)


def geomorphons(Z, cellsize=1, lookup_pixels=1, threshold_angle=1, enhance=False, fast=False, how_fast=20,
                return_margin=False):
    pos, neg, O = count_openness(Z, cellsize, lookup_pixels, threshold_angle, fast, how_fast, return_O=True)
    g = GEO[pos, neg]
    mg = margin(O, threshold_angle)
    if enhance and lookup_pixels > 16:
        Lsm = max(lookup_pixels // 4, 4)
        ps, ns, Os = count_openness(Z, cellsize, Lsm, threshold_angle, return_O=True)
        gs = GEO[ps, ns]
        g = g.copy()
        g[(g == 4) & (gs == 1)] = 1
        g[(g == 8) & (gs == 1)] = 1
        sel = (g == 2) | (g == 3)
        g[sel] = gs[sel]
        mg = np.minimum(mg, margin(Os, threshold_angle))
    return (g, mg) if return_margin else g


def lowest_table():
    def b3(x):
        return np.base_repr(x, 3).rjust(8, "0")
    out = np.zeros(3 ** 8, dtype=np.int64)
    for x in range(3 ** 8):
        s = b3(x)
        best = int(s, 3)
        for j in range(1, 16):
            s = s[-1] + s[:7]
            best = min(best, int(s, 3))
            if j == 7:
                s = s[::-1]
        out[x] = best
    return out


def ternary_pattern_from_openness(Z, cellsize=1, lookup_pixels=1, threshold_angle=0, use_negative_openness=True,
                                  lowest=False, return_margin=False):
    O = openness_differences(Z, cellsize, steps_of(lookup_pixels), use_negative_openness)
    with np.errstate(invalid="ignore"):
        digit = np.where(O < -threshold_angle, 0, np.where(O > threshold_angle, 2, 1))
    code = np.tensordot(3 ** np.arange(8), digit, axes=1).astype(np.int64)
    if lowest:
        code = lowest_table()[code]
    return (code, margin(O, threshold_angle)) if return_margin else code


def run(fn, Z, kw):
    """one golden case through the restatement (count_openness returns (pos, neg))"""
    kw = dict(kw)
    f = globals()[fn]
    if fn == "count_openness":
        return f(Z, kw.pop("cellsize"), kw.pop("lookup_pixels"), kw.pop("threshold_angle"), **kw)
    return f(Z, **kw)
