"""NumPy restatement of the relief-colouring and raster-statistics contract: test infrastructure
only.

Every function follows the reference's arithmetic as coded - operation order and the dtype of each step under NumPy 2
promotion - so tests can (a) check the contract against the reference's goldens and (b) check the GPU against the
contract on inputs the reference was never run on.  ``ordered_sum`` replays the device's summation order addition by
addition, so 'mean' and 'sum_sq' of ``raster_stats`` are compared bit for bit.  The product never imports this.
"""
import numpy as np

import surface_numpy as sn

PARTS = 1024          # workgroups at most (csrc/cloud_reduce.h: CLOUD_PARTS)
UNROLL = 4            # loads in flight per thread of the device's loop; the additions keep the index order


def _prep(X):
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    return X


# ------------------------------------------------------------------------------------------
# the documented summation order
# ------------------------------------------------------------------------------------------
def blocks_of(n):
    return int(max(1, min((n + 255) // 256, PARTS)))


def ordered_sum(v):
    """float64 sum of the float64 vector ``v`` (NaN cells already replaced by +0.0, which a chain that starts at +0.0
    cannot tell from a skipped cell) in the device's order: thread g of G = blocks x 256 adds cells g, g + G, ... in
    turn; 64 lanes fold as a shuffle tree (offsets 32 .. 1); a workgroup's four waves as (w0 + w1) + (w2 + w3); the
    workgroups in index order from 0.0."""
    v = np.asarray(v, dtype=np.float64).ravel()
    n = v.size
    B = blocks_of(n)
    G = B * 256
    k = -(-n // G)
    pad = np.zeros(k * G)
    pad[:n] = v
    t = np.zeros(G)
    for row in pad.reshape(k, G):
        t = t + row
    w = t.reshape(B * 4, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w[:, :o] = w[:, :o] + w[:, o:2 * o]
    w = w[:, 0].reshape(B, 4)
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    s = np.float64(0.0)
    for p in part:
        s = s + p
    return s


def chain_depth(n):
    """the longest chain of additions a cell's value passes through in ``ordered_sum`` of n cells"""
    B = blocks_of(n)
    return -(-n // (B * 256)) + 6 + 2 + B


# ------------------------------------------------------------------------------------------
# raster_stats
# ------------------------------------------------------------------------------------------
def raster_stats(X, what=('count', 'min', 'max', 'mean', 'median', 'sum_sq')):
    X = _prep(X)
    dt = X.dtype.type
    v = X.ravel()
    nan = np.isnan(v)
    ok = v[~nan]
    n = ok.size
    out = {}
    for w in what:
        if w == 'count':
            out[w] = int(n)
        elif n == 0:
            out[w] = np.float64(np.nan) if w in ('mean', 'sum_sq') else dt(np.nan)
        elif w == 'min':
            out[w] = ok.min()
        elif w == 'max':
            out[w] = ok.max()
        elif w == 'mean':
            with np.errstate(invalid='ignore', over='ignore'):
                out[w] = ordered_sum(np.where(nan, 0.0, v.astype(np.float64))) / np.float64(n)
        elif w == 'sum_sq':
            with np.errstate(invalid='ignore', over='ignore'):
                sq = (v * v).astype(np.float64)                     # X ** 2 in the raster's dtype, then widened
                out[w] = ordered_sum(np.where(nan, 0.0, sq))
        elif w == 'median':
            s = np.sort(ok)
            a, b = s[(n - 1) // 2], s[n // 2]
            with np.errstate(invalid='ignore', over='ignore'):
                out[w] = a if n % 2 else dt((a + b) / dt(2))
        else:
            raise ValueError(w)
    out['has_nan'] = bool(nan.any())
    return out


# ------------------------------------------------------------------------------------------
# normalize, rmse, cutter
# ------------------------------------------------------------------------------------------
def interp(x, xp, fp):
    """np.interp's formula written out (float64, no FMA): what the device evaluates per cell"""
    x = np.asarray(x, dtype=np.float64)
    xp = np.asarray(xp, dtype=np.float64)
    fp = np.asarray(fp, dtype=np.float64)
    out = np.empty(x.shape)
    it = np.nditer(x, flags=['multi_index'])
    n = len(xp)
    with np.errstate(all='ignore'):
        for xv in it:
            xv = np.float64(xv)
            if np.isnan(xv):
                r = xv
            elif xv > xp[-1]:
                r = fp[-1]
            elif xv < xp[0]:
                r = fp[0]
            else:
                j = 0
                for k in range(1, n):
                    if xp[k] <= xv:
                        j = k
                if j == n - 1 or xp[j] == xv:
                    r = fp[j]
                else:
                    slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
                    r = slope * (xv - xp[j]) + fp[j]
                    if np.isnan(r):
                        r = slope * (xv - xp[j + 1]) + fp[j + 1]
                        if np.isnan(r) and fp[j] == fp[j + 1]:
                            r = fp[j]
            out[it.multi_index] = r
    return out


def knots_of(X, xrange):
    X = _prep(X)
    names = [k for k in xrange if isinstance(k, str)]
    st = raster_stats(X, tuple(names)) if names else {}
    return np.array([st[k] if isinstance(k, str) else float(k) for k in xrange], dtype=np.float64)


def normalize(X, xrange=['min', 'max'], yrange=[0, 1], return_knots=False):
    X = _prep(X)
    knots = knots_of(X, xrange)
    with np.errstate(all='ignore'):
        out = np.interp(X, knots, [float(v) for v in yrange])
    return (out, knots) if return_knots else out


def rmse(X):
    X = _prep(X)
    st = raster_stats(X, ('count', 'sum_sq'))
    ss = np.float64(0.0) if st['count'] == 0 else st['sum_sq']
    with np.errstate(all='ignore'):
        return X.dtype.type(np.sqrt(ss / np.float64(X.size)))


def cutter(x, r, c):
    return [np.hsplit(i, c) for i in np.vsplit(x, r)]


# ------------------------------------------------------------------------------------------
# colour tables
# ------------------------------------------------------------------------------------------
def wrap_u8(v):
    """float -> uint8 as NumPy's astype gives it on x86: the low byte of the signed 32-bit truncation; NaN and values
    outside int32 give 0"""
    v = np.asarray(v, dtype=np.float64)
    ok = np.abs(v) < 2147483648.0                     # False for NaN
    out = np.zeros(v.shape, np.uint8)
    out[ok] = (np.trunc(v[ok]).astype(np.int64) & 255).astype(np.uint8)
    return out


def table3(lut):
    lut = np.asarray(lut)
    if not (lut.shape[:2] == (256, 256) and (lut.ndim == 2 or (lut.ndim == 3 and lut.shape[2] >= 3))):
        raise ValueError("a colour table is 256 x 256 or 256 x 256 x C with C >= 3")
    with np.errstate(invalid='ignore'):
        lut = lut.astype(np.uint8)
    if lut.ndim == 2:
        lut = np.stack((lut, lut, lut), axis=2)
    return lut[:, :, :3]


def table_index(Z):
    """zi = uint8(round(255 * (Z - Z.min()) / (Z.max() - Z.min()))) in the raster's dtype; NaN -> 0"""
    Z = _prep(Z)
    with np.errstate(all='ignore'):
        return wrap_u8(np.round(255 * (Z - Z.min()) / (Z.max() - Z.min())))


def colortable_shade(Z, name, cellsize=1, H=None):
    """``H``: the shade to use (the device's own, when the gather alone is under test); else the restatement's"""
    lut = table3(name)
    Zp = _prep(Z)
    if min(Zp.shape) < 2:
        raise ValueError("Shape of array too small to calculate a numerical gradient, "
                         "at least (edge_order + 1) elements are required.")
    if H is None:
        H = sn.hillshade(Zp, cellsize)
    return lut[table_index(Z), H]


def swiss_shading(Z, cellsize=1, lut=None, H=None):
    return colortable_shade(Z, np.asarray(lut)[:, :, :3], cellsize, H)


# ------------------------------------------------------------------------------------------
# Brassel
# ------------------------------------------------------------------------------------------
def brassel_value(H, Z, k, flat=180, Zmid=None, reverse=False, C2=0):
    """(H_new before the uint8 scaling, was_int)"""
    if k < 1:
        raise ValueError('k must be equal to or greater than one.')
    H = np.asarray(H)
    Z = _prep(Z)
    if H.shape != Z.shape:
        raise ValueError("H and Z differ in shape")
    if H.dtype not in (np.uint8, np.float32, np.float64):
        H = H.astype(np.float64)
    was_int = bool(np.any(H > 1))
    if was_int:
        H = H.astype(np.float64) / 255
    flat = float(flat)
    if flat > 1:
        flat = flat / 255
    with np.errstate(all='ignore'):
        Zmin = np.nanmin(Z) if not np.isnan(Z).all() else Z.dtype.type(np.nan)
        Zmax = np.nanmax(Z) if not np.isnan(Z).all() else Z.dtype.type(np.nan)
        if Zmid is None:
            Zstar = (Z - ((Zmax + Zmin) / 2)) / ((Zmax - Zmin) / 2)
        else:
            Zstar = np.interp(Z, [Zmin, float(Zmid), Zmax], [-1, 0, 1])
        if reverse:
            Zstar = -Zstar
        exponent = np.e ** (Zstar * np.log(k))
        H_new = ((H - flat) * exponent) + flat
        H_new[H_new < 0] = 0
        H_new[H_new > 1] = 1
        if C2 != 0:
            H_new = H_new + (float(C2) * (Zstar - 1)) / 2
    return H_new.astype(np.float64), was_int


def brassel_atmospheric_perspective(H, Z, k, flat=180, Zmid=None, reverse=False, C2=0):
    H_new, was_int = brassel_value(H, Z, k, flat, Zmid, reverse, C2)
    if was_int:
        return wrap_u8(np.round(255 * H_new))
    return H_new
