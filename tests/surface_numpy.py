"""Vectorised NumPy restatement of the surface-derivative contract: test infrastructure only.

Every function follows the reference's arithmetic as coded - operation order, the dtype of each step under NumPy 2
promotion, the three edge rules and the NaN fills - so tests can (a) check the contract against the reference's goldens
bit for bit and (b) check the GPU against the contract on inputs the reference was never run on.  The product never
imports this.

``esri_slope(..., scalar_pow=True)`` is the reference itself: its per-cell callback squares NumPy float64 scalars,
which calls C ``pow`` (not correctly rounded).  The library's contract (the default) squares by a product.
"""
import math

import numpy as np


def _prep(Z):
    Z = np.asarray(Z)
    if Z.dtype not in (np.float32, np.float64):
        Z = Z.astype(np.float64)
    return Z


def _rad2deg(x):
    """np.rad2deg: x * (180 / pi) with the constant formed in x's precision"""
    t = x.dtype.type
    return x * (t(180) / t(np.pi))


# ------------------------------------------------------------------------------------------
# neighbourhoods under the three edge rules
# ------------------------------------------------------------------------------------------
def clamped(Z):
    """ndimage 'reflect' on a 3 x 3 window: N[dr][dc] = Z[clamp(r + dr), clamp(c + dc)], each axis on its own"""
    P = np.pad(Z, 1, mode="edge")
    R, C = Z.shape
    return [[P[1 + dr:1 + dr + R, 1 + dc:1 + dc + C] for dc in (-1, 0, 1)] for dr in (-1, 0, 1)]


def ashift(Z, dr, dc):
    """the reference's ashift: the neighbour (r + dr, c + dc), or the cell itself where that is off the raster"""
    out = Z.copy()
    R, C = Z.shape
    rs = slice(max(dr, 0), R + min(dr, 0))      # source rows r + dr that exist
    rd = slice(max(-dr, 0), R + min(-dr, 0))
    cs = slice(max(dc, 0), C + min(dc, 0))
    cd = slice(max(-dc, 0), C + min(-dc, 0))
    out[rd, cd] = Z[rs, cs]
    return out


def _gradient(Z, h):
    if min(Z.shape) < 2:
        raise ValueError("Shape of array too small to calculate a numerical gradient, "
                         "at least (edge_order + 1) elements are required.")
    return np.gradient(Z, h)


# ------------------------------------------------------------------------------------------
# gradient family
# ------------------------------------------------------------------------------------------
def slope(Z, cellsize=1, z_factor=1, return_as='degrees'):
    Z = _prep(Z)
    gy, gx = _gradient(Z, float(cellsize) / float(z_factor))
    S = np.sqrt(gx * gx + gy * gy)
    if return_as in ('degrees', 'radians'):
        S = np.arctan(S)
        if return_as == 'degrees':
            S = _rad2deg(S)
    return S


def aspect(Z, return_as='degrees', flat_as='nan'):
    Z = _prep(Z)
    t = Z.dtype.type
    gy, gx = _gradient(Z, 1.0)
    A = t(np.pi / 2) - np.arctan2(gy, -gx)
    neg = A < 0
    A[neg] = A[neg] + t(2 * np.pi)
    if return_as == 'degrees':
        A = _rad2deg(A)
    A[(gx == 0) & (gy == 0)] = np.nan if flat_as == 'nan' else flat_as
    return A


def angles(zenith, azimuth):
    """(cos zenith, sin zenith, azimuth) in radians, float64, as hillshade's np.deg2rad((zenith, azimuth))"""
    z, a = np.deg2rad((zenith, azimuth))
    return float(np.cos(z)), float(np.sin(z)), float(a)


def hillshade_value(Z, cellsize=1, z_factor=1, zenith=45, azimuth=315):
    """H (float64, negatives set to 0) before the uint8 scaling"""
    Z = _prep(Z)
    cz, sz, az = angles(zenith, azimuth)
    S = slope(Z, cellsize, z_factor, 'radians')
    A = aspect(Z, 'radians', flat_as=0)
    H = (cz * np.cos(S).astype(np.float64)) + (sz * np.sin(S).astype(np.float64) * np.cos(az - A.astype(np.float64)))
    H[H < 0] = 0
    return H


def to_uint8(H):
    """np.round(255 * H).astype(np.uint8) on x86: NaN becomes 0"""
    v = np.round(255 * H)
    out = np.zeros(H.shape, np.uint8)
    ok = ~np.isnan(v)
    out[ok] = v[ok].astype(np.uint8)
    return out


def half_margin(H, flat=None):
    """distance of 255 * H from the nearest half-integer: the rounding's margin.  inf where H is NaN, and on ``flat``
    cells (zero slope: H is cos(zenith) exactly, whatever the cos / sin / atan of the device)"""
    v = 255 * H
    m = np.abs(v - (np.floor(v) + 0.5))
    m[np.isnan(v)] = np.inf
    if flat is not None:
        m[flat] = np.inf
    return m


def flat_cells(Z, cellsize=1, z_factor=1):
    return slope(Z, cellsize, z_factor, 'percent') == 0


def hillshade(Z, cellsize=1, z_factor=1, zenith=45, azimuth=315, return_uint8=True):
    H = hillshade_value(Z, cellsize, z_factor, zenith, azimuth)
    return to_uint8(H) if return_uint8 else H


def angle_lists(zeniths=np.array([45]), azimuths=4):
    """multiple_illumination's expansion of scalar arguments"""
    if np.isscalar(azimuths):
        azimuths = np.arange(0, 360, 360 / azimuths)
    if np.isscalar(zeniths):
        zeniths = 90 / (zeniths + 1)
        zeniths = np.arange(zeniths, 90, zeniths)
    return zeniths, azimuths


def multiple_illumination(Z, cellsize=1, z_factor=1, zeniths=np.array([45]), azimuths=4, return_margin=False):
    Z = _prep(Z)
    zs, azs = angle_lists(zeniths, azimuths)
    H = np.zeros(Z.shape, np.uint8)
    vals = [hillshade_value(Z, cellsize, z_factor, zen, az) for zen in zs for az in azs]
    for v in vals:
        H = np.maximum(H, to_uint8(v))
    if not return_margin:
        return H
    # the margin of the max: only shades that round to within 1 of it can change it
    flat = flat_cells(Z, cellsize, z_factor)
    m = np.full(Z.shape, np.inf)
    for v in vals:
        near = to_uint8(v).astype(int) >= H.astype(int) - 1
        m = np.where(near, np.minimum(m, half_margin(v, flat)), m)
    return H, m


# ------------------------------------------------------------------------------------------
# 3 x 3 stencils
# ------------------------------------------------------------------------------------------
def _sq_pow(x):
    return np.frompyfunc(lambda v: math.pow(v, 2), 1, 1)(x).astype(np.float64)


def esri_slope(Z, cellsize=1, z_factor=1, return_as='degrees', scalar_pow=False):
    Z = _prep(Z)
    t = Z.dtype.type
    N = clamped(Z.astype(np.float64))

    def wsum(a, b, c):
        return (a * 1 + b * 2) + c * 1

    dzdx = (wsum(N[0][2], N[1][2], N[2][2]) - wsum(N[0][0], N[1][0], N[2][0])) / 8
    dzdy = (wsum(N[2][0], N[2][1], N[2][2]) - wsum(N[0][0], N[0][1], N[0][2])) / 8
    sq = _sq_pow if scalar_pow else (lambda v: v * v)
    S = np.sqrt(sq(dzdx) + sq(dzdy)).astype(Z.dtype)
    cellsize, z_factor = float(cellsize), float(z_factor)
    if cellsize != 1:
        S = S / t(cellsize)
    if z_factor != 1:
        S = t(z_factor) * S
    if return_as == 'degrees':
        S = _rad2deg(np.arctan(S))
    return S


def curvature(X, cellsize=1):
    X = _prep(X)
    t = X.dtype.type
    Y = X / t(float(cellsize))
    N = clamped(Y.astype(np.float64))
    c = N[1][1]
    lap = (c * -2 + (N[0][1] + N[2][1])).astype(X.dtype) + (c * -2 + (N[1][0] + N[1][2])).astype(X.dtype)
    return t(-100) * lap


def _ring(X):
    """z1..z9 in reading order (z5 = X) under ashift's edge rule"""
    return {k: ashift(X, dr, dc) for k, (dr, dc) in
            {1: (-1, -1), 2: (-1, 0), 3: (-1, 1), 4: (0, -1), 6: (0, 1), 7: (1, -1), 8: (1, 0), 9: (1, 1)}.items()}


def _fill_opposite(X, z, order):
    t = X.dtype.type
    for a, b in order:
        idx = np.isnan(z[a])
        z[a][idx] = t(2) * X[idx] - z[b][idx]


_ZT_FILLS = ((1, 9), (2, 8), (3, 7), (4, 6), (6, 4), (7, 3), (8, 2), (9, 1))


def _zt_terms(X, z, L):
    t = X.dtype.type
    D = (((z[4] + z[6]) / t(2)) - X) / t(L ** 2)
    E = (((z[2] + z[8]) / t(2)) - X) / t(L ** 2)
    F = (-z[1] + z[3] + z[7] - z[9]) / t(4 * (L ** 2))
    G = (-z[4] + z[6]) / t(2 * L)
    H = (z[2] - z[8]) / t(2 * L)
    return D, E, F, G, H


def esri_curvature(X, cellsize=1):
    X = _prep(X)
    t = X.dtype.type
    z = _ring(X)
    for k in z:
        idx = np.isnan(z[k])
        z[k][idx] = X[idx]
    D, E, F, G, H = _zt_terms(X, z, float(cellsize))
    K = t(-200) * (D + E)
    with np.errstate(divide='ignore', invalid='ignore'):
        K_plan = t(200) * (D * (H * H) + E * (G * G) - F * G * H) / (G * G + H * H)
        K_profile = t(-200) * (D * (G * G) + E * (H * H) + F * G * H) / (G * G + H * H)
    K_plan[np.isnan(K_plan)] = 0
    K_profile[np.isnan(K_profile)] = 0
    return K, K_plan, K_profile


def zevenbergen_and_thorne_curvature(X, cellsize=1):
    X = _prep(X)
    t = X.dtype.type
    z = _ring(X)
    _fill_opposite(X, z, _ZT_FILLS)
    D, E, F, G, H = _zt_terms(X, z, float(cellsize))
    P = G * G + H * H
    Q = G * G + H * H + t(1)
    K = t(2) * (D + E)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        K_cross = t(2) * (D * (H * H) + E * (G * G) - F * G * H) / P
        K_long = t(-2) * (D * (G * G) + E * (H * H) + F * G * H) / P
        K_tan = -(D * (H * H) - t(2) * F * G * H + E * (G * G)) / (P * np.sqrt(Q))
        K_profile = (D * (G * G) + t(2) * F * G * H + E * (H * H)) / (P * np.power(Q, t(1.5)))
        K_plan = -(D * (E * E) - t(2) * F * G * H + E * (G * G)) / np.power(P, t(1.5))
    K_cross[np.isnan(K_cross)] = 0
    K_long[np.isnan(K_long)] = 0
    return K, K_profile, K_plan, K_tan, K_long, K_cross


def evans_curvature(X, cellsize=1):
    X = _prep(X)
    t = X.dtype.type
    z = _ring(X)
    _fill_opposite(X, z, _ZT_FILLS)
    L = float(cellsize)
    s6, s3, s4, l6 = t(6 * L ** 2), t(3 * L ** 2), t(4 * L ** 2), t(6 * L)
    A = (z[1] + z[3] + z[4] + z[6] + z[7] + z[9]) / s6 - (z[2] + X + z[8]) / s3
    B = (z[1] + z[2] + z[3] + z[7] + z[8] + z[9]) / s6 - (z[4] + X + z[6]) / s3
    C = (z[3] + z[7] - z[1] - z[9]) / s4
    D = (z[3] + z[6] + z[9] - z[1] - z[4] - z[7]) / l6
    E = (z[1] + z[2] + z[3] - z[7] - z[8] - z[9]) / l6
    K = t(-2) * (A + B)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        S2 = D * D + E * E
        K_profile = -(A * (D * D) + t(2) * C * D * E + B * (E * E)) / (S2 * np.power(S2 + t(1), t(1.5)))
        K_cross = t(-2) * (B * (D * D) + A * (E * E) - C * D * E) / S2
        K_long = t(-2) * (A * (D * D) + B * (E * E) + C * D * E) / S2
        K_tan = -(A * (E * E) - t(2) * C * D * E + B * (D * D)) / (S2 * np.sqrt(S2 + t(1)))
        K_plan = -(A * (E * E) - t(2) * C * D * E + B * (D * D)) / np.power(S2, t(1.5))
    fin = np.isfinite(X)
    for k in (K_profile, K_plan, K_cross, K_long, K_tan):
        k[np.isnan(k) & fin] = 0
    return K, K_profile, K_plan, K_tan, K_long, K_cross


def wilson_gallant_curvature(X, cellsize=1):
    X = _prep(X)
    t = X.dtype.type
    Hc = float(cellsize)
    # W&G's numbering: Z1 upper right, clockwise to Z6 left; the reference's ashift(X, 8) / ashift(X, 9) are X itself
    z = {1: ashift(X, -1, 1), 2: ashift(X, 0, 1), 3: ashift(X, 1, 1), 4: ashift(X, 1, 0), 5: ashift(X, 1, -1),
         6: ashift(X, 0, -1), 7: X.copy(), 8: X.copy()}
    for a, b in ((1, 5), (2, 6), (3, 7), (4, 8), (5, 1), (6, 2), (7, 3), (8, 4)):
        idx = np.isnan(z[a])
        z[a][idx] = t(2) * X[idx] - z[b][idx]
    ZX = (z[2] - z[6]) / t(2 * Hc)
    ZY = (z[8] - z[4]) / t(2 * Hc)
    ZXX = (z[2] - t(2) * X + z[6]) / t(Hc ** 2)
    ZYY = (z[8] - t(2) * X + z[4]) / t(Hc ** 2)
    ZXY = (-z[7] + z[1] + z[5] - z[3]) / t(4) * t(Hc ** 2)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        P = ZX * ZX + ZY * ZY
        Q = P + t(1)
        Kc = (ZXX * (ZY * ZY) - t(2) * ZXY * ZX * ZY + ZYY * (ZX * ZX)) / np.power(P, t(1.5))
        num = ZXX * (ZX * ZX) + t(2) * ZXY * ZX * ZY + ZYY * (ZY * ZY)
        Kp = num / (P * np.power(Q, t(1.5)))
        Kt = num / (P * np.sqrt(Q))
        K = ZXX * ZXX + t(2) * (ZXY * ZXY) + ZYY * ZYY
    return K, Kp, Kc, Kt


def z_factor(latitude):
    latitude = np.deg2rad(latitude)
    a = 6378137
    b = 6356752.3
    numer = (a ** 4) * (np.cos(latitude) ** 2) + (b ** 4) * (np.sin(latitude) ** 2)
    denom = (a * np.cos(latitude)) ** 2 + (b * np.sin(latitude)) ** 2
    return 1 / (np.pi / 180 * np.cos(latitude) * np.sqrt(numer / denom))


FUNCS = {f.__name__: f for f in (slope, aspect, hillshade, multiple_illumination, esri_slope, curvature, esri_curvature,
                                 zevenbergen_and_thorne_curvature, evans_curvature, wilson_gallant_curvature)}

# number of outputs of each raster function (1 = a single array)
N_OUT = {"esri_curvature": 3, "zevenbergen_and_thorne_curvature": 6, "evans_curvature": 6,
         "wilson_gallant_curvature": 4}


def decode_kw(kw):
    """golden / random-case keywords: lists become arrays (multiple_illumination's angle arrays)"""
    return {k: (np.array(v) if isinstance(v, list) else v) for k, v in kw.items()}


def run(fn, Z, kw, **extra):
    return FUNCS[fn](Z, **decode_kw(kw), **extra)
