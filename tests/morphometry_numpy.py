"""NumPy restatement of the strided-stencil contract: test infrastructure only.

Written from the contract, operation by operation: ashift's sampling rule, Wood's quadratic at stride n in the raster's
dtype with Python-float divisors, and the VIP score in float64 from differences formed in the raster's dtype.  It equals
every golden of the reference bit for bit (tests/test_morphometry_host.py) and is what the GPU is compared with on
inputs the reference was never run on.  The product never imports this.
"""
import numpy as np

KEYS = ("A", "S", "K", "K_profile", "K_cross", "K_long", "K_tan", "K_plan")

# direction -> (row step, column step) in units of n, clockwise from the upper left
TAPS = {0: (-1, -1), 1: (-1, 0), 2: (-1, 1), 3: (0, 1), 4: (1, 1), 5: (1, 0), 6: (1, -1), 7: (0, -1)}


def _prep(Z):
    Z = np.asarray(Z)
    if Z.dtype not in (np.float32, np.float64):
        Z = Z.astype(np.float64)
    return Z


def sample(Z, dr, dc):
    """Z[r + dr, c + dc] where that row and that column are on the raster, else Z[r, c]"""
    out = Z.copy()
    R, C = Z.shape
    if abs(dr) >= R or abs(dc) >= C:
        return out
    out[max(-dr, 0):R - max(dr, 0), max(-dc, 0):C - max(dc, 0)] = \
        Z[max(dr, 0):R - max(-dr, 0), max(dc, 0):C - max(-dc, 0)]
    return out


def ashift(surface, direction, n=1):
    Z = _prep(surface)
    tap = next((TAPS[k] for k in range(8) if direction == k), (0, 0))
    return sample(Z, tap[0] * n, tap[1] * n)


def _rad2deg(x):
    t = x.dtype.type
    return x * (t(180) / t(np.pi))


def scaled_morphometry(X, cellsize=1, lookup_pixels=1, outputs=None):
    X = _prep(X)
    t = X.dtype.type
    n = int(lookup_pixels)
    L = float(cellsize) * n
    d0, d1, d2, d3 = t(6 * L ** 2), t(3 * L ** 2), t(4 * L ** 2), t(6 * L)
    z1, z2, z3 = sample(X, -n, -n), sample(X, -n, 0), sample(X, -n, n)
    z4, z6 = sample(X, 0, -n), sample(X, 0, n)
    z7, z8, z9 = sample(X, n, -n), sample(X, n, 0), sample(X, n, n)
    with np.errstate(all='ignore'):
        A = (z1 + z3 + z4 + z6 + z7 + z9) / d0 - (z2 + X + z8) / d1
        B = (z1 + z2 + z3 + z7 + z8 + z9) / d0 - (z4 + X + z6) / d1
        C = (z3 + z7 - z1 - z9) / d2
        D = (z3 + z6 + z9 - z1 - z4 - z7) / d3
        E = (z1 + z2 + z3 - z7 - z8 - z9) / d3
        DD, EE = D * D, E * E
        S2 = DD + EE
        two_cde = t(2) * C * D * E
        cde = C * D * E
        SM = {}
        SM["A"] = np.mod(t(270) - _rad2deg(np.arctan2(E, D)), t(360))
        SM["S"] = _rad2deg(np.arctan(np.sqrt(S2)))
        SM["K"] = t(-2) * (A + B)
        SM["K_profile"] = -(A * DD + two_cde + B * EE) / (S2 * np.power(S2 + t(1), t(1.5)))
        SM["K_cross"] = t(-2) * (B * DD + A * EE - cde) / S2
        SM["K_long"] = t(-2) * (A * DD + B * EE + cde) / S2
        SM["K_tan"] = -(A * EE - two_cde + B * DD) / (S2 * np.sqrt(S2 + t(1)))
        SM["K_plan"] = -(A * EE - two_cde + B * DD) / np.power(S2, t(1.5))
    if outputs is not None:
        SM = {k: SM[k] for k in KEYS if k in outputs}
    return SM


def vip_constants(cellsize=1):
    """(x, b2) per parity of the direction: x = dlist[d % 2] * cellsize and b2 = (2x)**2, the power taken on a NumPy
    float64 scalar (C pow), as the reference's triangle_height takes it"""
    cs = float(cellsize)
    dlist = np.array([np.sqrt(2), 1])
    x = [dlist[k] * cs for k in (0, 1)]
    return x, [(2 * v) ** 2 for v in x]


def vip_score(Z, cellsize=1):
    Z = _prep(Z)
    x, b2 = vip_constants(cellsize)
    acc = np.zeros(Z.shape, np.float64)
    with np.errstate(all='ignore'):
        for d in range(4):
            h0 = (ashift(Z, d) - Z).astype(np.float64)
            h1 = (ashift(Z, d + 4) - Z).astype(np.float64)
            xd = float(x[d % 2])
            cp = np.abs(((-xd) * h1) - (h0 * xd))
            dh = h1 - h0
            acc = acc + cp / np.sqrt(float(b2[d % 2]) + dh * dh)
        return acc / 4.0


def triangle_height(h0, h1, x_dist=1):
    """the reference's formula with the 2-D cross product written out; the bits of np.cross"""
    h0 = np.asarray(h0)
    h1 = np.asarray(h1)
    a0 = -x_dist * np.ones(h0.shape)
    b0 = x_dist * np.ones(h1.shape)
    h0 = h0.astype(np.result_type(a0, h0))        # column_stack's promotion
    h1 = h1.astype(np.result_type(b0, h1))
    cp = np.abs(a0 * h1 - h0 * b0)
    dh = h1 - h0
    return cp / np.sqrt((2 * x_dist) ** 2 + dh * dh)
