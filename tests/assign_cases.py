"""The clouds and bounds of the point-set matching tests (tests/test_assign_host.py, tests/test_gpu_assign.py); a plain
helper module, no test in it.  DESIGN.md section 18."""
import numpy as np

import assign_numpy as an

OFFSET = np.array([5.4e6, 5.1e5])
SQUARE = (1, 2, 3, 63, 64, 65, 130)
RECT = ((1, 5), (5, 9), (9, 5), (64, 100), (40, 257))
TIES = ((8, 0, 20.0), (33, 3, 82.5), (64, 0, 160.0), (65, 7, 162.5))     # (rows, extra columns, the optimum's total)
ULP = 2.0 ** -52


def random_pair(nr, nc, d, seed):
    rng = np.random.default_rng([seed, nr, nc, d])
    return rng.uniform(0, 100, (nr, d)), rng.uniform(0, 100, (nc, d))


def offset_pair(nr, nc, seed):
    """clustered clouds shifted by (5.4e6, 5.1e5): 22 bits of the mantissa gone to the offset"""
    rng = np.random.default_rng([seed, nr, nc])
    centres = rng.uniform(0, 60, (6, 2))
    x = centres[rng.integers(0, 6, nr)] + rng.normal(0, 1.5, (nr, 2))
    a = centres[rng.integers(0, 6, nc)] + rng.normal(0, 1.5, (nc, 2))
    return x + OFFSET, a + OFFSET


def tie_pair(n, extra, seed):
    """points (3t, 4t), t a permutation of 0 .. n-1 on one side and of 0.5 .. n+extra-0.5 on the other: every cost is
    5 |t - s|, an exact multiple of 2.5, so the dual arithmetic is exact and optimal assignments abound"""
    rng = np.random.default_rng([seed, n, extra])
    t = rng.permutation(n).astype(np.float64)
    s = rng.permutation(n + extra).astype(np.float64) + 0.5
    return np.column_stack([3 * t, 4 * t]), np.column_stack([3 * s, 4 * s])


def degenerate_pairs():
    rng = np.random.default_rng(77)
    out = {}
    p = np.tile(np.array([[12.5, -3.25]]), (20, 1))
    out["all_equal"] = (p, p.copy())
    out["all_equal_rect"] = (p[:7], p)
    base = rng.uniform(0, 50, (12, 3))
    out["duplicated"] = (np.tile(base, (3, 1)), np.tile(base, (3, 1))[rng.permutation(36)])
    ii, jj = np.meshgrid(np.arange(6.0), np.arange(6.0), indexing="ij")
    ci, cj = np.meshgrid(np.arange(5.0) + 0.5, np.arange(5.0) + 0.5, indexing="ij")
    out["lattice"] = (np.column_stack([ii.ravel(), jj.ravel()]), np.column_stack([ci.ravel(), cj.ravel()]))
    return out


def scipy_assignment(x, a):
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial.distance import cdist
    C = cdist(x, a)
    rows, cols = linear_sum_assignment(C)
    return rows, cols, C[rows, cols]


def longdouble(G, name, key):
    v = G["bld_%s_%s" % (name, key)]
    return v[..., 0].astype(np.longdouble) + v[..., 1].astype(np.longdouble)


def rel_error(value, exact):
    """the largest |value - exact| over the field, relative to the field's largest magnitude"""
    exact = np.asarray(exact, np.longdouble)
    return float(np.max(np.abs(np.asarray(value, np.longdouble) - exact)) / np.max(np.abs(exact)))


def bdr_bounds(G, cases):
    """{field: (reference's worst relative error over the cases, allowed error = 4 x that + 4 ulp)} for the device-formed
    fields and scale / theta; 'P': (largest |closed form - reference|, 4 x that), absolute"""
    out = {}
    for key in an.DEVICE_FIELDS + ("scale", "theta"):
        worst = max(rel_error(G["bdr_%s_%s" % (name, key)], longdouble(G, name, key)) for name in cases)
        out[key] = (worst, 4 * worst + 4 * ULP)
    gap = max(abs(float((1 - G["bdr_%s_rsquare" % name]) ** (len(G["bx_" + name]) - 2)) - float(G["bdr_%s_P" % name]))
              for name in cases)
    out["P"] = (gap, 4 * gap)
    return out
