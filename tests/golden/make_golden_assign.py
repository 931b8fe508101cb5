#!/usr/bin/env python3
"""Generate tests/golden/assign.npz by RUNNING THE REFERENCE's hungarian_algorithm, bdr and bdr_bootstrap.

Like make_golden.py this only runs where the reference checkout is available; it imports ``neilpy`` through
``make_golden.import_reference()`` (nothing of the reference is copied here).

Layout of assign.npz:
  ``hx_<name>`` / ``ha_<name>``            the two clouds of a hungarian case; ``hr_`` / ``hc_`` / ``hm_<name>`` the
                                           reference's row_indices, col_indices, min_costs
  ``bx_<name>`` / ``ba_<name>``            the (n, 2) clouds of a bdr case; ``bdr_<name>_<key>`` the reference's value of
                                           every key; ``bld_<name>_<key>`` the reference run on np.longdouble copies,
                                           stored as float64 (hi, lo) pairs in a trailing axis of 2 (``P``: the closed
                                           form ``(1 - rsquare) ** (n - 2)``, there being no longdouble F distribution)
  ``sx_<name>`` / ``sa_<name>``            the clouds of a bdr_bootstrap case; ``ss_<name>`` the seed given to
                                           np.random.seed before the call, ``sr_`` / ``sd_<name>`` the reference's
                                           rsquare and DI (k = 64)
  ``hungarian_cases`` / ``bdr_cases`` / ``bootstrap_cases``   JSON lists of names
  ``numpy_version`` / ``scipy_version``
"""
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

OFFSET = np.array([5.4e6, 5.1e5])
KEYS = ("beta1", "beta2", "alpha1", "alpha2", "scale", "theta", "aPrime", "bPrime", "rsquare", "D", "Dmax", "DI", "F", "P")
K = 64


def similar(rng, n, noise, scale=1.7, deg=25.0, shift=(40.0, -15.0), extent=100.0):
    """XY uniform in a square, AB its similarity transform plus Gaussian noise: rsquare well inside (0, 1)"""
    xy = rng.uniform(0, extent, (n, 2))
    c, s = scale * np.cos(np.deg2rad(deg)), scale * np.sin(np.deg2rad(deg))
    ab = np.column_stack([shift[0] + c * xy[:, 0] - s * xy[:, 1], shift[1] + s * xy[:, 0] + c * xy[:, 1]])
    return xy, ab + rng.normal(0, noise, (n, 2))


def bdr_inputs():
    rng = np.random.default_rng(20261020)
    ins = {}
    for name, n, noise in (("n3", 3, 20.0), ("n5", 5, 30.0), ("n30", 30, 40.0), ("n64", 64, 25.0), ("n65", 65, 60.0),
                           ("n300", 300, 35.0)):
        ins[name] = similar(rng, n, noise)
    xy, ab = similar(rng, 100, 45.0, scale=0.8, deg=-130.0)
    ins["offset"] = (xy + OFFSET, ab + OFFSET)
    return ins


def hungarian_inputs():
    rng = np.random.default_rng(20261021)
    ins = {"sq30": (rng.uniform(0, 100, (30, 2)), rng.uniform(0, 100, (30, 2))),
           "wide3d": (rng.uniform(0, 100, (40, 3)), rng.uniform(0, 100, (57, 3))),
           "tall3d": (rng.uniform(0, 100, (57, 3)), rng.uniform(0, 100, (40, 3)))}
    centres = rng.uniform(0, 50, (8, 2))
    cl = np.vstack([c + rng.normal(0, 1.5, (8, 2)) for c in centres]) + OFFSET
    ins["offset64"] = (cl, cl[rng.permutation(64)] + rng.normal(0, 0.7, (64, 2)))
    return ins


def bootstrap_inputs():
    rng = np.random.default_rng(20261022)
    ins = {}
    for name, n, m, seed in (("30of60", 30, 60, 11), ("64of64", 64, 64, 12), ("65of130", 65, 130, 13)):
        xy, ab = similar(rng, m, 12.0)
        ins[name] = (xy[rng.permutation(m)[:n]], ab, seed)
    return ins


def pair(v):
    """a longdouble value or array as float64 (hi, lo) in a trailing axis"""
    v = np.asarray(v, dtype=np.longdouble)
    hi = v.astype(np.float64)
    lo = (v - hi.astype(np.longdouble)).astype(np.float64)
    return np.stack([hi, lo], axis=-1)


def bdr_longdouble(ref, XY, AB):
    """the reference's own bdr run on np.longdouble copies of the clouds: every array operation in it then rounds in
    longdouble.  Its ``P`` goes through scipy.stats, which computes in float64, so ``P`` is taken separately, as the
    closed form of the F tail with two numerator degrees of freedom, from the longdouble rsquare"""
    L = np.longdouble
    real = ref.stats

    class FloatF:                 # scipy's F distribution refuses a longdouble argument: hand it the float64 it computes in
        @staticmethod
        def cdf(x, dfn, dfd):
            return real.f.cdf(np.float64(x), dfn, dfd)
    ref.stats = types.SimpleNamespace(f=FloatF)
    try:
        r = dict(ref.bdr(XY.astype(L), AB.astype(L)))
    finally:
        ref.stats = real
    for key in KEYS:
        if key != "P":
            assert np.asarray(r[key]).dtype == L, (key, np.asarray(r[key]).dtype)
    r["P"] = (1 - r["rsquare"]) ** L(len(XY) - 2)
    return r


def main():
    warnings.simplefilter("ignore")
    ref = make_golden.import_reference()
    rec = {}
    for name, (x, a) in hungarian_inputs().items():
        rows, cols, costs = ref.hungarian_algorithm(x, a)
        rec["hx_" + name], rec["ha_" + name] = x, a
        rec["hr_" + name], rec["hc_" + name], rec["hm_" + name] = (np.asarray(rows, np.int64), np.asarray(cols, np.int64),
                                                                   np.asarray(costs, np.float64))
    for name, (x, a) in bdr_inputs().items():
        got, ld = ref.bdr(x, a), bdr_longdouble(ref, x, a)
        assert set(got) == set(KEYS)
        rec["bx_" + name], rec["ba_" + name] = x, a
        for key in KEYS:
            rec["bdr_%s_%s" % (name, key)] = np.asarray(got[key], np.float64)
            rec["bld_%s_%s" % (name, key)] = pair(ld[key])
    for name, (x, a, seed) in bootstrap_inputs().items():
        np.random.seed(seed)
        rsq, di = ref.bdr_bootstrap(x, a, K)
        rec["sx_" + name], rec["sa_" + name], rec["ss_" + name] = x, a, np.array(seed)
        rec["sr_" + name], rec["sd_" + name] = rsq, di
    rec["hungarian_cases"] = np.array(json.dumps(sorted(hungarian_inputs())))
    rec["bdr_cases"] = np.array(json.dumps(list(bdr_inputs())))
    rec["bootstrap_cases"] = np.array(json.dumps(list(bootstrap_inputs())))
    import scipy
    rec["numpy_version"] = np.array(np.__version__)
    rec["scipy_version"] = np.array(scipy.__version__)
    out = os.path.join(HERE, "assign.npz")
    np.savez_compressed(out, **rec)
    print("assign.npz: %.0f kB" % (os.path.getsize(out) / 1024))
    for name in bdr_inputs():
        print(name, "rsquare", float(rec["bdr_%s_rsquare" % name]), "P", float(rec["bdr_%s_P" % name]))
    for name in bootstrap_inputs():
        print(name, "rsquare", rec["sr_" + name].min(), rec["sr_" + name].max())


if __name__ == "__main__":
    main()
