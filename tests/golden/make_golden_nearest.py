#!/usr/bin/env python3
"""Generate tests/golden/nearest.npz and nearest_signatures.json by RUNNING THE REFERENCE's inpaint_nearest.

Like make_golden.py this only runs where the reference checkout is available; it imports ``neilpy`` through
``make_golden.import_reference()`` (nothing of the reference is copied here).  The reference only accepts square
rasters (its meshgrid uses 'xy' indexing), so every case is square.

Layout of nearest.npz:
  ``in_<name>`` / ``out_<name>``  input raster and the reference's result (it fills its argument and returns it)
  ``cases``                       JSON list of {"name", "unique": bool, "note"}; ``unique`` marks the cases in which at least
                                  half of the holes have a single nearest source, the ones that pin the values bit for bit
  ``returns_argument``            JSON {name: bool}: the reference returned the very array it was given
  ``numpy_version`` / ``scipy_version``
"""
import inspect
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402


def _base(rng, n):
    X = rng.normal(size=(n, n)) * 5 + 100
    return X


def inputs():
    rng = np.random.default_rng(20261017)
    ins = {}
    X = _base(rng, 96)
    X[rng.random(X.shape) < 0.10] = np.nan
    X[10:40, 20:70] = np.nan
    X[60:96, 0:17] = np.nan
    X[50, 50] = np.inf
    ins["blocks96"] = (X, True, "10 % scattered holes, two NaN blocks, one +inf")
    ins["blocks96_f32"] = (X.astype(np.float32), True, "the same in float32")
    X = _base(rng, 48)
    X[rng.random(X.shape) < 0.85] = np.nan
    X[np.unravel_index(np.flatnonzero(np.isfinite(X))[3], X.shape)] = np.inf
    ins["sparse48"] = (X, True, "85 % holes: the sources are sparse, one +inf")
    ins["sparse48_f32"] = (X.astype(np.float32), True, "the same in float32")
    X = _base(rng, 64)
    X[rng.random(X.shape) < 0.25] = np.nan
    X[31, 7] = np.inf
    X[5, 5] = -np.inf
    X[40, 40] = -0.0
    ins["scatter64"] = (X, False, "25 % scattered holes: nearly every hole is tied, valid-choice clause only")
    ins["allnan8"] = (np.full((8, 8), np.nan), False, "no source at all: the reference returns its argument unchanged")
    ins["nohole8"] = (_base(rng, 8), False, "no hole")
    ins["int8x8"] = (rng.integers(-50, 50, size=(8, 8)).astype(np.int64), False, "an int64 raster comes back int64")
    return ins


def main():
    warnings.simplefilter("ignore")
    ref = make_golden.import_reference()
    rec, cases, same = {}, [], {}
    for name, (X, unique, note) in inputs().items():
        arg = X.copy()
        res = ref.inpaint_nearest(arg)
        same[name] = res is arg
        rec["in_" + name] = X
        rec["out_" + name] = np.asarray(res)
        cases.append(dict(name=name, unique=unique, note=note))
    rec["cases"] = np.array(json.dumps(cases))
    rec["returns_argument"] = np.array(json.dumps(same))
    rec["numpy_version"] = np.array(np.__version__)
    import scipy
    rec["scipy_version"] = np.array(scipy.__version__)
    np.savez_compressed(os.path.join(HERE, "nearest.npz"), **rec)
    ps = inspect.signature(ref.inpaint_nearest).parameters.values()
    sig = {"inpaint_nearest": [dict(name=p.name, kind=p.kind.name,
                                    default=None if p.default is inspect.Parameter.empty else repr(p.default))
                               for p in ps]}
    with open(os.path.join(HERE, "nearest_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)
    print("nearest.npz: %d cases, %.0f kB" % (len(cases), os.path.getsize(os.path.join(HERE, "nearest.npz")) / 1024))


if __name__ == "__main__":
    main()
