#!/usr/bin/env python3
"""Generate tests/golden/points.npz by RUNNING THE REFERENCE's chamfer_distance.

Like make_golden.py this only runs where the reference checkout is available; it imports ``neilpy`` through
``make_golden.import_reference()`` (nothing of the reference is copied here).

Layout of points.npz:
  ``x_<name>`` / ``y_<name>``    the two clouds of a case, in the dtype they were handed to the reference
  ``cd_<name>``                  float64 (3,): the reference's chamfer_distance for 'y_to_x', 'x_to_y', 'bi'
  ``cases``                      JSON list of {"name", "note"}
  ``result_types``               JSON {name: type name of the reference's result} (numpy.float64 also for float32 clouds)
  ``raises``                     JSON {what: exception type name}: a wrong direction, an empty cloud
  ``sklearn_version`` / ``numpy_version``
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

DIRECTIONS = ("y_to_x", "x_to_y", "bi")
NX, NY = 3000, 2500
OFFSET = (5.4e6, 5.1e5, 300.0)


def inputs():
    rng = np.random.default_rng(20261018)
    ins = {}
    ins["uniform2d"] = (rng.uniform(0, 100, (NX, 2)), rng.uniform(0, 100, (NY, 2)), "2-D uniform")

    def flat3(n):
        return np.column_stack([rng.uniform(0, 100, n), rng.uniform(0, 100, n), rng.uniform(0, 5, n)])
    x3, y3 = flat3(NX), flat3(NY)
    ins["flat3d"] = (x3, y3, "3-D, the z extent 5 % of x and y")
    ins["flat3d_offset"] = (x3 + np.array(OFFSET), y3 + np.array(OFFSET), "the same clouds offset by %r" % (OFFSET,))
    ins["f32"] = (rng.uniform(0, 100, (NX, 3)).astype(np.float32), rng.uniform(0, 100, (NY, 3)).astype(np.float32),
                  "a float32 pair")
    same = rng.uniform(0, 100, (NY, 2))
    ins["equal"] = (same, same.copy(), "x equal to y")
    return ins


def main():
    warnings.simplefilter("ignore")
    ref = make_golden.import_reference()
    rec, cases, types = {}, [], {}
    for name, (x, y, note) in inputs().items():
        vals = [ref.chamfer_distance(x, y, direction=d) for d in DIRECTIONS]
        types[name] = type(vals[0]).__module__ + "." + type(vals[0]).__name__
        rec["x_" + name], rec["y_" + name] = x, y
        rec["cd_" + name] = np.array(vals, dtype=np.float64)
        cases.append(dict(name=name, note=note))
    raises = {}
    x, y = inputs()["uniform2d"][:2]
    for what, call in (("direction", lambda: ref.chamfer_distance(x, y, direction="both")),
                       ("empty", lambda: ref.chamfer_distance(x, y[:0]))):
        try:
            call()
            raises[what] = None
        except Exception as e:                      # recorded, whatever it is
            raises[what] = type(e).__name__
    rec["cases"] = np.array(json.dumps(cases))
    rec["result_types"] = np.array(json.dumps(types))
    rec["raises"] = np.array(json.dumps(raises))
    import sklearn
    rec["sklearn_version"] = np.array(sklearn.__version__)
    rec["numpy_version"] = np.array(np.__version__)
    out = os.path.join(HERE, "points.npz")
    np.savez_compressed(out, **rec)
    print("points.npz: %d cases, %.0f kB" % (len(cases), os.path.getsize(out) / 1024), types, raises)


if __name__ == "__main__":
    main()
