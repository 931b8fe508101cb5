#!/usr/bin/env python3
"""Generate tests/golden/morphometry.npz and morphometry_signatures.json by RUNNING THE REFERENCE's multi-scale tools:
scaled_morphometry, vip_score, ashift and triangle_height.

Like make_golden.py this only runs where the reference checkout is available; it imports ``neilpy`` through
``make_golden.import_reference()`` (nothing of the reference is copied here).  The functions run under the installed
NumPy 2 as they are; np.cross's deprecation warning for 2-vectors is silenced.

Layout of morphometry.npz:
  ``in_<name>``      input rasters: those of make_golden_surface.inputs()
  ``cases``          JSON list of {"id", "fn", "input", "kw"}; outputs are ``out_<id>`` or, for scaled_morphometry,
                     ``out_<id>_<key>`` for each key of the returned dict
  ``keys``           JSON list: the reference's dict order
  ``th_h0``, ``th_h1``, ``th_cases`` (JSON list of {"id", "x_dist"}), ``th_<id>``: triangle_height on 1-D arrays
  ``numpy_version``
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
import make_golden_surface  # noqa: E402

FUNCS = ["scaled_morphometry", "vip_score", "ashift", "triangle_height"]
LOOKUPS = (1, 2, 5, 19, 20, 26, 40)      # 20 x 26 rasters: n = rows - 1, rows, cols and beyond
CELLSIZES = (1, 0.5, 2.5)
SMALL = ("one", "row7", "col7", "sq2", "r2x5")


def cases():
    out = []

    def add(fn, inp, **kw):
        out.append(dict(id="c%03d" % len(out), fn=fn, input=inp, kw=kw))

    # every lookup distance on a float32 raster (half the bytes), a spread of (distance, cellsize) on the others
    for n in LOOKUPS:
        add("scaled_morphometry", "dtm21_f32", lookup_pixels=n)
    for n, cs in ((1, 0.5), (5, 2.5)):
        add("scaled_morphometry", "dtm21_f32", cellsize=cs, lookup_pixels=n)
    for n, cs in ((1, 1), (5, 0.5), (20, 2.5)):
        add("scaled_morphometry", "dtm11", cellsize=cs, lookup_pixels=n)
    for n, cs in ((2, 0.5), (26, 1)):
        add("scaled_morphometry", "nan", cellsize=cs, lookup_pixels=n)
    for n, cs in ((1, 1), (5, 1), (19, 2.5), (40, 0.5)):
        add("scaled_morphometry", "nan_f32", cellsize=cs, lookup_pixels=n)
    for n, cs in ((1, 1), (2, 2.5)):
        add("scaled_morphometry", "terrace", cellsize=cs, lookup_pixels=n)
    add("scaled_morphometry", "terrace_f32")
    for d in SMALL:
        for n in (1, 2, 5):
            for cs in CELLSIZES:
                add("scaled_morphometry", d, cellsize=cs, lookup_pixels=n)
    for d in make_golden_surface.inputs():
        add("vip_score", d)
    for d, cs in (("dtm11", 0.5), ("dtm21_f32", 2.5), ("nan", 2.5), ("terrace_f32", 0.5), ("r2x5", 0.5)):
        add("vip_score", d, cellsize=cs)
    for d in ("dtm21_f32", "r2x5", "col7"):
        for direction in range(10):
            for n in (1, 3, 25):
                add("ashift", d, direction=direction, n=n)
    return out


def write_signatures(ref, out):
    sig = {}
    for name in FUNCS:
        ps = inspect.signature(getattr(ref, name)).parameters.values()
        sig[name] = [dict(name=p.name, kind=p.kind.name,
                          default=None if p.default is inspect.Parameter.empty else repr(p.default)) for p in ps]
    with open(os.path.join(out, "morphometry_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


def main():
    warnings.simplefilter("ignore")
    ref = make_golden.import_reference()
    saved = np.geterr()
    ins = make_golden_surface.inputs()
    rec = {"in_" + k: v for k, v in ins.items()}
    cs = cases()
    keys = None
    for c in cs:
        Z = ins[c["input"]].copy()
        if c["fn"] == "ashift":
            res = ref.ashift(Z, c["kw"]["direction"], c["kw"]["n"])
        else:
            res = getattr(ref, c["fn"])(Z, **c["kw"])
        assert np.array_equal(Z, ins[c["input"]], equal_nan=True)      # inputs are left alone
        if c["fn"] == "scaled_morphometry":
            keys = keys or list(res)
            assert list(res) == keys
            for k, v in res.items():
                rec["out_%s_%s" % (c["id"], k)] = np.asarray(v)
        else:
            rec["out_" + c["id"]] = np.asarray(res)
    np.seterr(**saved)                                                  # the reference leaves 'warn' behind
    rec["cases"] = np.array(json.dumps(cs))
    rec["keys"] = np.array(json.dumps(keys))
    rng = np.random.default_rng(20261018)
    h0 = rng.normal(size=64) * 3
    h1 = rng.normal(size=64) * 3
    h0[:4] = (0.0, np.nan, np.inf, 1.0)
    h1[:4] = (0.0, 1.0, 1.0, 1.0)
    rec["th_h0"], rec["th_h1"] = h0, h1
    th = []
    for x in (1, 2, 0.5, float(np.sqrt(2)), float(np.sqrt(2) * 2.5)):
        t = dict(id="t%d" % len(th), x_dist=x)
        rec["th_" + t["id"]] = ref.triangle_height(h0, h1, x)
        th.append(t)
    rec["th_f32"] = ref.triangle_height(h0.astype(np.float32), h1.astype(np.float32))
    rec["th_default"] = ref.triangle_height(h0, h1)
    rec["th_cases"] = np.array(json.dumps(th))
    rec["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(os.path.join(HERE, "morphometry.npz"), **rec)
    write_signatures(ref, HERE)
    print("morphometry.npz: %d cases, %.0f kB" % (len(cs), os.path.getsize(os.path.join(HERE, "morphometry.npz")) / 1024))


if __name__ == "__main__":
    main()
