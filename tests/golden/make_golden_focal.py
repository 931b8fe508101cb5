#!/usr/bin/env python3
"""Generate tests/golden/focal.npz and focal_signatures.json by RUNNING THE REFERENCE's focal functions.

Like make_golden.py this only runs where the reference checkout is available; it imports ``neilpy`` through
``make_golden.import_reference()`` (nothing of the reference is copied here).  ``std``, ``topographic_position_index``,
``reduce_peaks`` and ``distance_kernel`` run under the installed NumPy 2 / SciPy as they are.

Layout of focal.npz:
  ``in_<name>``      input rasters
  ``k_<name>``       kernels (structuring elements / weights)
  ``cases``          JSON list of {"id", "fn", "input", "kernel", "kw"}; ``fn`` is a reference function or "convolve"
                     (raw ``scipy.ndimage.convolve(in, k, mode='nearest')``); the output is ``out_<id>``
  ``dk_cases``       JSON list of {"id", "kw"} for distance_kernel; the output is ``dk_<id>``
  ``numpy_version``, ``scipy_version``
"""
import inspect
import json
import os
import sys
import warnings

import numpy as np
import scipy
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

FOCAL_FUNCS = ["std", "topographic_position_index", "reduce_peaks", "distance_kernel"]
TINY = ("one", "row7", "col7", "r2x5", "r3x2")


def inputs():
    rng = np.random.default_rng(20261018)
    ins = {}
    for s, (r0, c0) in (("samp11", (60, 40)), ("samp21", (10, 50)), ("samp41", (30, 20))):
        z = np.load(os.path.join(HERE, "smrf_%s.npz" % s))["Zpro"]
        ins["dtm" + s[4:]] = np.ascontiguousarray(z[r0:r0 + 20, c0:c0 + 26])
    ins["dtm21_f32"] = ins["dtm21"].astype(np.float32)
    ins["dtm41_f32"] = ins["dtm41"].astype(np.float32)
    nan = ins["dtm41"].copy()
    nan[rng.random(nan.shape) < 0.04] = np.nan
    nan[8:11, 12:16] = np.nan
    nan[0, 0] = np.nan
    nan[0, -1] = np.nan
    nan[-1, 0] = np.nan
    nan[-1, -1] = np.nan
    ins["nan"] = nan
    ins["nan_f32"] = nan.astype(np.float32)
    ins["const"] = np.full((20, 26), 103.7)
    ins["const_f32"] = ins["const"].astype(np.float32)
    ins["one"] = np.array([[3.5]])
    ins["row7"] = rng.normal(size=(1, 7)) * 3
    ins["col7"] = rng.normal(size=(7, 1)) * 3
    ins["r2x5"] = (rng.normal(size=(2, 5)) * 2).astype(np.float32)
    ins["r3x2"] = rng.normal(size=(3, 2)) * 2
    return ins


def kernels(ref):
    rng = np.random.default_rng(20261019)
    ks = {}
    for r in (1, 3, 9):
        ks["disk%d" % r] = make_golden.disk(r)
    ks["ones33"] = np.ones((3, 3))
    ks["dist4"] = ref.distance_kernel(4, method='distance')
    for kh, kw in ((1, 5), (5, 1), (2, 2), (4, 3)):
        ks["pos%dx%d" % (kh, kw)] = rng.uniform(0.2, 2.0, size=(kh, kw))
    # zero weights: a cell whose NaN neighbours all lie under zeros comes out finite
    ks["cross0"] = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=np.float64)
    ring = np.zeros((5, 5))
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = rng.uniform(0.5, 1.5, size=5)
    ks["ring5"] = ring
    # signed weights, zeros included, for the raw convolution
    for kh, kw in ((3, 3), (7, 7), (1, 9), (9, 1), (2, 2), (6, 4), (1, 1)):
        w = rng.normal(size=(kh, kw))
        if w.size > 4:
            w[rng.random(w.shape) < 0.2] = 0.0
        ks["sgn%dx%d" % (kh, kw)] = w
    return ks


def cases():
    out = []

    def add(fn, inp, kernel=None, **kw):
        out.append(dict(id="c%03d" % len(out), fn=fn, input=inp, kernel=kernel, kw=kw))

    main = ("dtm11", "dtm21_f32", "nan", "nan_f32")
    for d in main:
        for k in ("disk1", "disk3", "disk9", "ones33", "dist4", "pos1x5", "pos5x1", "pos2x2", "pos4x3"):
            add("std", d, k)
        for k in ("cross0", "ring5"):
            add("std", d, k)
    add("std", "const", "disk3")
    add("std", "const_f32", "dist4")
    for d in TINY:
        add("std", d, "disk3")
    for d in ("dtm21", "dtm41_f32"):
        for r in (1, 2, 3, 9):
            for st in (True, False):
                add("topographic_position_index", d, radius=r, standardize=st)
    for d in ("nan", "nan_f32", "row7", "r2x5", "r3x2"):
        for st in (True, False):
            add("topographic_position_index", d, radius=2, standardize=st)
    add("topographic_position_index", "dtm11")
    for d in ("dtm11", "dtm21_f32"):
        for r in (3, 8):
            for b in (2, 3):
                add("reduce_peaks", d, radius=r, blend_rate=b)
                add("reduce_peaks", d, radius=r, blend_rate=b, kernel_rate=0.7)
    for d in ("const", "const_f32", "nan", "col7"):
        add("reduce_peaks", d, radius=3)
    for d in ("dtm41", "dtm21_f32", "nan_f32", "r3x2", "one"):
        for k in ("sgn3x3", "sgn7x7", "sgn1x9", "sgn9x1", "sgn2x2", "sgn6x4", "sgn1x1", "disk3", "cross0"):
            add("convolve", d, k)
    return out


def dk_cases():
    out = []
    for method in ("binary", "distance", "idw", "other"):
        for cs in (1, 2, 0.5):
            out.append(dict(id="d%02d" % len(out), kw=dict(radius=5, cellsize=cs, method=method)))
    out.append(dict(id="d%02d" % len(out), kw=dict(radius=3)))
    out.append(dict(id="d%02d" % len(out), kw=dict(radius=2.5, cellsize=1, method="idw", idw_power=3)))
    out.append(dict(id="d%02d" % len(out), kw=dict(radius=8, method="distance")))
    return out


def write_signatures(ref, out):
    sig = {}
    for name in FOCAL_FUNCS:
        ps = inspect.signature(getattr(ref, name)).parameters.values()
        sig[name] = [dict(name=p.name, kind=p.kind.name,
                          default=None if p.default is inspect.Parameter.empty else repr(p.default)) for p in ps]
    with open(os.path.join(out, "focal_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


def main():
    warnings.simplefilter("ignore")
    ref = make_golden.import_reference()
    ins = inputs()
    ks = kernels(ref)
    rec = {"in_" + k: v for k, v in ins.items()}
    rec.update({"k_" + k: v for k, v in ks.items()})
    cs = cases()
    with np.errstate(all="ignore"):
        for c in cs:
            X = ins[c["input"]].copy()
            if c["fn"] == "convolve":
                res = ndi.convolve(X, ks[c["kernel"]], mode='nearest')
            elif c["fn"] == "std":
                res = ref.std(X, ks[c["kernel"]].copy())
            else:
                res = getattr(ref, c["fn"])(X, **c["kw"])
            rec["out_" + c["id"]] = np.asarray(res)
        dks = dk_cases()
        for c in dks:
            rec["dk_" + c["id"]] = np.asarray(ref.distance_kernel(**c["kw"]))
    rec["cases"] = np.array(json.dumps(cs))
    rec["dk_cases"] = np.array(json.dumps(dks))
    rec["numpy_version"] = np.array(np.__version__)
    rec["scipy_version"] = np.array(scipy.__version__)
    np.savez_compressed(os.path.join(HERE, "focal.npz"), **rec)
    write_signatures(ref, HERE)
    print("focal.npz: %d cases, %.0f kB" % (len(cs), os.path.getsize(os.path.join(HERE, "focal.npz")) / 1024))


if __name__ == "__main__":
    main()
