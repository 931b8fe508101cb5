#!/usr/bin/env python3
"""Generate tests/golden/surface.npz and surface_signatures.json by RUNNING THE REFERENCE's surface derivatives.

Like make_golden.py this only runs where the reference checkout is available; it imports ``neilpy`` through
``make_golden.import_reference()`` (nothing of the reference is copied here).  The functions run under the installed
NumPy 2 / SciPy as they are.

Layout of surface.npz:
  ``in_<name>``      input rasters
  ``cases``          JSON list of {"id", "fn", "input", "kw"}; outputs are ``out_<id>`` or, for the multi-output
                     curvatures, ``out_<id>_<k>`` (k = 0.. in the reference's return order)
  ``z_factor_lat``   latitudes and ``z_factor``: the reference's z_factor of each
  ``angles``         JSON of [[zeniths, azimuths, expanded zeniths, expanded azimuths], ...]: multiple_illumination's
                     expansion of scalar / array arguments
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

SURFACE_FUNCS = ["slope", "aspect", "hillshade", "multiple_illumination", "esri_slope", "curvature", "esri_curvature",
                 "zevenbergen_and_thorne_curvature", "evans_curvature", "wilson_gallant_curvature", "z_factor"]
MULTI = ("esri_curvature", "zevenbergen_and_thorne_curvature", "evans_curvature", "wilson_gallant_curvature")
ANGLE_ARGS = [(np.array([45]), 4), (2, 6), (3, 4.0), (np.array([30.0, 60.0]), np.array([0, 90, 225])), (1, 1), (0, 3)]


def inputs():
    rng = np.random.default_rng(20261017)
    ins = {}
    for s, (r0, c0) in (("samp11", (60, 40)), ("samp21", (10, 50)), ("samp41", (30, 20))):
        z = np.load(os.path.join(HERE, "smrf_%s.npz" % s))["Zpro"]
        ins["dtm" + s[4:]] = np.ascontiguousarray(z[r0:r0 + 20, c0:c0 + 26])
    ins["dtm21_f32"] = ins["dtm21"].astype(np.float32)
    ins["one"] = np.array([[3.5]])
    ins["row7"] = rng.normal(size=(1, 7)) * 3
    ins["col7"] = rng.normal(size=(7, 1)) * 3
    ins["sq2"] = rng.normal(size=(2, 2)) * 2
    ins["r2x5"] = rng.normal(size=(2, 5)) * 2
    nan = ins["dtm41"].copy()
    nan[rng.random(nan.shape) < 0.06] = np.nan
    nan[8:11, 12:16] = np.nan
    nan[0, 0] = np.nan
    nan[0, -1] = np.nan
    nan[-1, 0] = np.nan
    nan[-1, -1] = np.nan
    ins["nan"] = nan
    ins["nan_f32"] = nan.astype(np.float32)
    y, x = np.mgrid[0:20, 0:26]
    terr = np.floor((0.35 * x + 0.2 * y + 2.0 * np.sin(x / 6.0)) / 2.0) * 2.0
    terr[6:12, 4:11] = 7.0
    ins["terrace"] = terr
    ins["terrace_f32"] = terr.astype(np.float32)
    return ins


def cases():
    out = []

    def add(fn, inp, **kw):
        out.append(dict(id="c%03d" % len(out), fn=fn, input=inp, kw=kw))

    main = ("dtm11", "dtm21_f32", "nan", "nan_f32", "terrace", "terrace_f32")
    for d in main:
        for ra in ("degrees", "radians", "percent"):
            add("slope", d, return_as=ra)
        add("aspect", d)
        add("aspect", d, return_as="radians", flat_as=-1)
        add("hillshade", d)
        add("esri_slope", d)
        add("esri_slope", d, return_as="none")
        add("curvature", d)
        for f in MULTI:
            add(f, d)
        add("multiple_illumination", d)
    for d in ("dtm41", "dtm21_f32"):
        for cs, zf in ((0.5, 1), (0.3, 2.5)):
            add("slope", d, cellsize=cs, z_factor=zf)
            add("slope", d, cellsize=cs, z_factor=zf, return_as="percent")
            add("hillshade", d, cellsize=cs, z_factor=zf, zenith=30, azimuth=100)
            add("esri_slope", d, cellsize=cs, z_factor=zf)
            add("esri_slope", d, cellsize=cs, z_factor=zf, return_as="percent")
            add("curvature", d, cellsize=cs)
            for f in MULTI:
                add(f, d, cellsize=cs)
    for d in ("dtm41", "nan", "dtm21_f32"):
        add("hillshade", d, return_uint8=False)
        add("hillshade", d, zenith=60, azimuth=0, return_uint8=False)
        add("aspect", d, flat_as=0)
        add("aspect", d, return_as="radians")
    for zs, az in ANGLE_ARGS:
        add("multiple_illumination", "dtm21", zeniths=zs, azimuths=az)
    add("multiple_illumination", "dtm41", cellsize=2, z_factor=1.5, zeniths=3, azimuths=8)
    add("multiple_illumination", "nan_f32", zeniths=2, azimuths=5)
    for d in ("one", "row7", "col7"):
        add("esri_slope", d)
        add("curvature", d)
        for f in MULTI:
            add(f, d)
    for d in ("sq2", "r2x5"):
        for ra in ("degrees", "percent"):
            add("slope", d, return_as=ra)
        add("aspect", d)
        add("hillshade", d)
        add("multiple_illumination", d)
        add("esri_slope", d)
        add("curvature", d)
        for f in MULTI:
            add(f, d)
    return out


def _json_kw(kw):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def write_signatures(ref, out):
    sig = {}
    for name in SURFACE_FUNCS:
        ps = inspect.signature(getattr(ref, name)).parameters.values()
        sig[name] = [dict(name=p.name, kind=p.kind.name,
                          default=None if p.default is inspect.Parameter.empty else repr(p.default)) for p in ps]
    with open(os.path.join(out, "surface_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


def main():
    warnings.simplefilter("ignore")
    ref = make_golden.import_reference()
    ins = inputs()
    rec = {"in_" + k: v for k, v in ins.items()}
    cs = cases()
    for c in cs:
        res = getattr(ref, c["fn"])(ins[c["input"]].copy(), **c["kw"])
        if c["fn"] in MULTI:
            for k, r in enumerate(res):
                rec["out_%s_%d" % (c["id"], k)] = np.asarray(r)
        else:
            rec["out_" + c["id"]] = np.asarray(res)
        c["kw"] = _json_kw(c["kw"])
    rec["cases"] = np.array(json.dumps(cs))
    lat = np.array([0.0, 12.5, 45.0, 60.0, -33.3, 89.0])
    rec["z_factor_lat"] = lat
    rec["z_factor"] = ref.z_factor(lat)
    angles = []
    for zs, az in ANGLE_ARGS:
        # the expansion at the top of multiple_illumination (neilpy.py:830-835), recorded through a hillshade spy
        seen = []
        real = ref.hillshade
        ref.hillshade = lambda Z, cellsize=1, z_factor=1, zenith=45, azimuth=315, **k: (
            seen.append((float(zenith), float(azimuth))) or np.zeros(np.shape(Z), np.uint8))
        try:
            ref.multiple_illumination(np.zeros((3, 3)), zeniths=zs, azimuths=az)
        finally:
            ref.hillshade = real
        angles.append([_json_kw({"z": zs})["z"], _json_kw({"a": az})["a"], seen])
    rec["angles"] = np.array(json.dumps(angles))
    rec["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(os.path.join(HERE, "surface.npz"), **rec)
    write_signatures(ref, HERE)
    print("surface.npz: %d cases, %.0f kB" % (len(cs), os.path.getsize(os.path.join(HERE, "surface.npz")) / 1024))


if __name__ == "__main__":
    main()
