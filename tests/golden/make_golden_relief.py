#!/usr/bin/env python3
"""Generate tests/golden/relief.npz and relief_signatures.json by RUNNING THE REFERENCE's relief-colouring functions.

Like make_golden.py this only runs where the reference checkout is available; it imports ``neilpy`` through
``make_golden.import_reference()`` (nothing of the reference is copied here).  The functions run under the installed
NumPy 2 / SciPy / matplotlib as they are.

Layout of relief.npz:
  ``in_<name>``      input rasters: the small rasters of make_golden_surface.inputs() plus ``const`` and ``inf``
  ``h_<name>``       shades for brassel: the reference's uint8 hillshade of ``in_<name>``; ``hf_<name>`` its float64
                     shade and ``hf32_<name>`` that one as float32
  ``lut_<name>``     colour tables, uint8.  ``swiss``, ``ghc`` (gray_high_contrast, stored 2-D: its three channels are
                     equal) and ``gray`` are the reference's own, recovered by running it on a 256 x 256 ramp
                     Z[i, j] = i with its hillshade replaced by one that returns j, so that the output is the table;
                     ``rand4`` is a seeded random 4-channel table
  ``cases``          JSON list of {"id", "fn", "input", "kw"} (+ "table" for the shading functions, "shade" for
                     brassel); outputs are ``out_<id>`` (cutter: the pieces stacked as (r, c, h, w))
  ``numpy_version``

The generator also checks what the GPU tests rely on: no golden cell of a shading case lies within the hillshade
rounding margin of tests/test_gpu_surface.py, and no uint8 brassel cell within 1e-9 of a half-integer.
"""
import inspect
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
import make_golden_surface  # noqa: E402

RELIEF_FUNCS = ["swiss_shading", "colortable_shade", "rmse", "cutter", "normalize", "brassel_atmospheric_perspective"]
MAIN = ("dtm11", "dtm21_f32", "nan", "nan_f32", "terrace", "terrace_f32")
SHADED = MAIN + ("sq2", "r2x5", "const", "inf")
TABLES = ("swiss", "ghc", "gray", "rand4")
MARGIN, MARGIN_F32 = 1e-9, 1e-4            # tests/test_gpu_surface.py


def inputs():
    ins = {k: v for k, v in make_golden_surface.inputs().items() if k in MAIN + ("sq2", "r2x5")}
    ins["const"] = np.full((20, 26), 7.25)
    inf = ins["dtm11"].copy()
    inf[0, 0] = np.inf          # a corner: its neighbours shade to 0, not to the tie 127.5 an inner inf gives
    ins["inf"] = inf
    return ins


def tables(ref):
    ramp = np.repeat(np.arange(256.0)[:, None], 256, axis=1)
    cols = np.repeat(np.arange(256, dtype=np.uint8)[None, :], 256, axis=0)
    real = ref.hillshade
    ref.hillshade = lambda Z, cellsize=1, *a, **k: cols
    try:
        swiss = ref.swiss_shading(ramp)
        ghc = ref.colortable_shade(ramp, 'gray_high_contrast')
        gray = ref.colortable_shade(ramp, 'gray')
    finally:
        ref.hillshade = real
    assert (ghc[:, :, 0] == ghc[:, :, 1]).all() and (ghc[:, :, 0] == ghc[:, :, 2]).all()
    rng = np.random.default_rng(20261019)
    return {"swiss": swiss, "ghc": np.ascontiguousarray(ghc[:, :, 0]), "gray": gray,
            "rand4": rng.integers(0, 256, size=(256, 256, 4), dtype=np.uint8)}


def cases(ins):
    out = []

    def add(fn, inp, kw=None, **more):
        out.append(dict(id="c%03d" % len(out), fn=fn, input=inp, kw=kw or {}, **more))

    for d in SHADED:
        for t in TABLES:
            add("colortable_shade", d, table=t)
        add("swiss_shading", d, table="swiss")
    for d in ("dtm11", "dtm21_f32", "nan"):
        for cs in (0.5, 2):
            add("colortable_shade", d, dict(cellsize=cs), table="rand4")
            add("swiss_shading", d, dict(cellsize=cs), table="swiss")
    for d in MAIN + ("const", "inf"):
        add("rmse", d)
    for d in MAIN:
        Z = ins[d]
        lo, hi = float(np.nanmin(Z)), float(np.nanmax(Z))
        q = [round(lo + f * (hi - lo), 2) for f in (0.1, 0.4, 0.75, 0.9)]
        add("normalize", d)
        add("normalize", d, dict(yrange=[-1, 1]))
        add("normalize", d, dict(xrange=['min', 'median', 'max'], yrange=[-1, 0, 1]))
        add("normalize", d, dict(xrange=['min', 'mean', 'max'], yrange=[-1, 0, 1]))
        add("normalize", d, dict(xrange=['median', 'max'], yrange=[0, 10]))
        add("normalize", d, dict(xrange=[q[0], q[3]], yrange=[5, -5]))
        add("normalize", d, dict(xrange=[q[0], q[1], q[3]], yrange=[0, 0.25, 1]))
        add("normalize", d, dict(xrange=[q[0], q[1], q[2], q[3]], yrange=[0, 3, 3, -1]))
        add("normalize", d, dict(xrange=['min', q[1], q[2], 'max'], yrange=[0, 1, 2, 3]))
    add("normalize", "const")
    for d in MAIN:
        Z = ins[d]
        mid = round(float(np.nanmean(Z)), 2)
        for shade in ("h", "hf"):
            add("brassel_atmospheric_perspective", d, dict(k=1.371), shade=shade)
            add("brassel_atmospheric_perspective", d, dict(k=4.303, reverse=True), shade=shade)
            add("brassel_atmospheric_perspective", d, dict(k=2.303, Zmid=mid), shade=shade)
            add("brassel_atmospheric_perspective", d, dict(k=2.303, flat=0.6, Zmid=mid, reverse=True), shade=shade)
            add("brassel_atmospheric_perspective", d, dict(k=1.371, C2=0.41), shade=shade)
            add("brassel_atmospheric_perspective", d, dict(k=1.371, flat=200, C2=-0.41), shade=shade)
            add("brassel_atmospheric_perspective", d, dict(k=3.101, Zmid=mid, C2=-0.31), shade=shade)
        add("brassel_atmospheric_perspective", d, dict(k=1), shade="h")
        add("brassel_atmospheric_perspective", d, dict(k=2.5, flat=0.7), shade="hf32")
        add("brassel_atmospheric_perspective", d, dict(k=2.5, flat=0.7, C2=0.21), shade="hf32")
    add("cutter", "dtm11", dict(r=2, c=2))
    add("cutter", "dtm21_f32", dict(r=5, c=13))
    add("cutter", "r2x5", dict(r=2, c=1))
    return out


def write_signatures(ref, out):
    sig = {}
    for name in RELIEF_FUNCS:
        ps = inspect.signature(getattr(ref, name)).parameters.values()
        sig[name] = [dict(name=p.name, kind=p.kind.name,
                          default=None if p.default is inspect.Parameter.empty else repr(p.default)) for p in ps]
    with open(os.path.join(out, "relief_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


def check_margins(ins, cs, rec):
    """what the GPU tests assume of the goldens: zero cells exempt by a rounding margin"""
    import relief_numpy as rn
    import surface_numpy as sn
    for c in cs:
        Z = ins[c["input"]]
        if c["fn"] in ("colortable_shade", "swiss_shading"):
            cell = c["kw"].get("cellsize", 1)
            with np.errstate(all='ignore'):
                m = sn.half_margin(sn.hillshade_value(Z, cell), sn.flat_cells(Z, cell))
            need = MARGIN_F32 if Z.dtype == np.float32 else MARGIN
            assert (m >= need).all(), ("hillshade margin", c, float(m.min()))
        elif c["fn"] == "brassel_atmospheric_perspective":
            v, was_int = rn.brassel_value(rec[c["shade"] + "_" + c["input"]], Z, **c["kw"])
            if was_int:
                v = 255 * v
                m = np.abs(v - (np.floor(v) + 0.5))
                assert not (m < 1e-9).any(), ("brassel margin", c)


def main():
    warnings.simplefilter("ignore")
    ref = make_golden.import_reference()
    ins = inputs()
    rec = {"in_" + k: v for k, v in ins.items()}
    luts = tables(ref)
    rec.update({"lut_" + k: v for k, v in luts.items()})
    for d in MAIN:
        rec["h_" + d] = ref.hillshade(ins[d].copy())
        rec["hf_" + d] = ref.hillshade(ins[d].copy(), return_uint8=False)
        rec["hf32_" + d] = rec["hf_" + d].astype(np.float32)
    cs = cases(ins)
    for c in cs:
        Z = ins[c["input"]].copy()
        kw = dict(c["kw"])
        if c["fn"] == "colortable_shade":
            res = ref.colortable_shade(Z, luts[c["table"]], **kw)
        elif c["fn"] == "swiss_shading":
            res = ref.swiss_shading(Z, **kw)                 # the reference reads its own table: lut_swiss
        elif c["fn"] == "brassel_atmospheric_perspective":
            res = ref.brassel_atmospheric_perspective(rec[c["shade"] + "_" + c["input"]].copy(), Z, **kw)
        elif c["fn"] == "cutter":
            res = np.array(ref.cutter(Z, **kw))
        else:
            res = getattr(ref, c["fn"])(Z, **kw)
        rec["out_" + c["id"]] = np.asarray(res)
    check_margins(ins, cs, rec)
    rec["cases"] = np.array(json.dumps(cs))
    rec["numpy_version"] = np.array(np.__version__)
    path = os.path.join(HERE, "relief.npz")
    np.savez_compressed(path, **rec)
    write_signatures(ref, HERE)
    print("relief.npz: %d cases, %.0f kB" % (len(cs), os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
