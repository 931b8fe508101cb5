#!/usr/bin/env python3
"""Generate tests/golden/terrain.npz and terrain_signatures.json by RUNNING THE REFERENCE's terrain functions.

Like make_golden.py this only runs where the reference checkout is available; it imports ``neilpy`` through
``make_golden.import_reference()`` (nothing of the reference is copied here).  The reference's openness family uses
three NumPy aliases that NumPy 2 removed (``np.Inf`` in openness, ``np.float`` in skyview_factor, ``np.int`` in
geomorphons(enhance=True)); they are set back to ``np.inf``, ``float`` and ``int`` before anything is called.

Layout of terrain.npz:
  ``in_<name>``           input rasters
  ``cases``               JSON list of {"id", "fn", "input", "kw"}; outputs are ``out_<id>`` (``out_<id>_pos`` /
                          ``out_<id>_neg`` for count_openness)
  ``lowest_table``        get_lowest_equivalent over all 3**8 codes
  ``geo_strict``, ``geo_loose``  terrain_code_to_geomorphon's tables (applied to arange(3**8))
  ``pw_<a>_<b>_<c>``      progressive_window(a, b, c)
  ``int2base``            JSON of [[x, b, result], ...];  ``cmap``: JSON of geomorphon_cmap()
  ``numpy_version``
"""
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

TERRAIN_FUNCS = ["openness", "skyview_factor", "count_openness", "geomorphons", "ternary_pattern_from_openness",
                 "progressive_window", "int2base", "get_lowest_equivalent", "terrain_code_to_geomorphon",
                 "geomorphon_cmap"]


def restore_numpy_aliases():
    np.Inf = np.inf
    np.float = float
    np.int = int


def inputs():
    rng = np.random.default_rng(20261016)
    ins = {}
    for s, (r0, c0) in (("samp11", (100, 20)), ("samp21", (20, 30)), ("samp41", (10, 40)), ("samp24", (5, 10))):
        z = np.load(os.path.join(HERE, "smrf_%s.npz" % s))["Zpro"]
        ins["dtm" + s[4:]] = np.ascontiguousarray(z[r0:r0 + 48, c0:c0 + 60])
    ins["dtm21_f32"] = ins["dtm21"].astype(np.float32)
    ins["one"] = np.array([[3.5]])
    ins["row7"] = rng.normal(size=(1, 7)) * 3
    ins["col7"] = rng.normal(size=(7, 1)) * 3
    ins["sq5"] = rng.normal(size=(5, 5)) * 2
    nan = ins["dtm41"][:40, :48].copy()
    nan[rng.random(nan.shape) < 0.06] = np.nan
    nan[12:16, 20:25] = np.nan
    nan[0, 0] = np.nan
    nan[39, 47] = np.nan
    ins["nan"] = nan
    y, x = np.mgrid[0:36, 0:44]
    terr = np.floor((0.35 * x + 0.2 * y + 2.0 * np.sin(x / 6.0)) / 2.0) * 2.0
    terr[10:18, 5:15] = 7.0
    ins["terrace"] = terr
    return ins


def cases():
    out = []

    def add(fn, inp, **kw):
        out.append(dict(id="c%03d" % len(out), fn=fn, input=inp, kw=kw))

    for d in ("dtm11", "dtm21", "dtm41", "dtm24"):
        add("openness", d, lookup_pixels=10)
        add("skyview_factor", d, lookup_pixels=10)
        add("geomorphons", d, lookup_pixels=10, threshold_angle=1)
        add("count_openness", d, cellsize=1, lookup_pixels=3, threshold_angle=1)
        add("ternary_pattern_from_openness", d, lookup_pixels=3, threshold_angle=1)
    for L in (0, 1, 3, 10, 20, 25):
        add("openness", "dtm21", lookup_pixels=L)
        add("geomorphons", "dtm41", lookup_pixels=L, threshold_angle=1)
        add("skyview_factor", "dtm24", lookup_pixels=L)
    add("openness", "dtm21", lookup_pixels=25, fast=True)
    add("geomorphons", "dtm11", lookup_pixels=25, threshold_angle=1, fast=True)
    add("count_openness", "dtm11", cellsize=1, lookup_pixels=25, threshold_angle=1, fast=True)
    add("openness", "dtm21", lookup_pixels=0, fast=True)
    add("geomorphons", "dtm21", lookup_pixels=20, threshold_angle=1, enhance=True)
    add("geomorphons", "dtm41", lookup_pixels=20, threshold_angle=0.5, enhance=True, fast=True)
    add("geomorphons", "dtm24", lookup_pixels=12, threshold_angle=1, enhance=True)
    for nb in ([0], [3, 1], [1, 1, 5]):
        add("openness", "dtm11", lookup_pixels=5, neighbors=nb)
    add("ternary_pattern_from_openness", "dtm21", lookup_pixels=5, threshold_angle=2, use_negative_openness=False)
    add("ternary_pattern_from_openness", "dtm41", lookup_pixels=5, threshold_angle=1, lowest=True)
    for d in ("one", "row7", "col7"):
        add("openness", d, lookup_pixels=3)
        add("skyview_factor", d, lookup_pixels=3)
        add("geomorphons", d, lookup_pixels=3, threshold_angle=1)
        add("ternary_pattern_from_openness", d, lookup_pixels=3, threshold_angle=1)
    add("openness", "sq5", lookup_pixels=9)
    add("skyview_factor", "sq5", lookup_pixels=9)
    add("geomorphons", "sq5", lookup_pixels=9, threshold_angle=1)
    add("count_openness", "sq5", cellsize=1, lookup_pixels=9, threshold_angle=1)
    add("ternary_pattern_from_openness", "sq5", lookup_pixels=9, threshold_angle=1)
    for f in ("openness", "skyview_factor"):
        add(f, "nan", lookup_pixels=6)
    add("geomorphons", "nan", lookup_pixels=6, threshold_angle=1)
    add("ternary_pattern_from_openness", "nan", lookup_pixels=6, threshold_angle=1)
    add("openness", "dtm21_f32", lookup_pixels=10)
    add("skyview_factor", "dtm21_f32", lookup_pixels=10)
    add("geomorphons", "dtm21_f32", lookup_pixels=10, threshold_angle=1)
    add("ternary_pattern_from_openness", "dtm21_f32", lookup_pixels=4, threshold_angle=1)
    for cs in (0.3, 2):
        add("openness", "dtm24", cellsize=cs, lookup_pixels=8)
        add("skyview_factor", "dtm24", cellsize=cs, lookup_pixels=8)
        add("geomorphons", "dtm24", cellsize=cs, lookup_pixels=8, threshold_angle=1)
    add("geomorphons", "terrace", lookup_pixels=6, threshold_angle=0)
    add("count_openness", "terrace", cellsize=1, lookup_pixels=6, threshold_angle=0)
    add("ternary_pattern_from_openness", "terrace", lookup_pixels=6, threshold_angle=0)
    add("ternary_pattern_from_openness", "terrace", lookup_pixels=6, threshold_angle=0, lowest=True)
    add("openness", "terrace", lookup_pixels=6)
    return out


def run_case(ref, c, Z):
    kw = dict(c["kw"])
    if "neighbors" in kw:
        kw["neighbors"] = np.array(kw["neighbors"])
    fn = getattr(ref, c["fn"])
    if c["fn"] == "count_openness":
        return fn(Z, kw.pop("cellsize"), kw.pop("lookup_pixels"), kw.pop("threshold_angle"), **kw)
    return fn(Z, **kw)


def write_signatures(ref, out):
    sig = {}
    for name in TERRAIN_FUNCS:
        ps = inspect.signature(getattr(ref, name)).parameters.values()
        sig[name] = [dict(name=p.name, kind=p.kind.name,
                          default=None if p.default is inspect.Parameter.empty else repr(p.default)) for p in ps]
    with open(os.path.join(out, "terrain_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


def main():
    ref = make_golden.import_reference()
    restore_numpy_aliases()
    ins = inputs()
    rec = {"in_" + k: v for k, v in ins.items()}
    cs = cases()
    for c in cs:
        res = run_case(ref, c, ins[c["input"]].copy())
        if c["fn"] == "count_openness":
            rec["out_%s_pos" % c["id"]], rec["out_%s_neg" % c["id"]] = res
        else:
            rec["out_" + c["id"]] = np.asarray(res)
    rec["cases"] = np.array(json.dumps(cs))
    codes = np.arange(3 ** 8)
    rec["lowest_table"] = np.array([ref.get_lowest_equivalent(x) for x in codes])
    rec["geo_strict"] = ref.terrain_code_to_geomorphon(codes, 'strict')
    rec["geo_loose"] = ref.terrain_code_to_geomorphon(codes, 'loose')
    for a, b, p in ((1, 25, 20), (1, 50, 20), (1, 1, 20), (1, 0, 20), (2, 40, 35), (1, 100, 10)):
        rec["pw_%d_%d_%d" % (a, b, p)] = ref.progressive_window(a, b, p)
    rec["int2base"] = np.array(json.dumps([[x, b, ref.int2base(x, b)] for x, b in
                                           ((0, 3), (5, 2), (241, 3), (6560, 3), (255, 16), (123456789, 36))]))
    rec["cmap"] = np.array(json.dumps({str(k): v for k, v in ref.geomorphon_cmap().items()}))
    rec["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(os.path.join(HERE, "terrain.npz"), **rec)
    write_signatures(ref, HERE)
    print("terrain.npz: %d cases, %.0f kB" % (len(cs), os.path.getsize(os.path.join(HERE, "terrain.npz")) / 1024))


if __name__ == "__main__":
    main()
