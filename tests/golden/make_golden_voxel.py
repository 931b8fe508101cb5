#!/usr/bin/env python3
"""Generate tests/golden/voxel.npz by RUNNING THE REFERENCE's voxelize(None, ...).

Like make_golden.py this only runs where the reference checkout is available; it imports ``neilpy`` through
``make_golden.import_reference()`` (nothing of the reference is copied here).

Layout of voxel.npz:
  ``x_<cloud>`` / ``y_<cloud>`` / ``z_<cloud>``   a cloud, in the dtype it was handed to the reference
  ``bits_<case>`` / ``shape_<case>``              np.packbits of the reference's boolean result and its shape
  ``cases``        JSON list of {"name", "cloud", "note", "kwargs"}; kwargs always holds ``resolution``
  ``signature``    JSON list of {"name", "kind", "default"} of the reference's voxelize, as inspect.signature gives it
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

N = 5000
OFFSET = (5.4e6, 5.1e5, 300.0)


def clouds():
    rng = np.random.default_rng(20261019)
    x = rng.uniform(1000.0, 1100.0, N)
    y = rng.uniform(500.0, 560.0, N)
    z = 40.0 + 8.0 * np.sin(x / 15.0) * np.cos(y / 11.0) + rng.normal(0.0, 0.4, N)
    out = {"strip": (x, y, z)}
    out["strip_f32"] = tuple(a.astype(np.float32) for a in (x, y, z))
    out["offset"] = (x - 1000.0 + OFFSET[0], y - 500.0 + OFFSET[1], z - 40.0 + OFFSET[2])
    out["tall_y"] = (y.copy(), x.copy(), z.copy())                                   # max_y > max_x
    # integer-valued extents, points exactly on the last edge of every axis (and on interior edges)
    ix = np.concatenate([rng.uniform(0.0, 64.0, 2000), rng.integers(0, 65, 500).astype(np.float64), [0.0, 64.0, 64.0]])
    iy = np.concatenate([rng.uniform(0.0, 32.0, 2000), rng.integers(0, 33, 500).astype(np.float64), [0.0, 32.0, 32.0]])
    iz = np.concatenate([rng.uniform(0.0, 16.0, 2000), rng.integers(0, 17, 500).astype(np.float64), [0.0, 16.0, 16.0]])
    out["on_edges"] = (ix + 200.0, iy + 100.0, iz + 10.0)
    # all x and y equal but one
    cx, cy = np.full(400, 250.0), np.full(400, 75.0)
    cx[137], cy[137] = 256.5, 79.25
    out["column"] = (cx, cy, rng.uniform(5.0, 30.0, 400))
    return out


def cases():
    out = [dict(name="strip", cloud="strip", note="5000-point float64 strip of terrain, defaults", kwargs=dict(resolution=50))]
    for key, values in (("bottom_fill", (False,)), ("threshold", (2, 3)), ("ve", (0.5, 2.5)), ("pad", (1, 3))):
        for v in values:
            out.append(dict(name="strip_%s_%s" % (key, str(v).replace(".", "p")), cloud="strip", note="%s=%r" % (key, v),
                            kwargs={"resolution": 50, key: v}))
    out.append(dict(name="strip_mixed", cloud="strip", note="threshold 2, no fill, ve 2.5, pad 3 together",
                    kwargs=dict(resolution=33, bottom_fill=False, threshold=2, ve=2.5, pad=3)))
    out.append(dict(name="strip_f32", cloud="strip_f32", note="a float32 copy of the strip", kwargs=dict(resolution=50)))
    out.append(dict(name="strip_f32_ve", cloud="strip_f32", note="float32, ve 2.5, threshold 2, pad 1",
                    kwargs=dict(resolution=40, threshold=2, ve=2.5, pad=1)))
    out.append(dict(name="offset", cloud="offset", note="the cloud offset by %r" % (OFFSET,), kwargs=dict(resolution=50)))
    out.append(dict(name="tall_y", cloud="tall_y", note="max_y > max_x", kwargs=dict(resolution=50)))
    out.append(dict(name="on_edges", cloud="on_edges", note="integer extents, points on the last edge of every axis",
                    kwargs=dict(resolution=64)))
    out.append(dict(name="on_edges_coarse", cloud="on_edges", note="the same at resolution 16, threshold 3",
                    kwargs=dict(resolution=16, threshold=3)))
    out.append(dict(name="column", cloud="column", note="all x and y equal but one", kwargs=dict(resolution=20)))
    out.append(dict(name="resolution_1", cloud="strip", note="resolution 1", kwargs=dict(resolution=1)))
    out.append(dict(name="resolution_100", cloud="strip", note="resolution 100", kwargs=dict(resolution=100, ve=0.5)))
    return out


def main():
    warnings.simplefilter("ignore")
    ref = make_golden.import_reference()
    rec = {}
    for name, (x, y, z) in clouds().items():
        rec["x_" + name], rec["y_" + name], rec["z_" + name] = x, y, z
    listed = cases()
    for c in listed:
        x, y, z = clouds()[c["cloud"]]
        kw = dict(c["kwargs"])
        H = ref.voxelize(None, x.copy(), y.copy(), z.copy(), kw.pop("resolution"), **kw)
        assert H.dtype == bool and H.ndim == 3
        rec["bits_" + c["name"]] = np.packbits(H)
        rec["shape_" + c["name"]] = np.array(H.shape, dtype=np.int64)
        print("%-24s %-16s filled %d" % (c["name"], H.shape, int(H.sum())))
    sig = [dict(name=p.name, kind=p.kind.name, default=None if p.default is inspect.Parameter.empty else repr(p.default))
           for p in inspect.signature(ref.voxelize).parameters.values()]
    rec["cases"] = np.array(json.dumps(listed))
    rec["signature"] = np.array(json.dumps(sig))
    rec["numpy_version"] = np.array(np.__version__)
    out = os.path.join(HERE, "voxel.npz")
    np.savez_compressed(out, **rec)
    print("voxel.npz: %d cases, %.0f kB" % (len(listed), os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
