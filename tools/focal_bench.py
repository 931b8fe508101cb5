#!/usr/bin/env python3
"""Time the focal tap kernels on device-resident rasters and relate them to their issue bound.

Cases: ``focal_convolve`` (one accumulated plane), ``std`` (two planes) and ``topographic_position_index`` (two planes
plus the reductions) with ``disk(radius)`` weights, a few raster sizes, radii and both dtypes; the largest radius lies
past the tile cap and takes the direct path.  Each case is warmed up once, then timed over --reps calls of the public
function between device events, so a figure is the time of a call on a device tensor: the kernel plus the upload of
the tap table and the launch overhead (kernel times alone: run with ``--reps 1`` under ``rocprofv3 --kernel-trace
--stats`` in a run of its own and read the ``focal_kernel`` rows).

Bound: per cell, tap and accumulated plane one fp64 multiply and one fp64 add, which the parity
contract keeps apart (no FMA).  The MI355X's vector fp64 peak of 78.6 TFLOP/s counts an FMA as two operations, i.e.
39.3e12 fp64 instructions x lanes per second; ``frac_of_bound`` = cells x taps x planes x 2 / 39.3e12 over the measured
time.  One JSON line per case; ``--md PATH`` also writes the table as Markdown.

    python tools/focal_bench.py [--reps 3] [--md profiles/focal_bench_table.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_LANE_OPS_PER_S = 78.6e12 / 2

CASES = [  # (function, n, dtype, radius)
    ("focal_convolve", 4096, "f32", 3), ("focal_convolve", 4096, "f32", 10), ("focal_convolve", 4096, "f32", 25),
    ("std", 4096, "f32", 3), ("std", 4096, "f32", 10), ("std", 4096, "f32", 25), ("std", 4096, "f32", 42),
    ("std", 4096, "f64", 3), ("std", 4096, "f64", 10), ("std", 4096, "f64", 25), ("std", 4096, "f64", 26),
    ("focal_convolve", 8192, "f32", 10), ("std", 8192, "f32", 10), ("std", 8192, "f64", 10),
    ("topographic_position_index", 8192, "f32", 10), ("topographic_position_index", 8192, "f64", 10),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import neilpy_amd as na
    from neilpy_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("focal_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def timed(f):
        f()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            f()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.reps

    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), reps=a.reps)), flush=True)
    rows = []
    rasters = {}
    for fn, n, dt, radius in CASES:
        if (n, dt) not in rasters:
            rasters.clear()
            torch.cuda.empty_cache()
            gen = torch.Generator(device=dev).manual_seed(11)
            rasters[(n, dt)] = torch.rand((n, n), device=dev, generator=gen,
                                          dtype=torch.float32 if dt == "f32" else torch.float64) * 50 + 100
        X = rasters[(n, dt)]
        strel = na.disk(radius)
        if fn == "topographic_position_index":
            taps, planes = int(strel.sum()) - 1, 2
            call = lambda: na.topographic_position_index(X, radius)  # noqa: E731
        elif fn == "std":
            taps, planes = int(strel.sum()), 2
            call = lambda: na.std(X, strel)  # noqa: E731
        else:
            taps, planes = int(strel.sum()), 1
            w = strel / np.sum(strel)
            call = lambda: na.focal_convolve(X, w)  # noqa: E731
        ms = timed(call)
        tiled = bool(lib.smrf_focal_fits_tile(2 * radius + 1, 2 * radius + 1, 4 if dt == "f32" else 8))
        cell_taps = float(n) * n * taps
        row = dict(fn=fn, n=n, dtype=dt, radius=radius, taps=taps, planes=planes, path="tiled" if tiled else "direct",
                   ms=round(ms, 3), cell_taps_per_s=float("%.4g" % (cell_taps / (ms * 1e-3))),
                   frac_of_bound=round(cell_taps * planes * 2 / FP64_LANE_OPS_PER_S / (ms * 1e-3), 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("| function | raster | dtype | radius | taps | planes | path | ms per call | cell x taps / s | "
                     "of the issue bound |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %s | %d^2 | %s | %d | %d | %d | %s | %.3f | %.3g | %.3f |\n" % (
                    r["fn"], r["n"], r["dtype"], r["radius"], r["taps"], r["planes"], r["path"], r["ms"],
                    r["cell_taps_per_s"], r["frac_of_bound"]))


if __name__ == "__main__":
    main()
