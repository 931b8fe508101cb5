#!/usr/bin/env python3
"""Time grey erosion by flat footprints on a device-resident raster: the runs and the taps path of csrc/footprint.hip,
and for disks the existing footprint-gather kernel of the disk filter.

Cases, at one raster of --n x --n float32 cells: ``disk(r)`` and ``square(2 r + 1)`` for r = 3, 10, 25, each through
``neilpy_amd.morphology.grey_erosion`` with ``impl`` forced to RUNS and to TAPS (a RUNS launch whose LDS planes pass
the cap is refused by the library and listed as such); for the disks also ``neilpy_amd.erosion(radius=r,
impl=IMPL_DIRECT)``, ``smrf_disk_filter_*``'s gather kernel, the one existing kernel that does comparable work.  Each
case is warmed up once, then timed over --reps calls between device events, so a figure is the time of a call on a
device tensor: the kernel plus the NaN count, the upload of the plan and the launch overhead (kernel times alone: run
with ``--reps 1`` under ``rocprofv3 --kernel-trace --stats`` in a run of its own and read the ``footprint_*_kernel``
rows).  Before anything is timed the three results of a case are compared: a figure for a wrong result is not printed.
One JSON line per case; ``--md PATH`` also writes the table as Markdown.

    python tools/footprint_bench.py [--n 4096] [--reps 3] [--md profiles/footprint_bench_table.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADII = (3, 10, 25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    import neilpy_amd as na
    from neilpy_amd import _lib, morphology as mo
    if not torch.cuda.is_available():
        raise SystemExit("footprint_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")

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

    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), n=a.n, reps=a.reps)), flush=True)
    gen = torch.Generator(device=dev).manual_seed(11)
    X = torch.rand((a.n, a.n), device=dev, generator=gen, dtype=torch.float32) * 50 + 100
    rows = []
    for r in RADII:
        for kind, fp in (("disk", na.disk(r)), ("square", mo.square(2 * r + 1))):
            P = mo.plan(fp, itemsize=4, impl=mo.IMPL_RUNS)
            row = dict(footprint="%s(%d)" % (kind, r if kind == "disk" else 2 * r + 1), members=len(P.offsets),
                       runs=len(P.runs), planes=P.nplanes, lds_bytes=P.lds_bytes)
            want = mo.grey_erosion(X, footprint=fp, impl=mo.IMPL_TAPS)
            row["taps_ms"] = round(timed(lambda: mo.grey_erosion(X, footprint=fp, impl=mo.IMPL_TAPS)), 3)
            if P.path == "runs":
                assert torch.equal(mo.grey_erosion(X, footprint=fp, impl=mo.IMPL_RUNS), want), row
                row["runs_ms"] = round(timed(lambda: mo.grey_erosion(X, footprint=fp, impl=mo.IMPL_RUNS)), 3)
            else:
                row["runs_ms"] = None                      # refused: the planes pass the LDS cap
            if kind == "disk":
                assert torch.equal(na.erosion(X, radius=r, impl=_lib.IMPL_DIRECT), want), row
                row["disk_direct_ms"] = round(timed(lambda: na.erosion(X, radius=r, impl=_lib.IMPL_DIRECT)), 3)
            else:
                row["disk_direct_ms"] = None
            row["auto"] = mo.plan(fp, itemsize=4).path
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.md:
        ms = lambda v: "refused (LDS cap)" if v is None else "%.3f" % v          # noqa: E731
        with open(a.md, "w") as fh:
            fh.write("| footprint | members | runs | LDS planes | LDS bytes | runs path, ms | taps path, ms | "
                     "disk filter DIRECT, ms | automatic path |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %s | %d | %d | %d | %d | %s | %.3f | %s | %s |\n" % (
                    r["footprint"], r["members"], r["runs"], r["planes"], r["lds_bytes"], ms(r["runs_ms"]), r["taps_ms"],
                    "-" if r["disk_direct_ms"] is None else "%.3f" % r["disk_direct_ms"], r["auto"]))


if __name__ == "__main__":
    main()
