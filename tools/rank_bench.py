#!/usr/bin/env python3
"""Time the rank filters of csrc/rank.hip on a device-resident raster: where COUNT stops beating BISECT, and medians of
larger footprints beside the grey erosion that visits the same samples once.

Crossover (``smrf_rank_count_max_taps``): ``median_filter`` of all-ones squares of 3^2 .. 19^2 members with ``impl``
forced to COUNT and to BISECT, on an --n x --n raster of float32 and of float64, terrain (``synth_dem``) and noise
(``rand * 50 + 100``) both, since BISECT's prefix skip depends on the data.  The two are timed in one process,
interleaved: after one warm-up call each, --reps rounds of one COUNT call then one BISECT call, each call between its
own pair of device events.  A figure is the median over the rounds of the time of a call on a device tensor: the kernel
plus the NaN count of the raster, the upload of the plan and the launch overhead, the same for both methods; the spread
(min .. max over the rounds) is printed beside it.  Before a pair is timed its results are compared with ``torch.equal``.

Context: medians of ``disk(3)``, ``square(7)``, ``disk(10)``, ``square(21)`` and ``square(51)`` on the float32 terrain
raster under the automatic choice, timed the same way, beside ``grey_erosion(impl=TAPS)`` of the same footprint (one
compare per sample: the floor for one pass over the samples).

``--scipy M`` needs no GPU: ``scipy.ndimage.median_filter`` of the same footprints on the top-left M x M cells of the
terrain raster on one host core, one call each, as seconds and as the same rate over --n x --n cells.

One JSON line per case; ``--md PATH`` also writes the tables as Markdown.

    python tools/rank_bench.py [--n 4096] [--reps 5] [--md profiles/rank_bench_table.md]
    python tools/rank_bench.py --scipy 1024
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = (3, 5, 7, 9, 11, 13, 15, 17, 19)


def context_footprints():
    import neilpy_amd as na
    from neilpy_amd import morphology as mo
    return (("disk(3)", na.disk(3)), ("square(7)", mo.square(7)), ("disk(10)", na.disk(10)), ("square(21)", mo.square(21)),
            ("square(51)", mo.square(51)))


def scipy_times(a):
    import scipy.ndimage as ndi
    from neilpy_amd.synth import synth_dem
    X = np.ascontiguousarray(synth_dem(a.n)[:a.scipy, :a.scipy])
    for tag, fp in context_footprints():
        t = time.perf_counter()
        ndi.median_filter(X, footprint=fp)
        s = time.perf_counter() - t
        print(json.dumps(dict(footprint=tag, members=int(fp.sum()), cells=X.size, scipy_s=round(s, 3),
                              scipy_s_at_n=round(s * a.n * a.n / X.size, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    ap.add_argument("--scipy", type=int, default=0)
    a = ap.parse_args()
    if a.scipy:
        return scipy_times(a)
    import torch
    from neilpy_amd import morphology as mo, rank as rk
    from neilpy_amd.synth import synth_dem
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")

    def once(f):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def interleaved(fs):
        """per callable the times of --reps rounds, one call of each per round after one warm-up call of each"""
        for f in fs:
            f()
        torch.cuda.synchronize()
        ts = [[] for _ in fs]
        for _ in range(a.reps):
            for k, f in enumerate(fs):
                ts[k].append(once(f))
        return [dict(ms=round(float(np.median(t)), 3), lo=round(min(t), 3), hi=round(max(t), 3)) for t in ts]

    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), n=a.n, reps=a.reps)), flush=True)
    dem = synth_dem(a.n)
    gen = torch.Generator(device=dev).manual_seed(11)
    cross, context = [], []
    for dtype in (torch.float32, torch.float64):
        rasters = (("terrain", torch.from_numpy(dem).to(dev).to(dtype)),
                   ("noise", (torch.rand((a.n, a.n), device=dev, generator=gen, dtype=torch.float32) * 50 + 100).to(dtype)))
        for data, X in rasters:
            for w in WIDTHS:
                fp = mo.square(w)
                count = lambda: rk.median_filter(X, footprint=fp, impl=rk.IMPL_COUNT)          # noqa: E731
                bisect = lambda: rk.median_filter(X, footprint=fp, impl=rk.IMPL_BISECT)        # noqa: E731
                assert torch.equal(count(), bisect()), (dtype, data, w)
                c, b = interleaved((count, bisect))
                row = dict(dtype=str(dtype).split(".")[1], data=data, members=w * w, count=c, bisect=b)
                cross.append(row)
                print(json.dumps(row), flush=True)
    X = torch.from_numpy(dem).to(dev)
    for tag, fp in context_footprints():
        median = lambda: rk.median_filter(X, footprint=fp)                                     # noqa: E731
        floor = lambda: mo.grey_erosion(X, footprint=fp, impl=mo.IMPL_TAPS)                    # noqa: E731
        m, e = interleaved((median, floor))
        P = mo.plan(fp, itemsize=4)
        path = rk._library().smrf_rank_path(P.head.ctypes.data, 4, rk.IMPL_AUTO)
        row = dict(footprint=tag, members=len(P.offsets), median=m, erosion_taps=e,
                   path=("BISECT" if path & rk.PATH_BISECT else "COUNT") + " / " + ("GLOBAL" if path & rk.PATH_GLOBAL else "TILE"))
        context.append(row)
        print(json.dumps(row), flush=True)
    if a.md:
        cell = lambda d: "%.3f (%.3f .. %.3f)" % (d["ms"], d["lo"], d["hi"])                    # noqa: E731
        with open(a.md, "w") as fh:
            fh.write("| dtype | raster | members | COUNT, ms | BISECT, ms | faster |\n|---|---|---|---|---|---|\n")
            for r in cross:
                fh.write("| %s | %s | %d | %s | %s | %s |\n" % (r["dtype"], r["data"], r["members"], cell(r["count"]), cell(r["bisect"]),
                                                             "COUNT" if r["count"]["ms"] <= r["bisect"]["ms"] else "BISECT"))
            fh.write("\n| footprint | members | path | median, ms | grey_erosion TAPS, ms |\n|---|---|---|---|---|\n")
            for r in context:
                fh.write("| %s | %d | %s | %s | %s |\n" % (r["footprint"], r["members"], r["path"], cell(r["median"]),
                                                         cell(r["erosion_taps"])))


if __name__ == "__main__":
    main()
