#!/usr/bin/env python3
"""Time nearest_points on device-resident clouds of 10^6 and 10^7 points against SciPy's KD-tree on the same machine.

Clouds come from ``neilpy_amd.synth.synth_points`` at four points per square unit: ``points`` from one seed, ``query``
from another, once as it is and once moved by half a cell of the search grid along both planar axes (the grid's cell is
``sqrt(2 * area / n)``: about two points per cell).  Per case, one JSON line:

- ``call_ms``: one ``nearest_points(query, points)`` on CUDA tensors between device events, warmed up once, mean of
  ``--reps`` calls: both clouds' bounds reductions, the grid build and the search;
- ``build_ms`` / ``search_ms``: the same call's two parts timed on their own;
- ``ckdtree_build_s`` / ``ckdtree_query_s``: ``scipy.spatial.cKDTree(points)`` and ``.query(query, workers=16)`` by the
  host clock, once;
- ``max_abs_diff`` of the two distance arrays and the share of equal indices (SciPy forms the distance in another
  order and leaves ties to its traversal: not a bit check - tests/test_gpu_points.py is that).

The registers, LDS and scratch of every kernel of csrc/points.hip are read from the compiler
(``-Rpass-analysis=kernel-resource-usage``).  ``--md PATH`` also writes both tables as Markdown.

    python tools/points_bench.py [--sizes 1000000 10000000] [--reps 3] [--md profiles/points_bench_table.md]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENSITY = 4.0        # points per square unit


def kernel_resources():
    """[(kernel, VGPRs, SGPRs, LDS bytes, scratch bytes per lane, waves per SIMD)] of csrc/points.hip for gfx950"""
    from neilpy_amd.build import CSRC, FLAGS, hipcc
    with tempfile.TemporaryDirectory() as d:
        cmd = [hipcc()] + [f for f in FLAGS if f != "-fPIC"] + [
            "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "points.hip"),
            "-o", os.path.join(d, "points.s")]
        err = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    rows = []
    for block in err.split("Function Name: ")[1:]:
        def num(key):
            return int(re.search(re.escape(key) + r":?\s*(?:\[[^\]]*\]:\s*)?(\d+)", block).group(1))
        name = re.sub(r"^_ZN4smrf\d+", "", block.split()[0])
        m = re.match(r"((?:points|cloud)_\w+?_kernel)(?:\w*?ILi(\d)E)?", name)   # <dimension>: its own, or its loader's
        rows.append((m.group(1) + ("<%s>" % m.group(2) if m.group(2) else ""), num("VGPRs"), num("TotalSGPRs"),
                     num("LDS Size [bytes/block]"), num("ScratchSize [bytes/lane]"), num("Occupancy [waves/SIMD]")))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from scipy.spatial import cKDTree
    import neilpy_amd as na
    from neilpy_amd import points as pts
    res = kernel_resources()
    for r in res:
        print(json.dumps(dict(zip(("kernel", "vgprs", "sgprs", "lds_bytes", "scratch_bytes_per_lane", "waves_per_simd"), r))),
              flush=True)
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

    rows = []
    for n in a.sizes:
        extent = (n / DENSITY) ** 0.5 + 1.0
        P = np.column_stack(na.synth_points(n, extent, seed=20241))
        Q0 = np.column_stack(na.synth_points(n, extent, seed=20242))
        half = 0.5 * (2.0 * (extent - 1.0) ** 2 / n) ** 0.5
        t = time.perf_counter()
        tree = cKDTree(P)
        tree_s = time.perf_counter() - t
        Pd = torch.from_numpy(P).to(dev)
        for case, Q in (("as is", Q0), ("moved by half a cell", Q0 + np.array([half, half, 0.0]))):
            Qd = torch.from_numpy(Q).to(dev)
            call_ms = timed(lambda: na.nearest_points(Qd, Pd))
            cq, cp = pts._Cloud(Qd, "query"), pts._Cloud(Pd, "points")

            def build():
                cp.ws = None
                cp.build()
            build_ms = timed(build)
            search_ms = timed(lambda: cp.search(cq, True, True))
            dist, index = na.nearest_points(Qd, Pd)
            t = time.perf_counter()
            kd, ki = tree.query(Q, workers=a.workers)
            query_s = time.perf_counter() - t
            row = dict(case=case, n=n, dim=3, call_ms=round(call_ms, 3), build_ms=round(build_ms, 3),
                       search_ms=round(search_ms, 3), mqueries_per_s=round(n / call_ms / 1e3, 1),
                       ckdtree_build_s=round(tree_s, 3), ckdtree_query_s=round(query_s, 3), workers=a.workers,
                       query_speedup=round(query_s * 1e3 / call_ms, 1),
                       max_abs_diff=float(np.abs(dist.cpu().numpy() - kd).max()),
                       equal_index_share=float((index.cpu().numpy() == ki).mean()))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del Qd, cq, cp, dist, index
            torch.cuda.empty_cache()
        del Pd, tree
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("| case | points per cloud | call ms | build ms | search ms | Mqueries/s | cKDTree build s | "
                     "cKDTree query s (%d workers) | query s / call | max abs diff | equal indices |\n" % a.workers)
            fh.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %s | %d | %.3f | %.3f | %.3f | %.1f | %.3f | %.3f | %.1f | %.3g | %.6f |\n" % (
                    r["case"], r["n"], r["call_ms"], r["build_ms"], r["search_ms"], r["mqueries_per_s"],
                    r["ckdtree_build_s"], r["ckdtree_query_s"], r["query_speedup"], r["max_abs_diff"],
                    r["equal_index_share"]))
            fh.write("\n| kernel | VGPRs | SGPRs | LDS per workgroup | scratch per lane | waves per SIMD |\n|---|---|---|---|---|---|\n")
            for r in res:
                fh.write("| `%s` | %d | %d | %d B | %d B | %d |\n" % r)


if __name__ == "__main__":
    main()
