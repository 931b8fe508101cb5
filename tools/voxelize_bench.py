#!/usr/bin/env python3
"""Time voxelize on device-resident float64 clouds.

Cases: ``synth_points`` clouds of 10**6 points over 1024 m and 2 x 10**7 points over 2048 m, each at resolution 256 and
1024 and threshold 1 (the bit set) and 2 (the counts).  Per case, between device events after one warm-up:

  call     ``neilpy_amd.voxelize`` on CUDA tensors: bounds reduction and its synchronisation, the host's edges and their
           upload, the allocation of workspace and result, mark, expand
  mark     ``smrf_voxel_mark_f64`` alone: clearing the marks and the scatter
  expand   ``smrf_voxel_expand`` alone: the column minima and the byte expansion
  torch    a plain torch composition on the same device, as a sanity baseline: ``torch.bucketize`` per axis against the
           same edges, ``bincount`` of the flat index, the compare, ``cummax`` from the top for the fill

``of_copy``: the byte model of DESIGN.md section 15 (3 x 8 B read per point, nz + pad B written per column, the
workspace cleared, marked - counted as one write - and read once) at the rate of a device-to-device copy measured in the
same process, over mark + expand.  One JSON line per case; ``--md PATH`` also writes the table as Markdown.

    python tools/voxelize_bench.py [--reps 5] [--md profiles/voxelize_bench.md]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLOUDS = ((10 ** 6, 1024.0), (2 * 10 ** 7, 2048.0))
RESOLUTIONS = (256, 1024)
THRESHOLDS = (1, 2)


def torch_voxelize(torch, x, y, z, mins, edges, threshold):
    """the same volume from stock torch operators (same edges, same rule at the last edge, bottom fill on, no pad)"""
    idx, keep = [], None
    for v, m, e in zip((x, y, z), mins, edges):
        d = v - m
        i = torch.bucketize(d, e, right=True) - 1
        i = torch.where(d == e[-1], i - 1, i)
        ok = (i >= 0) & (i < e.numel() - 1)
        keep = ok if keep is None else keep & ok
        idx.append(i)
    nx, ny, nz = (e.numel() - 1 for e in edges)
    flat = ((idx[0] * ny + idx[1]) * nz + idx[2])[keep]
    H = (torch.bincount(flat, minlength=nx * ny * nz) >= threshold).view(nx, ny, nz)
    above = torch.cummax(H.flip(2).to(torch.uint8), dim=2).values.flip(2).bool()       # a voxel at or above this level
    below = torch.cummax(H.to(torch.uint8), dim=2).values.bool()                        # a voxel at or below this level
    return H | (above & ~below)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    ap.add_argument("--small", action="store_true", help="10**5 and 10**6 points: a quick look, not the table")
    a = ap.parse_args()
    import torch
    import neilpy_amd as na
    from neilpy_amd import _lib, voxel
    from neilpy_amd._raster import _ptr, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def timed(f, reps=a.reps):
        f()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            f()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    src = torch.empty(1 << 27, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    copy_rate = 2 * src.numel() * 8 / (timed(lambda: dst.copy_(src)) * 1e-3)
    del src, dst
    print(json.dumps(dict(copy_gb_per_s=round(copy_rate / 1e9, 1), device=torch.cuda.get_device_name(dev))), flush=True)

    rows = []
    clouds = ((10 ** 5, 512.0), (10 ** 6, 1024.0)) if a.small else CLOUDS
    for npts, extent in clouds:
        x, y, z = (torch.from_numpy(v).to(dev) for v in na.synth_points(npts, extent))
        for resolution in RESOLUTIONS:
            H, edges, mins = na.voxelize(None, x, y, z, resolution, return_edges=True)
            nx, ny, nz = H.shape
            d_edges = [torch.from_numpy(e).to(dev) for e in edges]
            offsets = (C.c_double * 3)(*[float(m) for m in mins])
            for threshold in THRESHOLDS:
                H = na.voxelize(None, x, y, z, resolution, threshold=threshold)
                call_ms = timed(lambda: na.voxelize(None, x, y, z, resolution, threshold=threshold))
                nbytes = lib.smrf_voxel_workspace_bytes(nx, ny, nz, threshold)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                out = torch.empty((nx, ny, nz), dtype=torch.bool, device=dev)
                mark_ms = timed(lambda: _lib.check(lib.smrf_voxel_mark_f64(
                    _ptr(x), _ptr(y), _ptr(z), npts, offsets, _ptr(d_edges[0]), _ptr(d_edges[1]), _ptr(d_edges[2]), nx, ny, nz,
                    threshold, _ptr(ws), nbytes, _stream())))
                expand_ms = timed(lambda: _lib.check(lib.smrf_voxel_expand(_ptr(ws), nbytes, nx, ny, nz, threshold, 1, 0,
                                                                           _ptr(out), _stream())))
                assert torch.equal(out, H)
                del ws, out
                m64 = [torch.tensor(float(m), dtype=torch.float64, device=dev) for m in mins]
                ref = torch_voxelize(torch, x, y, z, m64, d_edges, threshold)
                same = bool(torch.equal(ref, H))
                del ref
                torch_ms = timed(lambda: torch_voxelize(torch, x, y, z, m64, d_edges, threshold), reps=2)
                torch.cuda.empty_cache()
                marks = nx * ny * ((nz + 31) // 32 * 4 if threshold == 1 else nz * 4)
                model = 3 * 8 * npts + nx * ny * nz + 3 * marks + 2 * 4 * nx * ny
                row = dict(points=npts, resolution=resolution, threshold=threshold, shape=[nx, ny, nz],
                           filled=round(float(H.float().mean()), 4), call_ms=round(call_ms, 3), mark_ms=round(mark_ms, 3),
                           expand_ms=round(expand_ms, 3), torch_ms=round(torch_ms, 2), torch_equal=same,
                           model_mb=round(model / 1e6, 1),
                           of_copy=round(model / copy_rate * 1e3 / (mark_ms + expand_ms), 3))
                rows.append(row)
                print(json.dumps(row), flush=True)
                del H
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("copy rate: %.1f GB/s (read + write)\n\n" % (copy_rate / 1e9))
            fh.write("| points | resolution | threshold | volume | filled | call ms | mark ms | expand ms | torch ms | "
                     "equals torch | model MB | of copy rate |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %d | %d | %d | %d x %d x %d | %.4f | %.3f | %.3f | %.3f | %.2f | %s | %.1f | %.3f |\n" % (
                    r["points"], r["resolution"], r["threshold"], *r["shape"], r["filled"], r["call_ms"], r["mark_ms"],
                    r["expand_ms"], r["torch_ms"], "yes" if r["torch_equal"] else "NO", r["model_mb"], r["of_copy"]))


if __name__ == "__main__":
    main()
