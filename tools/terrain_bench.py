#!/usr/bin/env python3
"""Time geomorphons() and openness() on a device-resident 16384^2 raster (float32 and float64).

Cases: L in {1, 5, 20, 50} for both functions, geomorphons(enhance=True) at L = 20, fast=True at L = 50.  Each case
is warmed up once, then timed over --reps calls with device events.  One JSON line per case: ms per call, Mcells/s,
and the fraction of the VALU issue bound.  The bound is the march's VALU lane-instructions - samples (8 directions
x steps x cells) times the instructions per sample of the kernel's inner loop, read from the generated gfx950
assembly (LDS loop for steps within the halo cap, global loop beyond) - over the device's issue rate (CUs x 4 SIMDs
x 16 lanes x 2.4 GHz).  Rate-limited instructions (v_rcp_f64, the f64 divide steps) make the real bound higher, so
the fraction is a lower bound on how close the kernel is to its VALU limit.

    python tools/terrain_bench.py [--n 16384] [--reps 3] [--only geomorphons]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLOCK_HZ = 2.4e9


def loop_costs():
    """{(dtype, mode): (VALU per sample in the LDS loop, VALU per sample in the global loop)} of the tiled kernels"""
    from neilpy_amd.build import CSRC, FLAGS, hipcc
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "terrain.s")
        cmd = [hipcc()] + [f for f in FLAGS if f != "-fPIC"] + ["--offload-device-only", "-S",
                                                               os.path.join(CSRC, "terrain.hip"), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True)
        text = open(out).read()
    res = {}
    for m in re.finditer(r"^(_ZN\w*rays_kernelI([fd])Li(\d)ELb1\w*):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M):
        body = m.group(4)
        lds = glob = None
        for lab, blk in re.findall(r"^(\.LBB\d+_\d+):[^\n]*Inner Loop Header[^\n]*\n(.*?)\n\s*s_cbranch_\w+ \1\b",
                                   body, re.S | re.M):
            n = blk.count("v_div_fixup_f64")
            if not n:
                continue
            valu = len(re.findall(r"^\s*v_", blk, re.M)) / n
            # the cheapest loop of each kind is the main march (the enhance prefix also keeps its own extremes)
            if "ds_read" in blk:
                lds = valu if lds is None else min(lds, valu)
            elif "global_load" in blk:
                glob = valu if glob is None else min(glob, valu)
        res[("f32" if m.group(2) == "f" else "f64", int(m.group(3)))] = (lds, glob)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import torch
    import neilpy_amd as na
    from neilpy_amd import _lib
    from neilpy_amd.terrain import _as_steps
    costs = loop_costs()
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rate = cus * 4 * 16 * CLOCK_HZ
    cases = []
    for fn in ("geomorphons", "openness"):
        for L in (1, 5, 20, 50):
            cases.append((fn, L, {}))
    cases += [("geomorphons", 20, dict(enhance=True)), ("geomorphons", 50, dict(fast=True)),
              ("openness", 50, dict(fast=True))]
    for dt in ("f32", "f64"):
        n = a.n
        y = torch.arange(n, device=dev, dtype=torch.float64)[:, None]
        x = torch.arange(n, device=dev, dtype=torch.float64)[None, :]
        Z = (torch.sin(x / 37.0) * 9 + torch.cos(y / 53.0) * 7 + torch.sin((x + y) / 11.0) * 2)
        Z = Z.to(torch.float32 if dt == "f32" else torch.float64).contiguous()
        del x, y
        cap = _lib.TERRAIN_HALO_CAP[dt]
        for fn, L, kw in cases:
            if a.only and fn != a.only:
                continue
            f = getattr(na, fn)
            args = dict(lookup_pixels=L, **kw)
            if fn == "geomorphons":
                args["threshold_angle"] = 1
            f(Z, **args)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                f(Z, **args)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.reps
            steps = [int(k) for k in _as_steps(L, kw.get("fast", False))]
            if kw.get("enhance") and L > 16:
                steps = sorted(set(steps) | set(range(1, max(L // 4, 4) + 1)))
            mode = _lib.TERRAIN_COUNT if fn == "geomorphons" else _lib.TERRAIN_OPENNESS
            lds, glob = costs.get((dt, mode), (None, None))
            n_lds = sum(1 for k in steps if k <= cap)
            samples = 8.0 * n * n * len(steps)
            bound_ms = None
            if lds is not None and glob is not None:
                bound_ms = 8.0 * n * n * (n_lds * lds + (len(steps) - n_lds) * glob) / rate * 1e3
            print(json.dumps(dict(fn=fn, dtype=dt, n=n, L=L, **kw, steps=len(steps), ms=round(ms, 3),
                                  mcells_per_s=round(n * n / ms / 1e3, 1), gsamples_per_s=round(samples / ms / 1e6, 1),
                                  valu_per_sample_lds=lds, valu_per_sample_global=glob,
                                  valu_bound_ms=None if bound_ms is None else round(bound_ms, 3),
                                  frac_of_valu_bound=None if bound_ms is None else round(bound_ms / ms, 3))),
                  flush=True)
        del Z
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
