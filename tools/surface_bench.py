#!/usr/bin/env python3
"""Time every surface-derivative function on a device-resident 16384^2 raster (float32 and float64).

Each case is warmed up once, then timed over --reps calls between device events.  One JSON line per case: ms per call,
Mcells/s, bytes moved per cell (raster in + every output), and that traffic's time at the rate of a device-to-device
copy measured in the same process (``frac_of_copy``: 1.0 = as fast as copying the same bytes).  For every mode the
VALU instructions of the kernel (a static count, an upper bound per cell) are read from the generated gfx950 assembly, with the VALU issue
bound they imply (CUs x 4 SIMDs x 16 lanes x 2.4 GHz; fp64 transcendentals run at a lower rate, so the real VALU bound is
higher for them).  ``--md PATH`` also writes the table as Markdown.

    python tools/surface_bench.py [--n 16384] [--reps 3] [--md profiles/surface_bench_table.md]
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
MODE = {"slope": 0, "aspect": 1, "hillshade": 2, "multiple_illumination": 2, "esri_slope": 3, "curvature": 4,
        "esri_curvature": 5, "zevenbergen_and_thorne_curvature": 6, "evans_curvature": 7,
        "wilson_gallant_curvature": 8}
N_OUT = {"esri_curvature": 3, "zevenbergen_and_thorne_curvature": 6, "evans_curvature": 6,
         "wilson_gallant_curvature": 4}
CASES = [("slope", dict(return_as="percent")), ("slope", {}), ("aspect", {}), ("hillshade", {}),
         ("hillshade", dict(return_uint8=False)), ("multiple_illumination", {}), ("esri_slope", dict(return_as="percent")),
         ("esri_slope", {}), ("curvature", {}), ("esri_curvature", {}), ("zevenbergen_and_thorne_curvature", {}),
         ("evans_curvature", {}), ("wilson_gallant_curvature", {})]


def loop_costs():
    """{(dtype, mode): VALU instructions of surface_kernel<T, MODE>}, a static count over the whole kernel: every branch
    and the strip's prologue (run once per 32 cells) are included, so it is an upper bound on the VALU per cell"""
    from neilpy_amd.build import CSRC, FLAGS, hipcc
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "surface.s")
        cmd = [hipcc()] + [f for f in FLAGS if f != "-fPIC"] + ["--offload-device-only", "-S",
                                                               os.path.join(CSRC, "surface.hip"), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True)
        text = open(out).read()
    parts = re.split(r"\n\s*\.type\s+(_ZN4smrf14surface_kernelI([fd])Li(\d)E\S+),@function\n", text)
    res = {}
    for i in range(1, len(parts), 4):
        body = parts[i + 3].split(".Lfunc_end")[0]
        res[("f32" if parts[i + 1] == "f" else "f64", int(parts[i + 2]))] = len(re.findall(r"^\s*v_", body, re.M))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    import neilpy_amd as na
    costs = loop_costs()
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rate = cus * 4 * 16 * CLOCK_HZ
    n = a.n
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def timed(f):
        f()
        torch.cuda.synchronize()
        t0, t1 = ev(), ev()
        t0.record()
        for _ in range(a.reps):
            f()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.reps

    # device-to-device copy rate (read + write bytes per second) on a 2 GiB buffer
    src = torch.empty(1 << 28, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src))
    copy_rate = 2 * src.numel() * 8 / (copy_ms * 1e-3)
    del src, dst
    print(json.dumps(dict(copy_gb_per_s=round(copy_rate / 1e9, 1))), flush=True)
    rows = []
    for dt in ("f32", "f64"):
        y = torch.arange(n, device=dev, dtype=torch.float64)[:, None]
        x = torch.arange(n, device=dev, dtype=torch.float64)[None, :]
        Z = (torch.sin(x / 37.0) * 9 + torch.cos(y / 53.0) * 7 + torch.sin((x + y) / 11.0) * 2)
        Z = Z.to(torch.float32 if dt == "f32" else torch.float64).contiguous()
        del x, y
        esz = 4 if dt == "f32" else 8
        for fn, kw in CASES:
            f = getattr(na, fn)
            ms = timed(lambda: f(Z, **kw))
            if fn == "multiple_illumination" or (fn == "hillshade" and kw.get("return_uint8", True)):
                out_b = 1
            elif fn == "hillshade":
                out_b = 8
            else:
                out_b = esz * N_OUT.get(fn, 1)
            bpc = esz + out_b
            copy_equiv_ms = n * n * bpc / copy_rate * 1e3
            valu = costs.get((dt, MODE[fn]))
            valu_ms = None if valu is None else n * n * valu / rate * 1e3
            row = dict(fn=fn, **kw, dtype=dt, n=n, ms=round(ms, 3), mcells_per_s=round(n * n / ms / 1e3, 1),
                       bytes_per_cell="%d in + %d out" % (esz, out_b), frac_of_copy=round(copy_equiv_ms / ms, 3),
                       valu_per_cell=valu, valu_bound_ms=None if valu_ms is None else round(valu_ms, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        del Z
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("copy rate: %.1f GB/s (read + write)\n\n" % (copy_rate / 1e9))
            fh.write("| function | options | dtype | ms | Mcells/s | bytes per cell | of copy rate | VALU per cell | "
                     "VALU bound ms |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                opts = ", ".join("%s=%s" % (k, r[k]) for k in ("return_as", "return_uint8") if k in r) or "defaults"
                fh.write("| %s | %s | %s | %.3f | %.0f | %s | %.2f | %s | %s |\n" % (
                    r["fn"], opts, r["dtype"], r["ms"], r["mcells_per_s"], r["bytes_per_cell"], r["frac_of_copy"],
                    r["valu_per_cell"], r["valu_bound_ms"]))


if __name__ == "__main__":
    main()
