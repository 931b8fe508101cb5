#!/usr/bin/env python3
"""Time scaled_morphometry and vip_score on a device-resident 16384^2 raster (float32 and float64).

Each case is warmed up once, then timed over --reps calls between device events.  One JSON line per case: ms per call,
Mcells/s, the byte model (one read of the raster plus one store per output plane) and that traffic's time at the rate
of a device-to-device copy measured in the same process (``frac_of_copy``: 1.0 = as fast as copying the same bytes).
Cases: all eight outputs at lookup_pixels 1, 8 and 64; ``outputs=('K',)`` alone; vip_score.

Two yardsticks run in the same process on the same raster, neither of them the code under test: ``evans_curvature``
(six outputs, the same pow / atan load per ratio; ``evans_x_8_6`` scales its time by 8 / 6 for the two extra planes) and
a plain torch composition of scaled_morphometry (slice-assigned shifts plus elementwise operations: what a user can
write today).  The static VALU count of each kernel is read from the generated gfx950 assembly.  ``--md PATH`` also
writes the table as Markdown.

    python tools/morphometry_bench.py [--n 16384] [--reps 3] [--md profiles/morphometry_bench_table.md]
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

LOOKUPS = (1, 8, 64)


def valu_counts():
    """{(kernel, dtype): VALU instructions}, a static count over the whole kernel (every branch included): an upper
    bound on the VALU per cell"""
    from neilpy_amd.build import CSRC, FLAGS, hipcc
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "morphometry.s")
        cmd = [hipcc()] + [f for f in FLAGS if f != "-fPIC"] + ["--offload-device-only", "-S",
                                                               os.path.join(CSRC, "morphometry.hip"), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True)
        text = open(out).read()
    parts = re.split(r"\n\s*\.type\s+_ZN4smrf\d+(\w+?)_kernelI([fd])E\S+,@function\n", text)
    res = {}
    for i in range(1, len(parts), 3):
        body = parts[i + 2].split(".Lfunc_end")[0]
        res[(parts[i], "f32" if parts[i + 1] == "f" else "f64")] = len(re.findall(r"^\s*v_", body, re.M))
    return res


def torch_shift(torch, X, dr, dc):
    """ashift by slice assignment: what the reference does, on a tensor"""
    out = X.clone()
    R, C = X.shape
    if abs(dr) >= R or abs(dc) >= C:
        return out
    out[max(-dr, 0):R - max(dr, 0), max(-dc, 0):C - max(dc, 0)] = \
        X[max(dr, 0):R - max(-dr, 0), max(dc, 0):C - max(-dc, 0)]
    return out


def torch_morphometry(torch, X, cellsize, n):
    """scaled_morphometry as a user composes it from torch operations today (yardstick only; not bit-checked)"""
    L = float(cellsize) * n
    z1, z2, z3 = torch_shift(torch, X, -n, -n), torch_shift(torch, X, -n, 0), torch_shift(torch, X, -n, n)
    z4, z6 = torch_shift(torch, X, 0, -n), torch_shift(torch, X, 0, n)
    z7, z8, z9 = torch_shift(torch, X, n, -n), torch_shift(torch, X, n, 0), torch_shift(torch, X, n, n)
    A = (z1 + z3 + z4 + z6 + z7 + z9) / (6 * L ** 2) - (z2 + X + z8) / (3 * L ** 2)
    B = (z1 + z2 + z3 + z7 + z8 + z9) / (6 * L ** 2) - (z4 + X + z6) / (3 * L ** 2)
    C = (z3 + z7 - z1 - z9) / (4 * L ** 2)
    D = (z3 + z6 + z9 - z1 - z4 - z7) / (6 * L)
    E = (z1 + z2 + z3 - z7 - z8 - z9) / (6 * L)
    del z1, z2, z3, z4, z6, z7, z8, z9
    DD, EE = D * D, E * E
    S2 = DD + EE
    cde = C * D * E
    SM = {}
    SM["A"] = torch.remainder(270 - torch.rad2deg(torch.atan2(E, D)), 360)
    SM["S"] = torch.rad2deg(torch.atan(torch.sqrt(S2)))
    SM["K"] = -2 * (A + B)
    SM["K_profile"] = -(A * DD + 2 * cde + B * EE) / (S2 * torch.pow(S2 + 1, 1.5))
    SM["K_cross"] = -2 * (B * DD + A * EE - cde) / S2
    SM["K_long"] = -2 * (A * DD + B * EE + cde) / S2
    SM["K_tan"] = -(A * EE - 2 * cde + B * DD) / (S2 * torch.sqrt(S2 + 1))
    SM["K_plan"] = -(A * EE - 2 * cde + B * DD) / torch.pow(S2, 1.5)
    return SM


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    import neilpy_amd as na
    valu = valu_counts()
    dev = torch.device("cuda:0")
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

    def report(case, dt, ms, in_b, out_b, kernel=None):
        copy_equiv_ms = n * n * (in_b + out_b) / copy_rate * 1e3
        row = dict(case=case, dtype=dt, n=n, ms=round(ms, 3), mcells_per_s=round(n * n / ms / 1e3, 1),
                   bytes_per_cell="%d in + %d out" % (in_b, out_b), frac_of_copy=round(copy_equiv_ms / ms, 3),
                   valu_static=valu.get((kernel, dt)) if kernel else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
        return ms

    for dt in ("f32", "f64"):
        y = torch.arange(n, device=dev, dtype=torch.float64)[:, None]
        x = torch.arange(n, device=dev, dtype=torch.float64)[None, :]
        Z = (torch.sin(x / 37.0) * 9 + torch.cos(y / 53.0) * 7 + torch.sin((x + y) / 11.0) * 2)
        Z = Z.to(torch.float32 if dt == "f32" else torch.float64).contiguous()
        del x, y
        esz = 4 if dt == "f32" else 8
        for k in LOOKUPS:
            report("scaled_morphometry lookup_pixels=%d, 8 outputs" % k, dt,
                   timed(lambda: na.scaled_morphometry(Z, 2.0, k)), esz, 8 * esz, "morphometry")
        for k in (1, 64):
            report("scaled_morphometry lookup_pixels=%d, outputs=('K',)" % k, dt,
                   timed(lambda: na.scaled_morphometry(Z, 2.0, k, outputs=("K",))), esz, esz, "morphometry")
        report("vip_score", dt, timed(lambda: na.vip_score(Z, 2.0)), esz, 8, "vip")
        ms = report("yardstick: evans_curvature, 6 outputs", dt, timed(lambda: na.evans_curvature(Z, 2.0)), esz, 6 * esz)
        rows.append(dict(case="yardstick: evans_curvature x 8/6", dtype=dt, n=n, ms=round(ms * 8 / 6, 3)))
        print(json.dumps(rows[-1]), flush=True)
        for k in (1, 64):
            report("yardstick: torch composition lookup_pixels=%d, 8 outputs" % k, dt,
                   timed(lambda: torch_morphometry(torch, Z, 2.0, k)), esz, 8 * esz)
        del Z
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("copy rate: %.1f GB/s (read + write)\n\n" % (copy_rate / 1e9))
            fh.write("| case | dtype | ms | Mcells/s | bytes per cell | of copy rate | static VALU |\n|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %s | %s | %.3f | %s | %s | %s | %s |\n" % (
                    r["case"], r["dtype"], r["ms"], r.get("mcells_per_s", ""), r.get("bytes_per_cell", ""),
                    r.get("frac_of_copy", ""), r.get("valu_static") or ""))


if __name__ == "__main__":
    main()
