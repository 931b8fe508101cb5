#!/usr/bin/env python3
"""Time colortable_shade and raster_stats' median on device-resident rasters.

colortable_shade (16384^2 float32 by default): ms per call of the fused path (one statistics pass for min / max, one
launch that shades, indexes, gathers and writes three bytes) against the composition a user can write without it, in
the same process: ``neilpy_amd.hillshade``, torch ``amin`` / ``amax`` and index arithmetic, a torch gather from a device
table.  The traffic model is 4 B read (min / max) + 4 B read + 3 B written per cell; ``frac_of_stream`` is that
traffic's time at the streaming rate divided by the measured time.  ``--variant-lib`` names a side build of the library
(``python -m neilpy_amd.build --variant NAME --defs=-DSMRF_RELIEF_RGB3_LUT=1``) whose kernel gathers three bytes from a
3-byte-per-entry table instead of one packed word; it is timed through the C ABI beside the product's kernel.

raster_stats median (16384^2 float32, 8192^2 float64): ms per call, the passes over the raster (one for the moments,
three or six for the select) times its bytes against the streaming rate, and torch's ``nanmedian`` beside it for
orientation.

The streaming rate is the best grid-stride copy of ``tools/ubench/stream_rate`` (read + write bytes per second) when
that binary has been built (``--stream-bin``), else a torch device-to-device copy in this process.  Each case is warmed
up once, then timed over --reps calls between device events.  One JSON line per case; ``--md PATH`` also writes the
tables as Markdown.

    python tools/relief_bench.py [--n 16384] [--reps 5] [--md profiles/relief_bench_table.md]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_rate_from_binary(path):
    """best 'copy ... grid-stride' line of tools/ubench/stream_rate, in bytes per second (None if it cannot run)"""
    if not os.path.exists(path):
        return None
    r = subprocess.run([path], capture_output=True, text=True, timeout=300)
    rates = [float(m) for m in re.findall(r"^copy.*?(\d+) GB/s\s*$", r.stdout, re.M)]
    return max(rates) * 1e9 if r.returncode == 0 and rates else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    ap.add_argument("--stream-bin", default=os.path.join(ROOT, "tools", "ubench", "stream_rate"))
    ap.add_argument("--variant-lib", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import neilpy_amd as na
    from neilpy_amd import _lib
    from neilpy_amd.surface import _angle_row
    dev = torch.device("cuda:0")
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

    rate = stream_rate_from_binary(a.stream_bin)
    rate_from = "tools/ubench/stream_rate, best grid-stride copy"
    if rate is None:
        src = torch.empty(1 << 28, dtype=torch.float64, device=dev)
        dst = torch.empty_like(src)
        rate = 2 * src.numel() * 8 / (timed(lambda: dst.copy_(src)) * 1e-3)
        rate_from = "torch device-to-device copy of 2 GiB"
        del src, dst
    print(json.dumps(dict(stream_gb_per_s=round(rate / 1e9, 1), source=rate_from)), flush=True)

    def terrain(n, dtype):
        y = torch.arange(n, device=dev, dtype=torch.float64)[:, None]
        x = torch.arange(n, device=dev, dtype=torch.float64)[None, :]
        Z = (torch.sin(x / 37.0) * 9 + torch.cos(y / 53.0) * 7 + torch.sin((x + y) / 11.0) * 2) * 30 + 400
        return Z.to(dtype).contiguous()

    rows = []
    n = a.n
    cells = n * n
    Z = terrain(n, torch.float32)
    rng = np.random.default_rng(1)
    lut = torch.from_numpy(rng.integers(0, 256, size=(256, 256, 3), dtype=np.uint8)).to(dev)
    model_ms = cells * 11 / rate * 1e3

    def composition():
        H = na.hillshade(Z)
        zmin, zmax = Z.amin(), Z.amax()
        zi = torch.round(255 * (Z - zmin) / (zmax - zmin)).to(torch.int32)
        return lut.view(-1, 3)[zi * 256 + H.to(torch.int32)]

    fused = na.colortable_shade(Z, lut)
    agree = float((fused == composition()).all(dim=2).float().mean())       # torch's float32 division need not be NumPy's
    print(json.dumps(dict(composition_cells_equal_to_fused=agree)), flush=True)
    del fused
    ms_fused = timed(lambda: na.colortable_shade(Z, lut))
    ms_stats = timed(lambda: na.raster_stats(Z, ('min', 'max')))
    ms_comp = timed(composition)
    ms_hill = timed(lambda: na.hillshade(Z))
    rows.append(dict(case="colortable_shade, fused (statistics + one launch)", dtype="f32", n=n, ms=round(ms_fused, 3),
                     model_ms=round(model_ms, 3), frac_of_stream=round(model_ms / ms_fused, 3)))
    rows.append(dict(case="  of which raster_stats(min, max)", dtype="f32", n=n, ms=round(ms_stats, 3),
                     model_ms=round(cells * 4 / rate * 1e3, 3), frac_of_stream=round(cells * 4 / rate * 1e3 / ms_stats, 3)))
    rows.append(dict(case="hillshade + torch amin / amax / index / gather", dtype="f32", n=n, ms=round(ms_comp, 3),
                     ratio_to_fused=round(ms_comp / ms_fused, 2)))
    rows.append(dict(case="  of which hillshade", dtype="f32", n=n, ms=round(ms_hill, 3)))
    if a.variant_lib:
        packed = na.relief._packed_table(lut, dev)
        rgb = torch.empty((n, n, 3), dtype=torch.uint8, device=dev)
        angle = (C.c_double * 3)(*_angle_row(45, 315))
        zmin, zmax = float(Z.amin()), float(Z.amax())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for name, path, table in (("packed word per entry (product)", _lib.LIB_PATH, packed),
                                  ("3 bytes per entry, three gathers (variant)", a.variant_lib, lut.contiguous())):
            fn = C.CDLL(path).smrf_colortable_f32
            fn.restype, fn.argtypes = _lib.SIGNATURES["smrf_colortable_f32"]
            call = lambda: _lib.check(fn(Z.data_ptr(), n, n, zmin, zmax, 1.0, angle, table.data_ptr(),  # noqa: E731
                                         rgb.data_ptr(), stream))
            ms = timed(call)
            rows.append(dict(case="colortable kernel alone, " + name, dtype="f32", n=n, ms=round(ms, 3),
                             model_ms=round(cells * 7 / rate * 1e3, 3), frac_of_stream=round(cells * 7 / rate * 1e3 / ms, 3)))
        del rgb
    for r in rows:
        print(json.dumps(r), flush=True)
    del Z
    torch.cuda.empty_cache()

    med = []
    for dt, m, esz, passes in ((torch.float32, n, 4, 3), (torch.float64, n // 2, 8, 6)):
        X = terrain(m, dt)
        got = na.raster_stats(X, 'median')['median']
        want = torch.nanmedian(X) if (m * m) % 2 else None          # torch takes the lower middle value of an even count
        ms = timed(lambda: na.raster_stats(X, 'median'))
        ms_mom = timed(lambda: na.raster_stats(X, ('min', 'max')))
        ms_torch = timed(lambda: torch.nanmedian(X))
        model = (passes + 1) * m * m * esz / rate * 1e3
        row = dict(case="raster_stats median", dtype="f32" if esz == 4 else "f64", n=m, ms=round(ms, 3),
                   ms_moments_alone=round(ms_mom, 3), passes="1 + %d" % passes, model_ms=round(model, 3),
                   frac_of_stream=round(model / ms, 3), torch_nanmedian_ms=round(ms_torch, 3), median=float(got),
                   torch_agrees=None if want is None else bool(float(want) == float(got)))
        med.append(row)
        print(json.dumps(row), flush=True)
        del X
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("streaming rate: %.0f GB/s (%s; a read-only pass is priced at the same bytes per second)\n\n" %
                     (rate / 1e9, rate_from))
            fh.write("| case | dtype | n | ms | model ms | of streaming rate | composition / fused |\n|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %s | %s | %d | %.3f | %s | %s | %s |\n" % (
                    r["case"], r["dtype"], r["n"], r["ms"], r.get("model_ms", ""), r.get("frac_of_stream", ""),
                    r.get("ratio_to_fused", "")))
            fh.write("\n| case | dtype | n | ms | moments alone ms | passes | model ms | of streaming rate | "
                     "torch.nanmedian ms |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in med:
                fh.write("| %s | %s | %d | %.3f | %.3f | %s | %.3f | %.3f | %.3f |\n" % (
                    r["case"], r["dtype"], r["n"], r["ms"], r["ms_moments_alone"], r["passes"], r["model_ms"],
                    r["frac_of_stream"], r["torch_nanmedian_ms"]))


if __name__ == "__main__":
    main()
