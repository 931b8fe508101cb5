#!/usr/bin/env python3
"""Time the nearest-source infill on device-resident float32 rasters.

Cases: 16384^2 with 5 % scattered holes, 16384^2 with one 4000-cell block, and 4096^2 scattered against 4096^2 with a
single source (the ratio of the two is the guard on the work bound: it must stay a small factor).  Each case is warmed
up once, then timed over --reps in-place fills of a fresh clone between device events (the clone is timed on its own and
subtracted).  Milliseconds per pass are kernel times: run this tool with ``--reps 1`` under
``rocprofv3 --kernel-trace --stats`` in a run of its own and read the four ``nearest_*_kernel`` rows.  Bytes per cell are
the model of DESIGN.md section 11, computed here from the shapes and the envelope sizes the run left in its workspace.  ``frac_of_copy``: the model's
bytes at the rate of a device-to-device copy measured in the same process, over the measured time.  One JSON line per
case; ``--md PATH`` also writes the table as Markdown.

    python tools/nearest_bench.py [--n 16384] [--reps 3] [--md profiles/nearest_bench_table.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_bytes_per_cell(rows, cols, esz, hole_share, envelope_share):
    """DESIGN.md section 11, Bound: pass 1 reads the raster and writes 1 bit per cell plus two carries per 32 cells
    (and reads the words again for them); pass 2's scan reads the words and carries of its tile and writes 12 B per
    envelope entry; the lookup reads the raster, and per hole a 12 B entry and the source's value, and writes the hole"""
    pass1 = esz + 4 / 32 + (4 + 8) / 32
    scan = (4 + 4 + 4) / 32 + 12 * envelope_share
    lookup = esz + hole_share * (12 + 2 * esz)
    return pass1, scan, lookup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    import neilpy_amd as na
    from neilpy_amd import nearest as nr
    dev = torch.device("cuda:0")
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

    def timed(f, reps=a.reps):
        f()
        torch.cuda.synchronize()
        t0, t1 = ev(), ev()
        t0.record()
        for _ in range(reps):
            f()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    src = torch.empty(1 << 28, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src))
    copy_rate = 2 * src.numel() * 8 / (copy_ms * 1e-3)
    del src, dst
    try:
        clock = torch.cuda.clock_rate()
    except Exception:                                   # no SMI binding in this environment
        clock = None
    print(json.dumps(dict(copy_gb_per_s=round(copy_rate / 1e9, 1), device=torch.cuda.get_device_name(dev),
                          sm_clock_mhz=clock)), flush=True)

    def raster(n, kind):
        gen = torch.Generator(device=dev).manual_seed(11)
        X = torch.rand((n, n), device=dev, generator=gen, dtype=torch.float32) * 50 + 100
        if kind == "scattered":
            X[torch.rand((n, n), device=dev, generator=gen) < 0.05] = float("nan")
        elif kind == "block":
            lo = (n - 4000) // 2
            X[lo:lo + 4000, lo:lo + 4000] = float("nan")
        elif kind == "single":
            X[:] = float("nan")
            X[n // 3, n // 5] = 1.0
        return X

    rows = []
    for n, kind in ((a.n, "scattered"), (a.n, "block"), (a.small, "scattered"), (a.small, "single")):
        X = raster(n, kind)
        holes = float((~torch.isfinite(X)).float().mean())
        work = torch.empty_like(X)
        clone_ms = timed(lambda: work.copy_(X))

        def fill():
            work.copy_(X)
            na.inpaint_nearest(work)
        ms = timed(fill) - clone_ms
        assert bool(torch.isfinite(work).all())
        # the envelope entries the scan wrote (a count the run leaves behind), for the model's variable term
        lib = nr._lib.load()
        nbytes = lib.smrf_nearest_workspace_bytes(n, n, 4)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        work.copy_(X)
        nr._lib.check(lib.smrf_nearest_f32(nr._ptr(work), nr._ptr(work), None, None, n, n, nr._ptr(ws), nbytes,
                                           nr._stream()))
        torch.cuda.synchronize()
        strips, nseg = (n + 31) // 32, (n + 1023) // 1024
        up256 = lambda v: (v + 255) & ~255  # noqa: E731
        cnt_off = 3 * up256(strips * n * 4)
        cnt = ws[cnt_off:cnt_off + n * nseg * 4].view(torch.int32)
        envelope_share = float(cnt.sum()) / (n * n)
        del ws
        p1, scan, look = model_bytes_per_cell(n, n, 4, holes, envelope_share)
        bpc = p1 + scan + look
        row = dict(case=kind, n=n, dtype="f32", hole_share=round(holes, 4), ms=round(ms, 3),
                   mcells_per_s=round(n * n / ms / 1e3, 1), envelope_entries_per_cell=round(envelope_share, 4),
                   model_bytes_per_cell=dict(pass1=round(p1, 2), scan=round(scan, 2), lookup=round(look, 2),
                                             total=round(bpc, 2)),
                   frac_of_copy=round(n * n * bpc / copy_rate * 1e3 / ms, 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del X, work
        torch.cuda.empty_cache()
    small = {r["case"]: r["ms"] for r in rows if r["n"] == a.small}
    ratio = small["single"] / small["scattered"]
    print(json.dumps(dict(single_over_scattered=round(ratio, 2), n=a.small)), flush=True)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("copy rate: %.1f GB/s (read + write)\n\n" % (copy_rate / 1e9))
            fh.write("| case | n | hole share | ms | Mcells/s | envelope entries per cell | model B per cell "
                     "(pass 1 + scan + lookup) | of copy rate |\n|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                m = r["model_bytes_per_cell"]
                fh.write("| %s | %d | %.4f | %.3f | %.0f | %.4f | %.2f + %.2f + %.2f = %.2f | %.4f |\n" % (
                    r["case"], r["n"], r["hole_share"], r["ms"], r["mcells_per_s"], r["envelope_entries_per_cell"],
                    m["pass1"], m["scan"], m["lookup"], m["total"], r["frac_of_copy"]))
            fh.write("\nsingle source / scattered at %d^2: %.2f\n" % (a.small, ratio))


if __name__ == "__main__":
    main()
