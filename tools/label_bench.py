#!/usr/bin/env python3
"""Time ``neilpy_amd.label.label`` on device-resident masks beside ``scipy.ndimage.label`` on the same host and beside the
byte model of DESIGN.md section 21.

Cases, at every ``--n`` (4096 and 16384 by default): random masks at p = 0.1 and 0.59 under the 4-neighbourhood and at
p = 0.41 under the 8-neighbourhood (0.59 and 0.41 lie near the site-percolation thresholds of the two lattices, where the
objects are largest and most tangled); the object mask ``progressive_filter`` gives on ``synth_dem`` (windows 1..18,
4-neighbourhood); and the one-object serpentine of the tests (every other row full, joined at alternating ends), the
adversarial case: the longest union chains across tile seams.

A figure is the median of ``--reps`` (at least 10) calls after ``--warmup`` calls, each call between its own pair of device
events, with its spread (min .. max).  A call is what a user pays on a ``bool`` tensor: the workspace allocation from the
caching allocator, the six launches, and the 4-byte read of the count.  Before a case is timed its labels are compared
with SciPy's (``--no-check`` skips that and the SciPy timing).  SciPy is timed once per case, single thread, on the
NumPy copy of the same mask.

The model is (25 + 4 p) bytes per cell, p the foreground fraction: tile 1 + 4, flatten 4 + 4, number 4, relabel 4 + 4 and
4 p for the gather of the roots' numbers; the walks to the roots, the seam pass and the roots' own writes are not in it.
``model_ms`` is that traffic at the streaming rate and ``frac_of_model`` is ``model_ms / ms``.  The streaming rate is the
best grid-stride copy of ``tools/ubench/stream_rate`` (read + write bytes per second) when that binary has been built
(``--stream-bin``), else a torch device-to-device copy in this process.

One JSON line per case; ``--md PATH`` also writes the table as Markdown.

    python tools/label_bench.py [--n 4096 16384] [--reps 10] [--md profiles/label_bench_table.md]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
EIGHT = np.ones((3, 3), dtype=bool)


def stream_rate_from_binary(path):
    """best 'copy ... grid-stride' line of tools/ubench/stream_rate, in bytes per second (None if it cannot run)"""
    if not os.path.exists(path):
        return None
    r = subprocess.run([path], capture_output=True, text=True, timeout=300)
    rates = [float(m) for m in re.findall(r"^copy.*?(\d+) GB/s\s*$", r.stdout, re.M)]
    return max(rates) * 1e9 if r.returncode == 0 and rates else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=None)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--stream-bin", default=os.path.join(ROOT, "tools", "ubench", "stream_rate"))
    a = ap.parse_args()
    import torch
    import neilpy_amd as na
    from neilpy_amd import label as lb
    if not torch.cuda.is_available():
        raise SystemExit("label_bench needs the GPU: nothing is measured without one")
    if a.reps < 10:
        raise SystemExit("--reps: a figure is the median of at least 10 calls")
    dev = torch.device("cuda:0")
    if not a.no_check:
        ndimage_label(np.eye(64, dtype=bool), FOUR)          # the import and SciPy's first call are not part of a figure

    def once(f):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def timed(f):
        for _ in range(a.warmup):
            f()
        torch.cuda.synchronize()
        t = [once(f) for _ in range(a.reps)]
        return dict(ms=round(float(np.median(t)), 3), lo=round(min(t), 3), hi=round(max(t), 3))

    rate = stream_rate_from_binary(a.stream_bin)
    rate_from = "tools/ubench/stream_rate, best grid-stride copy"
    if rate is None:
        src = torch.empty(1 << 27, dtype=torch.float64, device=dev)
        dst = torch.empty_like(src)
        dst.copy_(src)
        torch.cuda.synchronize()
        rate = 2 * src.numel() * 8 / (float(np.median([once(lambda: dst.copy_(src)) for _ in range(10)])) * 1e-3)
        rate_from = "torch device-to-device copy of 1 GiB"
        del src, dst
    print(json.dumps(dict(device=torch.cuda.get_device_name(dev), stream_gb_per_s=round(rate / 1e9, 1), source=rate_from,
                          reps=a.reps, warmup=a.warmup)), flush=True)

    def cases(n):
        gen = torch.Generator(device=dev).manual_seed(20270103)
        for p, structure, name in ((0.1, FOUR, "4"), (0.59, FOUR, "4"), (0.41, EIGHT, "8")):
            yield "random p = %g" % p, name, structure, torch.rand((n, n), device=dev, generator=gen) < p
        Z = na.synth_dem(n)
        yield "progressive_filter(synth_dem)", "4", FOUR, torch.from_numpy(na.progressive_filter(Z, np.arange(1, 19), 1, .15)).to(dev)
        del Z
        s = torch.zeros((n, n), dtype=torch.bool, device=dev)
        s[::2] = True
        s[1::4, -1] = True
        s[3::4, 0] = True
        yield "serpentine, one object", "4", FOUR, s

    rows = []
    for n in a.n:
        for case, conn, structure, M in cases(n):
            cells = M.numel()
            p = float(M.float().mean())
            L, count = lb.label(M, structure)
            row = dict(case=case, n=n, connectivity=conn, foreground=round(p, 4), objects=count)
            if not a.no_check:
                host = M.cpu().numpy()
                t = time.perf_counter()
                want, m = ndimage_label(host, structure)
                row["scipy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                assert m == count and np.array_equal(L.cpu().numpy(), want), (case, n)
                del host, want
            del L
            row.update(timed(lambda: lb.label(M, structure)))
            model = cells * (25 + 4 * p) / rate * 1e3
            row.update(mcells_per_s=round(cells / row["ms"] / 1e3, 1), model_ms=round(model, 3), frac_of_model=round(model / row["ms"], 3))
            if "scipy_ms" in row:
                row["scipy_over_device"] = round(row["scipy_ms"] / row["ms"], 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del M
            torch.cuda.empty_cache()
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("streaming rate: %.0f GB/s (%s); median of %d calls after %d warm-up calls, (min .. max)\n\n" %
                     (rate / 1e9, rate_from, a.reps, a.warmup))
            fh.write("| mask | n | connectivity | foreground | objects | label, ms | Mcells/s | scipy.ndimage.label, ms | SciPy / device | "
                     "model, ms | model / measured |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %s | %d | %s | %.3f | %d | %.3f (%.3f .. %.3f) | %.0f | %s | %s | %.3f | %.3f |\n" % (
                    r["case"], r["n"], r["connectivity"], r["foreground"], r["objects"], r["ms"], r["lo"], r["hi"], r["mcells_per_s"],
                    r.get("scipy_ms", ""), r.get("scipy_over_device", ""), r["model_ms"], r["frac_of_model"]))


def ndimage_label(mask, structure):
    import scipy.ndimage as ndi
    return ndi.label(mask, structure)


if __name__ == "__main__":
    main()
