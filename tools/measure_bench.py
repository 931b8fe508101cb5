#!/usr/bin/env python3
"""Time ``neilpy_amd.measure.region_stats`` on device-resident rasters beside the byte model of DESIGN.md section 22 and
beside ``scipy.ndimage`` on the same host, and derive what the kernels' 64-bit integer atomics cost.

Cases, at ``--n`` (4096 by default), float32 values, three label rasters: one object (every wave's atomics land on one
entry), the objects ``neilpy_amd.label.label`` finds in a Bernoulli mask with p = 0.59 (the 4-connected percolation
threshold: objects of every size), and a checkerboard of distinct labels (every stretch of equal labels has length 1, so
every labelled cell sends its own atomics).  Each is timed for ``what`` = count + min + max (one pass), + sum + mean and
the positions (two passes) and everything (three passes).

A figure is the median of ``--reps`` (at least 10) calls after ``--warmup`` calls, each call between its own pair of device
events, with its spread (min .. max).  A call is what a user pays on tensors with ``num_features`` given: the workspace and
result allocations from the caching allocator and the launches; nothing is read back.

The model is (input bytes + 4) bytes per cell and pass, table traffic aside.  ``model_ms`` is that traffic at the streaming
rate and ``frac_of_model`` is ``model_ms / ms``.  The streaming rate is the best grid-stride copy of
``tools/ubench/stream_rate`` (read + write bytes per second) when that binary has been built (``--stream-bin``), else a
torch device-to-device copy in this process.

The atomic figures are derived, not isolated: the second pass's time is the two-pass call minus the one-pass call with
``what`` = sum alone beside count alone, and the 64-bit integer adds it retires are three per stretch, the background's
(label 0) included.  On the checkerboard that is three adds per labelled cell to distinct entries and three per background
cell to entry 0; on the one-object raster three per 64 cells, all to one entry.

SciPy is timed once per label raster, single thread: ``sum_labels``, ``variance`` and ``extrema`` over all labels
(``--no-scipy`` skips it).

One JSON line per figure; the tables go to ``--md`` (profiles/measure_bench.md) as Markdown.

    python tools/measure_bench.py [--n 4096] [--reps 10] [--md profiles/measure_bench.md]
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

WHATS = (("count, min, max", ("count", "min", "max"), 1),
         ("+ sum, mean, positions", ("count", "min", "max", "sum", "mean", "min_index", "max_index"), 2),
         ("everything", ("count", "sum", "mean", "variance", "min", "max", "min_index", "max_index"), 3))


def stream_rate_from_binary(path):
    """best 'copy ... grid-stride' line of tools/ubench/stream_rate, in bytes per second (None if it cannot run)"""
    if not os.path.exists(path):
        return None
    r = subprocess.run([path], capture_output=True, text=True, timeout=300)
    rates = [float(m) for m in re.findall(r"^copy.*?(\d+) GB/s\s*$", r.stdout, re.M)]
    return max(rates) * 1e9 if r.returncode == 0 and rates else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "measure_bench.md"))
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--stream-bin", default=os.path.join(ROOT, "tools", "ubench", "stream_rate"))
    a = ap.parse_args()
    import torch
    from neilpy_amd import label as lb, measure as ms
    if not torch.cuda.is_available():
        raise SystemExit("measure_bench needs the GPU: nothing is measured without one")
    if a.reps < 10:
        raise SystemExit("--reps: a figure is the median of at least 10 calls")
    dev = torch.device("cuda:0")
    n = a.n

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
        return dict(ms=round(float(np.median(t)), 4), lo=round(min(t), 4), hi=round(max(t), 4))

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

    gen = torch.Generator(device=dev).manual_seed(20270307)
    r, c = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
    X = (312.5 + 0.31 * r - 0.17 * c + 9.0 * torch.sin(r / 7.0) * torch.cos(c / 11.0)).to(torch.float32)
    X += 0.4 * torch.randn((n, n), device=dev, generator=gen)
    board = ((r + c) % 2 == 0)
    checker = torch.where(board, torch.cumsum(board.reshape(-1).to(torch.int32), 0, dtype=torch.int32).reshape(n, n), 0).to(torch.int32)
    del r, c, board
    bern, count = lb.label(torch.rand((n, n), device=dev, generator=gen) < 0.59)
    rasters = (("one object", torch.ones((n, n), dtype=torch.int32, device=dev), 1),
               ("label(Bernoulli p = 0.59)", bern, count),
               ("checkerboard of distinct labels", checker, int(checker.max().item())))
    cells = n * n
    rows, atomics, scipy_rows = [], [], []
    for case, L, labels in rasters:
        stretches = int(((L.reshape(-1)[1:] != L.reshape(-1)[:-1]) | (torch.arange(1, cells, device=dev) % 64 == 0)).sum().item()) + 1
        for wname, what, passes in WHATS:
            row = dict(case=case, n=n, labels=labels, what=wname, passes=passes)
            row.update(timed(lambda: ms.region_stats(X, L, labels, what)))
            model = cells * passes * (4 + 4) / rate * 1e3
            row.update(mcells_per_s=round(cells / row["ms"] / 1e3, 1), model_ms=round(model, 4), frac_of_model=round(model / row["ms"], 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
        one = timed(lambda: ms.region_stats(X, L, labels, ("count",)))
        two = timed(lambda: ms.region_stats(X, L, labels, ("sum",)))
        extra = max(two["ms"] - one["ms"], 1e-6)
        arow = dict(case=case, stretches_per_wave=round(stretches / (cells / 64), 2), count_only_ms=one["ms"], sum_only_ms=two["ms"],
                    second_pass_ms=round(extra, 4), adds_u64=3 * stretches, adds_u64_per_ns=round(3 * stretches / (extra * 1e6), 3))
        atomics.append(arow)
        print(json.dumps(arow), flush=True)
        if not a.no_scipy:
            import scipy.ndimage as ndi
            Xh, Lh = X.cpu().numpy(), L.cpu().numpy()
            index = np.arange(1, labels + 1)
            srow = dict(case=case)
            for name in ("sum_labels", "variance", "extrema"):
                t = time.perf_counter()
                getattr(ndi, name)(Xh, Lh, index)
                srow[name + "_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            srow["device_everything_ms"] = rows[-1]["ms"]
            srow["scipy_over_device"] = round((srow["sum_labels_ms"] + srow["variance_ms"] + srow["extrema_ms"]) / rows[-1]["ms"], 1)
            scipy_rows.append(srow)
            print(json.dumps(srow), flush=True)
            del Xh, Lh
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("# region_stats at %d x %d, float32 (tools/measure_bench.py)\n\n" % (n, n))
            fh.write("%s; streaming rate: %.0f GB/s (%s); median of %d calls after %d warm-up calls, (min .. max)\n\n" %
                     (torch.cuda.get_device_name(dev), rate / 1e9, rate_from, a.reps, a.warmup))
            fh.write("| labels | label count | what | passes | region_stats, ms | Mcells/s | model, ms | model / measured |\n|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %s | %d | %s | %d | %.4f (%.4f .. %.4f) | %.0f | %.4f | %.3f |\n" % (
                    r["case"], r["labels"], r["what"], r["passes"], r["ms"], r["lo"], r["hi"], r["mcells_per_s"], r["model_ms"], r["frac_of_model"]))
            fh.write("\nThe model is 8 bytes per cell and pass (4 of float32 input + 4 of labels) at the streaming rate, table traffic aside.\n")
            fh.write("\n## 64-bit integer atomic adds, derived\n\nThe second pass's time is the call with `what` = sum minus the call with "
                     "`what` = count; it retires three 64-bit adds per stretch of equal labels within a wave (and reads the raster once "
                     "more), so the rate is a lower bound on what the atomics alone would reach.\n\n")
            fh.write("| labels | stretches per wave | count only, ms | sum only, ms | second pass, ms | 64-bit adds | adds per ns |\n|---|---|---|---|---|---|---|\n")
            for r in atomics:
                fh.write("| %s | %.2f | %.4f | %.4f | %.4f | %d | %.3f |\n" % (r["case"], r["stretches_per_wave"], r["count_only_ms"], r["sum_only_ms"],
                                                                            r["second_pass_ms"], r["adds_u64"], r["adds_u64_per_ns"]))
            if scipy_rows:
                fh.write("\n## scipy.ndimage on the host, one thread, once\n\n| labels | sum_labels, ms | variance, ms | extrema, ms | "
                         "region_stats (everything), ms | SciPy / device |\n|---|---|---|---|---|---|\n")
                for r in scipy_rows:
                    fh.write("| %s | %.1f | %.1f | %.1f | %.4f | %.0f |\n" % (r["case"], r["sum_labels_ms"], r["variance_ms"], r["extrema_ms"],
                                                                            r["device_everything_ms"], r["scipy_over_device"]))
            else:
                fh.write("\nSciPy was not timed in this run (--no-scipy).\n")


if __name__ == "__main__":
    main()
