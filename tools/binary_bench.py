#!/usr/bin/env python3
"""Time ``neilpy_amd.binary`` on device-resident masks beside ``scipy.ndimage`` on the same host and beside the byte model
of DESIGN.md section 23.

Three tables.

Functions.  At every ``--n`` (2048 and 8192 by default), on a random ``bool`` mask at p = 0.59: erosion and dilation (3 x 3
ones, one step and eight), opening and closing (cross, ``iterations=2``), hit-or-miss (a corner and its complement),
``binary_propagation`` of sparse seeds through the mask and ``binary_fill_holes``, the last two through the components of
the mask.  The model of a stepped call is pack (1 + 1/8 bytes per cell), k steps (2/8 each, 3/8 with a mask) and unpack
(1/8 + 1); of the label route two packs, one step, ``label``'s (25 + 4 p), the flag plane's 1, mark (2/8 + 4 p' + p', p' the
fraction marked) and select (2/8 + 4 + 1 + 1).  ``model_ms`` is that traffic at the streaming rate, ``frac_of_model`` is
``model_ms / ms``.

Routes.  ``impl='labels'`` against ``impl='iterate'`` for ``binary_propagation`` through a random mask and along the
serpentine of the tests from a seed at its end (``--route-n``), where the steps are as many as the path is long.

Batch size.  ``binary.CHECK_EVERY`` set to 1, 2, 4, ... 64 for an erosion with ``iterations=-1`` that takes
``--batch-steps`` steps: the cost of a flag read per batch against the surplus steps after convergence.

A figure is the median of ``--reps`` (at least 10) calls after ``--warmup`` calls, each between its own pair of device
events, with its spread (min .. max).  Before a case is timed its bits are compared with SciPy's (``--no-check`` skips
that and the SciPy timing).  The streaming rate is the best grid-stride copy of ``tools/ubench/stream_rate`` when that
binary has been built, else a torch device-to-device copy in this process.

One JSON line per case; ``--md PATH`` also writes the tables as Markdown.

    python tools/binary_bench.py [--n 2048 8192] [--reps 10] [--md profiles/binary_bench_table.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ONES = np.ones((3, 3), dtype=bool)
CORNER = np.array([[0, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--route-n", type=int, default=257)
    ap.add_argument("--batch-steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=None)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--stream-bin", default=os.path.join(ROOT, "tools", "ubench", "stream_rate"))
    a = ap.parse_args()
    import scipy.ndimage as ndi
    import torch
    from label_bench import stream_rate_from_binary
    from neilpy_amd import binary as bm
    if not torch.cuda.is_available():
        raise SystemExit("binary_bench needs the GPU: nothing is measured without one")
    if a.reps < 10:
        raise SystemExit("--reps: a figure is the median of at least 10 calls")
    dev = torch.device("cuda:0")

    def once(f):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def timed(f, reps=None):
        for _ in range(a.warmup):
            f()
        torch.cuda.synchronize()
        t = [once(f) for _ in range(reps or a.reps)]
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
                          reps=a.reps, warmup=a.warmup, check_every=bm.CHECK_EVERY)), flush=True)

    def stepped(k, masked=False):
        return 2.25 + k * (0.375 if masked else 0.25)

    def by_labels(p_mask, p_marked, has_input):
        return (1.125 if has_input else 0.125) + 1.125 + 0.375 + 25 + 4 * p_mask + 1 + 0.25 + 5 * p_marked + 6.25

    # ---- functions
    rows = []
    for n in a.n:
        gen = torch.Generator(device=dev).manual_seed(20270320)
        M = torch.rand((n, n), device=dev, generator=gen) < 0.59
        S = torch.rand((n, n), device=dev, generator=gen) < 0.001
        host, seeds = M.cpu().numpy(), S.cpu().numpy()
        p = float(host.mean())
        cases = [
            ("binary_erosion, 3 x 3, 1 step", lambda: bm.binary_erosion(M, ONES), lambda: ndi.binary_erosion(host, ONES), stepped(1)),
            ("binary_erosion, 3 x 3, 8 steps", lambda: bm.binary_erosion(M, ONES, 8), lambda: ndi.binary_erosion(host, ONES, 8), stepped(8)),
            ("binary_dilation, 3 x 3, 1 step", lambda: bm.binary_dilation(M, ONES), lambda: ndi.binary_dilation(host, ONES), stepped(1)),
            ("binary_opening, cross, iterations=2", lambda: bm.binary_opening(M, None, 2), lambda: ndi.binary_opening(host, None, 2), stepped(4)),
            ("binary_closing, cross, iterations=2", lambda: bm.binary_closing(M, None, 2), lambda: ndi.binary_closing(host, None, 2), stepped(4)),
            ("binary_hit_or_miss, corner", lambda: bm.binary_hit_or_miss(M, CORNER), lambda: ndi.binary_hit_or_miss(host, CORNER), stepped(1)),
        ]
        marked = float((ndi.binary_dilation(seeds, None, 1, host) & host).mean())
        cases.append(("binary_propagation, seeds p = 0.001, labels", lambda: bm.binary_propagation(S, None, M),
                      lambda: ndi.binary_propagation(seeds, None, host), by_labels(p, marked, True)))
        cases.append(("binary_fill_holes, labels", lambda: bm.binary_fill_holes(M), lambda: ndi.binary_fill_holes(host),
                      by_labels(1 - p, 4.0 / n, False)))
        for name, f, g, bytes_per_cell in cases:
            row = dict(table="functions", case=name, n=n, foreground=round(p, 4))
            got = f()
            if not a.no_check:
                t = time.perf_counter()
                ref = g()
                row["scipy_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                assert np.array_equal(got.cpu().numpy(), ref), (name, n)
                del ref
            del got
            row.update(timed(f))
            model = n * n * bytes_per_cell / rate * 1e3
            row.update(mcells_per_s=round(n * n / row["ms"] / 1e3, 1), bytes_per_cell=round(bytes_per_cell, 3), model_ms=round(model, 3),
                       frac_of_model=round(model / row["ms"], 3))
            if "scipy_ms" in row:
                row["scipy_over_device"] = round(row["scipy_ms"] / row["ms"], 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del M, S
        torch.cuda.empty_cache()

    # ---- routes
    n = a.route_n
    serp = np.zeros((n, n), dtype=bool)
    serp[::2] = True
    serp[1::4, -1] = True
    serp[3::4, 0] = True
    routes = []
    corner = np.zeros((n, n), dtype=bool)
    corner[0, 0] = True
    rng = np.random.default_rng(20270321)
    for name, mask, seed in (("random p = 0.59, seeds p = 0.001", rng.random((n, n)) < 0.59, rng.random((n, n)) < 0.001),
                             ("serpentine, one seed at its end", serp, corner)):
        Mt, St = torch.from_numpy(mask).to(dev), torch.from_numpy(seed).to(dev)
        ref = ndi.binary_propagation(seed, None, mask)
        for impl in ("labels", "iterate"):
            got = bm.binary_propagation(St, None, Mt, impl=impl)
            assert np.array_equal(got.cpu().numpy(), ref), (name, impl)
            row = dict(table="routes", case="binary_propagation, " + name, n=n, impl=impl)
            row.update(timed(lambda: bm.binary_propagation(St, None, Mt, impl=impl)))
            routes.append(row)
            print(json.dumps(row), flush=True)

    # ---- batch size
    side = 2 * (a.batch_steps - 1)
    full = torch.ones((side, side), dtype=torch.bool, device=dev)
    batches = []
    default = bm.CHECK_EVERY
    try:
        for every in (1, 2, 4, 8, 16, 32, 64):
            bm.CHECK_EVERY = every
            assert not bool(bm.binary_erosion(full, ONES, -1).any())
            row = dict(table="batch", case="binary_erosion of a full square, iterations=-1", n=side, steps=a.batch_steps, check_every=every)
            row.update(timed(lambda: bm.binary_erosion(full, ONES, -1)))
            row["us_per_step"] = round(1e3 * row["ms"] / a.batch_steps, 2)
            batches.append(row)
            print(json.dumps(row), flush=True)
    finally:
        bm.CHECK_EVERY = default

    if a.md:
        with open(a.md, "w") as fh:
            fh.write("streaming rate: %.0f GB/s (%s); median of %d calls after %d warm-up calls, (min .. max); CHECK_EVERY = %d\n\n" %
                     (rate / 1e9, rate_from, a.reps, a.warmup, default))
            fh.write("| function | n | foreground | ms | Mcells/s | scipy.ndimage, ms | SciPy / device | model, B/cell | model, ms | "
                     "model / measured |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %s | %d | %.3f | %.3f (%.3f .. %.3f) | %.0f | %s | %s | %.3f | %.3f | %.3f |\n" % (
                    r["case"], r["n"], r["foreground"], r["ms"], r["lo"], r["hi"], r["mcells_per_s"], r.get("scipy_ms", ""),
                    r.get("scipy_over_device", ""), r["bytes_per_cell"], r["model_ms"], r["frac_of_model"]))
            fh.write("\n| case | n | impl | ms |\n|---|---|---|---|\n")
            for r in routes:
                fh.write("| %s | %d | %s | %.3f (%.3f .. %.3f) |\n" % (r["case"], r["n"], r["impl"], r["ms"], r["lo"], r["hi"]))
            fh.write("\n| case | n | steps | CHECK_EVERY | ms | us per step |\n|---|---|---|---|---|---|\n")
            for r in batches:
                fh.write("| %s | %d | %d | %d | %.3f (%.3f .. %.3f) | %.2f |\n" % (r["case"], r["n"], r["steps"], r["check_every"], r["ms"],
                                                                                 r["lo"], r["hi"], r["us_per_step"]))


if __name__ == "__main__":
    main()
