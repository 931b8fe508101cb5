#!/usr/bin/env python3
"""Time bdr_bootstrap and single hungarian_algorithm calls against the host doing the same work with SciPy and NumPy.

bootstrap   k = 10 000 samples of n of m points, for 16 of 32, 30 of 60, 64 of 128, 128 of 256 and 512 of 1024.
            ``call_ms``: the public call with NumPy arrays and a sample table drawn beforehand - upload, range check,
            the one launch, download - by a host clock around a call that ends in a device synchronise.  ``device_ms``:
            the same call with everything already on the device, between device events.  ``draw_ms``: the k draws of
            np.random.choice on the host, which the default call makes first.  ``host_ms``: the baseline,
            linear_sum_assignment on cdist and the regression as a complex least-squares fit in NumPy for the same samples;
            it is timed on --host-k samples and scaled to k.
model       the serial depth of one problem is its scan steps (counted by tests/assign_numpy.py on the first samples)
            times the cost of a step: a pass over the wave's columns-per-lane and the 6-step cross-lane minimum.
            ``model_ms`` prices a step at STEP_BASE + STEP_COL * columns per lane cycles (STEP_COL_RECOMPUTE where the
            costs are recomputed) at CLOCK_GHZ, an estimate made before any run, over the waves the device holds at
            once; ``ns_per_step`` is what the measured ``device_ms`` comes to.  Where they disagree the measurement stands.
single      one hungarian_algorithm call (NumPy in, NumPy out) at n x n against cdist + linear_sum_assignment.

``host_over_device`` / ``host_over_call`` / ``host_over_call_and_draw``: the baseline over the device time, over the
public call with a ready table, and over that call plus the default host draw - the last is what a user of the default
call sees.  Every timed call is warmed up once at its own shape; a timed window holds as many calls as fill --window-ms
of device time (``calls_per_window``), and the bootstrap rows take the median of --reps windows.  The tool writes the
whole of --md; what the figures mean is DESIGN.md section 18.

    python tools/assign_bench.py [--k 10000] [--reps 5] [--md profiles/assign_bench.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ((16, 32), (30, 60), (64, 128), (128, 256), (512, 1024))
SINGLE = (30, 64, 256, 1024)
CUS, SIMD_WAVES = 256, 16              # waves of this kernel one CU holds by registers (4 per SIMD)
CLOCK_GHZ, STEP_BASE, STEP_COL, STEP_COL_RECOMPUTE = 2.4, 400.0, 60.0, 200.0


def clouds(n, m, seed):
    rng = np.random.default_rng(seed)
    ab = rng.uniform(0, 100, (m, 2))
    xy = ab[rng.permutation(m)[:n]] * 1.3 + rng.normal(0, 6.0, (n, 2))
    return xy, ab


def host_bdr(xy, ab):
    """rsquare and DI of the bidimensional regression as one complex least-squares fit w = alpha + beta z"""
    z, w = xy[:, 0] + 1j * xy[:, 1], ab[:, 0] + 1j * ab[:, 1]
    zc, wc = z - z.mean(), w - w.mean()
    beta = np.vdot(zc, wc) / np.vdot(zc, zc).real
    res = wc - beta * zc
    r2 = 1.0 - np.vdot(res, res).real / np.vdot(wc, wc).real
    return r2, np.sqrt(1.0 - r2)


def host_sample(xy, ab, idx):
    """one sample on the host: SciPy's assignment on cdist, then the regression in NumPy"""
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial.distance import cdist
    abs_ = ab[idx]
    _, col = linear_sum_assignment(cdist(xy, abs_))
    return host_bdr(xy, abs_[col])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-k", type=int, default=200)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least device time in one timed window")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    from neilpy_amd import matching as na
    from neilpy_amd.matching import assignment_route
    import assign_numpy as an
    if not torch.cuda.is_available():
        raise SystemExit("assign_bench needs the GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    rows, singles = [], []
    for n, m in CASES:
        xy, ab = clouds(n, m, n)
        rng = np.random.default_rng(n + 1)
        t0 = time.perf_counter()
        np.random.seed(n)
        for _ in range(a.k):
            np.random.choice(m, n, replace=False)
        draw_ms = (time.perf_counter() - t0) * 1e3
        table = np.stack([rng.permutation(m)[:n] for _ in range(a.k)]).astype(np.int64)
        xt, at, tt = (torch.from_numpy(v).to(dev) for v in (xy, ab, table))
        na.bdr_bootstrap(xy, ab, samples=table)                     # warm-up at this shape
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        na.bdr_bootstrap(xt, at, samples=tt)
        torch.cuda.synchronize()
        inner = max(1, min(200, int(a.window_ms / max((time.perf_counter() - t0) * 1e3, 1e-3))))   # calls per timed window
        call, device = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(inner):
                rsq, di = na.bdr_bootstrap(xy, ab, samples=table)
            torch.cuda.synchronize()
            call.append((time.perf_counter() - t0) * 1e3 / inner)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                na.bdr_bootstrap(xt, at, samples=tt)
            e1.record()
            torch.cuda.synchronize()
            device.append(e0.elapsed_time(e1) / inner)
        hk = min(a.host_k, a.k)
        host_sample(xy, ab, table[0])                    # warm-up: SciPy's imports and first calls
        t0 = time.perf_counter()
        host = np.array([host_sample(xy, ab, table[s]) for s in range(hk)])
        host_ms = (time.perf_counter() - t0) * 1e3 * a.k / hk
        assert np.allclose(host[:, 0], rsq[:hk], rtol=1e-9, atol=0), "the device and the host disagree"
        count = {}
        for s in range(4):
            an.solve(an.costs(xy, ab[table[s]]), count)
        steps = count["steps"] / 4
        route = assignment_route(n, n, 2)
        cpl = (n + 63) // 64
        per_cu = min(SIMD_WAVES, (160 * 1024 // (route["waves"] * route["lds_bytes"])) * route["waves"])
        resident = min(a.k, CUS * per_cu)
        rounds = -(-a.k // resident)
        cyc = STEP_BASE + (STEP_COL if route["cached"] else STEP_COL_RECOMPUTE) * cpl
        model_ms = rounds * steps * cyc / (CLOCK_GHZ * 1e6)
        cms, dms = float(np.median(call)), float(np.median(device))
        rows.append(dict(case="%d of %d" % (n, m), k=a.k, calls_per_window=inner, cached=route["cached"], waves_per_cu=per_cu,
                         steps_per_sample=round(steps, 1), draw_ms=round(draw_ms, 1), call_ms=round(cms, 2),
                         device_ms=round(dms, 2), device_ms_min=round(min(device), 2), device_ms_max=round(max(device), 2),
                         host_ms=round(host_ms, 0), host_over_device=round(host_ms / dms, 1), host_over_call=round(host_ms / cms, 1),
                         host_over_call_and_draw=round(host_ms / (cms + draw_ms), 1),
                         model_ms=round(model_ms, 2), ns_per_step=round(dms * 1e6 / (rounds * steps), 1)))
        print(json.dumps(rows[-1]), flush=True)
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial.distance import cdist
    from neilpy_amd.matching import assignment_limit
    for n in SINGLE + (assignment_limit(),):
        rng = np.random.default_rng(n)
        x, y = rng.uniform(0, 100, (n, 2)), rng.uniform(0, 100, (n, 2))
        na.hungarian_algorithm(x, y)
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r, c, mc = na.hungarian_algorithm(x, y)
            t.append((time.perf_counter() - t0) * 1e3)
        h = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            C = cdist(x, y)
            hr, hc = linear_sum_assignment(C)
            h.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(c, hc)
        count = {}
        if n <= 1024:
            an.solve(C, count)
        singles.append(dict(n=n, call_ms=round(float(np.median(t)), 3), scipy_ms=round(float(np.median(h)), 3),
                            steps=count.get("steps")))
        print(json.dumps(singles[-1]), flush=True)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# bdr_bootstrap and hungarian_algorithm on the MI355X (tools/assign_bench.py)\n\n")
            f.write("k = %d samples per case, median of %d runs after one warm-up; host baseline timed on %d samples and "
                    "scaled to k.  Columns: see the tool's docstring.\n\n" % (a.k, a.reps, min(a.host_k, a.k)))
            keys = list(rows[0])
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in rows:
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")
            f.write("\nSingle n x n hungarian_algorithm calls, NumPy in and out (one wave of the device against one host "
                    "core), median of %d:\n\n" % a.reps)
            keys = list(singles[0])
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in singles:
                f.write("| " + " | ".join(str(r[k]) for k in keys) + " |\n")


if __name__ == "__main__":
    main()
