"""csrc/pf_route.h on the host, for tests/test_pf_route_host.py, test_pf_fold_host.py and test_pf_steps_host.py: one stand-alone
program that asks smrf_pf_route, smrf_pf_fold and smrf_pf_steps one case per line, its build, the tables and random window
lists the three modules share, and the driver's plane rotation as it stood before smrf_pf_steps, restated with a symbolic replay
(tests/test_gpu_dil_cross.py holds the workspace of a real call against that replay, plane by plane, on the window lists of
tests/window_cases.py)."""
import os
import random
import re
import subprocess
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neilpy_amd", "csrc")
TWO_PASS, FUSED, DIRECT, COPY, CH = 0, 1, 2, 3, 4
AUTO, RING, DIRECT_IMPL = 0, 1, 2
NONE, CROSS, AFTER = 0, 1, 2
CHAIN, FUSED_OPEN, ERODE, INC_ERODE, DILATE, DILATE_CROSS = range(6)   # SmrfPfStep::kind
PLANE_Z, NO_PLANE = -1, -2
RIM_FREE = (16, 21, 36)                                   # the radii from 15 up whose leftover set P_R is empty (ero_inc.inc)
Mi = 1 << 20
# the launches morph_chain.h has kernels for, restated: radii, smallest raster in cells for fp32 / fp64 (None: no kernel)
PATTERNS = [((1, 2, 3), 0, 0), ((1, 2), 0, 0), ((2, 3), 0, 0), ((4, 5), 20 * Mi, None), ((4,), 0, 0), ((5,), 0, 0), ((6,), 0, None),
            ((7,), 0, 4 * Mi), ((8,), 0, 16 * Mi), ((9,), 0, None), ((10,), 20 * Mi, None)]

Plan = namedtuple("Plan", "route inc pattern fold runs steps")
Step = namedtuple("Step", "kind win len src aux dst dense closes")   # (the pattern index of a chain is Plan.pattern[win])

MAIN = r'''
#include <cstdio>
#include <vector>
#include "pf_route.h"
// one case per line: elem_size fused chain ero_inc impl nan_aware band dil_cross rows cells n w[0] .. w[n-1]
// -> one line: n routes, n incremental-erosion flags of the route, n pattern indices, n fold values, n "runs the incremental
//    erosion", the number of steps and nine numbers per step
int main() {
  SmrfPfRules k;
  int rows, n;
  long long cells;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %lld %d", &k.elem_size, &k.fused, &k.chain, &k.ero_inc, &k.impl, &k.nan_aware,
                    &k.band, &k.dil_cross, &rows, &cells, &n) == 11) {
    // exactly n entries each (2n steps), so that the sanitizer build sees any access beyond them
    std::vector<int32_t> w(n), route(n, -99), pattern(n, -99);
    std::vector<uint8_t> inc(n, 99), fold(n, 99);
    std::vector<SmrfPfStep> steps(2 * n);
    for (int i = 0; i < n; ++i)
      if (std::scanf("%d", &w[i]) != 1) return 2;
    smrf_pf_route(k, w.data(), n, rows, cells, route.data(), inc.data(), pattern.data());
    const std::vector<int32_t> route0 = route;
    const std::vector<uint8_t> inc0 = inc;
    smrf_pf_fold(k, w.data(), route.data(), inc.data(), n, fold.data());
    if (route != route0 || inc != inc0) return 3;         // the fold leaves the route's two lists alone
    const int m = smrf_pf_steps(w.data(), route.data(), inc.data(), fold.data(), pattern.data(), n, steps.data());
    if (m < 0 || m > 2 * n) return 4;
    for (int i = 0; i < n; ++i) std::printf("%d ", route[i]);
    for (int i = 0; i < n; ++i) std::printf("%d ", (int)inc[i]);
    for (int i = 0; i < n; ++i) std::printf("%d ", pattern[i]);
    for (int i = 0; i < n; ++i) std::printf("%d ", (int)fold[i]);
    for (int i = 0; i < n; ++i) std::printf("%d ", (int)smrf_pf_runs_inc(inc.data(), fold.data(), i));
    std::printf("%d ", m);
    for (int s = 0; s < m; ++s) {
      const SmrfPfStep& t = steps[s];
      std::printf("%d %d %d %d %d %d %d %d %d ", t.kind, t.win, t.len, t.src, t.aux, t.dst, t.dense, t.closes, t.pattern);
    }
    std::printf("\n");
  }
  return 0;
}
'''


def compile(tmp, extra_flags=(), name="pf_host"):
    src = tmp / "pf_host.cpp"
    src.write_text(MAIN)
    exe = tmp / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall"] + list(extra_flags) + ["-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    return str(exe)


SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def ask(exe, cases):
    """cases: dicts with windows and optionally elem, rows, cells, fused, chain, ero_inc, impl, nan, band, dil_cross -> [Plan]"""
    lines = []
    for c in cases:
        w = [int(v) for v in c["windows"]]
        rows = c.get("rows", 512)
        lines.append(" ".join(str(int(v)) for v in [c.get("elem", 4), c.get("fused", 1), c.get("chain", 1), c.get("ero_inc", 1), c.get("impl", AUTO),
                                                    c.get("nan", 0), c.get("band", 0), c.get("dil_cross", 1), rows, c.get("cells", rows * rows),
                                                    len(w)] + w))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    res = []
    for c, ln in zip(cases, out):
        v, n = [int(x) for x in ln.split()], len(c["windows"])
        m = v[5 * n]
        assert len(v) == 5 * n + 1 + 9 * m
        s = v[5 * n + 1:]
        steps = [Step(*s[9 * j:9 * j + 8]) for j in range(m)]
        for j, t in enumerate(steps):                        # a chain carries its pattern, nothing else carries one
            assert s[9 * j + 8] == (v[2 * n + t.win] if t.kind == CHAIN else -1), (c, t)
        res.append(Plan(v[:n], v[n:2 * n], v[2 * n:3 * n], v[3 * n:4 * n], v[4 * n:5 * n], steps))
    return res


def table(name, path):
    """a 65-entry per-radius table of csrc/<path>"""
    inc = open(os.path.join(CSRC, path)).read()
    v = [int(x) for x in re.search(name + r"\[65\] = \{(.*?)\}", inc, re.S).group(1).replace("\n", " ").split(",")]
    assert len(v) == 65
    return v


def restated(c, route, inc):
    """smrf_pf_fold's rule, independently: (fold, runs_inc)"""
    w, n = [int(v) for v in c["windows"]], len(c["windows"])
    ad, mode = table("kDilCrossAdoptF32", "dil_cross_adopt.inc"), c.get("dil_cross", 1)
    ok = mode != 0 and not c.get("band", 0) and not c.get("nan", 0) and c.get("elem", 4) == 4 and c.get("impl", AUTO) in (AUTO, RING)
    fold = []
    for i in range(n):
        if i and fold[i - 1] == CROSS:
            fold.append(AFTER)
            continue
        take = (ok and i > 0 and route[i] == TWO_PASS and route[i - 1] == TWO_PASS and w[i] == w[i - 1] + 1 and w[i] in RIM_FREE and
                (mode == 2 or (ad[w[i]] and i + 1 < n)))
        fold.append(CROSS if take else NONE)
    return fold, [int(inc[i] and fold[i] == NONE) for i in range(n)]


def route_cases(count, seed):
    """test_pf_route_host.py's sweep: every rule but dil_cross"""
    rnd = random.Random(seed)
    cases = []
    for _ in range(count):
        n = rnd.randint(1, 12)
        if rnd.random() < 0.6:                              # runs of consecutive radii, as real calls have them
            w, r = [], rnd.randint(0, 66)
            while len(w) < n:
                w.append(min(r, 70))
                r = r + 1 if rnd.random() < 0.8 else rnd.randint(0, 70)
        else:
            w = [rnd.randint(0, 70) for _ in range(n)]
        cases.append(dict(elem=rnd.choice((4, 8)), windows=w, rows=rnd.randint(1, 40000), cells=rnd.choice((1, 3 * Mi, 4 * Mi, 16 * Mi, 20 * Mi - 1, 20 * Mi,
                          rnd.randint(1, 1 << 30), 1 << 40)), fused=rnd.choice((0, 1, 1, 2)), chain=rnd.choice((0, 1, 1)), ero_inc=rnd.choice((0, 1, 2)),
                          impl=rnd.choice((AUTO, AUTO, RING, DIRECT_IMPL)), nan=rnd.choice((0, 0, 1)), band=rnd.choice((0, 0, 1, 2))))
    return cases


def fold_cases(seed, count):
    """test_pf_fold_host.py's sweep: runs around the rim-free radii"""
    rng = random.Random(seed)
    cases = []
    for _ in range(count):
        n = rng.randint(0, 12)
        w = []
        while len(w) < n:
            if rng.random() < .6:                            # a run around a rim-free radius
                a = rng.choice(RIM_FREE) - rng.randint(0, 3)
                w += list(range(a, a + rng.randint(1, 5)))
            else:
                w.append(rng.choice([0, 1, 2, 3, 5, 9, 14, 15, 16, 21, 36, 64, 65, 70]))
        rows = rng.choice([12, 300, 5000])
        cases.append(dict(windows=w[:n], elem=rng.choice([4, 4, 4, 8]), fused=rng.choice([0, 1, 2]), chain=rng.choice([0, 1]),
                          ero_inc=rng.choice([0, 1, 2]), impl=rng.choice([AUTO, AUTO, RING, DIRECT_IMPL]), nan=int(rng.random() < .2),
                          band=rng.choice([0, 0, 0, 1, 2]), dil_cross=rng.choice([0, 1, 2, 2]), rows=rows, cells=rows * rng.choice([40, 300, 5000])))
    return cases


def chain_lengths(route):
    """per window the length of the chained launch that starts there (0: none), read off the positions a route list reports"""
    out = [0] * len(route)
    for i, r in enumerate(route):
        if r == CH:
            k = 1
            while i + k < len(route) and route[i + k] == CH + k:
                k += 1
            out[i] = k
    return out


def parent_steps(windows, route, inc, fold, pattern_len=None):
    """The loop of progressive_filter_api as it stood before smrf_pf_steps, launch for launch: pe (the plane of the latest erosion)
    starts at 0, pl (the plane of `last`, -1 = Z) at -1, a launch writes into spare() = the lowest plane that is neither, and the
    five cases move pe and pl as that loop did."""
    n = len(windows)
    pattern_len = chain_lengths(route) if pattern_len is None else pattern_len
    pe, pl, steps, i = 0, -1, [], 0
    while i < n:
        po = min(k for k in range(3) if k != pe and k != pl)
        if route[i] == CH:                                   # windows i .. i + len - 1 in one launch
            ln = pattern_len[i]
            steps.append(Step(CHAIN, i, ln, pl, NO_PLANE, po, int(i == 0), 1))
            pl = po
            i += ln
            continue
        if route[i] == FUSED:
            steps.append(Step(FUSED_OPEN, i, 1, pl, NO_PLANE, po, int(i == 0), 1))
            pl = po
        elif fold[i] == CROSS:                               # no erosion: the dilation reads e_{R-1} in P[pe], which stays
            steps.append(Step(DILATE_CROSS, i, 1, pe, pl, po, 0, 1))
            pl = po
        elif inc[i] and fold[i] == NONE:                     # e_R into the spare plane, opened_R over e_{R-1}
            steps.append(Step(INC_ERODE, i, 1, pe, pl, po, 0, 0))
            steps.append(Step(DILATE, i, 1, po, pl, pe, 0, 1))
            pl, pe = pe, po
        else:
            steps.append(Step(ERODE, i, 1, pl, NO_PLANE, pe, 0, 0))
            steps.append(Step(DILATE, i, 1, pe, pl, po, int(i == 0), 1))
            pl = po
        i += 1
    return steps


def replay(windows, route, fold, steps):
    """The steps on three planes that hold labels instead of cells ("junk", ("e", i), ("o", i); plane -1 is "Z"): every launch reads
    what its kind must read and never what it writes or what nothing wrote, the windows close once each and in order, and the
    workspace ends as the callers of a whole-raster call find it.  Returns the three labels."""
    n = len(windows)
    planes = ["junk"] * 3
    at = lambda k: "Z" if k == PLANE_Z else planes[k]       # noqa: E731
    last, nxt, eroded_yet = "Z", 0, False
    assert len(steps) <= 2 * n
    for j, t in enumerate(steps):
        i = t.win
        assert i == nxt and t.dst in (0, 1, 2) and t.dst not in (t.src, t.aux), (j, t)
        assert t.len == (chain_lengths(route)[i] if t.kind == CHAIN else 1) and t.closes == int(t.kind not in (ERODE, INC_ERODE)), (j, t)
        assert t.dense == int(t.closes and i == 0), (j, t)
        if t.kind in (CHAIN, FUSED_OPEN, ERODE):
            assert t.aux == NO_PLANE and at(t.src) == last, (j, t, planes)
        else:
            assert t.src in (0, 1, 2) and at(t.aux) == last, (j, t, planes)
            assert at(t.src) == ("e", i if t.kind == DILATE else i - 1), (j, t, planes)
        assert "junk" not in (at(t.src), "" if t.aux == NO_PLANE else at(t.aux)), (j, t, planes)
        assert (t.kind == DILATE_CROSS) == (t.closes and fold[i] == CROSS), (j, t)
        if t.kind in (ERODE, INC_ERODE):
            eroded_yet = True
            assert j + 1 < len(steps) and steps[j + 1].kind == DILATE and steps[j + 1].win == i, (j, t)
            planes[t.dst] = ("e", i)
        else:
            assert eroded_yet or t.dst != 0, (j, t, "plane 0 holds the NaN flag of a speculative first launch until the first erosion")
            planes[t.dst] = last = ("o", i + t.len - 1)
            nxt += t.len
    assert nxt == n
    if steps and steps[0].kind == CHAIN:
        assert steps[0].src == PLANE_Z and steps[0].dst != 0
    if n:
        assert ("o", n - 1) in planes
        if fold[n - 1] == CROSS:
            assert n >= 2 and sorted(planes) == [("e", n - 2), ("o", n - 2), ("o", n - 1)]
        elif route[n - 1] in (TWO_PASS, DIRECT, COPY):
            assert ("e", n - 1) in planes
    return planes
