"""csrc/pf_route.h, smrf_pf_fold - which two-pass windows take their erosion inside their dilation pass (cross on load) - compiled
with g++ as a stand-alone program and asked directly (no GPU), also under the address and undefined-behaviour sanitizers: the
benchmark plan, the eligibility edges, "no incremental erosion after a folded window", and the invariants of any plan over
random window lists against the rule restated here."""
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neilpy_amd", "csrc")
TWO_PASS, FUSED, DIRECT, COPY, CH = 0, 1, 2, 3, 4
AUTO, RING, DIRECT_IMPL = 0, 1, 2
NONE, CROSS, AFTER = 0, 1, 2
RIM_FREE = (16, 21, 36)                                   # the radii from 15 up whose leftover set P_R is empty (ero_inc.inc)

_MAIN = r'''
#include <cstdio>
#include <vector>
#include "pf_route.h"
// one case per line: elem_size fused chain ero_inc impl nan_aware band dil_cross rows cells n w[0] .. w[n-1]
// -> one line: n routes, n incremental-erosion flags of the route, n fold values, n "runs the incremental erosion"
int main() {
  SmrfPfRules k;
  int rows, n;
  long long cells;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %lld %d", &k.elem_size, &k.fused, &k.chain, &k.ero_inc, &k.impl, &k.nan_aware,
                    &k.band, &k.dil_cross, &rows, &cells, &n) == 11) {
    // exactly n entries each, so that the sanitizer build sees any access beyond them
    std::vector<int32_t> w(n), route(n, -99);
    std::vector<uint8_t> inc(n, 99), fold(n, 99);
    for (int i = 0; i < n; ++i)
      if (std::scanf("%d", &w[i]) != 1) return 2;
    smrf_pf_route(k, w.data(), n, rows, cells, route.data(), inc.data());
    const std::vector<int32_t> route0 = route;
    const std::vector<uint8_t> inc0 = inc;
    smrf_pf_fold(k, w.data(), route.data(), inc.data(), n, fold.data());
    if (route != route0 || inc != inc0) return 3;         // the fold leaves the route's two lists alone
    for (int i = 0; i < n; ++i) std::printf("%d ", route[i]);
    for (int i = 0; i < n; ++i) std::printf("%d ", (int)inc[i]);
    for (int i = 0; i < n; ++i) std::printf("%d ", (int)fold[i]);
    for (int i = 0; i < n; ++i) std::printf("%d ", (int)smrf_pf_runs_inc(inc.data(), fold.data(), i));
    std::printf("\n");
  }
  return 0;
}
'''


def _compile(tmp, name, extra):
    src = tmp / "fold.cpp"
    src.write_text(_MAIN)
    exe = tmp / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall"] + extra + ["-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    return str(exe)


def ask(exe, cases):
    """cases: dicts with windows and optionally elem, rows, cells, fused, chain, ero_inc, impl, nan, band, dil_cross
    -> [(route, inc, fold, runs_inc)]"""
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
        assert len(v) == 4 * n
        res.append((v[:n], v[n:2 * n], v[2 * n:3 * n], v[3 * n:]))
    return res


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("pf_fold"), "fold", [])


def table(name, path):
    inc = open(os.path.join(CSRC, path)).read()
    v = [int(x) for x in re.search(name + r"\[65\] = \{(.*?)\}", inc, re.S).group(1).replace("\n", " ").split(",")]
    assert len(v) == 65
    return v


def adopted():
    return table("kDilCrossAdoptF32", "dil_cross_adopt.inc")


def test_the_radii_with_an_instance_are_the_rim_free_ones():
    """ero_inc.inc: the radii from the first two-pass window up whose P_R is empty, and the table adopts nothing else"""
    text = open(os.path.join(CSRC, "ero_inc.inc")).read()
    rows = re.findall(r"^    \{(\d+), (\d+), \{", text[text.index("kEroInc[65]"):], re.M)
    assert len(rows) == 65
    assert tuple(r for r in range(15, 65) if int(rows[r][0]) == 0) == RIM_FREE
    assert all(not a or r in RIM_FREE for r, a in enumerate(adopted()))


def test_benchmark_plan(exe):
    """16384^2 fp32, windows 1..50: the route and its incremental-erosion flags are the parent's; the windows the table adopts fold,
    the window after each runs the ring erosion, and every other window runs what the route says"""
    bench = dict(windows=range(1, 51), rows=16384)
    (route, inc, fold, runs), (_, inc2, fold2, runs2), (_, inc0, fold0, runs0), (_, _, foldx, runsx) = ask(
        exe, [bench, dict(bench, dil_cross=2, ero_inc=2), dict(bench, dil_cross=0), dict(bench, dil_cross=2, ero_inc=0)])
    assert route == [CH, CH + 1, CH + 2, CH, CH + 1, CH, CH, CH, CH, CH] + [FUSED] * 4 + [TWO_PASS] * 36
    ero_adopt = table("kEroIncAdoptF32", "ero_inc_adopt.inc")
    assert inc == [int(r >= 16 and ero_adopt[r]) for r in range(1, 51)] and inc0 == inc
    ad = adopted()
    for r in range(1, 51):
        i = r - 1
        want = CROSS if r in RIM_FREE and ad[r] else AFTER if r - 1 in RIM_FREE and ad[r - 1] else NONE
        assert fold[i] == want, (r, fold)
        assert runs[i] == int(inc[i] and want == NONE)
        assert fold2[i] == (CROSS if r in RIM_FREE else AFTER if r - 1 in RIM_FREE else NONE)
        assert runs2[i] == int(r >= 16 and fold2[i] == NONE)     # SMRF_ERO_INC=2: every window from 16 up but the folded ones and their successors
    assert fold0 == [NONE] * 50 and runs0 == inc0
    assert foldx == fold2 and runsx == [0] * 50


def test_eligibility_edges(exe):
    f = lambda **k: ask(exe, [dict(dil_cross=2, **k)])[0][2]          # noqa: E731
    assert f(windows=[15, 16]) == [NONE, CROSS]
    assert f(windows=[20, 21]) == [NONE, CROSS]
    assert f(windows=[14, 15, 16, 17], fused=0) == [NONE, NONE, CROSS, AFTER]
    assert f(windows=[14, 15, 16, 17]) == [NONE, NONE, CROSS, AFTER]                  # (on a raster this small 14 is a two-pass window as well)
    assert f(windows=[35, 36, 37]) == [NONE, CROSS, AFTER]
    # not taken
    assert f(windows=[16]) == [NONE]                                                   # no window before it
    assert f(windows=[19, 21]) == [NONE, NONE]                                         # not the previous radius + 1
    assert f(windows=[21, 21]) == [NONE, NONE] and f(windows=[22, 21]) == [NONE, NONE]
    assert f(windows=[15, 16], nan=1) == [NONE, NONE]
    assert f(windows=[15, 16], elem=8) == [NONE, NONE]
    assert f(windows=[15, 16], impl=DIRECT_IMPL) == [NONE, NONE]
    assert f(windows=[15, 16], impl=RING) == [NONE, CROSS]
    assert f(windows=[15, 16], band=1) == [NONE, NONE] and f(windows=[15, 16], band=2) == [NONE, NONE]
    assert f(windows=[16, 17, 18, 19, 20]) == [NONE] * 5                               # P_R is not empty
    assert f(windows=[11, 12], fused=0) == [NONE, NONE]                                # rim-free, but no instance below 16
    assert f(windows=[1, 2, 3, 16]) == [NONE] * 4                                      # the window before is no two-pass window
    assert ask(exe, [dict(windows=[15, 16], dil_cross=0)])[0][2] == [NONE, NONE]
    # SMRF_ERO_INC does not matter to the fold
    for mode in (0, 1, 2):
        assert f(windows=[20, 21, 22], ero_inc=mode) == [NONE, CROSS, AFTER]


def test_the_table_keeps_the_last_window_on_its_erosion(exe):
    """SMRF_DIL_CROSS=1 folds an adopted radius only when a window follows: the workspace ends with the last window's eroded and
    opened surfaces, as tests/test_gpu_incero_edges.py reads them; SMRF_DIL_CROSS=2 folds the last window too"""
    ad = adopted()
    for r in RIM_FREE:
        one, two = ask(exe, [dict(windows=[r - 1, r], dil_cross=1, ero_inc=2), dict(windows=[r - 1, r, r + 1], dil_cross=1, ero_inc=2)])
        assert one[2] == [NONE, NONE] and one[3] == [0, 1]
        if ad[r]:
            assert two[2] == [NONE, CROSS, AFTER] and two[3] == [0, 0, 0]
        else:
            assert two[2] == [NONE, NONE, NONE] and two[3] == [0, 1, 1]


def test_no_incremental_erosion_after_a_folded_window(exe):
    (route, inc, fold, runs), = ask(exe, [dict(windows=[35, 36, 37, 38], dil_cross=2, ero_inc=2)])
    assert inc == [0, 1, 1, 1]                            # the route's flags, as smrf_pf_plan reports them
    assert fold == [NONE, CROSS, AFTER, NONE] and runs == [0, 0, 0, 1]


def restated(c, route, inc):
    """the rule, independently: (fold, runs_inc)"""
    w, n = [int(v) for v in c["windows"]], len(c["windows"])
    ad, mode = adopted(), c.get("dil_cross", 1)
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


def random_cases(seed, count):
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


def check_invariants(cases, res):
    for c, (route, inc, fold, runs) in zip(cases, res):
        w, n = c["windows"], len(c["windows"])
        assert (fold, runs) == restated(c, route, inc), c
        for i in range(n):
            assert fold[i] in (NONE, CROSS, AFTER)
            if fold[i] == CROSS:
                assert i > 0 and fold[i - 1] != CROSS and route[i] == route[i - 1] == TWO_PASS and w[i] == w[i - 1] + 1 and w[i] in RIM_FREE
                assert c.get("elem", 4) == 4 and not c.get("nan", 0) and not c.get("band", 0) and c.get("impl", AUTO) != DIRECT_IMPL and c.get("dil_cross", 1)
            assert (fold[i] == AFTER) == (i > 0 and fold[i - 1] == CROSS)
            assert not (runs[i] and fold[i] != NONE) and not (runs[i] and not inc[i])
            if runs[i]:                                      # the incremental erosion starts from the previous window's erosion: it exists
                assert fold[i - 1] != CROSS


def test_invariants_over_random_window_lists(exe):
    cases = random_cases(2024, 600)
    res = ask(exe, cases)
    check_invariants(cases, res)
    assert sum(CROSS in r[2] for r in res) > 40 and sum(any(r[3]) for r in res) > 40


def test_under_the_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, on the edges and a random sweep: no report, same answers"""
    san = _compile(tmp_path, "fold_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    plain = _compile(tmp_path, "fold_plain", [])
    cases = random_cases(77, 300) + [dict(windows=[], dil_cross=2), dict(windows=[16], dil_cross=2), dict(windows=[15, 16], dil_cross=2),
                                     dict(windows=list(range(1, 51)), rows=16384)]
    res = ask(san, cases)
    assert res == ask(plain, cases)
    check_invariants(cases, res)
