"""csrc/pf_route.h, smrf_pf_fold - which two-pass windows take their erosion inside their dilation pass (cross on load) - asked through
the stand-alone program of tests/pf_host.py (no GPU), also under the address and undefined-behaviour sanitizers: the benchmark
plan, the eligibility edges, "no incremental erosion after a folded window", and the invariants of any plan over random window
lists against the rule restated in pf_host.py."""
import os
import re

import pytest

import pf_host
from pf_host import AFTER, AUTO, CH, CROSS, CSRC, DIRECT_IMPL, FUSED, NONE, RIM_FREE, RING, TWO_PASS, restated, table
from pf_host import fold_cases as random_cases


def ask(exe, cases):
    """cases: dicts with windows and optionally elem, rows, cells, fused, chain, ero_inc, impl, nan, band, dil_cross
    -> [(route, inc, fold, runs_inc)]"""
    return [(p.route, p.inc, p.fold, p.runs) for p in pf_host.ask(exe, cases)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pf_host.compile(tmp_path_factory.mktemp("pf_fold"))


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
    san = pf_host.compile(tmp_path, pf_host.SANITIZE, "fold_san")
    plain = pf_host.compile(tmp_path, name="fold_plain")
    cases = random_cases(77, 300) + [dict(windows=[], dil_cross=2), dict(windows=[16], dil_cross=2), dict(windows=[15, 16], dil_cross=2),
                                     dict(windows=list(range(1, 51)), rows=16384)]
    res = ask(san, cases)
    assert res == ask(plain, cases)
    check_invariants(cases, res)
