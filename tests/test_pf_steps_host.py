"""csrc/pf_route.h, smrf_pf_steps - the launches of a whole-raster progressive_filter call, each with the workspace planes it reads
and writes - asked through the stand-alone program of tests/pf_host.py (no GPU), also under the address and undefined-behaviour
sanitizers.  Two independent statements: the plane rotation of the driver's former loop, restated in Python
(pf_host.parent_steps: the same planes as before), and a replay on labelled planes (pf_host.replay: every launch reads the
surface its kind needs, never writes what it reads, and the workspace ends with the surfaces the GPU tests read there)."""
import pytest

import pf_host
from pf_host import CHAIN, CROSS, DILATE, DILATE_CROSS, ERODE, FUSED_OPEN, INC_ERODE, NO_PLANE, PATTERNS, PLANE_Z, Step, TWO_PASS
from window_cases import LISTS as ROTATION_LISTS, WINDOW_LISTS as DIL_CROSS_LISTS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pf_host.compile(tmp_path_factory.mktemp("pf_steps"))


def sweep():
    """the benchmark list, the window lists of the GPU tests of the cross on load and of the plane rotation at their rasters' sizes
    under every value of the three switches, and 600 random cases of each of the two generators"""
    bench = dict(windows=range(1, 51), rows=16384)
    cases = [bench, dict(bench, ero_inc=2), dict(bench, dil_cross=2), dict(bench, ero_inc=2, dil_cross=2), dict(bench, ero_inc=0, dil_cross=0)]
    for lists, rows, cols in ((DIL_CROSS_LISTS, 97, 257), (ROTATION_LISTS, 120, 400)):
        cases += [dict(windows=w, rows=rows, cells=rows * cols, fused=fused, ero_inc=inc, dil_cross=cross)
                  for w in lists for fused in (1, 0, 2) for inc in (0, 1, 2) for cross in (0, 1, 2)]
    cases += [dict(c, dil_cross=k % 3) for k, c in enumerate(pf_host.route_cases(600, 5))] + pf_host.fold_cases(6, 600)
    return cases


def check(cases, plans):
    kinds = set()
    for c, p in zip(cases, plans):
        w, n = list(c["windows"]), len(c["windows"])
        lengths = [len(PATTERNS[q][0]) if q >= 0 else 0 for q in p.pattern]
        assert lengths == pf_host.chain_lengths(p.route), (c, p)
        assert p.steps == pf_host.parent_steps(w, p.route, p.inc, p.fold, lengths), (c, p)
        planes = pf_host.replay(w, p.route, p.fold, p.steps)
        # the fold and the incremental erosion, read off the steps
        closing = {t.win: t.kind for t in p.steps if t.closes}
        for i in range(n):
            if p.route[i] <= pf_host.CH:                     # (the later windows of a chain close with its head)
                assert (closing[i] == DILATE_CROSS) == (p.fold[i] == CROSS), (c, p)
            assert any(t.kind == INC_ERODE and t.win == i for t in p.steps) == bool(p.runs[i]), (c, p)
        # under the table the last window is never folded: a last two-pass window leaves its erosion
        if n and c.get("dil_cross", 1) == 1:
            assert p.fold[n - 1] != CROSS
            if p.route[n - 1] == TWO_PASS:
                assert ("e", n - 1) in planes, (c, p)
        kinds |= {t.kind for t in p.steps}
    return kinds


def test_the_steps_are_the_former_loop_and_replay_soundly(exe):
    cases = sweep()
    plans = pf_host.ask(exe, cases)
    assert check(cases, plans) == {CHAIN, FUSED_OPEN, ERODE, INC_ERODE, DILATE, DILATE_CROSS}
    assert sum(any(t.kind == DILATE_CROSS for t in p.steps) for p in plans) > 100
    assert sum(any(t.kind == INC_ERODE for t in p.steps) for p in plans) > 100
    assert sum(bool(p.steps) and p.steps[0].kind == CHAIN for p in plans) >= 5        # (the benchmark lists alone are five)


def test_benchmark_steps(exe):
    """16384^2 fp32, windows 1..50, default switches: 7 chained launches, 4 fused openings, then 36 two-pass windows of which 16 and
    21 are one launch (cross on load) and the others two - 81 launches; the speculative first launch writes plane 1"""
    (p,) = pf_host.ask(exe, [dict(windows=range(1, 51), rows=16384)])
    kinds = [t.kind for t in p.steps]
    assert kinds[:11] == [CHAIN] * 7 + [FUSED_OPEN] * 4 and len(kinds) == 11 + 2 * 34 + 2
    assert [t.win + 1 for t in p.steps if t.kind == DILATE_CROSS] == [16, 21]
    assert [t.win for t in p.steps if t.kind == INC_ERODE] == [i for i in range(50) if p.runs[i]]
    assert p.steps[0] == Step(CHAIN, 0, 3, PLANE_Z, NO_PLANE, 1, 1, 1) and p.steps[1] == Step(CHAIN, 3, 2, 1, NO_PLANE, 2, 0, 1)
    assert all(t.dst != 0 for t in p.steps[:11]) and p.steps[11] == Step(ERODE, 14, 1, 1, NO_PLANE, 0, 0, 0)


def test_empty_and_degenerate_lists(exe):
    none, copy, direct, alone, fused, chain = pf_host.ask(exe, [dict(windows=[], dil_cross=2), dict(windows=[0]), dict(windows=[70]),
                                                               dict(windows=[16], dil_cross=2, ero_inc=2), dict(windows=[3]), dict(windows=[1, 2, 3])])
    assert none.steps == []
    two = [Step(ERODE, 0, 1, PLANE_Z, NO_PLANE, 0, 0, 0), Step(DILATE, 0, 1, 0, PLANE_Z, 1, 1, 1)]
    assert copy.route == [pf_host.COPY] and direct.route == [pf_host.DIRECT] and alone.route == [TWO_PASS]
    assert copy.steps == two and direct.steps == two and alone.steps == two
    assert fused.steps == [Step(FUSED_OPEN, 0, 1, PLANE_Z, NO_PLANE, 1, 1, 1)]
    assert chain.steps == [Step(CHAIN, 0, 3, PLANE_Z, NO_PLANE, 1, 1, 1)]
    for c, p in zip(([], [0], [70], [16], [3], [1, 2, 3]), (none, copy, direct, alone, fused, chain)):
        pf_host.replay(c, p.route, p.fold, p.steps)


def test_under_the_sanitizers(exe, tmp_path):
    """the same program built with -fsanitize=address,undefined (step buffers of exactly 2n entries), on the edges and a random
    sweep: no report, same answers"""
    san = pf_host.compile(tmp_path, pf_host.SANITIZE, "steps_san")
    cases = pf_host.fold_cases(78, 300) + [dict(windows=[], dil_cross=2), dict(windows=[0]), dict(windows=[70]), dict(windows=[16], dil_cross=2),
                                           dict(windows=[15, 16], dil_cross=2, ero_inc=2), dict(windows=list(range(1, 51)), rows=16384)]
    res = pf_host.ask(san, cases)
    assert res == pf_host.ask(exe, cases)
    check(cases, res)
