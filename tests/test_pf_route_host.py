"""csrc/pf_route.h - which launch every window of progressive_filter takes - asked through the stand-alone program of
tests/pf_host.py (no GPU): the route lists the GPU tests observe, the size thresholds, the invariants of any plan over a random sweep (also under the
address and undefined-behaviour sanitizers), and the row-band form against the band rule the driver used to restate."""
import ctypes as C
import os

import numpy as np
import pytest

import pf_host
from pf_host import AUTO, CH, COPY, DIRECT, DIRECT_IMPL, FUSED, PATTERNS, RING, TWO_PASS, Mi
from pf_host import route_cases as _random_cases


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = pf_host.compile(tmp_path_factory.mktemp("pf_route"))

    def plans(cases, exe=exe):
        """cases: dicts with elem, windows, rows, cells and optionally fused, chain, ero_inc, impl, nan, band -> [(route, inc, pattern)]"""
        return [(p.route, p.inc, p.pattern) for p in pf_host.ask(exe, cases)]
    return plans


def adopted_radii():
    return pf_host.table("kEroIncAdoptF32", "ero_inc_adopt.inc")


def test_route_lists_the_gpu_tests_observe(planner):
    """the route lists tests/test_gpu_w50.py asserts (test_window_routes, test_window_routes_f64), same switches, no device"""
    f32 = dict(elem=4, windows=range(1, 17), rows=512, cells=512 * 512)
    f64 = dict(elem=8, windows=range(1, 11), rows=384, cells=384 * 384)
    got = [p[0] for p in planner([f32, dict(f32, fused=2), dict(f32, fused=2, chain=0), dict(f32, fused=0, chain=0),
                                  f64, dict(f64, fused=2), dict(f64, fused=0), dict(f32, fused=0)])]
    assert got[7] == [TWO_PASS] * 16
    assert got[0] == [CH, CH + 1, CH + 2, CH, CH, CH, CH, CH, CH] + [TWO_PASS] * 7
    assert got[1] == [CH, CH + 1, CH + 2, CH, CH + 1, CH, CH, CH, CH, CH] + [FUSED] * 4 + [TWO_PASS] * 2
    assert got[2] == [FUSED] * 8 + [TWO_PASS] + [FUSED] * 5 + [TWO_PASS] * 2
    assert got[3] == [TWO_PASS] * 16
    assert got[4] == [CH, CH + 1, CH + 2, CH, CH, FUSED] + [TWO_PASS] * 4
    assert got[5] == [CH, CH + 1, CH + 2, CH, CH, FUSED, CH, CH] + [TWO_PASS] * 2
    assert got[6] == [TWO_PASS] * 10


def test_benchmark_plan(planner):
    """16384^2 fp32, windows 1..50, default switches: chains 1, 2, 3 and 4, 5, singles 6..10, fused 11..14, two passes from 15, and
    the incremental erosion exactly where ero_inc_adopt.inc adopts the radius, from 16 up (15 is the first two-pass window)"""
    bench = dict(elem=4, windows=range(1, 51), rows=16384, cells=16384 * 16384)
    (route, inc, pat), (route2, inc2, _), (route0, inc0, _) = planner([bench, dict(bench, ero_inc=2), dict(bench, ero_inc=0)])
    want = [CH, CH + 1, CH + 2, CH, CH + 1, CH, CH, CH, CH, CH] + [FUSED] * 4 + [TWO_PASS] * 36
    assert route == want and route2 == want and route0 == want
    adopt = adopted_radii()
    assert inc == [int(r >= 16 and adopt[r]) for r in range(1, 51)] and sum(inc) == 23
    assert inc2 == [int(r >= 16) for r in range(1, 51)] and inc0 == [0] * 50
    assert pat == [0, -1, -1, 3, -1, 6, 7, 8, 9, 10] + [-1] * 40


def test_chain_size_thresholds_as_plans(planner):
    """every case of test_abi.py's test_chain_length_size_thresholds, as the head of a plan"""
    cases = [(4, [1, 2, 3, 4], 1 * Mi, 3), (4, [2, 3, 4], 1 * Mi, 2), (4, [1, 2, 4], Mi, 2), (4, [4, 5, 6], 16 * Mi, 1), (4, [4, 5, 6], 24 * Mi, 2),
             (4, [9, 10], 1 * Mi, 1), (4, [10, 11], 16 * Mi, 0), (4, [10, 11], 24 * Mi, 1), (4, [11], 1 << 40, 0), (4, [6], 1, 1),
             (8, [1, 2, 3], 1 * Mi, 3), (8, [5], 1 * Mi, 1), (8, [4, 5], 1 << 40, 1), (8, [7], 2 * Mi, 0), (8, [7], 4 * Mi, 1),
             (8, [8], 8 * Mi, 0), (8, [8], 16 * Mi, 1), (8, [6], 1 << 40, 0), (8, [9], 1 << 40, 0)]
    got = planner([dict(elem=e, windows=w, rows=40000, cells=c) for e, w, c, _ in cases])
    for (e, w, c, n), (route, _, _) in zip(cases, got):
        head = 0
        while head < len(w) and route[head] == CH + head:
            head += 1
        assert head == n, (e, w, c, route)


def test_routes_without_small_disk_kernels(planner):
    """a raster with NaNs and impl = direct take no chained, fused or incremental launch; radius 0 copies; radius 65 is beyond the
    ring kernels; a raster with no more rows than a chain's halo takes no chain"""
    bench = dict(elem=4, windows=range(1, 51), rows=16384, cells=16384 * 16384, ero_inc=2, fused=2)
    nan, direct, ring = planner([dict(bench, nan=1), dict(bench, impl=DIRECT_IMPL), dict(bench, impl=RING)])
    assert nan[0] == [TWO_PASS] * 50 and nan[1] == [0] * 50 and nan[2] == [-1] * 50
    assert direct[0] == [DIRECT] * 50 and direct[1] == [0] * 50 and direct[2] == [-1] * 50
    assert ring[0][:14] == [CH, CH + 1, CH + 2, CH, CH + 1, CH, CH, CH, CH, CH] + [FUSED] * 4 and ring[1] == [0] * 15 + [1] * 35
    small = dict(elem=4, rows=3000, cells=3000 * 3000)
    (r0, i0, _), (r65, i65, _), (rd, _, _) = planner([dict(small, windows=[0, 1, 0, 20, 21]), dict(small, windows=[63, 64, 65, 66], ero_inc=2),
                                                      dict(small, windows=[0, 65], impl=DIRECT_IMPL)])
    assert r0 == [COPY, FUSED, COPY, TWO_PASS, TWO_PASS] and i0 == [0, 0, 0, 0, 1]      # (no table-free single below radius 4)
    assert r65 == [TWO_PASS, TWO_PASS, DIRECT, DIRECT] and i65 == [0, 1, 0, 0]
    assert rd == [COPY, DIRECT]
    # halo rows = sum(2R): 10 for 2, 3, 8 for the single 4, 12 for 1, 2, 3 (on 12 rows window 1 runs alone, then 2, 3 chain: halo 10)
    got = [p[0] for p in planner([dict(elem=4, windows=[2, 3], rows=10, cells=10 * 600), dict(elem=4, windows=[2, 3], rows=11, cells=11 * 600),
                                  dict(elem=8, windows=[4], rows=8, cells=8 * 600), dict(elem=8, windows=[4], rows=9, cells=9 * 600),
                                  dict(elem=4, windows=[1, 2, 3], rows=12, cells=12 * 600), dict(elem=4, windows=[1, 2, 3], rows=13, cells=13 * 600),
                                  dict(elem=4, windows=[2, 3], rows=10, cells=1 << 40, band=1)])]
    assert got == [[FUSED] * 2, [CH, CH + 1], [FUSED], [CH], [FUSED, CH, CH + 1], [CH, CH + 1, CH + 2], [FUSED] * 2]


def _check_invariants(c, route, inc, pat):
    w, n = list(c["windows"]), len(c["windows"])
    i = 0
    while i < n:                                            # every window exactly one route; chains whole, in table order
        if route[i] >= CH:
            assert route[i] == CH and 0 <= pat[i] < len(PATTERNS), (c, route, pat)
            radii, min32, min64 = PATTERNS[pat[i]]
            assert tuple(w[i:i + len(radii)]) == radii and route[i:i + len(radii)] == [CH + k for k in range(len(radii))], (c, route)
            assert pat[i + 1:i + len(radii)] == [-1] * (len(radii) - 1)
            mc = min64 if c["elem"] == 8 else min32
            assert mc is not None and (c["fused"] == 2 or c["cells"] >= mc) and sum(2 * r for r in radii) < c["rows"], (c, route)
            assert not c["nan"] and c["impl"] != DIRECT_IMPL and c["fused"] and c["chain"] and c["band"] != 2, (c, route)
            i += len(radii)
            continue
        assert route[i] in (TWO_PASS, FUSED, DIRECT, COPY) and pat[i] == -1, (c, route, pat)
        if route[i] == FUSED:
            assert not c["nan"] and c["impl"] != DIRECT_IMPL and c["fused"] and 1 <= w[i] <= 14, (c, route)
            assert not c["band"] or w[i] <= 8, (c, route)
        if route[i] == COPY:
            assert w[i] == 0
        if route[i] == DIRECT:
            assert c["impl"] == DIRECT_IMPL or (c["impl"] == AUTO and w[i] > 64), (c, route)
        if route[i] == TWO_PASS:
            assert w[i] >= 1 and (c["impl"] == RING or (c["impl"] == AUTO and w[i] <= 64)), (c, route)
        i += 1
    for i in range(n):
        assert inc[i] in (0, 1)
        if inc[i]:
            assert i > 0 and route[i] == TWO_PASS and route[i - 1] == TWO_PASS and w[i] == w[i - 1] + 1, (c, route, inc)
            assert not c["band"] and not c["nan"] and c["ero_inc"] and c["elem"] == 4 and 16 <= w[i] <= 64, (c, route, inc)
    if c["band"]:
        assert not any(inc)


def test_plan_invariants_random_and_sanitized(planner, tmp_path):
    """3000 random questions (dtype, 1..12 windows in 0..70, rows 1..40000, cells, every switch value, impl, nan_aware, band): every
    window gets one route, chain positions run 0..len-1 over a table pattern that exists at this dtype and size, the incremental
    erosion only after a two-pass window of the previous radius, bands take no fused opening above radius 8 and no incremental
    erosion.  The same sweep through a build with -fsanitize=address,undefined (output buffers of exactly n entries) gives the
    same plans and no report."""
    cases = _random_cases(3000, 11)
    got = planner(cases)
    for c, (route, inc, pat) in zip(cases, got):
        _check_invariants(c, route, inc, pat)
    kinds = {r for route, _, _ in got for r in route}
    assert {TWO_PASS, FUSED, DIRECT, COPY, CH, CH + 1, CH + 2} <= kinds and any(any(inc) for _, inc, _ in got)
    san = pf_host.compile(tmp_path, pf_host.SANITIZE, "plan_san")
    assert planner(cases, exe=san) == got


def test_band_plan_equals_the_old_band_rule():
    """The row-band driver (neilpy_amd/sharded.py) now asks smrf_pf_plan(band = 1) for the launch at the head of a group.  Under
    default switches that is what it used to work out itself from the two entries that remain: smrf_pf_chain_length, a chain
    whose halo is not shorter than the image refused, otherwise the fused opening for 1 <= r <= 8 where
    smrf_fused_open_supported, otherwise two passes.  Both dtypes, head radii 1..16 with 0..3 followers, five sizes either side of
    every threshold, an image longer and one shorter than the halos."""
    from neilpy_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from neilpy_amd.build import build
        build(verbose=False)
    lib = _lib.load()
    names = ("SMRF_FUSED", "SMRF_CHAIN", "SMRF_ERO_INC")
    saved = {k: os.environ.pop(k, None) for k in names}
    _lib.reload_switches()
    try:
        count = 0
        for elem in (4, 8):
            for head in range(1, 17):
                for followers in range(4):
                    radii = np.arange(head, head + followers + 1, dtype=np.int32)
                    for cells in (1 * Mi, 4 * Mi, 16 * Mi, 20 * Mi, 24 * Mi):
                        for img_rows in (4096, 10):
                            k = lib.smrf_pf_chain_length(elem, radii.ctypes.data_as(C.c_void_p), len(radii), cells)
                            if k >= 1 and sum(2 * int(r) for r in radii[:k]) >= img_rows:
                                k = 0
                            if k >= 1:
                                want = [CH + j for j in range(k)]
                            elif 1 <= head <= 8 and lib.smrf_fused_open_supported(elem, head):
                                want = [FUSED]
                            else:
                                want = [TWO_PASS]
                            route = np.full(len(radii), -1, dtype=np.int32)
                            inc = np.full(len(radii), 9, dtype=np.uint8)
                            _lib.check(lib.smrf_pf_plan(elem, radii.ctypes.data_as(C.c_void_p), len(radii), img_rows, cells, 0, AUTO, 1,
                                                        route.ctypes.data_as(C.c_void_p), inc.ctypes.data_as(C.c_void_p)))
                            got = [int(v) for v in route]
                            assert got[:len(want)] == want and (len(got) == len(want) or got[len(want)] != CH + len(want)), (elem, radii, cells, img_rows, got, want)
                            assert not inc.any()
                            count += 1
        assert count == 2 * 16 * 4 * 5 * 2
        # band = 2 (no chained launch): the same fused rule, never a chain; bad questions are refused
        radii = np.arange(1, 11, dtype=np.int32)
        route = np.zeros(10, dtype=np.int32)
        inc = np.zeros(10, dtype=np.uint8)
        _lib.check(lib.smrf_pf_plan(4, radii.ctypes.data_as(C.c_void_p), 10, 4096, 24 * Mi, 0, AUTO, 2, route.ctypes.data_as(C.c_void_p),
                                    inc.ctypes.data_as(C.c_void_p)))
        assert [int(v) for v in route] == [FUSED] * 8 + [TWO_PASS] * 2
        assert lib.smrf_pf_plan(4, radii.ctypes.data_as(C.c_void_p), 10, 4096, 24 * Mi, 0, AUTO, 3, route.ctypes.data_as(C.c_void_p),
                                inc.ctypes.data_as(C.c_void_p)) == -1
        assert lib.smrf_pf_plan(2, radii.ctypes.data_as(C.c_void_p), 10, 4096, 24 * Mi, 0, AUTO, 0, route.ctypes.data_as(C.c_void_p),
                                inc.ctypes.data_as(C.c_void_p)) == -1
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
        _lib.reload_switches()
