"""The restatements of tests/assign_numpy.py against SciPy and the reference's goldens, on the CPU.

The solver restatement is the yardstick the device is compared with bit for bit (tests/test_gpu_assign.py), so it is
itself held to SciPy here: the cost bits are cdist's, the assignment is linear_sum_assignment's wherever the optimum is
unique, and the total is SciPy's exactly where it is not.  The regression restatement is held to the longdouble
evaluation of the reference's formulas, within four times the reference's own float64 error plus 4 ulp."""
import json

import numpy as np
import pytest

import assign_cases as ac
import assign_numpy as an
from conftest import golden


@pytest.fixture(scope="module")
def G():
    return golden("assign.npz")


def problems():
    out = []
    for d in (2, 3):
        for n in ac.SQUARE:
            out.append(("sq%d_d%d" % (n, d),) + ac.random_pair(n, n, d, 1))
        for nr, nc in ac.RECT:
            out.append(("r%dx%d_d%d" % (nr, nc, d),) + ac.random_pair(nr, nc, d, 2))
    for nr, nc in ((30, 30), (64, 64), (65, 65), (33, 70), (70, 33), (130, 130)):
        out.append(("off%dx%d" % (nr, nc),) + ac.offset_pair(nr, nc, 3))
    return out


def test_costs_are_cdist_bits():
    from scipy.spatial.distance import cdist
    for name, x, a in problems():
        assert an.same_bits(an.costs(x, a), cdist(x, a)), name
    for n, extra, _ in ac.TIES:
        x, a = ac.tie_pair(n, extra, 5)
        c = an.costs(x, a)
        assert an.same_bits(c, cdist(x, a)) and np.all(c / 2.5 == np.round(c / 2.5))


def test_assignment_equals_scipy():
    """no problem may differ: the failure cap is zero"""
    differ = []
    for name, x, a in problems():
        rows, cols, mc = an.hungarian_algorithm(x, a)
        wr, wc, wm = ac.scipy_assignment(x, a)
        assert rows.dtype == np.int64 and cols.dtype == np.int64 and mc.dtype == np.float64
        if not (np.array_equal(rows, wr) and np.array_equal(cols, wc) and an.same_bits(mc, wm)):
            differ.append(name)
    assert not differ, differ


def test_goldens_hungarian(G):
    for name in json.loads(str(G["hungarian_cases"])):
        rows, cols, mc = an.hungarian_algorithm(G["hx_" + name], G["ha_" + name])
        assert np.array_equal(rows, G["hr_" + name]) and np.array_equal(cols, G["hc_" + name]), name
        assert an.same_bits(mc, G["hm_" + name]), name


@pytest.mark.parametrize("n,extra,total", ac.TIES)
def test_exact_ties(n, extra, total):
    x, a = ac.tie_pair(n, extra, 5)
    rows, cols, mc = an.hungarian_algorithm(x, a)
    assert an.valid_assignment(rows, cols, n, n + extra)
    want = ac.scipy_assignment(x, a)[2].sum()
    print(n, extra, mc.sum(), want)
    assert mc.sum() == want == total
    rows, cols, mc = an.hungarian_algorithm(a, x)                 # more rows than columns
    assert an.valid_assignment(rows, cols, n + extra, n) and mc.sum() == total


@pytest.mark.parametrize("name", sorted(ac.degenerate_pairs()))
def test_degenerate(name):
    x, a = ac.degenerate_pairs()[name]
    rows, cols, mc = an.hungarian_algorithm(x, a)
    assert an.valid_assignment(rows, cols, len(x), len(a))
    assert an.same_bits(mc, an.costs(x, a)[rows, cols])
    assert mc.sum() == ac.scipy_assignment(x, a)[2].sum()


def test_lane_sum_order():
    """element l, l + 64, ... on lane l, then the xor tree: checked against a plain loop"""
    rng = np.random.default_rng(4)
    for n in (1, 3, 63, 64, 65, 300):
        x = rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 4, n)
        p = [0.0] * 64
        for i, val in enumerate(x):
            p[i % 64] = p[i % 64] + val
        o = 32
        while o:
            p = [p[l] + p[l ^ o] for l in range(64)]
            o //= 2
        assert an.lane_sum(x) == p[0] and len(set(p)) == 1


def test_bdr_against_longdouble(G):
    cases = json.loads(str(G["bdr_cases"]))
    assert {"n3", "n64", "n65", "n300", "offset"} <= set(cases)
    bounds = ac.bdr_bounds(G, cases)
    for key, (worst, allowed) in bounds.items():
        print("%-8s reference error %.3e  allowed %.3e" % (key, worst, allowed))
    for name in cases:
        x, a = G["bx_" + name], G["ba_" + name]
        r2 = float(G["bdr_%s_rsquare" % name])
        assert 0.1 < r2 < 0.95, (name, r2)                         # 1 - rsquare does not cancel
        got = an.bdr(x, a)
        got.update(an.host_fields(got, len(x)))
        for key in an.DEVICE_FIELDS + ("scale", "theta"):
            err = ac.rel_error(got[key], ac.longdouble(G, name, key))
            print(name, key, "%.3e" % err)
            assert err <= bounds[key][1], (name, key, err, bounds[key])
        assert type(got["rsquare"]) is np.float64 and got["aPrime"].shape == (len(x),)
        gap = abs(float(got["P"]) - float(G["bdr_%s_P" % name]))
        print(name, "P", "%.3e" % gap)
        assert gap <= bounds["P"][1], (name, gap, bounds["P"])


def test_bootstrap_restatement_against_reference(G):
    """the seeded draw gives the reference's samples; its rsquare and DI stay within the bdr bounds"""
    cases = json.loads(str(G["bdr_cases"]))
    bounds = ac.bdr_bounds(G, cases)
    for name in json.loads(str(G["bootstrap_cases"])):
        x, a = G["sx_" + name], G["sa_" + name]
        np.random.seed(int(G["ss_" + name]))
        table = an.draw(len(a), len(x), 64)
        rsq, di = an.bdr_bootstrap(x, a, table)
        for got, want, key in ((rsq, G["sr_" + name], "rsquare"), (di, G["sd_" + name], "DI")):
            err = float(np.max(np.abs(got - want) / np.abs(want)))
            print(name, key, "%.3e" % err)
            assert err <= bounds[key][1], (name, key, err)


# ---- the C ABI, without a GPU: sizing, argument and workspace errors by status code -----
def test_abi_sizes_and_route():
    import streamed as S
    from neilpy_amd import _lib
    lib = _lib.load()
    assert {n for n in S.declarations() if n.startswith("smrf_assign_")} == {"smrf_assign_" + n for n in (
        "limit", "workspace_bytes", "route", "solve_f64", "samples_check", "bdr_f64")}
    limit = lib.smrf_assign_limit()
    assert limit >= 1024
    assert lib.smrf_assign_workspace_bytes(1, 1, 2) > 0 and lib.smrf_assign_workspace_bytes(limit, limit, 3) > 0
    for nr, nc, d in ((0, 5, 2), (5, 0, 2), (-1, 5, 2), (5, 5, 1), (5, 5, 4), (limit + 1, 5, 2), (5, limit + 1, 3)):
        assert lib.smrf_assign_workspace_bytes(nr, nc, d) == 0, (nr, nc, d)
    import ctypes as C
    r = (C.c_int * 5)()
    assert lib.smrf_assign_route(limit + 1, 5, 2, r) == -1 and lib.smrf_assign_route(5, 5, 2, None) == -1
    for d in (2, 3):
        assert lib.smrf_assign_route(8, 8, d, r) == 0
        regs, cached, waves, nbytes, square = list(r)
        assert regs == 256 and cached == 1 and waves == 4 and 1 <= square < regs
        assert lib.smrf_assign_route(square, square, d, r) == 0 and r[1] == 1
        assert lib.smrf_assign_route(square + 1, square + 1, d, r) == 0 and r[1] == 0
        # a workgroup never claims more than the 160 KiB of a CU
        for n in (1, 64, square, square + 1, 256, 257, 1024, limit):
            assert lib.smrf_assign_route(n, n, d, r) == 0
            assert 1 <= r[2] <= 4 and r[2] * r[3] <= 160 * 1024, (n, d, list(r))
    assert lib.smrf_assign_route(limit, limit, 3, r) == 0 and r[2] == 1


def test_abi_argument_errors():
    import ctypes as C
    from neilpy_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)                                            # never dereferenced: every call is refused first
    null = C.c_void_p(0)
    limit = lib.smrf_assign_limit()
    E_ARG, E_WS = -1, -3
    solve = lib.smrf_assign_solve_f64
    assert solve(p, 0, p, 5, 2, p, p, p, p, 256, null) == E_ARG
    assert solve(p, 5, p, 5, 4, p, p, p, p, 256, null) == E_ARG
    assert solve(p, limit + 1, p, 5, 2, p, p, p, p, 256, null) == E_ARG
    assert solve(null, 5, p, 5, 2, p, p, p, p, 256, null) == E_ARG
    assert solve(p, 5, p, 5, 2, p, null, p, p, 256, null) == E_ARG
    assert solve(p, 5, p, 5, 2, p, p, p, null, 256, null) == E_WS
    assert solve(p, 5, p, 5, 2, p, p, p, p, 8, null) == E_WS
    bdr = lib.smrf_assign_bdr_f64
    assert bdr(p, 2, p, 2, null, 1, 0, p, p, p, null, null, p, 256, null) == E_ARG       # n < 3
    assert bdr(p, 5, p, 6, null, 1, 0, p, p, p, null, null, p, 256, null) == E_ARG       # unequal lengths
    assert bdr(p, 5, p, 5, null, 0, 1, null, null, null, p, p, p, 256, null) == E_ARG    # no sample
    assert bdr(p, 5, p, 9, p, 4, 0, null, null, null, p, p, p, 256, null) == E_ARG       # samples without the solve
    assert bdr(p, limit + 1, p, limit + 1, null, 1, 1, null, null, null, p, p, p, 256, null) == E_ARG
    assert bdr(null, 5, p, 5, null, 1, 0, p, p, p, null, null, p, 256, null) == E_ARG
    assert bdr(p, 5, p, 5, null, 1, 0, null, p, p, null, null, p, 256, null) == E_ARG    # no output
    assert bdr(p, 5, p, 5, null, 1, 0, p, p, p, null, null, p, 16, null) == E_WS
    bad = C.c_int64(0)
    check = lib.smrf_assign_samples_check
    assert check(p, 0, 5, 9, C.byref(bad), p, 256, null) == E_ARG
    assert check(null, 4, 5, 9, C.byref(bad), p, 256, null) == E_ARG
    assert check(p, 4, 5, 9, None, p, 256, null) == E_ARG
    assert check(p, 4, 5, 9, C.byref(bad), p, 0, null) == E_WS


def test_public_names_and_no_cpu_fallback():
    import torch
    import neilpy_amd
    na = neilpy_amd.matching
    for name in ("hungarian_algorithm", "bdr", "bdr_bootstrap"):
        assert callable(getattr(na, name)) and name in na.__all__ and getattr(neilpy_amd, name) is getattr(na, name)
    x, a = ac.random_pair(5, 5, 2, 9)
    # shape errors need no GPU: they are raised before anything is uploaded
    with pytest.raises(ValueError):
        na.bdr(x, a[:4])
    with pytest.raises(ValueError):
        na.bdr(x[:2], a[:2])
    with pytest.raises(ValueError):
        na.hungarian_algorithm(x, np.zeros((5, 4)))
    with pytest.raises(ValueError):
        na.hungarian_algorithm(x[:0], a)
    if not torch.cuda.is_available():
        with pytest.raises(neilpy_amd.SmrfHipError):
            na.hungarian_algorithm(x, a)


def test_the_case_table_holds_inputs_the_restatement_accepts():
    """tests/family_cases.py's matching cases, walked without a GPU: each case's reference passes on the restatement's own
    result for its inputs, the assignment's optimum is unique (SciPy's assignment is the restatement's), and every name
    has a case for the stream and view runs"""
    import family_cases as FC
    names = ("hungarian_algorithm", "bdr", "bdr_bootstrap")
    marked = set()
    for case in FC.matching(names):
        got = getattr(an, case["name"])(*case["inputs"])
        case["reference"](FC.rebuild(got, FC.to_numpy))
        marked |= {case["name"]} if case["stream"] else set()
        if case["name"] == "hungarian_algorithm":
            assert all(an.same_bits(p, q) for p, q in zip(got, ac.scipy_assignment(*case["inputs"])))
    assert marked == set(names)
