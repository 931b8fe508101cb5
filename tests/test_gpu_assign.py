"""hungarian_algorithm / bdr / bdr_bootstrap on the device against the restatements (tests/assign_numpy.py), SciPy and the
reference's goldens (tests/golden/assign.npz).  DESIGN.md section 18.

The device is compared with the restatement on bits: the index arrays, ``min_costs``, every device-formed field of
``bdr`` and both arrays of ``bdr_bootstrap``.  The restatement is held to SciPy and to the longdouble formulas on the CPU
(tests/test_assign_host.py)."""
import json

import numpy as np
import pytest

import assign_cases as ac
import assign_numpy as an
from conftest import golden
from guarded import POISONS, guarded

pytestmark = pytest.mark.gpu

K = 64


@pytest.fixture(scope="module")
def G():
    return golden("assign.npz")


def assert_bits(got, want, keys, ctx):
    """the entries ``keys`` of a result - positions of a tuple, fields of bdr's dict - have the bits of ``want``'s: what
    tests/family_cases.py's matching cases compare with the restatement"""
    for k in keys:
        assert an.same_bits(got[k], want[k]), (ctx, k, got[k], want[k])


def check_hungarian(x, a, want=None):
    """the device's result equals the restatement's (or ``want``) on the indices and on min_costs' bits"""
    from neilpy_amd import matching as na
    rows, cols, mc = na.hungarian_algorithm(x, a)
    wr, wc, wm = want if want is not None else an.hungarian_algorithm(x, a)
    assert isinstance(rows, np.ndarray) and rows.dtype == np.int64 and cols.dtype == np.int64 and mc.dtype == np.float64
    assert np.array_equal(rows, wr) and np.array_equal(cols, wc), (x.shape, a.shape, int((cols != wc).sum()))
    assert an.same_bits(mc, wm), (x.shape, a.shape)
    return rows, cols, mc


def sizes(d):
    """the issue's sizes, and one on each side of every point where the kernel changes route, as the library reports"""
    from neilpy_amd.matching import assignment_route
    route = assignment_route(8, 8, d)
    reg, sq = route["register_columns"], route["cached_square"]
    assert assignment_route(sq, sq, d)["cached"] and not assignment_route(sq + 1, sq + 1, d)["cached"]
    out = [(n, n) for n in ac.SQUARE] + list(ac.RECT) + [(100, 64), (1, 300), (300, 1)]
    out += [(sq, sq), (sq + 1, sq + 1), (reg, reg), (reg + 1, reg + 1), (40, reg), (reg + 1, 40), (reg + 70, reg + 70)]
    return out


@pytest.mark.parametrize("d", [2, 3])
def test_sizes(gpu_device, d):
    for nr, nc in sizes(d):
        check_hungarian(*ac.random_pair(nr, nc, d, 10 + d))


def test_offset_clouds(gpu_device):
    for nr, nc in ((30, 30), (64, 64), (65, 65), (33, 70), (70, 33), (130, 130)):
        check_hungarian(*ac.offset_pair(nr, nc, 3))


def test_goldens_hungarian(gpu_device, G):
    for name in json.loads(str(G["hungarian_cases"])):
        check_hungarian(G["hx_" + name], G["ha_" + name], (G["hr_" + name], G["hc_" + name], G["hm_" + name]))


def test_input_types(gpu_device):
    """float32, integer and CUDA-tensor input give what their float64 NumPy widening gives; tensors in, tensors out"""
    import torch
    from neilpy_amd import matching as na
    for d in (2, 3):
        x, a = ac.random_pair(70, 90, d, 20)
        x32, a32 = x.astype(np.float32), a.astype(np.float32)
        want = an.hungarian_algorithm(x32.astype(np.float64), a32.astype(np.float64))
        check_hungarian(x32, a32, want)
        xi, ai = np.floor(x).astype(np.int32), np.floor(a).astype(np.int64)
        check_hungarian(xi, ai, an.hungarian_algorithm(xi, ai))
        for xt, at, w in ((torch.from_numpy(x).to(gpu_device), torch.from_numpy(a).to(gpu_device), None),
                          (torch.from_numpy(x32).to(gpu_device), torch.from_numpy(a32).to(gpu_device), want),
                          (torch.from_numpy(xi).to(gpu_device), ai, an.hungarian_algorithm(xi, ai))):
            rows, cols, mc = na.hungarian_algorithm(xt, at)
            assert rows.is_cuda and rows.device == gpu_device and rows.dtype == torch.int64 and mc.dtype == torch.float64
            wr, wc, wm = w if w is not None else an.hungarian_algorithm(x, a)
            assert np.array_equal(rows.cpu().numpy(), wr) and np.array_equal(cols.cpu().numpy(), wc)
            assert an.same_bits(mc.cpu().numpy(), wm)


def test_limit(gpu_device):
    """one problem at the documented limit against SciPy directly; one point more raises and names the limit"""
    from neilpy_amd import matching as na
    from neilpy_amd.matching import assignment_limit
    limit = assignment_limit()
    assert limit >= 1024
    x, a = ac.random_pair(limit, limit, 3, 30)
    rows, cols, mc = na.hungarian_algorithm(x, a)
    wr, wc, wm = ac.scipy_assignment(x, a)
    assert np.array_equal(rows, wr) and np.array_equal(cols, wc) and an.same_bits(mc, wm)
    big = np.zeros((limit + 1, 2))
    for call in (lambda: na.hungarian_algorithm(big, a[:5, :2]), lambda: na.hungarian_algorithm(x[:5, :2], big),
                 lambda: na.bdr_bootstrap(big, big, 2)):
        with pytest.raises(ValueError, match=str(limit)):
            call()


def test_ties_and_degenerate(gpu_device):
    """a valid assignment, SciPy's total exactly, the restatement's choice, and the same result on two runs"""
    from neilpy_amd import matching as na
    pairs = [ac.tie_pair(n, extra, 5) + (total,) for n, extra, total in ac.TIES]
    pairs += [(a, x, total) for x, a, total in pairs]
    pairs += [p + (None,) for p in ac.degenerate_pairs().values()]
    for x, a, total in pairs:
        rows, cols, mc = check_hungarian(x, a)
        assert an.valid_assignment(rows, cols, len(x), len(a))
        assert mc.sum() == ac.scipy_assignment(x, a)[2].sum()
        assert total is None or mc.sum() == total
        again = na.hungarian_algorithm(x, a)
        assert all(an.same_bits(p, q) for p, q in zip((rows, cols, mc), again))


def check_bdr(x, a):
    from neilpy_amd import matching as na
    got, want = na.bdr(x, a), an.bdr(x, a)
    want.update(an.host_fields(want, len(x)))
    assert set(got) == set(want) and len(got) == 14
    for key in an.DEVICE_FIELDS + ("scale", "theta", "P"):
        assert an.same_bits(got[key], want[key]), (key, got[key], want[key])
        if key not in ("aPrime", "bPrime"):
            assert type(got[key]) is np.float64, key
    return got


def test_bdr(gpu_device, G):
    import torch
    from neilpy_amd import matching as na
    cases = json.loads(str(G["bdr_cases"]))
    bounds = ac.bdr_bounds(G, cases)
    for name in cases:
        x, a = G["bx_" + name], G["ba_" + name]
        got = check_bdr(x, a)
        for key in an.DEVICE_FIELDS + ("scale", "theta"):
            err = ac.rel_error(got[key], ac.longdouble(G, name, key))
            assert err <= bounds[key][1], (name, key, err, bounds[key])
        assert abs(float(got["P"]) - float(G["bdr_%s_P" % name])) <= bounds["P"][1]
    x, a = ac.random_pair(3, 3, 2, 40)
    check_bdr(x, a)                                                       # n = 3
    x, a = ac.random_pair(5000, 5000, 2, 41)                              # no limit without the matching
    check_bdr(x, a + 0.5 * x)
    x, a = G["bx_n65"], G["ba_n65"]
    want = check_bdr(x, a)
    t = na.bdr(torch.from_numpy(x.astype(np.float32)).to(gpu_device), torch.from_numpy(a).to(gpu_device))
    assert t["aPrime"].is_cuda and t["aPrime"].dtype == torch.float64 and type(t["rsquare"]) is np.float64
    w32 = an.bdr(x.astype(np.float32).astype(np.float64), a)
    assert an.same_bits(t["aPrime"].cpu().numpy(), w32["aPrime"]) and an.same_bits(t["F"], w32["F"])
    assert set(t) == set(want)


@pytest.fixture(scope="module")
def boot(G):
    """{name: (XY, AB, seed, table, restatement rsquare, restatement DI)}, computed once"""
    out = {}
    for name in json.loads(str(G["bootstrap_cases"])):
        x, a, seed = G["sx_" + name], G["sa_" + name], int(G["ss_" + name])
        np.random.seed(seed)
        table = an.draw(len(a), len(x), K)
        out[name] = (x, a, seed, table) + an.bdr_bootstrap(x, a, table)
    return out


@pytest.mark.parametrize("name", ["30of60", "64of64", "65of130"])
def test_bootstrap(gpu_device, G, boot, name):
    import torch
    from neilpy_amd import matching as na
    x, a, seed, table, wr, wd = boot[name]
    assert (len(x), len(a)) == tuple(int(v) for v in name.split("of"))
    np.random.seed(seed)
    rsq, di = na.bdr_bootstrap(x, a, K)                                   # the seeded default draw
    assert isinstance(rsq, np.ndarray) and rsq.dtype == np.float64 and rsq.shape == (K,) and di.shape == (K,)
    assert an.same_bits(rsq, wr) and an.same_bits(di, wd)
    r2, d2 = na.bdr_bootstrap(x, a, samples=table)                        # the same table handed in
    assert an.same_bits(r2, rsq) and an.same_bits(d2, di)
    if name == "64of64":
        assert np.unique(rsq).size == 1 and np.unique(di).size == 1       # every sample is the whole of AB
    bounds = ac.bdr_bounds(G, json.loads(str(G["bdr_cases"])))
    for got, want, key in ((rsq, G["sr_" + name], "rsquare"), (di, G["sd_" + name], "DI")):
        err = float(np.max(np.abs(got - want) / np.abs(want)))
        print(name, key, "%.3e" % err)
        assert err <= bounds[key][1], (name, key, err)
    # k = 1, a k that is no multiple of the waves of a workgroup, repeated rows, an int32 tensor table
    for k in (1, 7):
        r, d = na.bdr_bootstrap(x, a, samples=table[:k])
        assert an.same_bits(r, wr[:k]) and an.same_bits(d, wd[:k])
    rep = table[:3].copy()
    rep[:, 1] = rep[:, 0]
    r, d = na.bdr_bootstrap(x, a, samples=rep)
    w = an.bdr_bootstrap(x, a, rep)
    assert an.same_bits(r, w[0]) and an.same_bits(d, w[1])
    r, d = na.bdr_bootstrap(torch.from_numpy(x).to(gpu_device), a, samples=torch.from_numpy(table[:5].astype(np.int32)).to(gpu_device))
    assert r.is_cuda and an.same_bits(r.cpu().numpy(), wr[:5]) and an.same_bits(d.cpu().numpy(), wd[:5])


def test_bootstrap_beyond_the_register_columns(gpu_device):
    """n past the columns held in registers, costs recomputed: 300 of 400"""
    from neilpy_amd import matching as na
    rng = np.random.default_rng(50)
    ab = rng.uniform(0, 100, (400, 2))
    xy = ab[rng.permutation(400)[:300]] * 1.3 + rng.normal(0, 6.0, (300, 2))
    table = np.stack([rng.permutation(400)[:300] for _ in range(3)])
    r, d = na.bdr_bootstrap(xy, ab, samples=table)
    w = an.bdr_bootstrap(xy, ab, table)
    assert an.same_bits(r, w[0]) and an.same_bits(d, w[1])


def test_errors(gpu_device):
    from neilpy_amd import matching as na
    x, a = ac.random_pair(20, 40, 2, 70)
    x3 = np.column_stack([x, x[:, 0]])
    bad = x.copy()
    bad[7, 1] = np.nan
    inf = a.copy()
    inf[3, 0] = -np.inf
    table = np.stack([np.arange(20), np.arange(20, 40)])
    over, under = table.copy(), table.copy()
    over[1, 5], under[0, 0] = 40, -1
    np.random.seed(1)
    state = np.random.get_state()[1].copy()
    for call, match in ((lambda: na.bdr(x, a), "row by row"),                         # unequal lengths
                        (lambda: na.bdr(x[:2], a[:2]), "at least 3"),                  # n < 3
                        (lambda: na.bdr_bootstrap(x[:2], a, 4), "at least 3"),
                        (lambda: na.bdr(x3, x3), "dimension 3"),                       # wrong d
                        (lambda: na.bdr_bootstrap(x, np.column_stack([a, a]), 4), "dimension 4"),
                        (lambda: na.hungarian_algorithm(x, np.column_stack([a, a])), "dimension 4"),
                        (lambda: na.hungarian_algorithm(x, x3), "dimension"),
                        (lambda: na.hungarian_algorithm(x[:0], a), "empty"),           # an empty cloud
                        (lambda: na.bdr(x[:0], a[:0]), "empty"),
                        (lambda: na.hungarian_algorithm(bad, a), "NaN or infinite"),   # a non-finite coordinate
                        (lambda: na.hungarian_algorithm(x, inf), "NaN or infinite"),
                        (lambda: na.bdr(bad, a[:20]), "NaN or infinite"),
                        (lambda: na.bdr_bootstrap(x, inf, 4), "NaN or infinite"),
                        (lambda: na.bdr_bootstrap(x, a, samples=over), "1 entries"),   # an out-of-range samples entry
                        (lambda: na.bdr_bootstrap(x, a, samples=under), "1 entries"),
                        (lambda: na.bdr_bootstrap(x, a, samples=table[:, :19]), "samples"),
                        (lambda: na.bdr_bootstrap(x, a, samples=table.astype(np.float64)), "integer"),
                        (lambda: na.bdr_bootstrap(x, a, -1), "count of samples")):
        with pytest.raises(ValueError, match=match):
            call()
    assert np.array_equal(np.random.get_state()[1], state)                             # no call above drew a sample
    with pytest.raises(ValueError, match="larger sample"):                             # len(XY) > len(AB): the draw's own error
        na.bdr_bootstrap(a, x, 4)
    r, d = na.bdr_bootstrap(x, a, 0)                                                   # the reference's two empty arrays
    assert r.shape == d.shape == (0,) and r.dtype == d.dtype == np.float64
    assert np.array_equal(np.random.get_state()[1], state)
    r, d = na.bdr_bootstrap(x, a, samples=table)                                       # the table itself is fine
    assert r.shape == (2,) and np.all((r > 0) & (r < 1))


def overflow_pair():
    """finite coordinates whose squared difference overflows: every cost of XY's row 3 is +inf, so no finite assignment
    exists; SciPy and the restatement raise, and so must the device, before it hands anything back"""
    x, a = ac.random_pair(40, 70, 2, 80)
    x[3, 0] = 1e200
    return x, a


@pytest.mark.parametrize("name", ["hungarian_algorithm", "hungarian_swapped", "bdr_bootstrap"])
def test_overflowed_costs_raise(gpu_device, name):
    from neilpy_amd import matching as na
    x, a = overflow_pair()
    with np.errstate(over="ignore"):
        with pytest.raises(ValueError):
            an.hungarian_algorithm(x, a)
    with pytest.raises(ValueError):
        ac.scipy_assignment(x, a)
    table = np.stack([np.random.default_rng(81 + s).permutation(70)[:40] for s in range(5)]).astype(np.int64)
    for poison in POISONS:
        with guarded(gpu_device, poison) as g:
            xt, at, tt = g.tensor(x), g.tensor(a), g.tensor(table)
            with pytest.raises(ValueError, match="overflowed"):
                if name == "hungarian_algorithm":
                    na.hungarian_algorithm(xt, at)
                elif name == "hungarian_swapped":
                    na.hungarian_algorithm(at, xt)
                else:
                    na.bdr_bootstrap(xt, at, samples=tt)
        g.check()
        assert g.unchanged(xt) and g.unchanged(at) and g.unchanged(tt)
    # the same clouds without the outlier are fine
    x[3, 0] = 50.0
    check_hungarian(x, a)
