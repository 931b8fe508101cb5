"""The incremental erosion's batch order (csrc/morph_incero.h): cross loads before the prefetch, stores one batch late,
the ring turned by an untied first update per slot.  Windows [R-1, R] for every R in 16..64 against the independent
reference (tests/morph_numpy.py), bit for bit: e_R, opened_R, mask and when_dropped - at the shapes where that order can go
wrong: segments of a single batch (the deferred store and the DELTA rows meet the segment ends), several strips and
segments with the ragged placement, the column fold over several periods and a one-column last strip, and a plateau raster
on which a slot whose first update were skipped or doubled changes the result.  SMRF_ERO_INC=2 throughout.
The CPU test states the plan of IncEroCfg (job order and first-update table) in Python from ero_inc.inc and the header's
batch geometry; the C++ table itself is guarded by the static_assert on IncEroCfg::plan_ok() in every instance."""
import os
import re

import numpy as np
import pytest

import morph_numpy as mn
from conftest import switch
from pf_run import run_pf

RADII = list(range(16, 65))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nz(gpu_device):
    import neilpy_amd
    neilpy_amd.load_library()
    return neilpy_amd


def rough(shape, seed):
    """finite, positive, rough at every scale, with isolated objects"""
    rng = np.random.default_rng(seed)
    Z = rng.normal(0, 1, shape).cumsum(0).cumsum(1) * .05 + 200 + rng.random(shape) * 2
    return (Z + (rng.random(shape) < .05) * rng.uniform(1, 25, shape)).astype(np.float32)


def plateau(shape):
    """constant except one low cell per 64 x 64 block, each at another place in its block and another depth: every eroded
    cell is the minimum over very few candidates, so one lost or doubled slot update shows"""
    rng = np.random.default_rng(5)
    Z = np.full(shape, 300, dtype=np.float32)
    for by in range(0, shape[0], 64):
        for bx in range(0, shape[1], 64):
            y = by + int(rng.integers(0, min(64, shape[0] - by)))
            x = bx + int(rng.integers(0, min(64, shape[1] - bx)))
            Z[y, x] = np.float32(300 - rng.uniform(1, 40))
    return Z


def holds(planes, want):
    import torch
    w = torch.from_numpy(want).to(planes.device)
    return any(torch.equal(planes[k], w) for k in range(3))


def same(t, a):
    return np.array_equal(t.cpu().numpy().astype(a.dtype), a)


def check_pairs(Zh, gpu_device):
    """every R in 16..64 alone: windows [R-1, R], the second one incremental.  Returns the failing (R, what)."""
    import torch
    Zd = torch.from_numpy(Zh).to(gpu_device)
    bad = []
    for r in RADII:
        m, w, planes, route, taken = run_pf(Zd, [r - 1, r])
        assert taken == [0, 1], (r, taken, route)
        rm, rw, er, op = mn.progressive_filter(Zh, [r - 1, r], 1, .15, return_when_dropped=True, return_surfaces=True)
        for what, ok in (("e_R", holds(planes, er[1])), ("opened_R", holds(planes, op[1])), ("mask", same(m, rm)), ("when", same(w, rw))):
            if not ok:
                bad.append((r, what))
    return bad


CASES = [  # id, raster, SMRF_RING_SEG
    ("1x300_seg8", lambda: rough((1, 300), 11), 8),        # every batch the first and the last of its segment
    ("7x300_seg8", lambda: rough((7, 300), 12), 8),
    ("9x300_seg8", lambda: rough((9, 300), 13), 8),
    ("17x300_seg8", lambda: rough((17, 300), 14), 8),
    ("40x2100_seg16", lambda: rough((40, 2100), 15), 16),  # nine strips, three segments, ragged placement
    ("33x1", lambda: rough((33, 1), 16), None),            # the column fold over many periods
    ("24x257", lambda: rough((24, 257), 17), None),        # a one-column last strip
    ("plateau_200x330", lambda: plateau((200, 330)), None),
    ("plateau_70x300_seg8", lambda: plateau((70, 300)), 8),
]


@pytest.mark.gpu
@pytest.mark.parametrize("make,seg", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_every_radius_alone_against_the_reference(nz, gpu_device, monkeypatch, make, seg):
    switch(monkeypatch, "SMRF_ERO_INC", "2")
    switch(monkeypatch, "SMRF_RING_SEG", seg)
    bad = check_pairs(make(), gpu_device)
    assert not bad, bad


# ---- the plan of a batch, restated from ero_inc.inc.  The guard of the C++ table itself is IncEroCfg<R>::plan_ok(), a
# static_assert in every instance (a build with a wrong plan does not compile); this is the same rule stated independently,
# with the batch geometry read from the header so that the two cannot drift apart. ----
def batch_geometry():
    """(ROWS, NP) of IncEroCfg in csrc/morph_incero.h"""
    src = open(os.path.join(ROOT, "neilpy_amd", "csrc", "morph_incero.h")).read()
    m = re.search(r"static constexpr int TW = 256, NP = (\d+), ROWS = 2 \* NP;", src)
    assert m, "IncEroCfg's batch geometry line changed: restate it here"
    assert "static constexpr int NACC = 2 * DY + ROWS;" in src
    assert "static constexpr int slot(int j) { return 2 * (j / N) - dy(j % N) + DY; }" in src
    assert "static_assert(C::plan_ok()" in src
    return 2 * int(m.group(1)), int(m.group(1))


ROWS, NP = batch_geometry()


def leftover_pairs():
    """kEroInc of csrc/ero_inc.inc: per radius (n, reach, [(dy, dx), ...])"""
    out = []
    for line in open(os.path.join(ROOT, "neilpy_amd", "csrc", "ero_inc.inc")):
        m = re.match(r"\s*\{(\d+), (\d+), \{(.*)\}\},", line)
        if m:
            pairs = [(int(a), int(b)) for a, b in re.findall(r"\{(-?\d+), (\d+)\}", m.group(3))]
            assert len(pairs) == int(m.group(1))
            out.append((int(m.group(1)), int(m.group(2)), pairs))
    assert len(out) == 65
    return out


def batch_plan(n, reach, pairs):
    """jobs (row pair p, cell pair k) by ascending slot 2p - dy + reach; first[s] = position of the first job updating slot s"""
    nacc = 2 * reach + ROWS
    slot = [2 * (j // n) - pairs[j % n][0] + reach for j in range(NP * n)]
    seq = [j for s in range(nacc) for j in range(NP * n) if slot[j] == s]
    first = {}
    for i, j in enumerate(seq):
        for h in (0, 1):
            first.setdefault(slot[j] + h, i)
    return nacc, slot, seq, first


def test_first_update_table_names_every_touched_slot_once():
    tab = leftover_pairs()
    for r in RADII:
        n, reach, pairs = tab[r]
        if n == 0:
            continue
        assert max(max(abs(dy), dx) for dy, dx in pairs) == reach
        nacc, slot, seq, first = batch_plan(n, reach, pairs)
        assert sorted(seq) == list(range(NP * n)), r                      # every job once
        touched = {}
        for i, j in enumerate(seq):
            for h in (0, 1):
                s = slot[j] + h
                assert 0 <= s < nacc, (r, s)
                touched.setdefault(s, []).append(i)
        assert set(first) == set(touched), r
        for s, where in touched.items():
            assert sum(i == first[s] for i in where) == 1, (r, s)         # exactly one first update
            assert first[s] == min(where), (r, s)
            # the value slot s continues is still there: slot s + 8 has its own first update later
            if s + ROWS in first:
                assert first[s] < first[s + ROWS], (r, s)
