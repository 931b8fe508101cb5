"""The incremental erosion's mirror plan (csrc/morph_incero.h, IncEroCfg::make_plan), restated in Python from ero_inc.inc.

A batch holds NP row pairs of `last`.  Job (row pair p, cell pair k) reads the pair's two rows at columns x - dx and x + dx and
updates ring slot 2p - dy + reach (and the next one, for the pair's second row).  The jobs (dy, dx) and (-dy, dx) of one row
pair read the same two LDS cells, so a mirror plan reads them once per GROUP (row pair, |dy|, dx) and updates the low slot
2p - |dy| + reach and the high slot 2p + |dy| + reach together.  The ring turns in place - slot s's first update of a batch
reads what slot s + ROWS held - so s must have its first update before s + ROWS has its own; with a low and a high slot per
item that is a constraint problem.  The header solves it greedily per radius and, where no group can run, either SPLITS one
(a half runs as a job of its own: a second pair of reads) or runs it anyway and lets the register allocator pay a COPY.

For every R in 16..64 and both fallbacks this checks: every contribution (row pair, cell pair) is applied exactly once; every
mirror group is read once or is one of the listed splits; every slot a batch touches has one first update, its earliest, and
it comes before slot + ROWS's - but for the listed copies, of which the split plan has none and the copy plan no splits.
The C++ table itself is guarded by the static_assert on IncEroCfg::plan_ok() in every instance; the item counts below were
read off the compiled kernels (ds_read_b64 per batch / 2), which ties the two statements of the planner together."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "neilpy_amd", "csrc", "morph_incero.h")
RADII = list(range(16, 65))
PLAIN, SPLIT, COPY = 0, 1, 2


def batch_geometry():
    src = open(HEADER).read()
    m = re.search(r"static constexpr int TW = 256, NP = (\d+), ROWS = 2 \* NP;", src)
    assert m, "IncEroCfg's batch geometry line changed: restate it here"
    assert "static constexpr int NACC = 2 * DY + ROWS;" in src
    assert "static constexpr int slot(int j) { return 2 * (j / N) - dy(j % N) + DY; }" in src
    assert "static constexpr int mirror(int j) { return (j / N) * N + N - 1 - j % N; }" in src
    assert "enum { kIncEroPlain = 0, kIncEroMirrorSplit = 1, kIncEroMirrorCopy = 2 };" in src
    assert "static_assert(C::plan_ok()" in src
    return 2 * int(m.group(1)), int(m.group(1))


ROWS, NP = batch_geometry()


def plan_kinds():
    """kIncEroPlanKind of the header: the plan each radius is built with"""
    src = open(HEADER).read()
    m = re.search(r"kIncEroPlanKind\[65\] = \{(.*?)\}", src, re.S)
    assert m, "the per-radius plan table changed: restate it here"
    kinds = [int(v) for v in m.group(1).replace("\n", " ").split(",")]
    assert len(kinds) == 65
    return kinds


def leftover_pairs():
    out = []
    for line in open(os.path.join(ROOT, "neilpy_amd", "csrc", "ero_inc.inc")):
        m = re.match(r"\s*\{(\d+), (\d+), \{(.*)\}\},", line)
        if m:
            pairs = [(int(a), int(b)) for a, b in re.findall(r"\{(-?\d+), (\d+)\}", m.group(3))]
            assert len(pairs) == int(m.group(1))
            out.append((int(m.group(1)), int(m.group(2)), pairs))
    assert len(out) == 65
    return out


TAB = leftover_pairs()


def make_plan(n, reach, pairs, kind):
    """-> items [(job, both)], the groups that were split, the slots whose first update comes too late (copies)"""
    nacc = 2 * reach + ROWS
    slot = [2 * (j // n) - pairs[j % n][0] + reach for j in range(NP * n)]
    mirror = [(j // n) * n + n - 1 - j % n for j in range(NP * n)]
    if kind == PLAIN:
        return [(j, False) for s in range(nacc) for j in range(NP * n) if slot[j] == s], [], 0
    nm = n // 2
    ngr = NP * nm
    jlo = [(g // nm) * n + nm + g % nm for g in range(ngr)]
    lo = [slot[j] for j in jlo]
    hi = [slot[mirror[j]] for j in jlo]
    touched, done, state = [False] * nacc, [False] * nacc, [0] * ngr
    for g in range(ngr):
        for t in (lo[g], lo[g] + 1, hi[g], hi[g] + 1):
            touched[t] = True

    def slots(g, part):
        return ([lo[g], lo[g] + 1] if part & 1 else []) + ([hi[g], hi[g] + 1] if part & 2 else [])

    def unready(g, part):
        return sum(not (done[t] or t < ROWS or not touched[t - ROWS] or done[t - ROWS]) for t in slots(g, part))

    items, splits, copies = [], [], 0
    left = 2 * ngr
    while left:
        best = None                                        # (key, g, part)
        for g in range(ngr):
            part = 3 & ~state[g]
            if part and not unready(g, part):
                key = lo[g] if part & 1 else hi[g]
                if best is None or key < best[0]:
                    best = (key, g, part)
        if best is None and kind == SPLIT:
            bcnt = -1
            for g in range(ngr):
                for part in (1, 2):
                    if state[g] or unready(g, part):
                        continue
                    s = lo[g] if part == 1 else hi[g]
                    was = done[s], done[s + 1]
                    done[s] = done[s + 1] = True
                    state[g] = part
                    cnt = sum(1 for h in range(ngr) if 3 & ~state[h] and not unready(h, 3 & ~state[h]))
                    state[g] = 0
                    done[s], done[s + 1] = was
                    if cnt > bcnt or (cnt == bcnt and s < best[0]):   # (best is set once bcnt >= 0)
                        best, bcnt = (s, g, part), cnt
            splits.append(best[1])
        elif best is None:
            bu = None
            for g in range(ngr):
                if state[g]:
                    continue
                u = unready(g, 3)
                if bu is None or u < bu or (u == bu and lo[g] < best[0]):   # (likewise)
                    best, bu = (lo[g], g, 3), u
        _, g, part = best
        copies += unready(g, part)
        for t in slots(g, part):
            done[t] = True
        state[g] |= part
        items.append((mirror[jlo[g]] if part == 2 else jlo[g], part == 3))
        left -= 2 if part == 3 else 1
    return items, splits, copies


def check_plan(r, kind):
    n, reach, pairs = TAB[r]
    assert max(max(abs(dy), dx) for dy, dx in pairs) == reach
    assert all(pairs[k][0] == -pairs[n - 1 - k][0] != 0 and pairs[k][1] == pairs[n - 1 - k][1] for k in range(n)), r
    nacc = 2 * reach + ROWS
    slot = [2 * (j // n) - pairs[j % n][0] + reach for j in range(NP * n)]
    mirror = [(j // n) * n + n - 1 - j % n for j in range(NP * n)]
    items, splits, copies = make_plan(n, reach, pairs, kind)
    # every contribution once
    applied = [j for j, both in items] + [mirror[j] for j, both in items if both]
    assert sorted(applied) == list(range(NP * n)), (r, kind)
    # every mirror group read once, or on the listed fallback (read twice)
    if kind != PLAIN:
        reads = {}
        for j, both in items:
            p, k = divmod(j, n)
            g = (p, abs(pairs[k][0]), pairs[k][1])
            reads[g] = reads.get(g, 0) + 1
            assert not both or pairs[k][0] > 0, (r, kind, j)     # a whole group is named by its low job
        assert len(reads) == NP * n // 2
        assert sorted(g for g, c in reads.items() if c == 2) == sorted(
            (g // (n // 2), pairs[n // 2 + g % (n // 2)][0], pairs[n // 2 + g % (n // 2)][1]) for g in splits), (r, kind)
        assert all(c in (1, 2) for c in reads.values())
        assert len(items) == NP * n // 2 + len(splits)
        assert not (kind == SPLIT and copies) and not (kind == COPY and splits), (r, kind)
    # the first-update order
    first = {}
    for i, (j, both) in enumerate(items):
        for s in [slot[j], slot[j] + 1] + ([slot[mirror[j]], slot[mirror[j]] + 1] if both else []):
            assert 0 <= s < nacc, (r, s)
            first.setdefault(s, i)
        if both:
            assert len({slot[j], slot[j] + 1, slot[mirror[j]], slot[mirror[j]] + 1}) == 4, (r, j)
    late = [s for s in first if s + ROWS in first and first[s] >= first[s + ROWS]]
    assert len(late) == copies, (r, kind, late, copies)
    if kind != COPY:
        assert not late, (r, kind, late)
    return len(items), len(splits), copies


@pytest.mark.parametrize("kind", [PLAIN, SPLIT, COPY], ids=["plain", "split", "copy"])
def test_every_radius_under_every_plan_kind(kind):
    for r in RADII:
        if TAB[r][0]:
            check_plan(r, kind)


def test_the_adopted_plan_of_every_radius():
    kinds = plan_kinds()
    for r in RADII:
        assert kinds[r] in (PLAIN, SPLIT, COPY), r
        if TAB[r][0]:
            check_plan(r, kinds[r])


# pairs of LDS reads per batch of the compiled instances (ds_read_b64 in the kernel / 2), split plan and copy plan
COMPILED_ITEMS = {SPLIT: {18: 8, 25: 36, 32: 37, 39: 53, 44: 63, 50: 51, 56: 64, 64: 62},
                  COPY: {18: 8, 25: 32, 39: 48, 44: 44, 50: 40, 64: 40}}


def test_the_restated_planner_reads_what_the_compiled_kernels_read():
    for kind, want in COMPILED_ITEMS.items():
        for r, items in want.items():
            got, splits, copies = check_plan(r, kind)
            assert got == items, (r, kind, got, items)
            assert got <= NP * TAB[r][0]                   # never more reads than one pair per job


# ---- the plain plan of a batch (job order and first-update table), restated on its own from ero_inc.inc and the header's
# batch geometry: cross loads before the prefetch, stores one batch late, the ring turned by an untied first update per slot ----
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
    for r in RADII:
        n, reach, pairs = TAB[r]
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


def test_mirror_plans_halve_the_reads_where_nothing_blocks():
    """8-cell rims (two mirror pairs far apart in dy) need no fallback: 8 pairs of reads for 16 jobs"""
    for r in (18, 23, 28, 31, 41, 46):
        assert TAB[r][0] == 4
        for kind in (SPLIT, COPY):
            assert check_plan(r, kind) == (8, 0, 0), r
