"""neilpy_amd.sharded.band_plan: the row arithmetic of the row-band progressive_filter, checked in plain Python.

The plan of every rank is replayed on a model of the buffers that only knows WHICH surface (how many windows opened)
every row of every buffer holds: a step may read only rows that hold the surface it is due to read, an exchange hands
a rank exactly the rows its neighbours send, and the group structure (one exchange of sum(2r) rows per group, margins
shrinking by 2r per window to the band itself, the edge-first split of ``overlap``) follows from the steps alone.
No torch process group, no tensors, no GPU.
"""
import pytest

from neilpy_amd import _lib
from neilpy_amd.sharded import band_plan, band_rows, band_sizes, window_groups

WINDOW_LISTS = [[1, 2, 3, 5, 8], [1, 4, 9, 12], [2, 1, 7, 11],                      # tests/test_sharded_gloo.py
                [1, 2, 3, 5, 4, 8], [2, 6, 1], list(range(1, 11)),                   # tests/test_gpu_edges.py
                [4]]                                                                 # a single window: buffers never flip
SCRIPTS = (None, "fused", "chain")


class Head:
    """a scripted HipBandOps.head_launch: two passes / fused up to r = 5 / chains of up to three radii <= 3; keeps the offers"""

    def __init__(self, script):
        self.script, self.offers = script, []

    def __call__(self, src, radii, rows, chain):
        self.offers.append((src, list(radii), rows, chain))
        if self.script == "chain" and chain and radii[0] <= 3:
            n = 1
            while n < min(3, len(radii)) and radii[n] <= 3:
                n += 1
            return _lib.ROUTE_CHAIN, n
        if radii[0] <= 5:
            return _lib.ROUTE_FUSED, 1
        return _lib.ROUTE_TWO_PASS, 1


def heights(world, windows):
    """the legal minimum (every band exactly 2 * max(windows) rows), one row more, and heights that do not divide evenly"""
    low = world * 2 * max(windows)
    return [low, low + 1] + [h for h in (61, 150, 331) if h > low + 1]


def replay(img_rows, world, rank, windows, groups, overlap, script):
    """run one rank's plan on the model; returns its exchanges as (M, sent up, received from above, sent down, received from below, inside a split)"""
    head = Head(script) if script else None
    steps = list(band_plan(img_rows, world, rank, windows, groups, overlap, head))
    b0, b1 = band_rows(img_rows, world, rank)
    multi, max_band = world > 1, max(band_sizes(img_rows, world))
    first = [sum(len(g) for g in groups[:gi]) for gi in range(len(groups) + 1)]      # windows opened before group gi
    halo = [sum(2 * windows[i] for i in g) if multi else 0 for g in groups]
    surf = [[None] * img_rows, [None] * img_rows]           # surf[buffer][row] = windows opened on the surface held there
    surf[0][b0:b1] = [0] * (b1 - b0)
    ero = [None] * img_rows                                  # ero[row] = (windows opened on the eroded surface, radius)
    top, bottom = rank > 0, rank < world - 1                 # sides with a neighbour

    def span(m):
        return (b0 - m if top else 0, b1 + m if bottom else img_rows)

    def holds(rows, y0, y1, what):
        return 0 <= y0 <= y1 <= img_rows and rows[y0:y1] == [what] * (y1 - y0)

    done, cur, M, exchanges, pieces, offers = 0, 0, 0, [], [], 0
    for n, s in enumerate(steps):
        gi = s.group
        if s.kind == "exchange":
            serves = gi + 1 if s.side else gi                # inside the previous group's split, or at its own group's head
            m = halo[serves]
            assert multi and s.halo == m > 0 and s.src == s.dst == (1 - cur if s.side else cur)
            assert (s.in0, s.in1) == (b0, b1) and (s.out0, s.out1) == span(m) and m <= b1 - b0
            assert len(pieces) == (2 if s.side else 0)       # an early exchange follows the two edge pieces
            rows = surf[s.src]
            assert holds(rows, b0, b0 + m, first[serves]) and holds(rows, b1 - m, b1, first[serves]), (n, s)
            rows[s.out0:b0] = [first[serves]] * (b0 - s.out0)                        # what the neighbours send
            rows[b1:s.out1] = [first[serves]] * (s.out1 - b1)
            exchanges.append((m, (b0, b0 + m) if top else None, (s.out0, b0) if top else None,
                              (b1 - m, b1) if bottom else None, (b1, s.out1) if bottom else None, s.side))
            if not s.side:
                assert M == 0 and done == first[gi]
                M = m
        else:
            assert s.members == list(range(done, done + len(s.members))), (n, s)    # every window once, in order
            assert all(first[gi] <= i < first[gi + 1] for i in s.members)
            assert s.src == cur and s.dst == (None if s.kind == "erode" else 1 - cur)    # the two surfaces alternate
            radii = [windows[i] for i in s.members]
            eaten = sum(2 * r for r in radii) if multi else 0
            valid = span(M)                                  # the band plus the current margin
            if head is not None and s.kind != "dilate" and not pieces:
                src, offered, rows, chain = head.offers[offers]
                offers += 1
                assert (src, offered, chain) == (cur, [windows[i] for i in range(done, first[gi + 1])], multi and not overlap)
                assert rows == min(img_rows, max_band + 2 * M)   # the same figure on every rank
            if s.kind == "erode":                            # r rows inside the valid rows
                assert not s.side and not pieces and (s.in0, s.in1) == valid and holds(surf[cur], *valid, done)
                assert (s.out0, s.out1) == span(M - radii[0])
                ero[s.out0:s.out1] = [(done, radii[0])] * (s.out1 - s.out0)
                continue
            if s.kind == "dilate":                           # reads that erosion, and `last` on the rows it writes
                assert (s.in0, s.in1) == span(M - radii[0])
                assert holds(ero, s.in0, s.in1, (done, radii[0])) and holds(surf[cur], s.out0, s.out1, done)
            else:
                assert s.kind in ("open", "chain") and (s.in0, s.in1) == valid and holds(surf[cur], *valid, done)
                assert s.kind == "open" or (len(radii) <= 3 and multi and not overlap)
            pieces.append((s.out0, s.out1, s.side))
            kind_of, radii_of = s.kind, s.members
            surf[s.dst][s.out0:s.out1] = [done + len(radii)] * (s.out1 - s.out0)
        nxt = steps[n + 1] if n + 1 < len(steps) else None
        if not pieces or nxt is not None and (nxt.kind == "exchange" and nxt.side or nxt.members == radii_of and nxt.kind == kind_of):
            continue
        # the window (or chain) in `pieces` is complete: its output is the valid rows shrunk by 2r per window on every
        # side with a neighbour, in one piece or split edge-first
        radii = [windows[i] for i in radii_of]
        eaten = sum(2 * r for r in radii) if multi else 0
        want = span(M - eaten)
        last_of_group = done + len(radii) == first[gi + 1]
        Mn = halo[gi + 1] if overlap and last_of_group and gi + 1 < len(groups) else 0
        if len(pieces) == 1:
            assert pieces == [want + (False,)]
            assert not (Mn > 0 and b1 - b0 >= 2 * Mn and kind_of != "chain")         # ... it would have been split
            M -= eaten
        else:                                                # two Mn-row edges, the next group's exchange, the interior
            assert kind_of != "chain" and Mn > 0 and b1 - b0 >= 2 * Mn and want == (b0, b1)
            assert pieces[:2] == [(b0, b0 + Mn, True), (b1 - Mn, b1, True)]
            assert pieces[2:] == ([(b0 + Mn, b1 - Mn, False)] if b1 - b0 > 2 * Mn else [])
            assert exchanges[-1][0] == Mn and exchanges[-1][5] and M == eaten
            M = Mn                                           # the next group starts with its halo in place
        if last_of_group:                                    # the margin is gone: the band itself
            assert want == (b0, b1) and M == (Mn if len(pieces) > 1 else 0)
        done += len(radii)
        pieces = []
        if len(windows) > 1:
            cur = 1 - cur
    assert done == len(windows) and not pieces
    assert [e[0] for e in exchanges] == [m for m in halo if m > 0]                   # one exchange per group
    if head is not None:
        assert offers == len(head.offers)
    if len(windows) == 1:
        assert all(s.src == 0 and s.dst == {"exchange": 0, "erode": None}.get(s.kind, 1) for s in steps)
    return exchanges, steps


@pytest.mark.parametrize("windows", WINDOW_LISTS, ids=lambda w: "w" + "_".join(map(str, w)))
@pytest.mark.parametrize("world", [1, 2, 3, 4, 5])
def test_band_plan(world, windows):
    for img_rows in heights(world, windows):
        min_band = min(band_sizes(img_rows, world))
        for budget in (None, 0, 24):
            groups = window_groups(windows, min_band, budget) if world > 1 else [[i] for i in range(len(windows))]
            for overlap in (False, True):
                for script in SCRIPTS:
                    ranks = [replay(img_rows, world, k, windows, groups, overlap, script)[0] for k in range(world)]
                    for k in range(world):
                        assert [e[0] for e in ranks[k]] == [e[0] for e in ranks[0]]          # the same M on all ranks
                        for g, (m, up, from_above, down, from_below, early) in enumerate(ranks[k]):
                            # what rank k sends are exactly the global rows rank k -+ 1 receives
                            assert up == (ranks[k - 1][g][4] if k > 0 else None)
                            assert down == (ranks[k + 1][g][2] if k < world - 1 else None)
                            assert (from_above is None) == (k == 0) and (from_below is None) == (k == world - 1)
                            # split where the band holds both edges, else at the head of its group: bands differ by a row
                            assert early == (overlap and g > 0 and band_sizes(img_rows, world)[k] >= 2 * m)


def test_split_only_where_the_band_holds_both_edges():
    """bands of 48 rows, groups (1, 2, 3, 5) | 8 | 11: the 8's exchange (16 rows) fits the split of the 5, the 11's
    (22 rows, 44 <= 48) too; on 40-row bands the second does not and sits at the head of its group"""
    windows = [1, 2, 3, 5, 8, 11]
    for rows, want in ((96, [True, True]), (80, [True, False])):
        groups = window_groups(windows, rows // 2, 22)
        assert groups == [[0, 1, 2, 3], [4], [5]]
        for rank in (0, 1):
            steps = list(band_plan(rows, 2, rank, windows, groups, True, None))
            ex = [s for s in steps if s.kind == "exchange"]
            assert [s.halo for s in ex] == [22, 16, 22] and [s.side for s in ex] == [False] + want
            assert [s.group for s in ex] == [0, 0, 1 if want[1] else 2]
    # without overlap nothing runs on the side stream
    assert not any(s.side for s in band_plan(96, 2, 0, windows, window_groups(windows, 48, 22), False, None))


def test_single_band_is_one_group_per_window_on_the_whole_raster():
    head = Head("chain")
    steps = list(band_plan(40, 1, 0, [1, 2, 9], [[0], [1], [2]], True, head))
    assert [s.kind for s in steps] == ["open", "open", "erode", "dilate"]
    assert all((s.in0, s.in1, s.out0, s.out1) == (0, 40, 0, 40) and not s.side and s.halo == 0 for s in steps)
    assert [(s.src, s.dst) for s in steps] == [(0, 1), (1, 0), (0, None), (0, 1)]
    assert [o[1:] for o in head.offers] == [([1], 40, False), ([2], 40, False), ([9], 40, False)]
