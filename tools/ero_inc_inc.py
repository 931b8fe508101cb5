#!/usr/bin/env python3
"""Leftover cells of the incremental erosion (csrc/morph_incero.h) -> neilpy_amd/csrc/ero_inc.inc.

Window R of progressive_filter erodes opened_{R-1} = dilate(e_{R-1}, D_{R-1}) by the disk D_R.  For R = 2..64
    D_R = (D_{R-1} (+) B) u P_R,   B = the 5-point cross,   P_R = D_R \\ (D_{R-1} (+) B)
so  e_R = min(erode(e_{R-1}, B), min over p in P_R of opened_{R-1}[x + p])   (DESIGN.md 4.1c).
This script derives B and P_R by brute force from dx^2 + dy^2 <= R^2, asserts the decomposition, and writes P_R as
(dy, |dx|) pairs - the cells (dy, dx) and (dy, -dx) are both in P_R, one min3 takes both - sorted by dy.

    python tools/ero_inc_inc.py            # rewrite the .inc
    python tools/ero_inc_inc.py --check    # exit 1 if the committed .inc differs
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "neilpy_amd", "csrc", "ero_inc.inc")
RMIN, RMAX = 2, 64
CROSS = frozenset({(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)})


def disk(r):
    return frozenset((dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r)


def minkowski(a, b):
    return frozenset((p[0] + q[0], p[1] + q[1]) for p in a for q in b)


def residue(big, small):
    """big (-) small: the offsets b with b + small inside big"""
    cand = {(p[0] - q[0], p[1] - q[1]) for p in big for q in list(small)[:1]}
    return frozenset(b for b in cand if all((b[0] + q[0], b[1] + q[1]) in big for q in small))


def leftover(r):
    """P_r as a set of (dy, dx); asserts the decomposition of D_r"""
    d, dprev = disk(r), disk(r - 1)
    assert residue(d, dprev) == CROSS, "D_%d (-) D_%d is not the cross" % (r, r - 1)
    grown = minkowski(dprev, CROSS)
    assert grown <= d
    p = d - grown
    assert (grown | p) == d and not (p & grown)
    for (dy, dx) in p:                                      # 8-fold symmetric, and never on the column axis
        assert dx != 0 and {(dy, -dx), (-dy, dx), (dx, dy)} <= p
    return p


def pairs(r):
    """P_r as (dy, |dx|) pairs sorted by dy, then |dx|"""
    return sorted((dy, dx) for (dy, dx) in leftover(r) if dx > 0)


def render():
    tabs = {r: pairs(r) for r in range(RMIN, RMAX + 1)}
    nmax = max(len(t) for t in tabs.values())
    out = ["// Leftover cells P_R = D_R \\ (D_{R-1} (+) cross) of the incremental erosion (morph_incero.h; DESIGN.md 4.1c), R = 2..64,",
           "// written by tools/ero_inc_inc.py (brute force from dx^2 + dy^2 <= R^2; it asserts D_R (-) D_{R-1} = the 5-point cross and",
           "// (D_{R-1} (+) cross) u P_R = D_R).  A pair {dy, dx} stands for the two cells (dy, dx) and (dy, -dx); sorted by dy.",
           "// n = pairs (|P_R| / 2), reach = largest |dy| = largest dx.  (Included inside namespace smrf.)",
           "struct EroIncPair { signed char dy; unsigned char dx; };",
           "struct EroIncTab { int n, reach; EroIncPair p[%d]; };" % nmax,
           "inline constexpr EroIncTab kEroInc[%d] = {" % (RMAX + 1)]
    for r in range(RMAX + 1):
        t = tabs.get(r, [])
        reach = max([abs(dy) for dy, _ in t] + [0])
        assert reach == max([dx for _, dx in t] + [0])
        cells = ", ".join("{%d, %d}" % p for p in t)
        out.append("    {%d, %d, {%s}},%s" % (len(t), reach, cells, "" if r >= RMIN else "   // unused"))
    out.append("};")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    text = render()
    if a.check:
        if not os.path.exists(INC) or open(INC).read() != text:
            print("ero_inc.inc is stale: run tools/ero_inc_inc.py")
            return 1
        return 0
    open(INC, "w").write(text)
    print("wrote", INC)
    return 0


if __name__ == "__main__":
    sys.exit(main())
