"""The premises the large-disk window tests on the GPU rest on (tests/test_gpu_incero_edges.py, tests/test_gpu_dil_cross.py), held
where no GPU is needed: the case tables of tests/window_cases.py are what those tests take them for, and the comparisons of
tests/pf_run.py tell what they claim to tell, fed CPU tensors instead of a launch's results."""
import numpy as np
import pytest

import morph_numpy as mn
import window_cases as wc
from pf_run import bits, holds, pair_failures, rotation_plan


@pytest.fixture(scope="module")
def rasters():
    return list(wc.rasters())


def test_ids_are_unique(rasters):
    ids = [c.id for c in wc.ALONE]
    assert len(ids) == 36 and len(set(ids)) == 36
    assert len({name for name, _ in rasters}) == len(rasters)
    assert len({tuple(w) for w in wc.LISTS}) == 30
    assert all(c.restated == c.id.startswith("mirror_") for c in wc.ALONE)


def test_rasters_are_float32_without_nan_and_with_one_sign_of_zero(rasters):
    """so the reference (min and max do not order -0.0 against +0.0) decides every bit, and a comparison of bit patterns
    is at least the comparison by value"""
    for name, Z in rasters:
        assert Z.dtype == np.float32 and Z.ndim == 2, name
        assert not np.isnan(Z).any(), name
        zero = Z == 0
        assert not ((zero & np.signbit(Z)).any() and (zero & ~np.signbit(Z)).any()), name


@pytest.mark.parametrize("rows,cols,seg,grid,branch", wc.GRIDS, ids=["%dx%d" % (g[0], g[1]) for g in wc.GRIDS])
def test_grids_reach_their_remap_branch(rows, cols, seg, grid, branch):
    wc.assert_grid(rows, cols, seg, grid, branch)


def test_rotation_lists_take_the_route_and_leave_it():
    for win in wc.LISTS:
        plan = rotation_plan(win)
        assert any(plan[i] and not plan[i + 1] for i in range(len(win) - 1)), win


# ---- the comparisons -------------------------------------------------------------------------------------------------
def test_holds_tells_the_two_zeros_apart():
    import torch
    planes = torch.zeros((3, 4, 5), dtype=torch.float32)
    planes[1] = -0.0
    assert holds(planes, np.zeros((4, 5), np.float32)) and holds(planes, np.full((4, 5), -0.0, np.float32))
    assert not holds(planes[:1].expand(3, 4, 5), np.full((4, 5), -0.0, np.float32))
    mixed = np.zeros((4, 5), np.float32)
    mixed[2, 3] = -0.0
    assert not holds(planes, mixed) and np.array_equal(mixed, planes[0].numpy())
    assert bits(np.float32(-0.0)) != bits(np.float32(0.0)) and bits(np.array([-0.0])).dtype == np.uint64


def test_holds_finds_a_plane_among_three():
    import torch
    Z = wc.rough((6, 9), 1)
    for k in range(3):
        planes = torch.full((3, 6, 9), 7.0)
        planes[k] = torch.from_numpy(Z)
        assert holds(planes, Z)
        other = Z.copy()
        other[5, 8] = np.nextafter(other[5, 8], np.float32(np.inf))
        assert not holds(planes, other)
    assert not holds(torch.from_numpy(Z).double().expand(3, 6, 9), Z)     # another number format is another surface


def test_pair_failures_name_the_radius_and_the_quantity_of_one_altered_cell():
    import torch
    r, Z = 16, wc.rough((20, 30), 2)
    ref = mn.progressive_filter(Z, [r - 1, r], 1, .15, return_when_dropped=True, return_surfaces=True)
    rm, rw, er, op = ref
    restated = mn.erosion(mn.dilation(mn.erosion(Z, r - 1, "rows"), r - 1, "rows"), r, "rows")
    assert len({a.tobytes() for a in (er[1], op[1], op[0])}) == 3

    def result():
        return (torch.from_numpy(rm.astype(np.uint8)), torch.from_numpy(rw.copy()),
                torch.from_numpy(np.stack([op[0], er[1], op[1]])))

    assert pair_failures(r, *result(), ref, restated) == []
    for k, at, what in ((0, (3, 4), ["mask"]), (1, (19, 29), ["when"]), (2, (0, 7, 11), ["opened_R-1"]),
                        (2, (1, 7, 11), ["e_R", "e_R restated"]), (2, (2, 7, 11), ["opened_R"])):
        got = result()
        got[k][at] = 1 - got[k][at]
        assert pair_failures(r, *got, ref, restated) == [(r, q) for q in what]
        assert pair_failures(r, *got, ref) == [(r, q) for q in what[:1]]
    # a restatement that disagrees with the reference is reported under its own name
    restated[0, 0] -= 1
    assert pair_failures(r, *result(), ref, restated) == [(r, "e_R restated")]
