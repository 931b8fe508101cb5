"""The incremental erosion of progressive_filter (csrc/morph_incero.h), without a GPU: the leftover-cell
tables against a brute-force derivation, the identity  e_R = min(erode(e_{R-1}, cross), min over P_R of opened_{R-1})
against the oracle's own erosion on rasters larger and much smaller than the disks, and the compiled instances."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import smrf_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("ero_inc_inc", os.path.join(ROOT, "tools", "ero_inc_inc.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

CROSS = {(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)}
# |P_R| for R = 2..64, as derived when the decomposition was proposed
CARD = [0, 4, 0, 8, 0, 0, 8, 8, 12, 0, 0, 20, 8, 16, 0, 12, 8, 16, 20, 0, 24, 8, 8, 32, 16, 20, 8, 16, 24, 8, 32, 16, 28, 32, 0,
        36, 8, 48, 24, 8, 32, 24, 44, 32, 8, 32, 24, 40, 40, 44, 32, 16, 36, 24, 56, 24, 44, 24, 40, 52, 32, 40, 40]


def brute_disk(r):
    return {(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r}


def test_tables_equal_a_brute_force_derivation():
    for r in range(2, 65):
        d, dprev = brute_disk(r), brute_disk(r - 1)
        grown = {(p[0] + q[0], p[1] + q[1]) for p in dprev for q in CROSS}
        # B = D_R (-) D_{R-1}: every offset b with b + D_{R-1} inside D_R
        b = {(by, bx) for by in range(-3, 4) for bx in range(-3, 4) if all((by + p[0], bx + p[1]) in d for p in dprev)}
        assert b == CROSS, r
        cells = set()
        for dy, dx in gen.pairs(r):
            assert dx > 0
            cells |= {(dy, dx), (dy, -dx)}
        assert len(cells) == 2 * len(gen.pairs(r)) == CARD[r - 2], r
        assert (grown | cells) == d, r
        assert not (cells & grown), r
        assert cells == d - grown, r


def test_committed_inc_is_the_generators_output():
    assert open(gen.INC).read() == gen.render()


def fold(i, n):
    p = np.mod(i, 2 * n)
    return np.where(p < n, p, 2 * n - 1 - p)


def identity_erosion(e_prev, last, r):
    """e_R by the identity, with the library's period-2n reflect written as a plain gather"""
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=np.uint8)
    out = so.erosion(e_prev, cross)
    rows, cols = last.shape
    yy, xx = np.arange(rows)[:, None], np.arange(cols)[None, :]
    for dy, dx in gen.pairs(r):
        fy = fold(yy + dy, rows)
        out = np.minimum(out, last[fy, fold(xx + dx, cols)])
        out = np.minimum(out, last[fy, fold(xx - dx, cols)])
    return out


@pytest.mark.parametrize("shape,nwin", [((150, 600), 50), ((12, 600), 30), ((12, 40), 30)])
def test_identity_is_bit_equal_to_the_oracles_direct_erosion(shape, nwin):
    """every window's e_R, radii up to 2.5 times the raster's rows included: the identity needs no raster-size condition
    under the period-2n reflect.  (Rasters of a few cells are left out: scipy's own erosion returns uninitialised memory on
    5 x 7 at R = 20, so there is no oracle to compare with.)"""
    rng = np.random.default_rng(7)
    Z = (rng.random(shape) * 30 + 5 * np.sin(np.arange(shape[1]) / 9.0)[None, :]).astype(np.float32)
    last = Z
    e_prev = None
    for r in range(1, nwin + 1):
        e = so.erosion(last, so.disk(r))
        if e_prev is not None:
            got = identity_erosion(e_prev, last, r)
            assert got.dtype == e.dtype and np.array_equal(got, e), (shape, r, int((got != e).sum()))
        last = so.dilation(e, so.disk(r))
        e_prev = e


def _compile_unit(tmp_path):
    from neilpy_amd.build import CSRC, FLAGS, hipcc
    out = str(tmp_path / "incero.s")
    cmd = [hipcc()] + [f for f in FLAGS if f != "-fPIC"] + ["--offload-device-only", "-S", os.path.join(CSRC, "incero.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def test_incremental_erosion_instances_hold_their_ring_in_registers(tmp_path):
    """every shipped instance (fp32, R = 16..64): no scratch, and the LDS reads of the leftover cells are not fused into
    half-rate ds_read2 / ds_write2 forms"""
    text = _compile_unit(tmp_path)
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    names = [k for k in kernels if "inc_erode_kernel" in k]
    assert len(names) == 64 - 16 + 1, len(names)
    for name in names:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", kernels[name]).group(1)) == 0, name
    assert "ds_read2" not in text and "ds_write2" not in text
    assert "scratch_" not in text
