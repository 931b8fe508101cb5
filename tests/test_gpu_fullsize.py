"""Parity at BASELINE.json's full sizes (cfg4: 16384^2 fp32, windows 1..50; cfg2: 4096^2, 1..18).

The oracle cannot reach these sizes in seconds, so the checks are size-independent properties of
the operators (each one exact, bit for bit): min/max duality between the erosion and dilation
instances, anti-extensivity and idempotence of the opening, the ring kernels against the
independent direct (footprint-gather) kernel, the row-band form against the whole raster, the
sharded driver against the single-device driver, monotone growth of the object mask with the
window list, and one pinned checksum of the headline result.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N4, W4 = 16384, 50            # cfg4
N2, W2 = 4096, 18             # cfg2


@pytest.fixture(scope="module")
def nz(gpu_device):
    import neilpy_amd
    neilpy_amd.load_library()
    return neilpy_amd


@pytest.fixture(scope="module")
def Z4(nz, gpu_device):
    import torch
    return torch.from_numpy(nz.synth_dem(N4, seed=20240)).to(gpu_device)


def test_cfg4_duality_opening_properties(nz, Z4):
    import torch
    for r in (2, 13, 50):
        e = nz.erosion(Z4, radius=r)
        assert torch.equal(e, -nz.dilation(-Z4, radius=r))     # min/max duality: two different kernel instances
        assert bool((e <= Z4).all())
        o = nz.dilation(e, radius=r)                            # opening
        assert bool((o <= Z4).all()) and bool((e <= o).all())  # anti-extensive
        assert torch.equal(nz.opening(o, radius=r), o)         # idempotent
        del e, o


def test_cfg4_ring_equals_direct_small_radius_and_band(nz, Z4, gpu_device):
    """ring kernel == direct kernel over the whole 16384^2 raster at R = 3; at R = 50 on a row band
    through the band form of the C ABI (halo rows given, reflect only at the true borders)."""
    import torch
    from neilpy_amd import _lib
    assert torch.equal(nz.erosion(Z4, radius=3), nz.erosion(Z4, radius=3, impl=_lib.IMPL_DIRECT))
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = 50
    full = nz.erosion(Z4, radius=r)
    for b0, b1 in ((0, 700), (8000, 8600), (N4 - 640, N4)):
        lo, hi = max(0, b0 - r), min(N4, b1 + r)
        src = Z4[lo:hi]
        for impl in (_lib.IMPL_RING, _lib.IMPL_DIRECT):
            out = torch.empty((b1 - b0, N4), dtype=Z4.dtype, device=gpu_device)
            _lib.check(lib.smrf_disk_filter_f32(C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), N4, N4, N4, lo,
                                                hi - lo, b0, b1 - b0, r, 0, 0, impl, st))
            assert torch.equal(out, full[b0:b1]), (b0, impl)


def test_cfg4_progressive_filter_monotone_and_pinned(nz, Z4):
    """windows 1..k flag a subset of windows 1..50; when_dropped agrees with the mask; checksum pinned."""
    import torch
    win = np.arange(1, W4 + 1)
    m50, w50 = nz.progressive_filter(Z4, win, 1, .15, return_when_dropped=True)
    m10, w10 = nz.progressive_filter(Z4, win[:10], 1, .15, return_when_dropped=True)
    assert m50.dtype == torch.bool and w50.dtype == torch.uint8
    assert bool((m10 <= m50).all())                            # the first 10 windows are the same computation
    assert bool(((w50 > 0) <= m50).all()) and bool(((w10 > 0) <= m10).all())
    assert bool((w50[m10] >= w10[m10]).all())                  # a later window can only raise the last-writer index
    assert int(w50.max()) <= W4 - 1
    # the headline workload's result, pinned (bench.py reports the same count as config.object_cells)
    assert int(m50.sum()) == 51388194
    # second call: same bits (no atomics, no order dependence)
    assert torch.equal(nz.progressive_filter(Z4, win, 1, .15), m50)


def test_cfg4_sharded_driver_equals_single_device(nz, Z4):
    """neilpy_amd.sharded's row-band driver on the 8 bands of cfg4, one rank after the other on this GPU.
    The neighbour exchange is replaced by copying the same rows out of the surface that enters each group
    of windows (computed on the whole raster), which is what the neighbours would send."""
    import torch
    from sharded_one_gpu import run_bands
    win = np.arange(1, 19)                                     # groups (1..15), (16..18) on 2048-row bands
    want = nz.progressive_filter(Z4, win, 1, .15)
    mask, _, groups = run_bands(nz, Z4, win, 8)                # one exchange per group, sum(2r) rows: checked in there
    assert [len(g) for g in groups] == [15, 3]
    for k in range(8):
        assert torch.equal(mask[k * 2048:(k + 1) * 2048], want[k * 2048:(k + 1) * 2048]), k


def test_cfg2_full_call_vs_direct_kernel_chain(nz, gpu_device):
    """cfg2 whole call against the same chain built from the direct kernel (no ring code involved)."""
    import torch
    from neilpy_amd import _lib
    Z = torch.from_numpy(nz.synth_dem(N2, seed=20240)).to(gpu_device)
    win = np.arange(1, W2 + 1)
    got, when = nz.progressive_filter(Z, win, 1, .15, return_when_dropped=True)
    last = Z
    mask = torch.zeros_like(got)
    wd = torch.zeros_like(when)
    for i, r in enumerate(win):
        o = nz.dilation(nz.erosion(last, radius=int(r), impl=_lib.IMPL_DIRECT), radius=int(r), impl=_lib.IMPL_DIRECT)
        new = (last - o).double() > np.float64(.15) * (int(r) * 1)
        mask |= new
        wd[new] = i
        last = o
    assert torch.equal(got, mask) and torch.equal(when, wd)
