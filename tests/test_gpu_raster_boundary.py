"""The array boundary (neilpy_amd/_raster.py) on the MI355X, one function per raster family: what kind of array comes
back, that tensors, views and integer rasters give the bits of the plain NumPy call, empty rasters, and the one place
where two families compute the same thing - Evans' quadratic of evans_curvature and of scaled_morphometry at stride 1."""
import numpy as np
import pytest

import morphometry_numpy as mn
import surface_numpy as sn
from family_checks import same_bits

pytestmark = pytest.mark.gpu

W = np.array([[0.5, 1.0, 0.0], [2.0, -1.0, 0.25], [0.0, 3.0, 1.5]])
GRADIENT_MSG = "too small to calculate a numerical gradient"


def _na():
    import neilpy_amd
    return neilpy_amd


def _planes(v):
    """a function's result as a list of arrays, whatever its container"""
    if isinstance(v, dict):
        return list(v.values())
    return list(v) if isinstance(v, tuple) else [v]


# name -> (call, output dtypes for a float32 / float64 raster as the golden tests pin them; None = the raster's)
FAMILIES = {
    "slope": (lambda na, Z: na.slope(Z), [None]),
    "evans_curvature": (lambda na, Z: na.evans_curvature(Z), [None] * 6),
    "focal_convolve": (lambda na, Z: na.focal_convolve(Z, W), [None]),
    "openness": (lambda na, Z: na.openness(Z, 1, 2), [np.float64]),
    "scaled_morphometry": (lambda na, Z: na.scaled_morphometry(Z, 1, 2), [None] * 8),
    "ashift": (lambda na, Z: na.ashift(Z, 2, 1), [None]),
    "nearest_source": (lambda na, Z: na.nearest_source(Z), [np.float64, np.int64]),
    "erosion": (lambda na, Z: na.erosion(Z, radius=1), [None]),
}


def _raster(name, dtype):
    """5 x 7, drawn once per family and dtype; nearest_source's has one hole"""
    rng = np.random.default_rng(20261102)
    Z = (rng.normal(size=(5, 7)) * 10).astype(dtype)
    if name == "nearest_source":
        Z[2, 3] = np.nan
    return Z


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_arrays_in_and_out(gpu_device, name, dtype):
    import torch
    na = _na()
    call, dtypes = FAMILIES[name]
    Z = _raster(name, dtype)
    before = Z.copy()
    # NumPy in, NumPy out, in the dtype the family's golden test pins
    host = _planes(call(na, Z))
    assert len(host) == len(dtypes)
    for h, d in zip(host, dtypes):
        assert isinstance(h, np.ndarray) and h.dtype == np.dtype(d or dtype), (name, h.dtype)
        assert h.shape[-2:] == Z.shape, name
    assert same_bits(Z, before)
    # a CUDA tensor in: tensors on its device, the same bits, the input untouched
    Zt = torch.from_numpy(Z).to(gpu_device)
    dev = _planes(call(na, Zt))
    assert len(dev) == len(host)
    for t, h in zip(dev, host):
        assert isinstance(t, torch.Tensor) and t.device == Zt.device, name
        assert same_bits(t.cpu().numpy(), h), name
    assert same_bits(Zt.cpu().numpy(), before), name
    # a transposed (non-contiguous) view: the bits of its contiguous copy
    Vt = torch.from_numpy(np.ascontiguousarray(Z.T)).to(gpu_device).t()
    assert not Vt.is_contiguous() and tuple(Vt.shape) == Z.shape
    for t, h in zip(_planes(call(na, Vt)), host):
        assert same_bits(t.cpu().numpy(), h), name


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_integer_rasters_are_float64_rasters(gpu_device, name):
    na = _na()
    call, _ = FAMILIES[name]
    Zi = np.round(_raster(name, np.float64)[:, ::-1] * 3)
    Zi = np.nan_to_num(Zi).astype(np.int32)
    a, b = _planes(call(na, Zi)), _planes(call(na, Zi.astype(np.float64)))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert same_bits(x, y), name


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_empty_rasters(gpu_device, name, dtype):
    """0 x 7: an empty result of the right dtype and shape.  slope is the exception it has always been: np.gradient
    needs two cells per axis, and says so before the device is touched"""
    na = _na()
    call, dtypes = FAMILIES[name]
    Z = np.zeros((0, 7), dtype)
    if name == "slope":
        with pytest.raises(ValueError, match=GRADIENT_MSG):
            call(na, Z)
        return
    got = _planes(call(na, Z))
    assert len(got) == len(dtypes)
    for g, d in zip(got, dtypes):
        assert isinstance(g, np.ndarray) and g.dtype == np.dtype(d or dtype), (name, g.dtype)
        assert g.shape[-2:] == (0, 7) and g.size == 0, (name, g.shape)


def evans_raster(dtype):
    """8 x 9 from a fixed seed: no NaN, and no cell whose quadratic is flat (D = E = 0)"""
    rng = np.random.default_rng(20261101)
    return (rng.normal(size=(8, 9)) * 10).astype(dtype)


@pytest.mark.parametrize("cellsize", [1, 2.5])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_evans_curvature_is_scaled_morphometry_at_stride_one(gpu_device, dtype, cellsize):
    """The two families share one quadratic (csrc/raster_stencil.h).  On a raster without NaN and without a flat cell
    neither evans_curvature's NaN fill nor its NaN repair acts, so its K, K_cross, K_long and K_tan (the outputs built
    from + - * / and sqrt only) are scaled_morphometry's at lookup_pixels=1, bit for bit - as the two restatements are."""
    na = _na()
    X = evans_raster(dtype)
    order = ("K", "K_profile", "K_plan", "K_tan", "K_long", "K_cross")       # evans_curvature's tuple
    exact = ("K", "K_cross", "K_long", "K_tan")
    ev_np, sm_np = dict(zip(order, sn.evans_curvature(X, cellsize))), mn.scaled_morphometry(X, cellsize, 1)
    assert sm_np["S"].min() > 0
    ev, sm = dict(zip(order, na.evans_curvature(X, cellsize))), na.scaled_morphometry(X, cellsize, 1)
    for k in exact:
        assert same_bits(ev_np[k], sm_np[k]) and not np.isnan(sm_np[k]).any(), k
        assert same_bits(ev[k], sm[k]), (k, int(np.sum(ev[k] != sm[k])))
        assert same_bits(ev[k], ev_np[k]), k
