"""Local surface derivatives of a DTM: slope, aspect, hillshade and curvatures (MI355X only).

Mirrors, argument for argument, the reference functions (paths relative to the reference checkout):
``esri_slope`` (neilpy/neilpy.py:434), ``slope`` (:456), ``aspect`` (:471), ``curvature`` (:487), ``esri_curvature``
(:520), ``zevenbergen_and_thorne_curvature`` (:596), ``evans_curvature`` (:671), ``wilson_gallant_curvature`` (:753),
``hillshade`` (:814), ``multiple_illumination`` (:830) and the host helper ``z_factor`` (:871).

Every raster function is one launch of the 3 x 3 stencil kernel family of ``csrc/surface.hip`` (``smrf_surface_*``);
the multi-output curvatures write all their rasters from one read of the DTM.  The arithmetic contract is DESIGN.md
section 10.  NumPy in -> NumPy out; a CUDA tensor in -> a CUDA tensor out on the same device.  float32 and float64
rasters keep their dtype wherever the reference keeps it (hillshade's float output is float64, as NumPy 2 promotes
it); other dtypes are widened to float64.  There is no CPU fallback: without the library or a GPU every raster function
raises :class:`neilpy_amd.SmrfHipError`.

Deviations from the reference (each in DESIGN.md section 10): an unsupported ``return_as`` of ``slope`` / ``aspect``
raises ``ValueError``; NumPy-scalar parameters are taken as Python floats; the np.gradient functions (``slope``,
``aspect``, ``hillshade``, ``multiple_illumination``) raise ``ValueError`` below 2 cells per axis; ``esri_slope`` squares
its window differences by a product where the reference's per-cell callback calls C ``pow``.
"""
import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped
from ._raster import Raster, _ptr, _pyfloat as _f, _torch

__all__ = ["slope", "aspect", "hillshade", "multiple_illumination", "esri_slope", "curvature", "esri_curvature",
           "zevenbergen_and_thorne_curvature", "evans_curvature", "wilson_gallant_curvature", "z_factor"]

_GRADIENT_MSG = ("Shape of array too small to calculate a numerical gradient, "
                 "at least (edge_order + 1) elements are required.")


# ------------------------------------------------------------------------------------------
# host helpers (scalar code)
# ------------------------------------------------------------------------------------------
def z_factor(latitude):
    """z-factor of a degree-referenced DEM at ``latitude`` (degrees): vertical units per degree of arc."""
    latitude = np.deg2rad(latitude)
    a = 6378137
    b = 6356752.3
    numer = (a ** 4) * (np.cos(latitude) ** 2) + (b ** 4) * (np.sin(latitude) ** 2)
    denom = (a * np.cos(latitude)) ** 2 + (b * np.sin(latitude)) ** 2
    return 1 / (np.pi / 180 * np.cos(latitude) * np.sqrt(numer / denom))


def _angle_row(zenith, azimuth):
    """(cos zenith, sin zenith, azimuth) in radians, float64: hillshade's np.deg2rad((zenith, azimuth))"""
    z, a = np.deg2rad((zenith, azimuth))
    return [float(np.cos(z)), float(np.sin(z)), float(a)]


def _angle_lists(zeniths, azimuths):
    """multiple_illumination's expansion: a scalar azimuths is arange(0, 360, 360 / n), a scalar zeniths is
    arange(s, 90, s) with s = 90 / (zeniths + 1)"""
    if np.isscalar(azimuths):
        azimuths = np.arange(0, 360, 360 / azimuths)
    if np.isscalar(zeniths):
        zeniths = 90 / (zeniths + 1)
        zeniths = np.arange(zeniths, 90, zeniths)
    return zeniths, azimuths


# ------------------------------------------------------------------------------------------
# the launch
# ------------------------------------------------------------------------------------------
def _need_gradient(Z):
    """np.gradient's size check, made before anything touches the device"""
    shape = tuple(np.shape(Z))
    if len(shape) == 2 and min(shape) < 2:
        raise ValueError(_GRADIENT_MSG)


def _launch(R, mode, outs, params=(), options=0, angles=None):
    p = [float(v) for v in params] + [0.0] * (4 - len(params))
    o = list(outs) + [None] * (6 - len(outs))
    tab = None
    if angles is not None:
        tab = _torch().from_numpy(np.asarray(angles, dtype=np.float64).reshape(-1)).to(R.t.device)
    R.call("surface", _ptr(R.t), R.rows, R.cols, mode, options, p[0], p[1], p[2], p[3], _ptr(tab),
           0 if angles is None else len(angles), *[_ptr(t) for t in o])
    # the angle table is freed by the caching allocator on this stream only after the launch has read it


def _check_return_as(return_as, options):
    if return_as not in options:
        raise ValueError("return_as %r is not supported (one of %s)" % (return_as, list(options)))


# ------------------------------------------------------------------------------------------
# public raster functions
# ------------------------------------------------------------------------------------------
@_device_scoped
def slope(Z, cellsize=1, z_factor=1, return_as='degrees'):
    """Slope from np.gradient with spacing ``cellsize / z_factor``: 'degrees', 'radians' or 'percent' (the gradient
    norm, 1 = 100 %).  Same arguments and results as neilpy.slope."""
    _check_return_as(return_as, ('degrees', 'radians', 'percent'))
    _need_gradient(Z)
    R = Raster(Z)
    h = _f(cellsize) / _f(z_factor)
    opt = {'percent': 0, 'radians': _lib.SURFACE_OPT_RADIANS, 'degrees': _lib.SURFACE_OPT_DEGREES}[return_as]
    S = R.empty()
    _launch(R, _lib.SURFACE_SLOPE, [S], (h,), opt)
    return R.out(S)


@_device_scoped
def aspect(Z, return_as='degrees', flat_as='nan'):
    """Aspect clockwise from north, from np.gradient at unit spacing, in 'degrees' or 'radians'; cells with a zero
    gradient get ``flat_as`` ('nan' or a number).  Same arguments and results as neilpy.aspect."""
    _check_return_as(return_as, ('degrees', 'radians'))
    flat = np.nan if isinstance(flat_as, str) and flat_as == 'nan' else _f(flat_as)
    _need_gradient(Z)
    R = Raster(Z)
    A = R.empty()
    _launch(R, _lib.SURFACE_ASPECT, [A], (flat,), _lib.SURFACE_OPT_DEGREES if return_as == 'degrees' else 0)
    return R.out(A)


@_device_scoped
def hillshade(Z, cellsize=1, z_factor=1, zenith=45, azimuth=315, return_uint8=True):
    """ESRI-style hillshade from slope(radians) and aspect(radians, flat_as=0): uint8 ``round(255 * H)`` (NaN cells
    0), or H as float64 with ``return_uint8=False``.  Same arguments and results as neilpy.hillshade."""
    _need_gradient(Z)
    R = Raster(Z)
    h = _f(cellsize) / _f(z_factor)
    H = R.empty(_torch().uint8 if return_uint8 else _torch().float64)
    outs = [H] if return_uint8 else [None, H]
    _launch(R, _lib.SURFACE_HILLSHADE, outs, (h,), angles=[_angle_row(zenith, azimuth)])
    return R.out(H)


@_device_scoped
def multiple_illumination(Z, cellsize=1, z_factor=1, zeniths=np.array([45]), azimuths=4):
    """Largest uint8 hillshade over every zenith x azimuth pair (scalar arguments expand as the reference's do).
    Slope and aspect are computed once per cell; the pairs are a table walked in registers.  Same arguments and
    results as neilpy.multiple_illumination."""
    zs, azs = _angle_lists(zeniths, azimuths)
    _need_gradient(Z)
    R = Raster(Z)
    H = R.empty(_torch().uint8)
    table = [_angle_row(z, a) for z in zs for a in azs]
    if not table:
        H.zero_()
    else:
        _launch(R, _lib.SURFACE_HILLSHADE, [H], (_f(cellsize) / _f(z_factor),), angles=table)
    return R.out(H)


@_device_scoped
def esri_slope(Z, cellsize=1, z_factor=1, return_as='degrees'):
    """ESRI's 3 x 3 (Horn) slope with ndimage's 'reflect' edges, divided by ``cellsize`` and scaled by ``z_factor``;
    in degrees for return_as='degrees', otherwise the rise over run.  Same arguments and results as neilpy.esri_slope
    (which accepts any other ``return_as`` as "not degrees")."""
    R = Raster(Z)
    S = R.empty()
    _launch(R, _lib.SURFACE_HORN, [S], (_f(cellsize), _f(z_factor)),
            _lib.SURFACE_OPT_DEGREES if return_as == 'degrees' else 0)
    return R.out(S)


@_device_scoped
def curvature(X, cellsize=1):
    """``-100 * laplace(X / cellsize)`` with ndimage's 'reflect' edges.  Same arguments and results as
    neilpy.curvature."""
    R = Raster(X)
    K = R.empty()
    _launch(R, _lib.SURFACE_LAPLACE, [K], (_f(cellsize),))
    return R.out(K)


def _multi(X, mode, n, params):
    R = Raster(X)
    outs = [R.empty() for _ in range(n)]
    _launch(R, mode, outs, params)
    return tuple(R.out(t) for t in outs)


@_device_scoped
def esri_curvature(X, cellsize=1):
    """``(K, K_plan, K_profile)``: ESRI's curvatures (Zevenbergen & Thorne, signs reversed, x 100).  A NaN or
    off-raster neighbour is the cell itself; NaN plan / profile curvature is 0.  Same results as
    neilpy.esri_curvature."""
    L = _f(cellsize)
    return _multi(X, _lib.SURFACE_ESRI, 3, (L ** 2, 4 * (L ** 2), 2 * L))


@_device_scoped
def zevenbergen_and_thorne_curvature(X, cellsize=1):
    """``(K, K_profile, K_plan, K_tan, K_long, K_cross)`` of Zevenbergen & Thorne (1987), NaN neighbours filled as
    2X - opposite.  Same results as neilpy.zevenbergen_and_thorne_curvature, its ``D*E**2`` in K_plan included."""
    L = _f(cellsize)
    return _multi(X, _lib.SURFACE_ZT, 6, (L ** 2, 4 * (L ** 2), 2 * L))


@_device_scoped
def evans_curvature(X, cellsize=1):
    """``(K, K_profile, K_plan, K_tan, K_long, K_cross)`` from Evans' quadratic (Wood 1991); NaN ratios are 0 where X
    is finite.  Same results as neilpy.evans_curvature."""
    L = _f(cellsize)
    return _multi(X, _lib.SURFACE_EVANS, 6, (6 * L ** 2, 3 * L ** 2, 4 * L ** 2, 6 * L))


@_device_scoped
def wilson_gallant_curvature(X, cellsize=1):
    """``(K, Kp, Kc, Kt)`` of Wilson & Gallant (2000).  Same results as neilpy.wilson_gallant_curvature, its quirks
    included: Z7 = Z8 = X, ZXY multiplied by H**2 and Kt sharing Kp's numerator."""
    H = _f(cellsize)
    return _multi(X, _lib.SURFACE_WG, 4, (2 * H, H ** 2))
