"""Terrain analysis of a DTM: openness, sky-view factor, ternary terrain codes and geomorphons (MI355X only).

Mirrors, argument for argument, the reference functions (paths relative to the reference checkout):
``openness`` (neilpy/neilpy.py:1325), ``skyview_factor`` (:1360), ``ternary_pattern_from_openness`` (:1404),
``count_openness`` (:1600), ``geomorphons`` (:1617) and the host helpers ``progressive_window`` (:1314),
``int2base`` (:1438), ``get_lowest_equivalent`` (:1466), ``terrain_code_to_geomorphon`` (:1490) and
``geomorphon_cmap`` (:1544).  Build-specific options are keyword-only and come last.

Every raster function is one launch of the ray-march kernel family of ``csrc/terrain.hip``
(``smrf_terrain_rays_*``); the arithmetic contract is DESIGN.md section 9.  NumPy in -> NumPy out; a CUDA tensor in ->
a CUDA tensor out on the same device.  float32 and float64 rasters keep their dtype for the elevation differences (as
the reference does); other dtypes are widened to float64.  There is no CPU fallback: without the library or a GPU
every raster function raises :class:`neilpy_amd.SmrfHipError`.  The reference's functions stopped running under
NumPy 2 (``np.Inf``, ``np.float``, ``np.int``); the results here are what they compute with those names restored.
"""
import functools

import numpy as np

from . import _lib
from ._device import device_scoped as _device_scoped, is_tensor as _is_tensor
from ._raster import Raster, _ptr, _torch

__all__ = ["openness", "skyview_factor", "count_openness", "geomorphons", "ternary_pattern_from_openness",
           "progressive_window", "int2base", "get_lowest_equivalent", "terrain_code_to_geomorphon",
           "geomorphon_cmap", "GEOMORPHON_TABLE"]

_DLIST = np.array([np.sqrt(2), 1])      # neilpy.py:1336 / :1367: distance factor of even (diagonal) / odd directions

#: geomorphons()'s 9 x 9 table [num_pos, num_neg] -> class 1..10 (neilpy.py:1626-1636; Jasiewicz & Stepinski 2013)
GEOMORPHON_TABLE = np.zeros((9, 9), dtype=np.uint8)
GEOMORPHON_TABLE[0, :] = [1, 1, 1, 8, 8, 9, 9, 9, 10]
GEOMORPHON_TABLE[1, :8] = [1, 1, 8, 8, 8, 9, 9, 9]
GEOMORPHON_TABLE[2, :7] = [1, 4, 6, 6, 7, 7, 9]
GEOMORPHON_TABLE[3, :6] = [4, 4, 6, 6, 6, 7]
GEOMORPHON_TABLE[4, :5] = [4, 4, 5, 6, 6]
GEOMORPHON_TABLE[5, :4] = [3, 3, 5, 5]
GEOMORPHON_TABLE[6, :3] = [3, 3, 3]
GEOMORPHON_TABLE[7, :2] = [3, 3]
GEOMORPHON_TABLE[8, :1] = [2]
GEOMORPHON_TABLE.setflags(write=False)


# ------------------------------------------------------------------------------------------
# host helpers (scalar and table code)
# ------------------------------------------------------------------------------------------
def progressive_window(min_value, max_value, percent):
    """Window list growing by ``percent`` per step from ``min_value`` up to at most ``max_value`` (int32)."""
    this_list = np.array([min_value], dtype=np.int32)
    last_value = min_value
    while last_value < max_value:
        last_value = np.ceil(last_value * (100 + percent) / 100).astype(np.int32)
        if last_value <= max_value:
            this_list = np.append(this_list, last_value)
    return this_list


def int2base(x, b, alphabet='0123456789abcdefghijklmnopqrstuvwxyz', min_digits=8):
    """Base-``b`` string of the integer ``x``, zero-padded to ``min_digits``."""
    rets = ''
    while x > 0:
        x, idx = divmod(x, b)
        rets = alphabet[idx] + rets
    if len(rets) < min_digits:
        rets = '0' * (min_digits - len(rets)) + rets
    return rets


def get_lowest_equivalent(terrain_code):
    """Smallest terrain code among the rotations of ``terrain_code``'s 8 base-3 digits and of their reversal
    (the reference reverses the string at its 7th rotation; this follows the code, not its comment)."""
    s = int2base(terrain_code, 3)
    min_val = int(s, 3)
    for j in range(1, 16):
        s = s[-1] + s[:7]
        min_val = min(min_val, int(s, 3))
        if j == 7:
            s = s[::-1]
    return min_val


@functools.lru_cache(maxsize=None)
def _lowest_table():
    t = np.array([get_lowest_equivalent(x) for x in np.arange(3 ** 8)])
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _geomorphon_code_table(method):
    lookup_table = np.zeros(3 ** 8, np.uint8)
    if method == 'strict':
        for code, cls in ((3280, 1), (0, 2), (82, 3), (121, 4), (26, 5), (160, 6), (242, 7), (3293, 8), (4346, 9),
                          (6560, 10)):
            lookup_table[code] = cls
    else:
        for i in range(3 ** 8):
            base = int2base(i, 3)
            lookup_table[i] = GEOMORPHON_TABLE[base.count('2'), base.count('0')]
    lookup_table.setflags(write=False)
    return lookup_table


_device_tables = {}


def _device_table(name, table, device):
    key = (name, device)
    if key not in _device_tables:
        _device_tables[key] = _torch().from_numpy(np.array(table)).to(device)
    return _device_tables[key]


def terrain_code_to_geomorphon(terrain_code, method='loose'):
    """Geomorphon class (uint8, 0 = undefined) of each terrain code by the 'strict' or 'loose' table.

    The 6561-entry table is built on the host; a CUDA tensor of codes is looked up on its device.  An unknown
    ``method`` raises ``ValueError`` (the reference prints the options and then fails on an unbound name)."""
    method_options = ['strict', 'loose']
    if method not in method_options:
        raise ValueError('method should be one of %s' % method_options)
    table = _geomorphon_code_table(method)
    if _is_tensor(terrain_code):
        t = _device_table("geo_" + method, table, terrain_code.device)
        return t[terrain_code.long()]
    return table[terrain_code]


def geomorphon_cmap():
    """RGB colour of each geomorphon class 1..10."""
    return {1: (220, 220, 220),
            2: (56, 0, 0),
            3: (200, 0, 0),
            4: (255, 80, 20),
            5: (250, 210, 60),
            6: (255, 255, 60),
            7: (180, 230, 20),
            8: (60, 250, 150),
            9: (0, 0, 255),
            10: (0, 0, 56)}


# ------------------------------------------------------------------------------------------
# step lists and the distance table
# ------------------------------------------------------------------------------------------
def _as_steps(lookup_pixels, fast=False, how_fast=20):
    """The reference's step list, element types included (they feed the distance products below)."""
    if fast == True:  # noqa: E712  (the reference's own test)
        return list(progressive_window(1, lookup_pixels, how_fast))
    return list(np.arange(1, lookup_pixels + 1))


def _distance(cellsize, k, parity):
    """D(d, k) = (cellsize * k) * (sqrt(2) if d even else 1), the reference's expression and types (:1348-1349)."""
    return float(cellsize * k * _DLIST[parity])


class _March:
    """Step list, flags and the [2][n] distance table of one launch, on the device."""

    def __init__(self, main, small=(), cellsize=1):
        main_k = {int(k): k for k in main}
        small_k = {int(k): k for k in small}
        ks = sorted(set(main_k) | set(small_k))
        if ks and ks[0] < 1:
            raise ValueError("lookup steps must be >= 1")
        self.n = len(ks)
        self.max_step = ks[-1] if ks else 0
        self.steps = np.array(ks, dtype=np.int32)
        self.flags = np.array([(k in main_k) | (2 * (k in small_k)) for k in ks], dtype=np.uint8)
        self.dist = np.array([[_distance(cellsize, main_k.get(k, small_k.get(k)), p) for k in ks] for p in (0, 1)],
                             dtype=np.float64).reshape(-1)

    def to(self, device):
        torch = _torch()
        arrays = (self.steps, self.flags, self.dist) if self.n else \
            (np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(2, np.float64))     # no steps: nothing is read
        return tuple(torch.from_numpy(a).to(device) for a in arrays)


def _lookup_int(lookup_pixels):
    L = int(lookup_pixels)
    if L != lookup_pixels:
        raise TypeError("lookup_pixels must be an integer (got %r)" % (lookup_pixels,))
    return L


# ------------------------------------------------------------------------------------------
# the launch
# ------------------------------------------------------------------------------------------
def _rays(R, mode, march, outs, neighbors=None, dir_mask=0xFF, threshold=0.0, options=0, lut=None, impl=0):
    if R.rows == 0 or R.cols == 0:
        return
    if impl not in (_lib.TERRAIN_IMPL_AUTO, _lib.TERRAIN_IMPL_TILED, _lib.TERRAIN_IMPL_DIRECT):
        raise ValueError("impl must be one of 0 (auto), 1 (tiled), 2 (direct)")
    device = R.t.device
    steps, flags, dist = march.to(device)
    nbr = _torch().from_numpy(np.asarray(neighbors, dtype=np.int32)).to(device) if neighbors is not None else None
    o = list(outs) + [None] * (3 - len(outs))
    R.call("terrain_rays", _ptr(R.t), R.rows, R.cols, mode, _ptr(steps), _ptr(flags), _ptr(dist), march.n,
           march.max_step, _ptr(nbr), 0 if nbr is None else nbr.numel(), dir_mask, float(threshold), options, _ptr(lut),
           _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), int(impl))
    # the step tables are freed by the caching allocator on this stream only after the launch has read them


# ------------------------------------------------------------------------------------------
# public raster functions
# ------------------------------------------------------------------------------------------
@_device_scoped
def openness(Z, cellsize=1, lookup_pixels=1, neighbors=np.arange(8), skyview=False, fast=False, how_fast=20, *,
             impl=_lib.TERRAIN_IMPL_AUTO):
    """Mean over ``neighbors`` of each direction's smallest zenith angle within ``lookup_pixels`` steps, in degrees.

    Same arguments and results as neilpy.openness (``skyview`` is accepted and ignored there too).  A direction whose
    samples are all NaN contributes +inf.  Deviation: ``neighbors`` entries outside 0..7 or an empty list raise
    ``ValueError`` (the reference silently treats an unknown direction as flat and averages an empty list to NaN).
    """
    torch = _torch()
    nb = np.asarray(neighbors).reshape(-1)
    if nb.size == 0:
        raise ValueError("neighbors must not be empty")
    if not np.issubdtype(nb.dtype, np.integer) or nb.min() < 0 or nb.max() > 7:
        raise ValueError("neighbors must hold directions 0..7 (got %s)" % (list(nb),))
    R = Raster(Z)
    out = R.empty(torch.float64)
    march = _March(_as_steps(_lookup_int(lookup_pixels), fast, how_fast), cellsize=cellsize)
    mask = int(np.bitwise_or.reduce(1 << nb.astype(np.int64)))
    _rays(R, _lib.TERRAIN_OPENNESS, march, [out], neighbors=nb, dir_mask=mask, impl=impl)
    return R.out(out)


@_device_scoped
def skyview_factor(Z, cellsize=1, lookup_pixels=1, *, impl=_lib.TERRAIN_IMPL_AUTO):
    """1 - mean over the 8 directions of sin(largest elevation angle, clipped at 0) within ``lookup_pixels`` steps.

    Same arguments and results as neilpy.skyview_factor (float64); a ray stops at the raster's edge."""
    torch = _torch()
    R = Raster(Z)
    out = R.empty(torch.float64)
    L = _lookup_int(lookup_pixels)
    march = _March(list(range(1, L + 1)), cellsize=cellsize)      # python ints, as the reference's range (:1370)
    _rays(R, _lib.TERRAIN_SKYVIEW, march, [out], impl=impl)
    return R.out(out)


def _counts(R, cellsize, lookup_pixels, threshold_angle, fast, how_fast, want_counts, want_geo, enhance, impl):
    torch = _torch()
    L = _lookup_int(lookup_pixels)
    small = ()
    if enhance:
        Lsm = int(np.floor(L / 4))
        Lsm = max(Lsm, 4)
        small = list(np.arange(1, Lsm + 1))
    march = _March(_as_steps(L, fast, how_fast), small, cellsize=cellsize)
    mk = lambda: R.empty(torch.uint8)  # noqa: E731
    pos, neg = (mk(), mk()) if want_counts else (None, None)
    geo = mk() if want_geo else None
    lut = _device_table("geo9", GEOMORPHON_TABLE, R.t.device) if want_geo else None
    _rays(R, _lib.TERRAIN_COUNT, march, [pos, neg, geo], threshold=threshold_angle,
          options=2 if enhance else 0, lut=lut, impl=impl)
    return pos, neg, geo


@_device_scoped
def count_openness(Z, cellsize, lookup_pixels, threshold_angle, fast=False, how_fast=20, *,
                   impl=_lib.TERRAIN_IMPL_AUTO):
    """``(num_pos, num_neg)`` (uint8): per cell, the directions whose positive minus negative openness is above
    ``threshold_angle`` / below ``-threshold_angle`` degrees.  Same arguments and results as neilpy.count_openness."""
    R = Raster(Z)
    pos, neg, _ = _counts(R, cellsize, lookup_pixels, threshold_angle, fast, how_fast, True, False, False, impl)
    return R.out(pos), R.out(neg)


@_device_scoped
def geomorphons(Z, cellsize=1, lookup_pixels=1, threshold_angle=1, enhance=False, fast=False, how_fast=20, *,
                impl=_lib.TERRAIN_IMPL_AUTO):
    """Geomorphon class 1..10 (uint8) of each cell from its openness counts (9 x 9 table, :data:`GEOMORPHON_TABLE`).

    Same arguments and results as neilpy.geomorphons.  ``enhance=True`` with ``lookup_pixels > 16`` also counts with
    ``max(lookup_pixels // 4, 4)`` steps and applies the reference's correction of forms (:1640-1649); both counts
    come from one march.
    """
    R = Raster(Z)
    enh = enhance == True and lookup_pixels > 16  # noqa: E712  (the reference's own test, :1640)
    _, _, geo = _counts(R, cellsize, lookup_pixels, threshold_angle, fast, how_fast, False, True, enh, impl)
    return R.out(geo)


@_device_scoped
def ternary_pattern_from_openness(Z, cellsize=1, lookup_pixels=1, threshold_angle=0, use_negative_openness=True,
                                  lowest=False, *, impl=_lib.TERRAIN_IMPL_AUTO):
    """Terrain code sum_i digit_i * 3**i (int64), digit 2 / 1 / 0 where direction i's openness difference is above
    ``threshold_angle``, within it, or below ``-threshold_angle``; ``lowest=True`` maps each code to its lowest
    rotation / reflection equivalent.  Same arguments and results as neilpy.ternary_pattern_from_openness under
    NumPy 2 (whose type promotion turns the reference's uint16 accumulator into int64)."""
    torch = _torch()
    R = Raster(Z)
    out = R.empty(torch.int64)
    march = _March(_as_steps(_lookup_int(lookup_pixels)), cellsize=cellsize)
    lut = _device_table("lowest", _lowest_table().astype(np.int64), R.t.device) if lowest else None
    _rays(R, _lib.TERRAIN_TERNARY, march, [out], threshold=threshold_angle,
          options=1 if use_negative_openness else 0, lut=lut, impl=impl)
    return R.out(out)
