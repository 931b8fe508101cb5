"""Checks that every raster family's tests make the same way: signatures against the reference's, the generated code of
a csrc unit, and array comparisons (bit for bit, or within ulps where a transcendental function is involved)."""
import inspect
import json
import os
import re
import subprocess

import numpy as np

from conftest import GOLDEN

ULPS = 8


def signatures_match(json_name, count):
    """Every function of tests/golden/<json_name> has the reference's parameters (name, kind, default) in the
    reference's order; parameters this package adds come after them and are keyword-only.  Returns the JSON."""
    import neilpy_amd
    with open(os.path.join(GOLDEN, json_name)) as f:
        want = json.load(f)
    assert len(want) == count
    for name, params in want.items():
        got = list(inspect.signature(getattr(neilpy_amd, name)).parameters.values())
        assert len(got) >= len(params), name
        for g, p in zip(got, params):
            assert (g.name, g.kind.name) == (p["name"], p["kind"]), (name, g, p)
            assert (None if g.default is inspect.Parameter.empty else repr(g.default)) == p["default"], (name, g, p)
        for g in got[len(params):]:
            assert g.kind is inspect.Parameter.KEYWORD_ONLY, (name, g)
    return want


def device_asm(unit, tmp_path):
    """csrc/<unit>.hip compiled to gfx950 assembly with the library's flags (no GPU needed):
    ``(text, {kernel name: its .amdhsa_kernel block})``"""
    from neilpy_amd.build import CSRC, FLAGS, hipcc
    out = str(tmp_path / (unit + ".s"))
    cmd = [hipcc()] + [f for f in FLAGS if f != "-fPIC"] + ["--offload-device-only", "-S",
                                                           os.path.join(CSRC, unit + ".hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    return text, dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))


def assert_no_scratch(text, kernels):
    """every kernel keeps its state in registers"""
    for name, body in kernels.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    assert set(re.findall(r"ScratchSize:\s*(\d+)", text)) == {"0"}


def same_bits(a, b):
    """dtype, shape, values, NaN positions and the signs of zeros"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and \
        np.array_equal(np.signbit(a[a == 0]), np.signbit(b[b == 0]))


def assert_exact(got, want, ctx):
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=True), (ctx, int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want))))))


def assert_close(got, want, scale, ctx, unit=None, circular=None):
    """Within ULPS units in the last place of each value plus ULPS ulps of ``scale``, NaN and inf positions identical.
    ``unit``: the dtype whose ulp of ``scale`` is allowed (hillshade's float64 shade of a float32 raster carries float32
    cos / sin); ``circular``: the period of an angle, compared on the shorter arc."""
    assert got.dtype == want.dtype and got.shape == want.shape, (ctx, got.dtype, want.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), ctx
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), ctx
    fin = np.isfinite(want)
    if fin.any():
        unit = np.dtype(unit or want.dtype)
        tol = ULPS * (np.spacing(np.abs(want[fin]).astype(want.dtype)).astype(np.float64) +
                      float(np.spacing(unit.type(scale))))
        err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
        if circular is not None:
            err = np.minimum(err, circular - err)
        assert np.all(err <= tol), (ctx, float(np.max(err / tol)))
