"""The side-stream harness (tests/streamed.py) as far as it can be proven without a GPU: where the stream goes in every
declaration, what the recording proxy does to a call, when tests/guarded.py's hook runs, and that every guarded export
has a stream case."""
import ctypes as C
import re

import pytest
import torch

import guarded as G
import streamed as S

# entries of include/smrf_hip.h that launch nothing: sizes, version, device count, error text, plans and switches
NO_LAUNCH = re.compile(r"^smrf_(\w+_workspace_bytes|abi_version|device_count|last_error|switches_reload|pf_plan|pf_chain_length|"
                       r"pf_ero_inc_windows|fused_open_supported|focal_fits_tile|springs_band_layout|assign_limit|assign_route|"
                       r"footprint_tile_bytes|footprint_path)$")


def test_every_launching_entry_has_a_stream_slot():
    from neilpy_amd import _lib
    decl, slots = S.declarations(), S.stream_slots()
    assert set(decl) == set(_lib.SIGNATURES)
    launching = sorted(n for n in _lib.SIGNATURES if not NO_LAUNCH.match(n))
    assert len(launching) == 79 and len(_lib.SIGNATURES) - len(launching) == 24
    for n in launching:
        k = slots[n]
        assert k is not None, n + " launches and takes no stream"
        assert len(decl[n]) == len(_lib.SIGNATURES[n][1]) and _lib.SIGNATURES[n][1][k] is C.c_void_p, n
    assert all(slots[n] is None for n in _lib.SIGNATURES if NO_LAUNCH.match(n))
    # not always last
    assert slots["smrf_progressive_filter_timed_f32"] == 12 and len(decl["smrf_progressive_filter_timed_f32"]) == 15
    assert slots["smrf_progressive_filter_f32"] == 12 == len(decl["smrf_progressive_filter_f32"]) - 1
    assert slots["smrf_ashift_f64"] == 6


def test_the_parser_on_a_declaration_of_its_own():
    text = ("SMRF_API int smrf_one(const float* d_a /* in, out */, int64_t n,\n          void* stream, float* h_ms);\n"
            "SMRF_API size_t smrf_two(void);\nSMRF_API const char* smrf_three(int stream_count);\n")
    assert S.declarations(text) == {"smrf_one": ["d_a", "n", "stream", "h_ms"], "smrf_two": [], "smrf_three": ["stream_count"]}
    assert S.stream_slots(text) == {"smrf_one": 2, "smrf_two": None, "smrf_three": None}


class Lib:
    value = 7

    def __init__(self):
        self.got = []

    def smrf_fake(self, ptr, n, stream):
        self.got.append((ptr, n, stream))
        return ("result", n)

    def smrf_plain(self, n):
        return n + 1

    def smrf_raises(self, stream):
        raise ZeroDivisionError


def test_the_proxy_forwards_and_records():
    from neilpy_amd import _lib
    real, before = Lib(), _lib._lib
    p, st = C.c_void_p(64), C.c_void_p(0xABC0)
    with S.recording(real, {"smrf_fake": 2, "smrf_raises": 0}) as rec:
        lib = _lib.load()
        assert lib is rec and lib is not real
        assert lib.smrf_fake(p, 5, st) == ("result", 5)                # the return value as it is
        assert lib.smrf_fake(p, 6, None) == ("result", 6)
        assert lib.smrf_fake(p, 7, 0x10) == ("result", 7)
        assert lib.smrf_plain(1) == 2 and lib.value == 7
    assert real.got[0][0] is p and real.got[0][2] is st and real.got[1][2] is None      # the arguments as they are
    assert rec.calls == [("smrf_fake", 0xABC0), ("smrf_fake", 0), ("smrf_fake", 0x10)]
    assert _lib._lib is before
    with pytest.raises(S.HandleError, match="smrf_fake got 0x0"):
        S.check_handles(rec.calls, {0xABC0, 0x10}, "t")
    with pytest.raises(S.HandleError, match="smrf_fake got 0x10"):
        S.check_handles(rec.calls[:1] + rec.calls[2:], {0xABC0}, "t")
    with pytest.raises(S.HandleError, match="no library call"):
        S.check_handles([], {0xABC0}, "t")
    S.check_handles(rec.calls[:1], {0xABC0}, "t")


def test_the_proxy_is_removed_after_an_exception():
    from neilpy_amd import _lib
    before = _lib._lib
    with pytest.raises(ZeroDivisionError):
        with S.recording(Lib(), {"smrf_raises": 0}) as rec:
            _lib.load().smrf_raises(C.c_void_p(3))
    assert _lib._lib is before and rec.calls == [("smrf_raises", 3)]
    with pytest.raises(KeyError):
        with S.recording(Lib(), {}):
            raise KeyError("body")
    assert _lib._lib is before


def test_the_hook_runs_once_per_allocation_and_before_the_fill():
    events = []
    fill = G._ORIG["full"]

    def hook():
        events.append("hook")

    def full(*a, **k):
        events.append("fill")
        return fill(*a, **k)
    G._ORIG["full"] = full
    try:
        with G.guarded("cpu", 0x5A, before_fill=hook) as g:
            torch.empty((3, 5), dtype=torch.float32)
            torch.zeros(7, dtype=torch.int64)
            g.tensor(torch.arange(4.0))
            g.bytes_of(13)
            torch.empty(0)                                   # passes through: no arena, no hook
            torch.empty(4, device="meta")
            assert len(g.arenas) == 4 and events == ["hook", "fill"] * 4
            g.before_fill = None
            torch.empty(2)
            assert len(g.arenas) == 5 and events == ["hook", "fill"] * 4 + ["fill"]
        g.check()
        with G.guarded("cpu", 0x5A) as g:                    # no hook: as before
            torch.empty(2)
        assert events == ["hook", "fill"] * 4 + ["fill"] * 2 and g.before_fill is None
    finally:
        G._ORIG["full"] = fill


def test_a_decoy_is_another_draw_of_the_same_values():
    import numpy as np
    a = np.random.default_rng(1).normal(size=(5, 7)).astype(np.float32)
    a[2, 3] = np.nan
    d = S.decoy_of(a)
    assert d.shape == a.shape and d.dtype == a.dtype and d.tobytes() != a.tobytes()
    assert np.array_equal(np.sort(d.ravel()), np.sort(a.ravel()), equal_nan=True)
    assert S.decoy_of(a, 1).tobytes() != d.tobytes() and S.decoy_of(a).tobytes() == d.tobytes()
    two = np.array([1.0, 2.0])
    assert S.decoy_of(two).tobytes() != two.tobytes()


def test_every_guarded_export_has_a_stream_case():
    """tests/test_gpu_streams.py runs, per name of family_cases.GUARDED (which tests/test_guarded_host.py ties to the
    package's exports), the cases that name's builder marks for it, and fails on the GPU where a builder marks none: a
    family added later cannot join without a stream case"""
    import family_cases as T
    import test_gpu_streams as M
    assert set(T.BUILDERS) == set(T.GUARDED), sorted(set(T.BUILDERS) ^ set(T.GUARDED))
    assert not T.LEFT_OUT                                    # a name left out there needs its written reason here as well
    assert set(T.EXTRA) == {"smrf_spline", "sharded"} and not set(T.EXTRA) & set(T.GUARDED)
    marks = {f: [m.args for m in getattr(M, f).pytestmark if m.name == "parametrize"] for f in ("test_family", "test_extra")}
    assert marks == {"test_family": [("name", T.GUARDED)], "test_extra": [("name", sorted(T.EXTRA))]}, marks
    assert set(M.OPTIONS) <= set(T.EXTRA)
