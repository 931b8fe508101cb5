"""The row-band driver makes the calls it made before its row arithmetic moved into sharded.band_plan.

tests/golden/band_trace.json holds every ops call and exchange of progressive_filter_sharded, with its integer arguments
and the rows of each buffer it touches, recorded before that change (tests/golden/make_golden_band_trace.py: the
cases, the scripted routings and the recorder).  The same cases run again here through ``comm=`` - on CPU tensors, in
process, no process group - and must give the identical call sequence.
"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

spec = importlib.util.spec_from_file_location("make_golden_band_trace", os.path.join(GOLDEN, "make_golden_band_trace.py"))
rec = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rec)
KEYS = dict(rec.keys())


@pytest.fixture(scope="module")
def traces():
    with open(os.path.join(GOLDEN, "band_trace.json")) as f:
        return json.load(f)["traces"]


def test_trace_file_covers_the_cases(traces):
    from neilpy_amd import _lib
    assert (rec.ROUTE_TWO_PASS, rec.ROUTE_FUSED, rec.ROUTE_CHAIN) == (_lib.ROUTE_TWO_PASS, _lib.ROUTE_FUSED, _lib.ROUTE_CHAIN)
    assert sorted(traces) == sorted(KEYS) and len(KEYS) == 90 + 6           # 15 ranks x 3 routings x overlap off / on, + NaNs
    kinds = {c[0] for t in traces.values() for c in t}
    assert kinds == {"head_launch", "chain_flag", "open_flag", "erode", "dilate_flag", "exchange"}
    assert not any(c[0] in ("head_launch", "chain_flag", "open_flag") for k, t in traces.items() if "/nan/" in k for c in t)


@pytest.mark.parametrize("case", list(rec.CASES))
def test_driver_replays_the_recorded_calls(traces, case):
    for key, args in KEYS.items():
        if args[0] == case:
            assert rec.trace(*args) == traces[key], key
