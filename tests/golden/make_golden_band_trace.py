#!/usr/bin/env python3
"""Generate tests/golden/band_trace.json: every call neilpy_amd.sharded.progressive_filter_sharded makes.

This project's own output, not the reference's: the file was first written by this recorder at the commit before the
band plan (sharded.band_plan) existed, with the halo exchange stubbed at that commit's module-level exchange function,
and pins "the same launches as before" (tests/test_band_trace_host.py replays the cases and compares).  It runs
in-process on CPU tensors, no process group and no GPU: a recording ops object stands in for HipBandOps and a
recording communicator for the neighbours.

A trace is the list of calls in order.  A call is ``[name, argument, ...]``; a tensor argument is
``[buffer, first row, rows]`` with buffers numbered by storage in order of first appearance, ``None`` stays ``null``.
``band_trace.json``: ``{"traces": {"<case>/<script>/o<overlap>/r<rank>": [call, ...]}}``.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
COLS = 4

# (world, raster rows, windows, halo budget)
CASES = {
    "w1_40": (1, 40, [1, 2, 9], None),
    "w2_96": (2, 96, [1, 2, 3, 5, 8], None),
    "w2_96_b0": (2, 96, [1, 2, 3, 5, 8], 0),
    "w3_150": (3, 150, [2, 1, 7, 11], 20),
    "w4_512": (4, 512, list(range(1, 11)), 40),
    "w3_331": (3, 331, [1, 2, 3, 5, 4, 8], 24),
}
SCRIPTS = ("two_pass", "fused", "chain")
NAN_CASE = "w3_331"                                           # also traced with a has_nan that answers True

ROUTE_TWO_PASS, ROUTE_FUSED, ROUTE_CHAIN = 0, 1, 4            # neilpy_amd._lib's values (asserted in the test)


def head_script(script, radii, chain):
    """what a scripted HipBandOps.head_launch answers for the windows ``radii`` left in a group"""
    if script == "chain" and chain and radii[0] <= 3:
        n = 1
        while n < min(3, len(radii)) and radii[n] <= 3:
            n += 1
        return ROUTE_CHAIN, n
    if script != "two_pass" and radii[0] <= 5:
        return ROUTE_FUSED, 1
    return ROUTE_TWO_PASS, 1


class Recorder:
    """the calls of one run; tensors by (buffer, first row, rows)"""

    def __init__(self):
        self.calls, self.buffers = [], {}

    def arg(self, v):
        import torch
        if isinstance(v, torch.Tensor):
            buf = self.buffers.setdefault(v.untyped_storage().data_ptr(), len(self.buffers))
            return [buf, v.storage_offset() // COLS, v.shape[0]]
        if isinstance(v, (list, tuple)):
            return [self.arg(x) for x in v]
        if isinstance(v, (bool, np.bool_)):
            return bool(v)
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            return float(v)
        assert v is None, v
        return None

    def add(self, name, *args, **kw):
        self.calls.append([name] + [self.arg(v) for v in args] + [[k, self.arg(v)] for k, v in sorted(kw.items())])


class RecordingOps:
    def __init__(self, rec, script):
        self.rec, self.script = rec, script

    def head_launch(self, t, radii, img_rows, cells, chain=True):
        self.rec.add("head_launch", t, radii, img_rows, cells, chain)
        return head_script(self.script, radii, chain)

    def chain_flag(self, *args):
        self.rec.add("chain_flag", *args)

    def open_flag(self, *args):
        self.rec.add("open_flag", *args)

    def erode(self, *args, **kw):
        self.rec.add("erode", *args, **kw)

    def dilate_flag(self, *args, **kw):
        self.rec.add("dilate_flag", *args, **kw)


class NanRecordingOps(RecordingOps):
    def has_nan(self, band):
        return True


def drive(rec, ops, Z, img_rows, win, thr, rank, world, budget, overlap):
    """one call of the driver with the exchange recorded instead of made"""
    from neilpy_amd import sharded

    class RecordingComm(sharded.BandComm):
        def exchange(self, send_up, recv_up, send_down, recv_down):
            rec.add("exchange", send_up, recv_up, send_down, recv_down)

    sharded.progressive_filter_sharded(Z, img_rows, win, thr, rank=rank, world_size=world, ops=ops,
                                       return_when_dropped=True, halo_budget=budget, overlap=overlap,
                                       comm=RecordingComm(None, rank, world))


def trace(case, script, overlap, rank, nan=False):
    import torch
    from neilpy_amd import sharded
    world, rows, windows, budget = CASES[case]
    b0, b1 = sharded.band_rows(rows, world, rank)
    rec = Recorder()
    ops = (NanRecordingOps if nan else RecordingOps)(rec, script)
    win = np.asarray(windows)
    drive(rec, ops, torch.zeros((b1 - b0, COLS), dtype=torch.float32), rows, win, .15 * (win * 1), rank, world, budget,
          overlap)
    return rec.calls


def keys():
    """(key, trace arguments) of every recorded run"""
    for case, (world, _, _, _) in CASES.items():
        for script in SCRIPTS:
            for overlap in (False, True):
                for rank in range(world):
                    yield "%s/%s/o%d/r%d" % (case, script, overlap, rank), (case, script, overlap, rank, False)
    for overlap in (False, True):
        for rank in range(CASES[NAN_CASE][0]):
            yield "%s/nan/o%d/r%d" % (NAN_CASE, overlap, rank), (NAN_CASE, "chain", overlap, rank, True)


def main():
    sys.path.insert(0, ROOT)
    traces = {k: trace(*a) for k, a in keys()}
    out = os.path.join(HERE, "band_trace.json")
    with open(out, "w") as f:
        json.dump({"traces": traces}, f, separators=(",", ":"))
        f.write("\n")
    print("band_trace.json: %d traces, %d calls, %.0f kB" % (len(traces), sum(len(t) for t in traces.values()),
                                                            os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
