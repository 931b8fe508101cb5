"""Row-band sharded progressive_filter: one process per GPU, halo exchange between neighbours.

The raster's rows are split into ``world_size`` contiguous bands.  A grey opening by ``disk(r)``
needs ``last`` on 2r rows either side of the band (r for the erosion the dilation reads, r more
for that erosion's own footprint), so a window costs 2r rows of the neighbours' bands.
Consecutive windows are grouped (``window_groups``): a group does ONE exchange of sum(2r) rows
with each neighbour (RCCL send/recv over the direct xGMI link; nearest-neighbour only, no
collective) and recomputes its shrinking margins redundantly, so windows 1..50 on 2048-row bands
take 12 exchanges instead of 50.
Image borders use scipy's reflect rule inside the kernels, exactly as on one GPU, so the result
is bit-identical to the single-device path (neilpy.py:1659-1680 semantics).

Overlap (``overlap=True``): the rows a group's exchange sends are the band's outermost sum(2r) rows of the
surface the previous group leaves.  That group's last dilation is split: the two edge strips run first, on
a side stream, followed by the exchange; the interior runs beside them on the main stream, which only
waits for the exchange before the next group's first erosion.

The communication goes through one :class:`BandComm` (``torch.distributed``: ``nccl`` = RCCL with CUDA tensors, ``gloo``
with CPU tensors), the compute through a ``BandOps`` object (the product default is :class:`HipBandOps`, libsmrf_hip), and
the row arithmetic between them is :func:`band_plan`, a pure function.  Every entry point takes ``ops=`` and ``comm=``: the
CPU tests inject an oracle-backed ops object, the one-GPU tests a communicator that plays the neighbours.
"""
import collections
import ctypes as C
import itertools

import numpy as np

from . import _cloud, _lib
from ._raster import _ptr, _stream, _suffix

__all__ = ["band_rows", "window_groups", "HipBandOps", "progressive_filter_sharded", "HipSpringsOps",
           "inpaint_nans_by_springs_sharded", "create_dem_band", "HipPointOps", "create_dem_sharded", "smrf_sharded"]


def band_rows(img_rows, world_size, rank):
    """Global row range [b0, b1) owned by ``rank`` (bands differ by at most one row)."""
    base, rem = divmod(img_rows, world_size)
    b0 = rank * base + min(rank, rem)
    return b0, b0 + base + (1 if rank < rem else 0)


def band_sizes(img_rows, world_size):
    """Rows of every rank's band."""
    return [b1 - b0 for b0, b1 in (band_rows(img_rows, world_size, k) for k in range(world_size))]


class BandComm:
    """The ranks of one call: ``rank``, ``world``, ``multi`` (more than one rank), ``live`` (a process group is initialised),
    ``gloo``, and every message the row-band entry points send.  ONE staging rule underneath all of them: CUDA tensors on a
    gloo group (multi-process rehearsals on a one-GPU box) travel through host memory; anything else goes straight to
    the backend (nccl = RCCL moves the CUDA blocks over xGMI).  A subclass that overrides :meth:`exchange` stands in for
    the neighbours (tests/sharded_one_gpu.py, tools/band_compute.py)."""

    def __init__(self, group=None, rank=None, world_size=None):
        import torch.distributed as dist
        self.dist, self.group, self.live = dist, group, dist.is_initialized()
        self.world = world_size if world_size is not None else (dist.get_world_size(group) if self.live else 1)
        self.rank = rank if rank is not None else (dist.get_rank(group) if self.live else 0)
        self.multi = self.world > 1
        self.gloo = self.live and dist.get_backend(group) == "gloo"

    def _staged(self, *tensors):
        return self.gloo and any(t is not None and t.is_cuda for t in tensors)

    def sendrecv(self, pairs):
        """One batch of ``(send | None, recv | None, peer rank)``: per peer the send, then the recv, in the order given;
        a peer beyond the first or last rank is skipped."""
        dist, group = self.dist, self.group
        staged = self._staged(*[t for snd, rcv, _ in pairs for t in (snd, rcv)])
        ops, back = [], []
        for snd, rcv, p in pairs:
            if not 0 <= p < self.world:
                continue
            p = dist.get_global_rank(group, p) if group is not None else p
            if snd is not None:                              # (row blocks of the halo are contiguous already)
                ops.append(dist.P2POp(dist.isend, snd.cpu() if staged else snd.contiguous(), p, group))
            if rcv is not None:
                if staged:
                    back.append((rcv, rcv.cpu()))
                ops.append(dist.P2POp(dist.irecv, back[-1][1] if staged else rcv, p, group))
        if ops:
            for req in dist.batch_isend_irecv(ops):
                req.wait()
        for dst, h in back:
            dst.copy_(h)

    def exchange(self, send_up, recv_up, send_down, recv_down):
        """send_up -> rank-1 (its bottom halo), send_down -> rank+1 (its top halo); the upper neighbour first."""
        self.sendrecv([(send_up, recv_up, self.rank - 1), (send_down, recv_down, self.rank + 1)])

    def shift(self, send, recv, up):
        """up=True: every rank sends `send` to rank-1 and receives `recv` from rank+1 (down: the reverse)."""
        dst, src = (self.rank - 1, self.rank + 1) if up else (self.rank + 1, self.rank - 1)
        self.sendrecv([(send, None, dst), (None, recv, src)])

    def all_reduce(self, t, op="SUM"):
        """in place"""
        h = t.cpu() if self._staged(t) else t
        self.dist.all_reduce(h, op=getattr(self.dist.ReduceOp, op), group=self.group)
        if h is not t:
            t.copy_(h)

    def reduced(self, value, dtype, op, device):
        """``value`` (a number, or a list of them) reduced over the ranks, as Python numbers; the message is made on
        ``device`` unless the group is gloo.  One rank: ``value`` itself."""
        import torch
        if not self.multi:
            return value
        t = torch.tensor(value if isinstance(value, list) else [value], dtype=dtype, device="cpu" if self.gloo else device)
        self.dist.all_reduce(t, op=getattr(self.dist.ReduceOp, op), group=self.group)
        return t.tolist() if isinstance(value, list) else t.item()

    def all_to_all(self, out, inp, out_splits=None, in_splits=None):
        """all_to_all_single"""
        h = out.cpu() if self._staged(inp) else out
        self.dist.all_to_all_single(h, inp.cpu() if h is not out else inp, output_split_sizes=out_splits,
                                    input_split_sizes=in_splits, group=self.group)
        if h is not out:
            out.copy_(h)

    def all_gather_rows(self, part, sizes):
        """Concatenate every rank's leading-dimension block (``sizes[k]`` rows on rank k) on every rank.
        Blocks are padded to the largest one (all_gather wants equal shapes)."""
        import torch
        if not self.multi:
            return part
        buf = torch.zeros((max(sizes),) + tuple(part.shape[1:]), dtype=part.dtype, device=part.device)
        buf[:part.shape[0]].copy_(part)
        staged = self._staged(part)
        src = buf.cpu() if staged else buf
        outs = [torch.empty_like(src) for _ in sizes]
        self.dist.all_gather(outs, src, group=self.group)
        full = torch.cat([o[:n] for o, n in zip(outs, sizes)], dim=0)
        return full.to(part.device) if staged else full


class HipBandOps:
    """Band compute on the GPU through the C ABI (smrf_disk_filter_* / smrf_pf_dilate_flag_*)."""

    def __init__(self, impl=_lib.IMPL_AUTO):
        self.lib = _lib.load()
        _lib.require_gpu()
        self.impl = impl

    def has_nan(self, band):
        """NaNs in this rank's rows?  (scipy's filters let the first visited footprint element decide NaN-ness; the
        kernels follow that rule only when told to, so the driver asks once per call and all-reduces the answer)"""
        cnt = C.c_int64(0)
        fn = getattr(self.lib, "smrf_count_nan_" + _suffix(band))
        _lib.check(fn(_ptr(band), band.numel(), C.byref(cnt), _stream()))
        return cnt.value > 0

    def head_launch(self, t, radii, img_rows, cells, chain=True):
        """(route, n): the launch the library's routing rule (csrc/pf_route.h, asked through smrf_pf_plan with band = 1 and this
        object's impl) takes for the window at the head of ``radii`` on a NaN-free row band, and how many of those windows it
        covers: ``ROUTE_CHAIN`` with the n windows one chained / table-free launch opens (:meth:`chain_flag`),
        ``ROUTE_FUSED`` (:meth:`open_flag`), or any other route for the two passes; n = 1 for both.  ``cells``: the cells such
        a launch marches; ``chain=False``: a band whose launches cannot be chained.  The library applies its own SMRF_FUSED
        / SMRF_CHAIN switches, the ones smrf_progressive_filter_* routes by."""
        import torch
        r = np.ascontiguousarray(np.asarray(radii[:4], dtype=np.int32))
        route = np.zeros(r.size, dtype=np.int32)
        taken = np.zeros(r.size, dtype=np.uint8)
        _lib.check(self.lib.smrf_pf_plan(4 if t.dtype == torch.float32 else 8, r.ctypes.data_as(C.c_void_p), int(r.size),
                                         int(img_rows), int(cells), 0, self.impl, 1 if chain else 2,
                                         route.ctypes.data_as(C.c_void_p), taken.ctypes.data_as(C.c_void_p)))
        n = 1
        while route[0] == _lib.ROUTE_CHAIN and n < r.size and route[n] == _lib.ROUTE_CHAIN + n:
            n += 1
        return int(route[0]), n

    def chain_flag(self, last, last_row0, opened, mask, when, radii, thr, widx, out_row0, out_rows, img_rows):
        """the windows ``radii`` opened one after the other in ONE launch: ``opened`` = the last surface on global rows
        [out_row0, out_row0 + out_rows), every window's flags on those rows; ``last`` reaches sum(2r) rows beyond them"""
        fn = getattr(self.lib, "smrf_pf_chain_flag_" + _suffix(last))
        cols = last.shape[1]
        r = np.ascontiguousarray(np.asarray(radii, dtype=np.int32))
        t = np.ascontiguousarray(np.asarray(thr, dtype=np.float64))
        w = np.ascontiguousarray(np.asarray(widx, dtype=np.int32))
        _lib.check(fn(_ptr(last), _ptr(opened), _ptr(mask), _ptr(when), r.ctypes.data_as(C.c_void_p),
                      t.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), int(r.size), img_rows, cols, cols, last_row0,
                      last.shape[0], out_row0, out_rows, _stream()))

    def open_flag(self, last, last_row0, opened, mask, when, thr, widx, out_row0, out_rows, img_rows, radius):
        """opened = opening(last, disk(r)) on global rows [out_row0, out_row0 + out_rows) + the flag step, one launch;
        ``last`` holds global rows from ``last_row0`` and reaches 2r rows beyond the outputs"""
        fn = getattr(self.lib, "smrf_pf_open_flag_" + _suffix(last))
        cols = last.shape[1]
        _lib.check(fn(_ptr(last), _ptr(opened), _ptr(mask), _ptr(when), float(thr), int(widx), img_rows, cols, cols,
                      last_row0, last.shape[0], out_row0, out_rows, int(radius), _stream()))

    def erode(self, src, src_row0, dst, dst_row0, dst_rows, img_rows, radius, nan_aware=0):
        fn = getattr(self.lib, "smrf_disk_filter_" + _suffix(src))
        _lib.check(fn(_ptr(src), _ptr(dst), img_rows, src.shape[1], src.shape[1], src_row0, src.shape[0], dst_row0,
                      dst_rows, int(radius), 0, int(nan_aware), self.impl, _stream()))

    def dilate_flag(self, eroded, er_row0, er_rows, last_band, opened_band, mask, when, thr, widx, band_row0,
                    band_nrows, img_rows, radius, nan_aware=0):
        fn = getattr(self.lib, "smrf_pf_dilate_flag_" + _suffix(eroded))
        cols = eroded.shape[1]
        _lib.check(fn(_ptr(eroded), _ptr(last_band), _ptr(opened_band), _ptr(mask), _ptr(when), float(thr), int(widx),
                      img_rows, cols, cols, er_row0, er_rows, band_row0, band_nrows, int(radius), int(nan_aware), self.impl,
                      _stream()))


def window_groups(windows, min_band_rows, budget=None):
    """Consecutive windows that share ONE halo exchange: a group needs sum(2r) rows of the
    neighbours' bands up front and recomputes its margins redundantly while they shrink by 2r per
    window.  Greedy: a group grows while its halo stays within ``budget`` rows (default: 1/16 of
    the shortest band, at least 256; a single window always fits).  Fewer, larger messages: the
    small radii, whose kernels are short, would otherwise pay one exchange latency each.  The
    default trades about 5 % redundant compute on a 2048-row band (tools/band_compute.py) for 12
    exchanges instead of 50 over windows 1..50."""
    if budget is None:
        budget = max(256, min_band_rows // 16)
    budget = min(budget, min_band_rows)
    groups, cur, need = [], [], 0
    for i, r in enumerate(windows):
        if cur and need + 2 * r > budget:
            groups.append(cur)
            cur, need = [], 0
        cur.append(i)
        need += 2 * r
    if cur:
        groups.append(cur)
    return groups


Step = collections.namedtuple("Step", "kind group members src dst in0 in1 out0 out1 side halo")
Step.__doc__ = """One call of the band driver, rows as GLOBAL ranges [x0, x1); ``group``: its window group; ``side``: on
the side stream (the edge-first split of ``overlap``).  ``kind``:
``exchange``  ``halo`` rows with each neighbour on surface buffer ``src``: the band [in0, in1) is valid before, [out0, out1) after;
``chain``     windows ``members`` in one launch: reads buffer ``src`` on [in0, in1), writes ``dst`` on [out0, out1);
``erode``     window ``members[0]``: reads ``src`` on [in0, in1), writes the erosion buffer on [out0, out1);
``open``      fused opening + flags: reads ``src`` on [in0, in1), writes ``dst`` on [out0, out1);
``dilate``    dilation + flags: reads the erosion on [in0, in1) and ``src`` on [out0, out1), writes ``dst`` on [out0, out1)."""


def band_plan(img_rows, world, rank, windows, groups, overlap=False, head=None):
    """The steps (:class:`Step`) ``rank`` runs for the window ``groups`` (lists of indices into ``windows``, the radii), in
    order: the row arithmetic of :func:`progressive_filter_sharded` and nothing else (no torch, no process group).

    A group starts with ONE exchange of M = sum(2r) rows, after which ``last`` is valid on the band plus M rows either
    side (clipped to the raster).  Every window erodes r rows inside the valid rows and opens r more rows inside, so
    the margin shrinks by 2r per window and is zero - the band itself - at the group's end.  With ``overlap`` the
    group's last dilation is split edge-first where the band holds the 2 * Mn rows: the two Mn-row edge pieces and the
    NEXT group's exchange (the neighbours need exactly those rows of the opened surface) go to the side stream, the
    interior follows; that next group then starts without an exchange.  Otherwise the exchange sits at its group's head.
    One band (``world == 1``): no exchange, whole-raster ranges.  The two surface buffers swap roles after every launch
    that writes one, unless there is a single window.

    ``head(src, radii, rows, chain) -> (route, n)`` answers what ``HipBandOps.head_launch`` answers for the windows
    ``radii`` left in a group; None (ops without a routing rule, or a NaN-aware call): two passes per window.  It is asked
    about ``rows`` = the rows a launch of this group marches, the longest band with a two-sided margin: the SAME figure
    on every rank, so that all ranks route a window the same way (an edge rank's one-sided margin would otherwise put it
    on the other side of a size threshold than its neighbour; every route gives the same bits, but the ranks' launches
    should not differ).  ``chain`` is off on a single band and where the group's last window may be split (overlap).
    A generator: ``head`` is asked about a window when the consumer reaches it.
    """
    b0, b1 = band_rows(img_rows, world, rank)
    multi = world > 1
    max_band = max(band_sizes(img_rows, world))
    halo = [sum(2 * windows[i] for i in g) if multi else 0 for g in groups]

    def span(m):                                             # the band and m rows either side
        return (max(0, b0 - m), min(img_rows, b1 + m)) if multi else (0, img_rows)
    cur, early = 0, False                                    # early: this group's exchange ran inside the previous group's split
    for gi, grp in enumerate(groups):
        M = halo[gi]                                         # rows of `last` still valid beyond the band,
        lo, hi = span(M)                                     # and the rows that are valid
        if M > 0 and not early:
            yield Step("exchange", gi, [], cur, cur, b0, b1, lo, hi, False, M)
        early, pos = False, 0
        while pos < len(grp):
            i, r = grp[pos], windows[grp[pos]]
            route, k = (None, 1) if head is None else head(cur, [windows[j] for j in grp[pos:]],
                                                           min(img_rows, max_band + 2 * M), multi and not overlap)
            if route == _lib.ROUTE_CHAIN:                    # a run of small windows: the margin they eat is the sum of theirs
                members = grp[pos:pos + k]
                M = max(0, M - sum(2 * windows[j] for j in members))
                o0, o1 = span(M)
                yield Step("chain", gi, members, cur, 1 - cur, lo, hi, o0, o1, False, 0)
                pos += k
            else:
                q0, q1 = span(M - r)                         # erosion: r rows inside the valid ones
                M = max(0, M - 2 * r)
                o0, o1 = span(M)                             # opening: r more rows inside (the band at the group's end)
                pos += 1
                if route == _lib.ROUTE_FUSED:
                    kind, in0, in1 = "open", lo, hi
                else:
                    kind, in0, in1 = "dilate", q0, q1
                    yield Step("erode", gi, [i], cur, None, lo, hi, q0, q1, False, 0)
                # margin rows are flagged too (same values the neighbour computes for them); only the band's are returned
                Mn = halo[gi + 1] if overlap and pos == len(grp) and gi + 1 < len(groups) else 0
                if Mn > 0 and o0 == b0 and o1 == b1 and b1 - b0 >= 2 * Mn:
                    yield Step(kind, gi, [i], cur, 1 - cur, in0, in1, b0, b0 + Mn, True, 0)
                    yield Step(kind, gi, [i], cur, 1 - cur, in0, in1, b1 - Mn, b1, True, 0)
                    yield Step("exchange", gi, [], 1 - cur, 1 - cur, b0, b1, *span(Mn), True, Mn)
                    if b1 - b0 > 2 * Mn:
                        yield Step(kind, gi, [i], cur, 1 - cur, in0, in1, b0 + Mn, b1 - Mn, False, 0)
                    early = True
                else:
                    yield Step(kind, gi, [i], cur, 1 - cur, in0, in1, o0, o1, False, 0)
            lo, hi = o0, o1                                  # what this launch wrote is what the next one may read
            if len(windows) > 1:
                cur = 1 - cur


def progressive_filter_sharded(Z_band, img_rows, windows, thresholds, *, rank=None, world_size=None, group=None,
                               ops=None, return_when_dropped=False, state=None, halo_budget=None, overlap=False, comm=None):
    """progressive_filter on this rank's row band ``Z_band`` (rows ``band_rows(img_rows, W, rank)``).

    Returns the band's ``(mask, when_dropped | None)`` as uint8 tensors on ``Z_band``'s device.
    ``thresholds`` = ``slope_threshold * (windows * cellsize)`` in float64, as on one device.
    Every band must have at least ``2 * max(windows)`` rows (a halo never spans two ranks).
    ``state`` (a dict) keeps the extended buffers and their row views between calls so a benchmark loop does not
    re-allocate (and reports ``state["exchanges"]``; with ``state["profile"] = True`` also ``exchange_events``, a pair
    of CUDA events around every exchange, ``exchange_bytes``, the bytes this rank sent in each, and ``groups``).  ``halo_budget``: rows of halo a group of
    consecutive windows may share in one exchange (see :func:`window_groups`; 0 = one exchange
    per window).  ``overlap=True`` splits every group's last dilation edge-first and posts the next group's exchange
    on a side stream beside the interior (module docstring).  Off by default: on a 2048-row band the two edge
    strips cost about 160 us per group, more than an exchange of up to about 0.45 ms returns
    (tools/band_compute.py, gpurun_out/r02/band_compute.log); it pays on slower links only.
    ``comm``: the :class:`BandComm` to use instead of one built from ``group`` / ``rank`` / ``world_size``.
    """
    import torch
    if comm is None:
        comm = BandComm(group, rank, world_size)
    rank, world_size = comm.rank, comm.world
    if ops is None:
        ops = HipBandOps()
    windows = [int(w) for w in np.asarray(windows).ravel()]
    thresholds = np.asarray(thresholds, dtype=np.float64).ravel()
    if len(windows) != thresholds.size:
        raise ValueError("windows and thresholds differ in length")
    b0, b1 = band_rows(img_rows, world_size, rank)
    nloc = b1 - b0
    if Z_band.shape[0] != nloc:
        raise ValueError("band has %d rows, expected %d" % (Z_band.shape[0], nloc))
    cols = Z_band.shape[1]
    rmax = max(windows) if windows else 0
    min_band = min(band_sizes(img_rows, world_size))
    if comm.multi and min_band < 2 * rmax:
        raise ValueError("row bands of %d rows are shorter than the 2*%d halo rows a window needs; "
                         "use fewer ranks for this raster" % (min_band, rmax))
    dev, dt = Z_band.device, Z_band.dtype
    groups = window_groups(windows, min_band, halo_budget) if comm.multi else [[i] for i in range(len(windows))]
    H = max([sum(2 * windows[i] for i in g) for g in groups], default=0) if comm.multi else 0
    e0, e1 = max(0, b0 - H), min(img_rows, b1 + H)          # rows the extended buffers can hold
    st = state if state is not None else {}
    key = (nloc, cols, H, str(dt), str(dev))
    if st.get("key") != key:
        keep = st.get("profile")
        st.clear()
        st["key"] = key
        if keep:
            st["profile"] = keep
        st["ext"] = [torch.empty((e1 - e0, cols), dtype=dt, device=dev) for _ in range(2)]
        st["ero"] = torch.empty((e1 - e0, cols), dtype=dt, device=dev)
        st["mask"] = torch.empty((e1 - e0, cols), dtype=torch.uint8, device=dev)
        st["when"] = torch.empty((e1 - e0, cols), dtype=torch.uint8, device=dev)
    ext, ero, mask = st["ext"], st["ero"], st["mask"]
    when = st["when"] if return_when_dropped else None
    mask.zero_()
    if when is not None:
        when.zero_()
    ext[0][b0 - e0:b1 - e0].copy_(Z_band)
    st["exchanges"] = 0
    # scipy's NaN rule (first visited footprint element decides) costs the kernels a read per cell: only when some
    # band holds a NaN, as the single-device path decides with one count
    nan_aware = 0
    if hasattr(ops, "has_nan"):
        nan_aware = int(bool(ops.has_nan(ext[0][b0 - e0:b1 - e0])))      # the band's contiguous copy: Z_band may be any view
        if comm.live:
            nan_aware = comm.reduced(nan_aware, torch.int32, "MAX", dev)
    kw = {"nan_aware": nan_aware} if nan_aware else {}
    # overlap (CUDA tensors): the exchange a group needs is posted on a side stream as soon as the previous group's
    # last dilation has produced the band's edge rows, and runs beside that dilation's interior
    side = st.get("side")
    if side is None and Z_band.is_cuda and comm.multi:
        side = st["side"] = torch.cuda.Stream(device=dev)
    st["groups"] = [[windows[i] for i in g] for g in groups]
    profile = bool(st.get("profile")) and Z_band.is_cuda      # bench.py: events either side of every exchange
    if profile:
        st["exchange_events"], st["exchange_bytes"] = [], []

    # The launch at the head of the windows left in a group, by the library's one routing rule (ops without it, the oracle-backed
    # ones of the CPU tests, run two passes per window).  Not with NaNs: scipy's NaN rule lives in the two-pass kernels only.
    # Asked about the cells a launch marches, not the whole raster: the chain 4, 5 and the table-free R = 10 only pay from 20 Mi up.
    def head(src, radii, rows, chain):
        return ops.head_launch(ext[src], radii, img_rows, rows * cols, chain=chain)
    plan = band_plan(img_rows, world_size, rank, windows, groups, overlap,
                     head if not nan_aware and hasattr(ops, "head_launch") else None)
    views = st.setdefault("views", {})                       # row views of the buffers, kept with them between calls

    def cut(t, y0, y1):                                      # global rows [y0, y1) of an extended buffer
        k = (id(t), y0, y1)
        if k not in views:
            views[k] = t[y0 - e0:y1 - e0] if t is not None else None
        return views[k]

    def run(s):
        last, out = ext[s.src], (s.out0, s.out1)
        if s.kind == "exchange":
            if profile:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            comm.exchange(cut(last, b0, b0 + s.halo), cut(last, s.out0, b0) if rank > 0 else None,
                          cut(last, b1 - s.halo, b1), cut(last, b1, s.out1) if rank < world_size - 1 else None)
            if profile:
                ev1.record()
                st["exchange_events"].append((ev0, ev1))
                st["exchange_bytes"].append(s.halo * cols * Z_band.element_size() * ((rank > 0) + (rank < world_size - 1)))
            st["exchanges"] += 1
            return
        i = s.members[0]
        if s.kind == "erode":
            ops.erode(cut(last, s.in0, s.in1), s.in0, cut(ero, *out), s.out0, s.out1 - s.out0, img_rows, windows[i], **kw)
            return
        dst = cut(ext[s.dst], *out), cut(mask, *out), cut(when, *out)
        if s.kind == "chain":
            ops.chain_flag(cut(last, s.in0, s.in1), s.in0, *dst, [windows[j] for j in s.members],
                           [float(thresholds[j]) for j in s.members], s.members, s.out0, s.out1 - s.out0, img_rows)
        elif s.kind == "open":
            ops.open_flag(cut(last, s.in0, s.in1), s.in0, *dst, float(thresholds[i]), i, s.out0, s.out1 - s.out0, img_rows,
                          windows[i])
        else:
            ops.dilate_flag(cut(ero, s.in0, s.in1), s.in0, s.in1 - s.in0, cut(last, *out), *dst, float(thresholds[i]), i,
                            s.out0, s.out1 - s.out0, img_rows, windows[i], **kw)

    posted, g = None, 0
    for (gi, on_side), steps in itertools.groupby(plan, key=lambda s: (s.group, s.side and side is not None)):
        if gi != g and posted is not None:                   # the next group's first read waits for the exchange posted ahead
            torch.cuda.current_stream().wait_event(posted)
            posted = None
        g = gi
        if on_side:                                          # edge pieces, then the next group's exchange, beside the interior
            ready = torch.cuda.Event()
            ready.record()                                   # the erosion is enqueued before this point
            with torch.cuda.stream(side):
                side.wait_event(ready)
                for s in steps:
                    run(s)
                posted = torch.cuda.Event()
                posted.record()
        else:                                                # the main stream (CPU tensors, the gloo tests: every step, in order)
            for s in steps:
                run(s)
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)        # nothing of this call is left running on the side stream
    return mask[b0 - e0:b1 - e0], (when[b0 - e0:b1 - e0] if when is not None else None)


# ------------------------------------------------------------------------------------------
# inpaint_nans_by_springs over row bands: 1-row halos + one scalar all-reduce per reduction
# ------------------------------------------------------------------------------------------
# phases of smrf_springs_band_phase (include/smrf_hip.h; 9 is retired)
PH_MASK, PH_RHS, PH_BNORM, PH_ATU, PH_INIT_ALFA, PH_AV, PH_BETA_RHO, PH_ATUXW, PH_ALFA_TESTS = range(9)
PH_SCATTER = 10


class HipSpringsOps:
    """The band phases of libsmrf_hip's LSQR (smrf_springs_band_*) on this rank's rows."""

    def __init__(self, A_band, has_above, has_below):
        import torch
        self.lib = _lib.load()
        _lib.require_gpu()
        if A_band.dtype != torch.float64 or not A_band.is_contiguous() or not A_band.is_cuda:
            raise TypeError("the band must be a contiguous float64 CUDA tensor")
        self.A = A_band
        self.rows, self.cols = A_band.shape
        self.flags = (int(bool(has_above)), int(bool(has_below)))
        self.nbytes = self.lib.smrf_springs_band_workspace_bytes(self.rows, self.cols)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=A_band.device)
        lay = (C.c_int64 * 8)()
        _lib.check(self.lib.smrf_springs_band_layout(self.rows, self.cols, lay))
        ld = int(lay[6])                                      # cells between plane rows (>= cols: padded to cache lines)
        n2 = (self.rows + 2) * ld
        self.v = self.ws[lay[0]:lay[0] + n2 * 8].view(torch.float64).view(self.rows + 2, ld)[:, :self.cols]
        self.uv = self.ws[lay[1]:lay[1] + n2 * 8].view(torch.float64).view(self.rows + 2, ld)[:, :self.cols]
        self.hole = self.ws[lay[2]:lay[2] + n2].view(self.rows + 2, ld)[:, :self.cols]
        self.abelow = self.ws[lay[3]:lay[3] + self.cols * 8].view(torch.float64)
        self.red2 = self.ws[lay[4]:lay[4] + 16].view(torch.float64)      # [|v|^2, |dk|^2] of the ATUXW phase
        self.red = self.red2[:1]                                          # the single sum of the other phases

    def begin(self, atol, btol, conlim, iter_lim):
        _lib.check(self.lib.smrf_springs_band_begin(self.rows, self.cols, atol, btol, conlim, iter_lim,
                                                    _ptr(self.ws), self.nbytes, _stream()))

    def phase(self, ph):
        _lib.check(self.lib.smrf_springs_band_phase(ph, _ptr(self.A), self.rows, self.cols,
                                                    self.flags[0], self.flags[1], _ptr(self.ws),
                                                    self.nbytes, _stream()))

    def status(self):
        istop, itn, nunk, done = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
        _lib.check(self.lib.smrf_springs_band_status(_ptr(self.ws), self.rows, self.cols, C.byref(istop),
                                                     C.byref(itn), C.byref(nunk), C.byref(done), _stream()))
        return istop.value, itn.value, nunk.value, bool(done.value)


def inpaint_nans_by_springs_sharded(A_band, img_rows, *, rank=None, world_size=None, group=None, ops=None,
                                    atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=-1, poll=8, comm=None):
    """Spring infill (SciPy-LSQR semantics) of a raster split into row bands; ``A_band`` (this rank's
    rows, float64) is filled in place.  Returns ``(istop, itn, n_unknown)`` - equal on every rank.

    Per LSQR iteration: rank r sends the first row of ``v`` up and the last row of ``uv`` down (one
    row each, nearest neighbour) and TWO all-reduces replace the three norms: ``|u|^2`` alone (beta
    must exist before ``v = S^T u - beta v``), then ``[|v|^2, |dk|^2]`` as one 2-element buffer:
    the plane rotation's ``rho`` needs only ``rhobar`` and ``beta`` (csrc/lsqr_core.h: rho_step), so
    ``dk = w / rho`` (lsqr.py:459) - and with it the x and w steps - ride in the pass that makes
    ``v`` (csrc/springs.hip: atuxw_kernel, the single-device solver's kernel; round 5).  Two
    synchronisation points per iteration is LSQR's own minimum (beta, then alfa).  The scalar
    recurrence runs replicated on every rank from the same reduced sums, so all ranks stop at the
    same iteration.  Summation order differs from one device (block partials per band), so
    values agree to ~1e-12 and ``itn`` is normally identical (hard part 1).
    """
    if comm is None:
        comm = BandComm(group, rank, world_size)
    rank, world_size, multi = comm.rank, comm.world, comm.multi
    b0, b1 = band_rows(img_rows, world_size, rank)
    if A_band.shape[0] != b1 - b0:
        raise ValueError("band has %d rows, expected %d" % (A_band.shape[0], b1 - b0))
    if ops is None:
        ops = HipSpringsOps(A_band, rank > 0, rank < world_size - 1)
    n = ops.rows

    def reduce(t=None):
        if multi:
            comm.all_reduce(ops.red if t is None else t)

    ops.begin(atol, btol, conlim, iter_lim)
    ops.phase(PH_MASK)
    if multi:
        comm.shift(ops.hole[1], ops.hole[n + 1], up=True)
        comm.shift(ops.A[0], ops.abelow, up=True)
    reduce()
    ops.phase(PH_RHS)
    reduce()
    ops.phase(PH_BNORM)
    if multi:
        comm.shift(ops.uv[n], ops.uv[0], up=False)
    ops.phase(PH_ATU)
    reduce()
    ops.phase(PH_INIT_ALFA)
    istop, itn, nunk, done = ops.status()
    while not done:
        for _ in range(poll):
            if multi:
                comm.shift(ops.v[1], ops.v[n + 1], up=True)
            ops.phase(PH_AV)                                 # u_k = S v_{k-1} - alfa u_{k-1}
            reduce()
            ops.phase(PH_BETA_RHO)                           # beta_k; rho_k, t1_k, 1/rho_k need nothing else
            if multi:
                comm.shift(ops.uv[n], ops.uv[0], up=False)
            ops.phase(PH_ATUXW)                              # w_{k-1}, dk_k, (x_k every second k), v_k
            reduce(ops.red2)                                      # [|v|^2, |dk|^2] as one buffer
            ops.phase(PH_ALFA_TESTS)                         # alfa_k, rest of the rotation, stopping tests
        istop, itn, nunk, done = ops.status()
    if nunk > 0:
        ops.phase(PH_SCATTER)
    return istop, itn, nunk


def create_dem_band(xd, yd, zd, inv_affine, grid_shape, *, rank, world_size, bin_type='min'):
    """This rank's row band of create_dem's raster from the FULL point set (points are replicated or
    streamed to every rank; no exchange): returns (float64 band, uint8 empty mask, n_outside).

    The binning kernel takes the band as (row0, rows_local) and ignores points of other bands, so N
    ranks read the points N times but write disjoint rows (the all-to-all of points by
    destination band is the alternative when the points do not fit every rank)."""
    b0, b1 = band_rows(grid_shape[0], world_size, rank)
    return _cloud.grid_rows(xd, yd, zd, inv_affine, grid_shape, b0, b1 - b0, bin_type)


class HipPointOps:
    """Point-side device operators of the sharded create_dem (libsmrf_hip, include/smrf_hip.h)."""

    def __init__(self):
        self.lib = _lib.load()
        _lib.require_gpu()

    def extent(self, xd, yd):
        """(xmin, xmax, ymin, ymax) of this rank's points; (+inf, -inf, +inf, -inf) for none"""
        return _cloud.extent(xd, yd)

    def bucket(self, xd, yd, zd, inv, rows_total, nbands):
        """points grouped by destination row band: (counts int64[nbands] on the device, x, y, z packed runs)"""
        import torch
        h_inv = (C.c_double * 6)(*[float(v) for v in inv])
        counts = torch.zeros(nbands, dtype=torch.int64, device=xd.device)
        _lib.check(self.lib.smrf_points_band_count_f64(_ptr(xd), _ptr(yd), xd.numel(), h_inv, rows_total, nbands,
                                                       _ptr(counts), _stream()))
        cursors = torch.cumsum(counts, 0) - counts               # exclusive prefix sum: each band's first slot
        ox, oy, oz = torch.empty_like(xd), torch.empty_like(yd), torch.empty_like(zd)
        _lib.check(self.lib.smrf_points_band_pack_f64(_ptr(xd), _ptr(yd), _ptr(zd), xd.numel(), h_inv, rows_total, nbands,
                                                      _ptr(cursors), _ptr(ox), _ptr(oy), _ptr(oz), _stream()))
        return counts, ox, oy, oz

    def bin_band(self, xd, yd, zd, inv, grid_shape, row0, rows_local, bin_type):
        """(float64 band, uint8 empty mask, points outside the raster) from the points this rank received"""
        return _cloud.grid_rows(xd, yd, zd, inv, grid_shape, row0, rows_local, bin_type)


def create_dem_sharded(xd, yd, zd, cellsize=1, bin_type='max', *, rank=None, world_size=None, group=None, ops=None,
                       comm=None):
    """create_dem (neilpy/neilpy.py:1110-1166) with the POINTS sharded: every rank passes its own 1/N of the cloud
    and gets its row band of the raster - nothing is replicated (the all-to-all form).

    1. extents: local min/max (device reduction), a count of ranks with an undefined extent (all-reduce sum) and one
       4-double all-reduce(min) -> the same edges, shape and
       transform on every rank (:1117-1124, :1141);
    2. every point is routed to the rank whose band holds ``floor(row)`` of ``~t * (x, y)`` - bucketed on the device
       (count, prefix sum, pack), the counts and then the three coordinate runs exchanged with ``all_to_all_single``
       (RCCL; about 24 B per point cross the links once);
    3. the received points are binned into the band with the same 64-bit ``atomicMin`` as on one device (:1151-1156).
    Returns ``(band float64, empty uint8, transform, (ny, nx), (b0, b1))``.  Bit-identical to the rows
    ``b0:b1`` of the single-device raster: min / max do not depend on the order points arrive in.
    """
    import torch
    from . import api
    from .affine import from_origin
    if comm is None:
        comm = BandComm(group, rank, world_size)
    rank, world_size, multi = comm.rank, comm.world, comm.multi
    if bin_type not in ('max', 'min'):
        raise ValueError('This type not supported.')                  # neilpy.py:1158
    if ops is None:
        ops = HipPointOps()
    xmin, xmax, ymin, ymax = ops.extent(xd, yd)
    # A rank whose extent is undefined (a NaN / inf coordinate, or no points) must stop EVERY rank.  MIN does not carry
    # a NaN reliably (RCCL's float min is fmin-like and drops it, gloo's std::min keeps it or not by operand order), so
    # the ranks agree on an explicit count of bad extents first and only reduce finite values.
    if comm.reduced(int(not np.isfinite([xmin, xmax, ymin, ymax]).all()), torch.int32, "SUM", xd.device):
        raise ValueError("zero-size or non-finite point set: the raster's extent is undefined")
    e = comm.reduced([xmin, ymin, -xmax, -ymax], torch.float64, "MIN", xd.device)
    xmin, ymin, xmax, ymax = e[0], e[1], -e[2], -e[3]
    xedges, yedges = api._edges_from_extent(np.float64(xmin), np.float64(xmax), np.float64(ymin), np.float64(ymax), cellsize)
    nx, ny = len(xedges) - 1, len(yedges) - 1
    t = from_origin(xedges[0], yedges[0], cellsize, cellsize)
    inv = tuple(~t)[:6]
    if multi and ny < world_size:
        raise ValueError("a raster of %d rows cannot be split over %d ranks" % (ny, world_size))
    b0, b1 = band_rows(ny, world_size, rank)
    if multi:
        counts, sx, sy, sz = ops.bucket(xd, yd, zd, inv, ny, world_size)
        cnt = counts.cpu() if comm.gloo else counts
        got = torch.empty_like(cnt)
        comm.all_to_all(got, cnt)                                      # how many points every rank sends me
        in_splits = [int(v) for v in counts.cpu().tolist()]
        out_splits = [int(v) for v in got.cpu().tolist()]
        n_in = sum(out_splits)
        rx, ry, rz = (torch.empty(n_in, dtype=torch.float64, device=xd.device) for _ in range(3))
        for dst_t, src_t in ((rx, sx), (ry, sy), (rz, sz)):
            comm.all_to_all(dst_t, src_t, out_splits, in_splits)
        xd, yd, zd = rx, ry, rz
    band, empty, n_out = ops.bin_band(xd, yd, zd, inv, (ny, nx), b0, b1 - b0, bin_type)
    if comm.reduced(int(n_out), torch.int64, "SUM", band.device) > 0:
        raise ValueError("invalid entry in coordinates array")       # np.ravel_multi_index, neilpy.py:1151
    return band, empty, t, (ny, nx), (b0, b1)


# ------------------------------------------------------------------------------------------
# the whole smrf() over row bands
# ------------------------------------------------------------------------------------------
def smrf_sharded(x, y, z, cellsize=1, windows=5, slope_threshold=.15, elevation_threshold=.5, elevation_scaler=1.25,
                 low_filter_slope=5, low_outlier_fill=False, *, rank=None, world_size=None, group=None,
                 points="replicated", comm=None):
    """neilpy.smrf (neilpy/neilpy.py:1685-1808) with the raster split into row bands, one rank per GPU.

    ``points="replicated"``: every rank passes the FULL point set (or reads it from the same file) and bins it
    into its own rows (create_dem_band, no exchange).  ``points="sharded"``: every rank passes only its own part of
    the cloud; the points are routed to the rank that owns their row with one all-to-all (create_dem_sharded) and the
    tail classifies the rank's own points - nothing is replicated but the DTM the spline needs.
    Both spring inpaints and both progressive filters run on this rank's band
    (inpaint_nans_by_springs_sharded, progressive_filter_sharded).  The tail's
    bicubic spline is global along both axes, so the DTM bands are all-gathered and every rank
    solves the spline on the whole raster ("replicas only") but evaluates and tests only
    its own 1/N of the points; the point flags are all-gathered.

    Returns ``(dtm_band, transform, object_cells_band, is_object_point, (b0, b1))``: the rank's rows
    ``b0:b1`` of the DTM (float64 CUDA) and of the object raster (bool CUDA), and the point flags (bool CUDA): of
    ALL points, the same on every rank (replicated), or of the rank's own points (sharded).
    """
    import torch
    from . import api
    if comm is None:
        comm = BandComm(group, rank, world_size)
    rank, world_size = comm.rank, comm.world
    if np.isscalar(windows):
        windows = np.arange(windows) + 1
    windows = np.asarray(windows)
    lib = _lib.load()
    if points not in ("replicated", "sharded"):
        raise ValueError("points must be 'replicated' or 'sharded'")
    xd, yd, zd = api._points_to_device(x, y, z)
    if points == "sharded":
        band, empty, t, (ny, nx), (b0, b1) = create_dem_sharded(xd, yd, zd, cellsize, 'min', comm=comm)        # :1741
    else:
        xedges, yedges = api._dem_edges(xd, yd, cellsize)                          # :1117-1124, same on every rank
        nx, ny = len(xedges) - 1, len(yedges) - 1
        from .affine import from_origin
        t = from_origin(xedges[0], yedges[0], cellsize, cellsize)
        b0, b1 = band_rows(ny, world_size, rank)
        band, empty, n_out = create_dem_band(xd, yd, zd, tuple(~t)[:6], (ny, nx), rank=rank, world_size=world_size,
                                             bin_type='min')                       # :1741
        if n_out > 0:
            raise ValueError("invalid entry in coordinates array")
    stats = {"inpaint1": inpaint_nans_by_springs_sharded(band, ny, comm=comm)}
    neg = torch.empty_like(band)
    _lib.check(lib.smrf_negate_f64(_ptr(band), _ptr(neg), band.numel(), _stream()))
    low, _ = progressive_filter_sharded(neg, ny, np.array([1]), low_filter_slope * (np.array([1]) * cellsize),
                                        comm=comm)                                 # :1744
    low = low.clone()
    del neg
    if low_outlier_fill:                                                           # :1747-1749
        _lib.check(lib.smrf_mask_apply_f64(_ptr(band), _ptr(low), None, None, None, band.numel(), _stream()))
        stats["inpaint1b"] = inpaint_nans_by_springs_sharded(band, ny, comm=comm)
    obj, _ = progressive_filter_sharded(band, ny, windows, slope_threshold * (windows * cellsize), comm=comm)   # :1752-1755
    obj = obj.contiguous()
    object_cells = torch.empty_like(obj)
    _lib.check(lib.smrf_mask_apply_f64(_ptr(band), _ptr(empty), _ptr(low), _ptr(obj), _ptr(object_cells), band.numel(),
                                       _stream()))                                 # :1762-1763
    stats["inpaint2"] = inpaint_nans_by_springs_sharded(band, ny, comm=comm)       # :1764
    # tail: the spline needs the whole DTM; the points are split evenly
    Zpro = comm.all_gather_rows(band, band_sizes(ny, world_size))
    npts = xd.numel()
    p0, p1 = (0, npts) if points == "sharded" else band_rows(npts, world_size, rank)    # sharded: the rank's own points
    if p1 > p0:
        flags = api._classify_points_device(Zpro, t, cellsize, xd[p0:p1].contiguous(), yd[p0:p1].contiguous(),
                                            zd[p0:p1].contiguous(), elevation_threshold, elevation_scaler)[2]
    else:
        flags = torch.empty(0, dtype=torch.uint8, device=xd.device)
    if points == "replicated":
        flags = comm.all_gather_rows(flags, band_sizes(npts, world_size))
    api.last_stats["sharded"] = stats
    return band, t, object_cells.bool(), flags.bool(), (b0, b1)
