"""neilpy_amd.sharded's row-band driver exercised on ONE GPU (test helper, no test in here).

Every rank's band runs in turn on the same device through the driver's ``comm=`` seam: the communicator handed in plays
the neighbours.  The message a neighbour would send in exchange g is the same rows of the surface entering group g,
computed on the whole raster with the single-device opening; only those halo rows are kept (sum(2r) rows either side of
every band border), so a full-size caller holds no whole surface per group.  What rank k sends up is what rank k-1
receives from below, so every message a rank sends is checked bit for bit against those kept rows (NaNs compare equal).
Returns the per-band masks (and when_dropped) stitched back into whole rasters plus the window groups.
"""
import numpy as np


def run_bands(nz, Z, windows, world, cellsize=1, slope=.15, return_when_dropped=False, budget=None, ops=None,
              overlap=lambda rank: False):
    """``ops``: a factory of the band ops object (default: the driver's own HipBandOps); ``overlap``: rank -> bool"""
    import torch
    from neilpy_amd import sharded
    N = Z.shape[0]
    win = [int(w) for w in windows]
    thr = slope * (np.asarray(windows) * cellsize)
    groups = sharded.window_groups(win, min(sharded.band_sizes(N, world)), budget)
    want_calls = [sum(2 * win[i] for i in g) for g in groups]
    halo, last = {}, Z
    for gi, grp in enumerate(groups):
        for k in range(world):
            b0, b1 = sharded.band_rows(N, world, k)
            if k > 0:
                halo[(gi, k, "up")] = last[b0 - want_calls[gi]:b0].clone()
            if k < world - 1:
                halo[(gi, k, "down")] = last[b1:b1 + want_calls[gi]].clone()
        for i in grp:
            last = nz.opening(last, radius=win[i])
    del last

    def same(a, b):
        return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))

    class Neighbours(sharded.BandComm):
        def __init__(self, rank):
            super().__init__(None, rank, world)
            self.calls = []

        def exchange(self, send_up, recv_up, send_down, recv_down):
            gi, k = len(self.calls), self.rank
            self.calls.append(send_up.shape[0])
            if k > 0:
                assert same(send_up, halo[(gi, k - 1, "down")]), (k, gi, "rows sent up")
                recv_up.copy_(halo[(gi, k, "up")])
            if k < world - 1:
                assert same(send_down, halo[(gi, k + 1, "up")]), (k, gi, "rows sent down")
                recv_down.copy_(halo[(gi, k, "down")])

    mask = torch.empty(Z.shape, dtype=torch.uint8, device=Z.device)
    when = torch.empty(Z.shape, dtype=torch.uint8, device=Z.device) if return_when_dropped else None
    for k in range(world):
        b0, b1 = sharded.band_rows(N, world, k)
        comm = Neighbours(k)
        m, w = sharded.progressive_filter_sharded(Z[b0:b1], N, windows, thr, ops=ops() if ops else None,
                                                  return_when_dropped=return_when_dropped, halo_budget=budget,
                                                  overlap=overlap(k), comm=comm)
        mask[b0:b1].copy_(m)
        if when is not None:
            when[b0:b1].copy_(w)
        assert comm.calls == want_calls, (k, comm.calls, want_calls)    # one exchange per group, sum(2r) rows
    return mask.bool(), when, groups
