// How a marching launch (ring / fused / chain / incremental-erosion kernels) is cut into row segments: how many
// (smrf_pick_nseg), how long (smrf_seg_len) and, for a ring pass, where every output row goes (smrf_ring_plan).  Plain C++,
// no HIP: included by smrf_common.h and compiled on its own by tests/test_host_logic.py.
#pragma once
#include <algorithm>

// Rows of segments for a launch of `strips` workgroups per row of segments over `rows` output rows, on 256 CUs that hold
// `resident` workgroups each; every segment marches `warm` extra rows first and is a multiple of `batch` rows.
// Rule 0 (default, round 5): the count that minimises  k x (segment + warm + 20) / X(k),  k = workgroups on the busiest CU,
// X(k) = 1, 1.57, 2.1, 2.37 (+0.1 per further one) = what k resident workgroups of these kernels get out of a CU beside one -
// measured on 1024^2 ... 16384^2 rasters (profiles/r05_segment_balance.md section 4): a lone workgroup runs twice as fast as one of three, so
// a raster too small to give every slot a long segment is better cut so that the workgroup count fills the CUs
// k times exactly (1024^2 windows 15..50: 5.4 -> 2.7 ms, 2048^2: 5.5 -> 3.8, 4096^2 -8 %); for a large raster it is one full
// round as before; a launch that asks for several rounds is taken at its word only when that is cheaper.  Rules 1, 2: one full round of `rounds x resident x 256 / strips` segments, rounded to nearest (rounds
// 1-4; a second, nearly empty round whenever that rounds up) or down, with segments of at least `min_seg` rows.
inline double smrf_cu_rate(int k) {   // what k resident workgroups get out of a CU beside one
  return k <= 1 ? 1.0 : k == 2 ? 1.57 : k == 3 ? 2.1 : 2.37 + 0.1 * (k - 4);
}
inline int smrf_pick_nseg(int rows, int strips, int resident, int rounds, int warm, int batch, int min_seg, int rule) {
  // the full-rounds count of rules 1, 2 (and rule 0's candidate for a launch that asks for several rounds)
  const int full = (rounds * resident * 256 + (rule == 1 ? strips / 2 : 0)) / strips;
  int full_seg = (rows + (full > 1 ? full : 1) - 1) / (full > 1 ? full : 1);
  full_seg = full_seg > min_seg ? full_seg : min_seg;
  full_seg = full_seg < rows ? full_seg : rows;
  const int full_nseg = (rows + full_seg - 1) / full_seg;
  if (rule != 0) return full_nseg;
  int best = 1;
  double best_cost = 0.0;
  for (int k = 1; k <= resident; ++k) {
    int nseg = (int)(((long long)k * 256) / strips);
    if (nseg < 1) continue;
    const int most = rows / batch > 1 ? rows / batch : 1;
    nseg = nseg < most ? nseg : most;
    int seg = (rows + nseg - 1) / nseg;
    seg = ((seg + batch - 1) / batch) * batch;
    nseg = (rows + seg - 1) / seg;
    const int busiest = (int)(((long long)nseg * strips + 255) / 256);
    const double cost = busiest * (double)(seg + warm + 20) / smrf_cu_rate(busiest);
    if (best_cost == 0.0 || cost < best_cost) {
      best_cost = cost;
      best = nseg;
    }
  }
  if (rounds > 1 && best_cost > 0.0) {
    // A launch that asks for several rounds (the chained kernels: three) against the best single round.  Several rounds keep
    // every CU at `resident` workgroups until the end - a single round ends with the 3 % per residency class its youngest
    // workgroups are behind (profiles/r05_segment_balance.md section 1) - but march more warm-up rows.  Measured, windows
    // 1..10: one round wins below ~10^8 cells (8193^2 -6 %, 4096^2 -6.5 %, 1024^2 -17 %), three win at 16384^2 (+1.9 %).
    const int seg = ((full_seg + batch - 1) / batch) * batch;
    const int nseg = (rows + seg - 1) / seg;
    const double per_cu = (double)nseg * strips / 256.0;               // workgroups a CU runs one after the other, resident at a time
    const double many = (per_cu > resident ? per_cu : resident) * (double)(seg + warm + 20) / smrf_cu_rate(resident);
    const int k1 = (int)(((long long)best * strips + 255) / 256);
    if (many < best_cost * (1.0 + 0.03 * (k1 - 1))) return nseg;
  }
  return best;
}

// Output rows per workgroup of a marching launch: `forced` rounded up to the batch, or (forced <= 0) the rows divided over
// smrf_pick_nseg's count.
inline int smrf_seg_len(int rows, int strips, int resident, int rounds, int warm, int batch, int min_seg, int rule, int forced) {
  int seg = forced;
  if (seg <= 0) {
    const int nseg = smrf_pick_nseg(rows, strips, resident, rounds, warm, batch, min_seg, rule);
    seg = (rows + nseg - 1) / nseg;
  }
  return ((seg + batch - 1) / batch) * batch;
}

// Where the output rows of one ring pass go.  seg_cls = number of residency classes (0: segment `by` is rows by * seg ...,
// `seg` rows each); class c holds the segments seg_first[c] .. seg_first[c + 1] - 1, each seg_len[c] rows, the first at row
// seg_row0[c] (ring_kernel decodes it; tests/test_host_logic.py restates that decode and checks that every row is taken once).
struct SmrfRingPlan {
  int seg;            // rows of the longest segment
  int grid_y;         // rows of segments launched
  int seg_cls;
  int seg_first[8], seg_row0[8], seg_len[8];
  int seg_equal;      // the length with equal segments (the mean length: what the dual-radius rule looks at)
};

// `slope`: permille of segment length per residency class (0 = equal segments); `forced`: SMRF_RING_SEG / the caller's
// segment length (<= 0: by smrf_pick_nseg); `max_rows`: the longest segment the instance's addressing allows (0 = any).
inline SmrfRingPlan smrf_ring_plan(int out_rows, int strips, int radius, int batch, int resident, int rounds, int rule,
                                   int slope, int forced, int max_rows) {
  SmrfRingPlan p = {};
  // output rows per workgroup: one round (every workgroup resident at once, the longest segments, the fewest re-read
  // halo rows) is the fastest from radius 20 up and as fast as any below (tools/ring_tune.py cur@SMRF_RING_ROUNDS=n);
  // how many rows of segments that round holds - all slots on a large raster, the CUs k times over on a small one -
  // is smrf_pick_nseg's cost model
  p.seg = smrf_seg_len(out_rows, strips, resident, rounds, 2 * radius, batch, std::max(32, 4 * radius), rule, forced);
  p.seg_equal = p.seg;
  p.grid_y = (out_rows + p.seg - 1) / p.seg;
  // Segments of unequal length.  All workgroups of a one-round launch start within ~1 us, but they do not run at one speed:
  // a CU's SIMDs issue oldest wave first, so the workgroup that reached a CU first finishes first - measured per workgroup
  // (tools/experiments/ring_tails.py, profiles/r05_segment_balance.md): the k-th workgroup of a CU takes 5-9 % longer than the
  // (k-1)-th at every radius, the launch lasts as long as the youngest, and the workgroups are resident for only 0.87-0.90 of
  // it on average.  Workgroups are dealt to the CUs in dispatch order, 256 at a time (8 XCDs x 32 CUs), and ring_kernel's tile
  // mapping makes `by` grow with the dispatch id: segment `by` is of residency class (by * strips + strips / 2) / 256 (where most
  // of its workgroups are), and the segments of class c get 1 + slope * ((classes - 1) / 2 - c) times the mean length.  Any
  // segmentation gives the same bits.
  // Measured (profiles/r05_segment_balance.md): -1.4 ... -2.1 % of the 16384^2 step at 60 permille per class (40 ... 100 are
  // within 0.3 % of it), nothing for fp64 (its classes differ by 3 %), and -1 ... +1 % where the classes do not fall on
  // whole rows of segments (strips does not divide 256) - so the caller's built-in slope is for fp32 rasters whose strips do.
  const bool one_round = forced <= 0 && rounds == 1;
  const auto cls_of = [&](int by) { return std::min(7, (int)(((long long)by * strips + strips / 2) / 256)); };
  const int ncls = cls_of(p.grid_y - 1) + 1;
  if (slope > 0 && one_round && strips <= 256 && ncls >= 2) {
    int n[8] = {0};
    for (int by = 0; by < p.grid_y; ++by) n[cls_of(by)]++;
    double wsum = 0.0, w[8];
    for (int c = 0; c < ncls; ++c) {
      w[c] = 1.0 + 1e-3 * slope * (0.5 * (ncls - 1) - c);
      wsum += w[c] * n[c];
    }
    const double base = (double)out_rows / wsum;
    int first = 0, row0 = 0, longest = 0;
    bool ok = true;
    for (int c = 0; c < 8; ++c) {
      int len = batch;
      if (c < ncls) {
        len = std::max(1, (int)(base * w[c] / batch + 0.999)) * batch;          // up to a multiple of the batch
        ok = ok && n[c] > 0 && 2 * len >= std::max(32, 4 * radius);
      }
      p.seg_first[c] = c < ncls ? first : p.grid_y;
      p.seg_row0[c] = row0;
      p.seg_len[c] = len;
      if (c < ncls) {
        first += n[c];
        row0 += n[c] * len;
        longest = std::max(longest, len);
      }
    }
    if (ok && row0 >= out_rows) {
      p.seg_cls = ncls;
      p.seg = longest;                                                      // what the span clamp below looks at
    }
  }
  if (max_rows > 0 && p.seg > max_rows) {                                   // (the caller has refused max_rows < batch)
    p.seg_cls = 0;
    p.seg = std::min(p.seg_equal, (max_rows / batch) * batch);
  }
  if (p.seg_cls == 0) p.grid_y = (out_rows + p.seg - 1) / p.seg;
  return p;
}
