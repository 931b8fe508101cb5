// Which launch every window of progressive_filter takes: the whole rule, as tables and one pure function (smrf_pf_route).
// The row-band driver (neilpy_amd/sharded.py) asks that function through smrf_pf_plan of the C ABI.  smrf_pf_fold, a second pure
// function after it, marks the two-pass windows whose erosion is taken inside their dilation pass, and smrf_pf_steps, the third,
// turns the three lists into the launches of a whole-raster call, each with the workspace planes it reads and writes: the
// whole-raster driver (morph.hip, progressive_filter_api) is a flat loop over that list.  Plain C++, no HIP: included by
// smrf_common.h and compiled on its own by tests/pf_host.py for tests/test_pf_route_host.py, test_pf_fold_host.py and
// test_pf_steps_host.py.
#pragma once
#include <cstdint>

// The values of include/smrf_hip.h the rule speaks in (SMRF_IMPL_*, SMRF_RING_MAX_RADIUS, SMRF_ROUTE_*), restated so that the
// header compiles without it and checked wherever both are seen.
constexpr int kPfImplAuto = 0, kPfImplRing = 1, kPfImplDirect = 2, kPfRingMaxRadius = 64;
constexpr int kPfRouteTwoPass = 0, kPfRouteFused = 1, kPfRouteDirect = 2, kPfRouteCopy = 3, kPfRouteChain = 4;
#ifdef SMRF_HIP_H
static_assert(kPfImplAuto == SMRF_IMPL_AUTO && kPfImplRing == SMRF_IMPL_RING && kPfImplDirect == SMRF_IMPL_DIRECT &&
              kPfRingMaxRadius == SMRF_RING_MAX_RADIUS && kPfRouteTwoPass == SMRF_ROUTE_TWO_PASS &&
              kPfRouteFused == SMRF_ROUTE_FUSED && kPfRouteDirect == SMRF_ROUTE_DIRECT && kPfRouteCopy == SMRF_ROUTE_COPY &&
              kPfRouteChain == SMRF_ROUTE_CHAIN, "pf_route.h restates include/smrf_hip.h");
#endif

// ------------------------------------------------------------------------------------------
// chained / table-free launches (morph_chain.h; chain.hip instantiates one kernel per pattern index)
// ------------------------------------------------------------------------------------------
struct SmrfChainPattern { int n; int r[4]; long long min_cells; long long min_cells_f64; };   // min_cells < 0: no kernel at that dtype
// The launches that exist, in the order they are tried (NP row pairs per batch - SMRF_CHAIN_NP - and the occupancy a kernel
// is built for are per pattern, chain.hip).  A single window is a chain of one: the same table-free stages, which up to
// R = 10 beat the table-building fused kernel of morph_fused.h (and the two ring passes of R = 9): at R <= 6 they run at the
// device's copy rate (0.55 ms for the 10 B/cell of a 16384^2 fp32 window).  min_cells: the smallest raster a pattern is
// taken for (a chain's segments start sum(2R) rows early and its strips lose sum(2R) columns per side).
// Measured on 16384^2 fp32 against round 2's one fused launch (two ring passes at R = 9) per window, ms
// (profiles/r03_chain_windows.md): 1, 2, 3: 0.79 against 1.96; 4, 5: 0.84 against 1.42 (on 4096^2 two single launches
// win: 0.103 against 0.114); 6: 0.55 against 0.76; 7: 0.67 against 0.79; 8: 0.65 against 0.84; 9: 0.72 against 1.07;
// 10: 0.79 against 0.99; a chain 6, 7 takes 1.31 (two singles 1.22; round 4, built for 3 waves per SIMD - 154-158 registers,
// no scratch: 1.28 against 1.18, profiles/r04_logs/chain_6_7_ab.log), a chain 8, 9 (172 registers, two workgroups per CU)
// 3.1 against 2.0: neither exists.
// Round 4 (grouped neighbour reads, chain_stage_grouped; profiles/r04_chain_grouped.md): fp64 singles exist at R = 4, 5, 7, 8
// (8192^2: 0.279 against the fused opening's 0.374 ms at R = 4, 0.308 / 0.330 at 5, 0.425 against two ring passes' 0.549 at 7,
// 0.461 / 0.531 at 8; R = 6 loses to the fused kernel by 7 %, R = 9, 10 - 174-186 registers, two waves per SIMD - to the ring
// passes by 14-20 %; on 4096^2 only R = 4 and 7 still win).  The fp32 singles R = 11..14 in the grouped form (139-166
// registers, 3 waves per SIMD) measured 12-16 % SLOWER than the fused kernels (0.99 / 1.01 / 1.08 / 1.14 against 0.85 / 0.89 /
// 0.96 / 1.02 ms on 16384^2): the cell-by-cell window growth costs R min / max per row and stage where the table costs
// K - 1 + ~3, and from R = 11 that outweighs the table's two extra barriers.  They do not exist.
// The fp64 chain 1, 2, 3 (134 registers at one row pair per batch, 3 waves per SIMD): 0.578 against 0.615 ms for chain 1, 2 + the
// fused R = 3 on 8192^2, slower on 4096^2 and 1024^2 (profiles/r04_logs/chain_123_f64_ab.log): from 48 Mi cells in round 4.
// Round 5: the thresholds below were measured again after the launches' segmentation changed (seg_rule.h: one round cut by the
// cost model on rasters this small; profiles/r05_logs/segments/min_cells_f32.log, min_cells_f64.log: default routing against
// every kind that exists on 1024^2 ... 6000^2).  fp32: the chain 4, 5 wins from 5000^2 (-6 %, 6000^2 -11 %; loses 7-19 % on
// 2048^2 and 4096^2), the singles R = 9, 10 win 17-27 % on 5000^2 and 6000^2; R = 9 also wins 9-13 % on 1024^2 ... 3000^2 and ties
// on 4096^2 (any size now), R = 10 ties below 5000^2.  fp64: the chain
// 1, 2, 3 and the single R = 5 win on every raster tried (-4 ... -16 %), R = 7 from 2048^2 (-7 %), R = 8 from 4096^2
// (-11 ... -21 %; +10 ... +14 % below).
constexpr long long kLarge = 20ll << 20;
constexpr long long kMid = 16ll << 20;
constexpr long long kSmall = 4ll << 20;
constexpr long long kNever = -1;
constexpr SmrfChainPattern kPatterns[] = {{3, {1, 2, 3, 0}, 0, 0}, {2, {1, 2, 0, 0}, 0, 0}, {2, {2, 3, 0, 0}, 0, 0}, {2, {4, 5, 0, 0}, kLarge, kNever},
                                          {1, {4, 0, 0, 0}, 0, 0}, {1, {5, 0, 0, 0}, 0, 0}, {1, {6, 0, 0, 0}, 0, kNever}, {1, {7, 0, 0, 0}, 0, kSmall},
                                          {1, {8, 0, 0, 0}, 0, kMid}, {1, {9, 0, 0, 0}, 0, kNever}, {1, {10, 0, 0, 0}, kLarge, kNever}};
constexpr int kNPatterns = (int)(sizeof(kPatterns) / sizeof(kPatterns[0]));
constexpr long long kPfAnySize = 1ll << 62;   // `cells` of a question that no size threshold is to answer

// the pattern a window list starts with on a raster of `cells` cells (-1: none), its length and its halo rows sum(2R)
inline int smrf_chain_match(int elem_size, const int32_t* windows, int n, long long cells) {
  for (int p = 0; p < kNPatterns; ++p) {
    const long long mc = elem_size == 8 ? kPatterns[p].min_cells_f64 : kPatterns[p].min_cells;
    if (kPatterns[p].n > n || mc < 0 || cells < mc) continue;
    bool ok = true;
    for (int i = 0; i < kPatterns[p].n; ++i) ok = ok && windows[i] == kPatterns[p].r[i];
    if (ok) return p;
  }
  return -1;
}
inline int smrf_chain_length(int pat) { return pat >= 0 && pat < kNPatterns ? kPatterns[pat].n : 0; }
inline int smrf_chain_halo(int pat) {
  int s = 0;
  if (pat >= 0 && pat < kNPatterns)
    for (int i = 0; i < kPatterns[pat].n; ++i) s += 2 * kPatterns[pat].r[i];
  return s;
}

// ------------------------------------------------------------------------------------------
// fused opening + flag (morph_fused.h)
// ------------------------------------------------------------------------------------------
// radii whose progressive_filter window runs as ONE fused opening + flag launch, per dtype: measured
// against the two ring passes per radius on the 16384^2 benchmark DEM (gpurun_out/r02/fused3_per_radius_f32.log,
// fused2_per_radius_f64.log, fused_hi_f32.log).  fp32: 1..8 and 10..14 (9 loses by 3 %, 15 and up by 20 % and more);
// fp64, whose tables are twice as large: 1..6.
#ifndef SMRF_FUSED_MAX_RADIUS
#define SMRF_FUSED_MAX_RADIUS 14
#endif
constexpr bool smrf_fused_radius(int elem_size, int r) {
  if (r < 1 || r > SMRF_FUSED_MAX_RADIUS) return false;
  return elem_size == 4 ? (r != 9) : (r <= 6);
}
// above R = 8 the fused kernel's 4R warm-up rows per segment only pay on rasters large enough for long segments
// (4096^2, windows 1..18: 1.64 ms with R <= 8 fused, 1.70 ms with 10..14 as well; 8192^2: 5.9 -> 5.2 ms with them);
// round 5, after the launches' segmentation changed: from 20 Mi cells (5000^2: R = 11..13 -7 ... -11 %, 6000^2 -10 ... -17 %,
// R = 14 equal; 4096^2 and below +3 ... +20 %: profiles/r05_logs/segments/min_cells_fused.log); 48 Mi until then.
// A row band takes the fused opening up to kFusedSmallRadius only, whatever its size: a band's segments are short against
// the 4R warm-up rows (tools/band_compute.py).
constexpr int kFusedSmallRadius = 8;
constexpr long long kFusedLargeCells = 20ll << 20;

// ------------------------------------------------------------------------------------------
// incremental erosion (morph_incero.h; incero.hip instantiates one kernel per radius)
// ------------------------------------------------------------------------------------------
#define SMRF_INCERO_MIN_RADIUS 16   // the first window after the first two-pass window of a default call (15)
#define SMRF_INCERO_MAX_RADIUS 64
namespace smrf {
#include "ero_inc_adopt.inc"
}  // namespace smrf
// has = an instance exists for this dtype and radius, adopted = the measured per-radius table takes it
inline bool smrf_inc_erode_has(int elem_size, int radius) {
  return elem_size == 4 && radius >= SMRF_INCERO_MIN_RADIUS && radius <= SMRF_INCERO_MAX_RADIUS;
}
inline bool smrf_inc_erode_adopted(int elem_size, int radius) {
  return smrf_inc_erode_has(elem_size, radius) && smrf::kEroIncAdoptF32[radius] != 0;
}

// ------------------------------------------------------------------------------------------
// cross on load (morph_ring.h, ring_cross_kernel; ring_part.hip instantiates one per radius)
// ------------------------------------------------------------------------------------------
// The radii whose leftover set P_R is empty (ero_inc.inc; morph_incero.h checks this list against it): there
// e_R = erode(e_{R-1}, 5-point cross) exactly, and the window's dilation pass can take that cross while it loads e_{R-1}.
constexpr bool smrf_dil_cross_has(int elem_size, int radius) {
  return elem_size == 4 && (radius == 16 || radius == 21 || radius == 36);
}
namespace smrf {
#include "dil_cross_adopt.inc"
}  // namespace smrf
inline bool smrf_dil_cross_adopted(int elem_size, int radius) {
  return smrf_dil_cross_has(elem_size, radius) && smrf::kDilCrossAdoptF32[radius] != 0;
}

// ------------------------------------------------------------------------------------------
// the plan
// ------------------------------------------------------------------------------------------
struct SmrfPfRules {
  int elem_size;   // 4 or 8
  int fused;       // SMRF_FUSED: 0 = never a fused / chained launch, 1 = by the size rules, 2 = every one that exists whatever the size (tests)
  int chain;       // SMRF_CHAIN: 0 = no chained / table-free launches (every window its own launch)
  int ero_inc;     // SMRF_ERO_INC: 0 = never, 1 = where ero_inc_adopt.inc says it wins, 2 = every eligible window
  int impl;        // SMRF_IMPL_*: the fused, chained and incremental kernels are ring kernels (auto or ring only)
  int nan_aware;   // != 0: the raster may hold NaNs.  scipy's NaN rule lives in the two-pass kernels only
  int band;        // 0 = a whole raster; 1 = the row-band driver: `rows` is the image's rows, `cells` what one launch marches (the
                   // longest band with its two-sided margin), fused openings up to kFusedSmallRadius only, and no incremental erosion
                   // (its kernel takes whole rasters: a band's e_{R-1} margin rows are stale after a halo exchange);
                   // 2 = a row band whose launches cannot be chained either (the edge-first split of overlap=True, a single band)
  int dil_cross;   // SMRF_DIL_CROSS (smrf_pf_fold only): 0 = never, 1 = where dil_cross_adopt.inc says it wins, 2 = every eligible window
};

// Window by window, for i = 0 .. n - 1 (windows[i] >= 0):
//   route[i]    SMRF_ROUTE_*.  A chained launch takes the windows i .. i + len - 1, which read SMRF_ROUTE_CHAIN + position.
//   ero_inc[i]  1 = the window's erosion comes from the previous window's (inc_erode_kernel); only beside SMRF_ROUTE_TWO_PASS
//   pattern[i]  (may be NULL) at the head of a chained launch its index in kPatterns, -1 everywhere else
// chain: no NaN, impl auto or ring, SMRF_FUSED and SMRF_CHAIN on, a pattern matches the windows from i on at this size, and the
// raster has more rows than the pattern's halo; else fused: the first three again, a fused kernel for the radius, and the
// radius small or the (whole) raster large; else copy for radius 0, two ring passes up to kPfRingMaxRadius under auto, the
// direct kernel beyond.  Incremental erosion: a whole raster without NaN, this window and the one before both two ring passes,
// radius = the previous radius + 1, an instance exists, and the table adopts it or SMRF_ERO_INC = 2.  The identity holds on
// any raster size (tests/test_ero_inc.py), so there is no size condition.
inline void smrf_pf_route(const SmrfPfRules& k, const int32_t* windows, int n, int rows, long long cells, int32_t* route,
                          uint8_t* ero_inc, int32_t* pattern = nullptr) {
  const bool fuse_ok = !k.nan_aware && (k.impl == kPfImplAuto || k.impl == kPfImplRing) && k.fused != 0;
  const bool chain_ok = fuse_ok && k.chain != 0 && k.band != 2;
  for (int i = 0; i < n; ++i) {
    ero_inc[i] = 0;
    if (pattern) pattern[i] = -1;
  }
  for (int i = 0; i < n;) {
    const int r = windows[i];
    const int pat = chain_ok ? smrf_chain_match(k.elem_size, windows + i, n - i, k.fused == 2 ? kPfAnySize : cells) : -1;
    const int len = pat >= 0 && smrf_chain_halo(pat) < rows ? smrf_chain_length(pat) : 0;
    if (len) {
      if (pattern) pattern[i] = pat;
      for (int j = 0; j < len; ++j) route[i + j] = kPfRouteChain + j;
      i += len;
      continue;
    }
    if (fuse_ok && smrf_fused_radius(k.elem_size, r) &&
        (r <= kFusedSmallRadius || (!k.band && (k.fused == 2 || cells >= kFusedLargeCells)))) {
      route[i++] = kPfRouteFused;
      continue;
    }
    const int eff = k.impl == kPfImplAuto ? (r <= kPfRingMaxRadius ? kPfImplRing : kPfImplDirect) : k.impl;
    route[i] = r == 0 ? kPfRouteCopy : eff == kPfImplRing ? kPfRouteTwoPass : kPfRouteDirect;
    ero_inc[i] = !k.band && k.ero_inc != 0 && !k.nan_aware && i > 0 && route[i] == kPfRouteTwoPass &&
                 route[i - 1] == kPfRouteTwoPass && r == windows[i - 1] + 1 && smrf_inc_erode_has(k.elem_size, r) &&
                 (k.ero_inc == 2 || smrf_inc_erode_adopted(k.elem_size, r));
    ++i;
  }
}

// Which two-pass windows fold their erosion into their dilation pass (cross on load), after smrf_pf_route has made route[] and
// ero_inc[] (both are read only and keep their meaning: smrf_pf_ero_inc_windows and smrf_pf_plan report them as before).
//   fold[i] = kPfFoldCross  window i launches no erosion: its dilation reads e_{R-1} (the plane of window i - 1's erosion), takes the
//                           5-point cross on load and writes the opened surface into the spare plane.  When: fp32, a whole raster
//                           without NaN, impl auto or ring, windows i - 1 and i both two ring passes, radius = the previous radius
//                           + 1, P_radius empty (smrf_dil_cross_has), window i - 1 not folded itself (its e is then not in the
//                           workspace), and SMRF_DIL_CROSS = 2 - or = 1, dil_cross_adopt.inc adopts the radius and a window
//                           follows: under the table the call's last window keeps its erosion pass, so that the workspace ends with
//                           the last window's eroded and opened surfaces as it always has (the tests of the incremental erosion
//                           read them there).
//   fold[i] = kPfFoldAfter  window i - 1 was folded: the workspace holds e_{R-2}, not e_{R-1}, so window i runs the ring erosion
//                           whatever ero_inc[i] says (smrf_pf_runs_inc), also under SMRF_ERO_INC = 2
//   fold[i] = kPfFoldNone   everything else
constexpr uint8_t kPfFoldNone = 0, kPfFoldCross = 1, kPfFoldAfter = 2;
inline void smrf_pf_fold(const SmrfPfRules& k, const int32_t* windows, const int32_t* route, const uint8_t* ero_inc, int n,
                         uint8_t* fold) {
  (void)ero_inc;   // (a window the incremental erosion would take is folded all the same: the fold removes the pass, not a part of it)
  const bool ok = k.dil_cross != 0 && !k.band && !k.nan_aware && k.elem_size == 4 && (k.impl == kPfImplAuto || k.impl == kPfImplRing);
  for (int i = 0; i < n; ++i) {
    fold[i] = i > 0 && fold[i - 1] == kPfFoldCross ? kPfFoldAfter : kPfFoldNone;
    if (!ok || i == 0 || fold[i] != kPfFoldNone) continue;
    const int r = windows[i];
    if (route[i] != kPfRouteTwoPass || route[i - 1] != kPfRouteTwoPass || r != windows[i - 1] + 1 || !smrf_dil_cross_has(k.elem_size, r))
      continue;
    if (k.dil_cross == 2 || (smrf_dil_cross_adopted(k.elem_size, r) && i + 1 < n)) fold[i] = kPfFoldCross;
  }
}
// window i's erosion comes from inc_erode_kernel: the route's flag, unless the window is folded or follows a folded one
inline bool smrf_pf_runs_inc(const uint8_t* ero_inc, const uint8_t* fold, int i) { return ero_inc[i] != 0 && fold[i] == kPfFoldNone; }

// ------------------------------------------------------------------------------------------
// the launches of a whole-raster call, in order, each with its planes
// ------------------------------------------------------------------------------------------
// The workspace is three planes, 0 .. 2; kPfPlaneZ is the caller's raster, kPfPlaneNone "the launch has no such operand".
//   kind               launches                                                  src          aux    dst
//   kPfStepChain       smrf_chain_f32 / f64(pattern), windows win .. win+len-1   last         -      spare
//   kPfStepFused       fused opening + flag                                      last         -      spare
//   kPfStepErode       erosion by impl (ring, direct, the radius-0 copy)         last         -      pe
//   kPfStepIncErode    smrf_inc_erode_f32                                        e_{R-1}: pe  last   spare
//   kPfStepDilate      dilation + flag by impl                                   e_R          last   spare; after an inc-erode the old pe
//   kPfStepDilateCross ring_cross_kernel                                         e_{R-1}: pe  last   spare
// `last` is the surface the window is compared with (Z, then the previous window's opening), pe the plane of the latest written
// erosion, spare the lowest plane that holds neither.  closes: the step ends its window (a chain: all len of them) - the route
// report and the timing event belong there.  dense: the step writes every mask / when byte: the closing step of window 0.
constexpr int kPfStepChain = 0, kPfStepFused = 1, kPfStepErode = 2, kPfStepIncErode = 3, kPfStepDilate = 4, kPfStepDilateCross = 5;
constexpr int kPfPlaneZ = -1, kPfPlaneNone = -2;
struct SmrfPfStep { int kind, win, len, src, aux, dst, dense, closes, pattern; };

// After smrf_pf_route and smrf_pf_fold: steps[] (2n entries, the caller's) gets the call's launches, the count is returned.
// The roles rotate.  The plain two passes write e_R into pe and opened_R into the spare plane.  The incremental erosion needs
// e_{R-1} beside `last`: e_R goes into the spare plane (it held opened_{R-2}), then opened_R goes over e_{R-1}.  A folded window
// writes only opened_R and leaves e_{R-1} in pe, which the next window's ring erosion overwrites.  Chained and fused launches
// leave pe alone, so plane 0 stays untouched until the first erosion (the first word of it is the NaN flag of a speculative
// first chain), and the workspace ends with the last window's opened surface beside the latest erosion written.
// tests/test_pf_steps_host.py replays the list on labelled planes.
inline int smrf_pf_steps(const int32_t* windows, const int32_t* route, const uint8_t* ero_inc, const uint8_t* fold,
                         const int32_t* pattern, int n, SmrfPfStep* steps) {
  (void)windows;   // (a step names its window, the driver reads the radius there)
  int pe = 0, pl = kPfPlaneZ, m = 0;
  for (int i = 0; i < n;) {
    int po = 0;
    while (po == pe || po == pl) ++po;
    int len = 1;
    if (route[i] == kPfRouteChain) {
      len = smrf_chain_length(pattern[i]);
      steps[m++] = {kPfStepChain, i, len, pl, kPfPlaneNone, po, i == 0, 1, pattern[i]};
      pl = po;
    } else if (route[i] == kPfRouteFused) {
      steps[m++] = {kPfStepFused, i, 1, pl, kPfPlaneNone, po, i == 0, 1, -1};
      pl = po;
    } else if (fold[i] == kPfFoldCross) {
      steps[m++] = {kPfStepDilateCross, i, 1, pe, pl, po, 0, 1, -1};
      pl = po;
    } else if (smrf_pf_runs_inc(ero_inc, fold, i)) {
      steps[m++] = {kPfStepIncErode, i, 1, pe, pl, po, 0, 0, -1};
      steps[m++] = {kPfStepDilate, i, 1, po, pl, pe, 0, 1, -1};
      pl = pe;
      pe = po;
    } else {
      steps[m++] = {kPfStepErode, i, 1, pl, kPfPlaneNone, pe, 0, 0, -1};
      steps[m++] = {kPfStepDilate, i, 1, pe, pl, po, i == 0, 1, -1};
      pl = po;
    }
    i += len;
  }
  return m;
}
