// Incremental disk erosion for progressive_filter's consecutive windows (gfx950): window R's erosion from window R-1's.
//
// Window R erodes last = opened_{R-1} = dilate(e_{R-1}, D_{R-1}) by the disk D_R.  For R = 2..64 (ero_inc.inc)
//     D_R = (D_{R-1} (+) B) u P_R,  B = the 5-point cross,  P_R = a few cells on the rim of D_R
// and erode(dilate(erode(f, A), A), A) = erode(f, A), so
//     e_R = min( erode(e_{R-1}, B),  min over p in P_R of last[x + p] )
// - an identity on min, bit-exact, and the period-2n reflect commutes with it.  2 min3 for the cross and
// |P_R| / 2 min3 for the rim instead of the ring erosion's R + K min / max per cell: the pass is bound by its 3 plane
// touches (read e_{R-1}, read last, write e_R; 2 where P_R is empty).
//
// How: a workgroup owns a strip of 256 columns (one per lane) and marches down its row segment, 4 row PAIRS of `last` per
// batch.  As in the ring kernels a pair is interleaved per cell in LDS, so one ds_read_b64 serves both rows, and the next
// batch is prefetched into registers with coalesced loads while this one is consumed; the staging area is double
// buffered: one barrier per batch.  Every input row is SCATTERED into the accumulators of the output rows it reaches:
// slot s of a register ring of 2 reach + 8 slots belongs to output row (first input row of the batch) - reach + s, the
// cell pair (dy, +-dx) of input row j updates slot j - dy + reach with one v_min3 - all indices compile-time, a slot that
// receives nothing costs one move - and the ring turns by 8 slots per batch inside those updates (IncEroCfg::Plan).  The
// cell pairs (dy, +-dx) and (-dy, +-dx) of one input row pair read the same two LDS cells: a mirror plan reads them once and
// updates the low and the high slot together (|P_R| / 4 + a few ds_read_b64 per row pair instead of |P_R| / 2).  The 8
// rows a batch completes take the cross of e_{R-1} (five loads per cell, issued before the batch's LDS phase and before
// the prefetch, so that the waits for them leave the prefetch in flight - or, at five large rims, after the LDS phase, which
// frees 26 registers for a third wave per SIMD) and are stored one batch late.  No scratch.
#pragma once
#include "morph_ring.h"

namespace smrf {

#include "ero_inc.inc"
// (SMRF_INCERO_MIN_RADIUS / _MAX_RADIUS, the radii with an instance, and the adoption table ero_inc_adopt.inc: pf_route.h)
// the radii pf_route.h folds into the dilation pass (cross on load) are exactly the rim-free ones from the first two-pass window up
constexpr bool dil_cross_radii_are_rim_free() {
  for (int r = SMRF_INCERO_MIN_RADIUS; r <= SMRF_INCERO_MAX_RADIUS; ++r)
    if (smrf_dil_cross_has(4, r) != (kEroInc[r].n == 0)) return false;
  return true;
}
static_assert(dil_cross_radii_are_rim_free(), "smrf_dil_cross_has (pf_route.h) against ero_inc.inc");

// Two choices per radius, both made by measurement on MI355X at 16384^2 (profiles/incero_mirror.md sections 1 and 3):
//   kIncEroPlanKind  how a batch's LDS reads are planned (IncEroCfg::make_plan).  The mirror plan with split groups everywhere;
//                    with copies at 44 and 45, the radii whose split plan reads most groups twice (19 and 11 of 44 and 32).
//   kIncEroCrossLate 1 = the cross of e_{R-1} is loaded AFTER the LDS phase, which frees its 26 load destinations during it.
//                    Taken where that buys the third wave per SIMD (168 VGPRs) and measures faster: 39, 44, 45, 49, 50.  Where
//                    the early loads fit three waves they are 2-5 percent faster, and loading half of the cross late measured
//                    slower than either at every radius.
// R = 51..64 are not measured (the benchmark stops at 50) and take the defaults.
enum { kIncEroPlain = 0, kIncEroMirrorSplit = 1, kIncEroMirrorCopy = 2 };
inline constexpr unsigned char kIncEroPlanKind[65] = {
    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 1, 1, 1, 1, 1,
    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
inline constexpr unsigned char kIncEroCrossLate[65] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#ifndef SMRF_INCERO_MIRROR_GROUP
#define SMRF_INCERO_MIRROR_GROUP 2   // mirror groups (two reads, four updates each) per lookup group
#endif
constexpr int inc_ero_plan_kind(int radius) {
#ifdef SMRF_INCERO_PLAN              // developer A/B builds: one kind for every radius
  return SMRF_INCERO_PLAN;
#else
  return kIncEroPlanKind[radius];
#endif
}
constexpr bool inc_ero_cross_late(int radius) {
#ifdef SMRF_INCERO_LATE              // developer A/B builds
  return SMRF_INCERO_LATE;
#else
  return kIncEroCrossLate[radius] != 0;
#endif
}

template <typename T>
struct IncEroArgs {
  const T* e_prev;    // e_{R-1}
  const T* last;      // opened_{R-1}
  T* out;             // e_R
  int rows, cols;
  long long ld;
  int seg;            // output rows per workgroup
  int nt;             // streaming stores (morph.hip nt_rule)
  int plain_tiles;    // SMRF_XCD_REMAP=0
};

template <int R>
struct IncEroCfg {
  static constexpr int N = kEroInc[R].n;                 // cell pairs (dy, +-dx)
  static constexpr int DY = kEroInc[R].reach;            // largest |dy| = largest dx
  static constexpr int TW = 256, NP = 4, ROWS = 2 * NP;
  static constexpr int W = TW + 2 * DY;                  // staged cells per row
  static constexpr int NPOS = (W + TW - 1) / TW;
  static constexpr int NACC = 2 * DY + ROWS;
  // How a batch's LDS reads are planned (inc_ero_plan_kind): kIncEroPlain = one pair of reads per job; the mirror kinds read the
  // two cells of (row pair, dx) once for the jobs (dy, dx) and (-dy, dx), which update slots 2p - |dy| + DY and 2p + |dy| + DY.
  static constexpr int KIND = N > 0 ? inc_ero_plan_kind(R) : kIncEroPlain;
  static constexpr int NM = N / 2;                       // mirror pairs: cell pair k < NM is (-d, dx), cell pair N - 1 - k is (d, dx)
  static constexpr int G = KIND == kIncEroPlain ? 4 : SMRF_INCERO_MIRROR_GROUP;   // items (two reads each) per lookup group, two groups in flight
  static constexpr int NJ = NP * N;                      // jobs per batch: job j = row pair j / N, cell pair j % N
  static constexpr int dy(int k) { return kEroInc[R].p[k].dy; }
  static constexpr int dx(int k) { return kEroInc[R].p[k].dx; }
  // job j = (row pair j / N, cell pair j % N) updates the ring slots slot(j) (row A of its pair) and slot(j) + 1 (row B)
  static constexpr int slot(int j) { return 2 * (j / N) - dy(j % N) + DY; }
  static constexpr int mirror(int j) { return (j / N) * N + N - 1 - j % N; }
  static constexpr bool mirrored() {
    for (int k = 0; k < N; ++k)
      if (dy(k) != -dy(N - 1 - k) || dx(k) != dx(N - 1 - k) || dy(k) == 0) return false;
    return N % 2 == 0;
  }
  // The ring turns in place: the first update slot s receives in a batch reads what slot s + ROWS held and writes slot s's
  // own register, so it has to come before slot s + ROWS receives its own first update and overwrites that value (the two
  // never live at once).  first[s] = the item that updates slot s first, NONE if the batch leaves the slot alone.
  //   kIncEroPlain: an item is one job, the jobs run by ascending slot, which keeps the rule by construction.
  //   mirror kinds: an item is a mirror group (one pair of reads, four updates: a low and a high slot at once), so the order
  // is a constraint problem, solved greedily: run the ready group (every slot it would update first has slot - ROWS done or
  // untouched) with the lowest slot; where none is ready, kIncEroMirrorSplit runs one ready half of a group as a job of its
  // own (a second pair of reads for that group; the half that makes most groups ready) and kIncEroMirrorCopy runs the group
  // with the fewest unready slots anyway (each costs the allocator one copy: the plan counts them, the C++ below is
  // right in any order because it reads the ring's previous state from `old`).
  static constexpr short NONE = 32767;
  struct Item { short j; bool both; };                   // the job whose two cells are read; both: its mirror job is applied too
  struct Plan { short n, splits, copies; Item item[NJ > 0 ? NJ : 1]; short first[NACC]; };
  static constexpr Plan make_plan() {
    Plan pl{};
    for (int s = 0; s < NACC; ++s) pl.first[s] = NONE;
    auto emit = [&](int j, bool both) {
      for (int h = 0; h < (both ? 2 : 1); ++h)
        for (int b = 0; b < 2; ++b) {
          short& f = pl.first[slot(h ? mirror(j) : j) + b];
          if (f == NONE) f = pl.n;
        }
      pl.item[pl.n++] = Item{(short)j, both};
    };
    if constexpr (KIND == kIncEroPlain) {
      for (int s = 0; s < NACC; ++s)
        for (int j = 0; j < NJ; ++j)
          if (slot(j) == s) emit(j, false);
    } else {
      constexpr int NGR = NP * NM;                        // mirror groups: g = (row pair g / NM, mirror pair g % NM)
      auto jlo = [](int g) { return (g / NM) * N + NM + g % NM; };      // dy > 0: the lower slot
      auto lo = [&](int g) { return slot(jlo(g)); };
      auto hi = [&](int g) { return slot(mirror(jlo(g))); };
      bool touched[NACC] = {}, done[NACC] = {};
      unsigned char state[NGR > 0 ? NGR : 1] = {};        // bit 0: the low half has run, bit 1: the high half
      for (int g = 0; g < NGR; ++g) touched[lo(g)] = touched[lo(g) + 1] = touched[hi(g)] = touched[hi(g) + 1] = true;
      auto unready = [&](int g, int part) {               // how many first updates of (g, part) would break the rule now
        int u = 0;
        for (int h = 0; h < 2; ++h)
          if (part >> h & 1)
            for (int b = 0; b < 2; ++b) {
              const int t = (h ? hi(g) : lo(g)) + b;
              u += !(done[t] || t < ROWS || !touched[t - ROWS] || done[t - ROWS]);
            }
        return u;
      };
      auto run = [&](int g, int part) {
        pl.copies += (short)unready(g, part);
        if (part & 1) done[lo(g)] = done[lo(g) + 1] = true;
        if (part & 2) done[hi(g)] = done[hi(g) + 1] = true;
        state[g] |= (unsigned char)part;
        emit(part == 2 ? mirror(jlo(g)) : jlo(g), part == 3);
      };
      for (int left = 2 * NGR; left > 0;) {
        int bg = -1, bpart = 0, bkey = 0;
        for (int g = 0; g < NGR; ++g) {                   // a ready group, or the ready other half of a split one
          const int part = 3 & ~state[g];
          if (!part || unready(g, part)) continue;
          const int key = part & 1 ? lo(g) : hi(g);
          if (bg < 0 || key < bkey) bg = g, bpart = part, bkey = key;
        }
        if (bg < 0 && KIND == kIncEroMirrorSplit) {
          int bcnt = -1;
          for (int g = 0; g < NGR; ++g)
            for (int part = 1; part <= 2 && !state[g]; ++part) {
              if (unready(g, part)) continue;
              const int s = part == 1 ? lo(g) : hi(g);
              const bool was[2] = {done[s], done[s + 1]};
              done[s] = done[s + 1] = true;
              state[g] |= (unsigned char)part;
              int cnt = 0;                                // what this half makes ready: only what touches s + ROWS, s + 1 + ROWS
              for (int h = 0; h < NGR; ++h) {
                const int rest = 3 & ~state[h];
                const int a = lo(h) - s - ROWS, c = hi(h) - s - ROWS;
                if (rest && ((a >= -1 && a <= 1) || (c >= -1 && c <= 1)) && !unready(h, rest)) ++cnt;
              }
              state[g] = 0;
              done[s] = was[0], done[s + 1] = was[1];
              if (cnt > bcnt || (cnt == bcnt && s < bkey)) bg = g, bpart = part, bkey = s, bcnt = cnt;
            }
          ++pl.splits;
        } else if (bg < 0) {
          int bu = 0;
          for (int g = 0; g < NGR; ++g) {
            if (state[g]) continue;
            const int u = unready(g, 3);
            if (bg < 0 || u < bu || (u == bu && lo(g) < bkey)) bg = g, bpart = 3, bkey = lo(g), bu = u;
          }
        }
        run(bg, bpart);
        left -= bpart == 3 ? 2 : 1;
      }
    }
    return pl;
  }
  static constexpr Plan plan = make_plan();
  static constexpr int NI = plan.n;                      // items = pairs of reads per batch
  static constexpr int NG = (NI + G - 1) / G;
  static constexpr int gsize(int g) { const int n = NI - g * G; return n < 0 ? 0 : n > G ? G : n; }
  // every job is applied once; a mirror group is read once unless it is one of the counted splits; every slot a batch updates
  // has exactly one first update, which is its earliest, and slot s has it before slot s + ROWS - but for the counted copies
  // (tests/test_incero_plan_host.py states the same in Python from ero_inc.inc)
  static constexpr bool plan_ok() {
    if (N > 0 && !mirrored()) return false;
    int seen[NJ > 0 ? NJ : 1] = {};
    for (int i = 0; i < NI; ++i) {
      ++seen[plan.item[i].j];
      if (plan.item[i].both) ++seen[mirror(plan.item[i].j)];
    }
    for (int j = 0; j < NJ; ++j)
      if (seen[j] != 1) return false;
    if (KIND == kIncEroPlain ? NI != NJ || plan.splits || plan.copies : NI != NP * NM + plan.splits) return false;
    if ((KIND == kIncEroMirrorSplit && plan.copies) || (KIND == kIncEroMirrorCopy && plan.splits)) return false;
    int late = 0;
    for (int s = 0; s < NACC; ++s) {
      int earliest = NONE, touches = 0;
      for (int i = NI - 1; i >= 0; --i)
        for (int h = 0; h < (plan.item[i].both ? 2 : 1); ++h)
          for (int b = 0; b < 2; ++b)
            if (slot(h ? mirror(plan.item[i].j) : plan.item[i].j) + b == s) { ++touches; earliest = i; }
      if (plan.first[s] != earliest) return false;
      if (touches && s + ROWS < NACC && plan.first[s + ROWS] != NONE && plan.first[s] >= plan.first[s + ROWS]) ++late;
    }
    return late == plan.copies;
  }
  // The cross of e_{R-1} loaded after the LDS phase instead of before it (kIncEroCrossLate): its wait is then covered by the
  // other waves only, and there is one more of them.
  static constexpr bool LATE = N > 0 && inc_ero_cross_late(R);
  // the row loop starts DELTA rows early so that the 8 rows a batch completes never straddle the segment's first row
  static constexpr int DELTA = (ROWS - (2 * DY) % ROWS) % ROWS;
  static constexpr int LDS_CELLS = N > 0 ? 2 * NP * W : 1;
};

template <typename T, int R>
__global__ __launch_bounds__(256) void inc_erode_kernel(const IncEroArgs<T> a) {
  using C = IncEroCfg<R>;
  using T2 = typename Vec2<T>::type;
  constexpr int N = C::N, DY = C::DY, TW = C::TW, NP = C::NP, ROWS = C::ROWS, W = C::W, NPOS = C::NPOS, NACC = C::NACC, G = C::G;
  __shared__ T2 L[C::LDS_CELLS];
  const int tid = threadIdx.x;
  int bx, by;   // neighbouring strips (which share 2 reach halo columns) on one XCD's L2
  smrf_xcd_tile(a.plain_tiles, [] { return true; }, bx, by);
  const int x0 = bx * TW, x = x0 + tid;
  const int ys = by * a.seg, ye = min(a.rows, ys + a.seg);   // output rows [ys, ye)
  if (ys >= ye) return;
  const int xc = x < a.cols ? x : a.cols - 1;
  const int xl = smrf_fold(xc - 1, a.cols), xr = smrf_fold(xc + 1, a.cols);
  int cpos[NPOS];
  bool act[NPOS];
#pragma unroll
  for (int i = 0; i < NPOS; ++i) {
    act[i] = tid + i * TW < W;
    cpos[i] = smrf_fold(x0 - DY + tid + (act[i] ? i * TW : 0), a.cols);
  }
  T acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = ident<T>(false);

  static_assert(C::plan_ok(), "the batch plan");
  int o0 = ys - 2 * DY - C::DELTA;                        // first of the 8 output rows the next batch completes
  const int nb = (ye - o0 + ROWS - 1) / ROWS;
  RowFold rf(o0 + DY, a.rows);                            // tracks the NEXT batch to prefetch (its first input row)
  T2 pf[NP][NPOS];
  auto prefetch = [&]() {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const T* ra = a.last + (long long)rf.at(2 * p) * a.ld;
      const T* rb = a.last + (long long)rf.at(2 * p + 1) * a.ld;
#pragma unroll
      for (int i = 0; i < NPOS; ++i)
        { pf[p][i].x = ra[cpos[i]]; pf[p][i].y = rb[cpos[i]]; }   // (a lane without a cell in the last position re-reads
    }                                                               // its first: no branch, so the waits can count the loads)
    rf.advance(ROWS);
  };
  if constexpr (N > 0) prefetch();

  // The order of a batch's memory operations is what lets its loads overlap the LDS phase AND the epilogue: the counter of
  // outstanding vector-memory operations retires in order, so a wait for one load also waits for everything issued
  // before it.  Per batch, after the barrier: (1) the stores of the PREVIOUS batch's rows (outv: deferred, so that no wait
  // for a load ever covers a fresh store), (2) the cross loads of this batch's rows, (3) the prefetch of the next batch -
  // unconditionally (past the last batch it re-reads folded rows nobody uses): a prefetch under a branch would make the
  // epilogue's waits assume the path without it and drain it.  The epilogue then waits for (2) only and leaves the NP * NPOS * 2
  // loads of (3) in flight until the next batch's staging, where nothing younger is outstanding.
  T outv[ROWS];
  auto store_rows = [&](int ob) {                         // the 8 rows from output row ob
#pragma unroll
    for (int j = 0; j < ROWS; ++j)
      if (ob + j < ye && x < a.cols) smrf_store_out(a.out + (long long)(ob + j) * a.ld + x, outv[j], a.nt);
  };
  for (int b = 0; b < nb; ++b, o0 += ROWS) {
    const unsigned lds_b = (unsigned)(size_t)(__attribute__((address_space(3))) void*)(L + (b & 1) * NP * W + tid);
    if constexpr (N > 0) {
      // stage the prefetched batch.  The other half of L may still be read by a slower wave (batch b - 1): it is not touched
      // before the NEXT barrier, which that wave reaches only after it has finished reading.  No branch here either: a lane
      // without a cell in the last position writes the copy of its first cell (prefetch) over that cell, so every path
      // waits for every prefetched register and none is left pending for the load that next writes it.
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < NPOS; ++i)
          lds_write2(lds_b + (unsigned)((p * W + (i < NPOS - 1 || act[i] ? i * TW : 0)) * (int)sizeof(T2)), pf[p][i]);
      lds_wait<0>();
      __syncthreads();
    }
    if (o0 - ROWS >= ys) store_rows(o0 - ROWS);            // (whole batches: DELTA)
    // the cross of e_{R-1} for the rows this batch completes: loads issued now, used after the LDS phase - or, where that
    // costs a wave per SIMD (IncEroCfg::LATE), issued after the LDS phase
    const bool store = o0 >= ys;
    T ec[ROWS + 2], el[ROWS], er[ROWS];
    auto cross_loads = [&]() {
      RowFold rfe(o0 - 1, a.rows);
#pragma unroll
      for (int j = 0; j < ROWS + 2; ++j) {
        const T* row = a.e_prev + (long long)rfe.at(j) * a.ld;
        ec[j] = row[xc];
        if (j >= 1 && j <= ROWS) { el[j - 1] = row[xl]; er[j - 1] = row[xr]; }
      }
    };
    if constexpr (!C::LATE)
      if (store) cross_loads();
    if constexpr (N > 0) {
      __builtin_amdgcn_sched_barrier(0);                  // the cross loads stay older than the prefetch
      prefetch();
      __builtin_amdgcn_sched_barrier(0);
      // the ring turns by one batch WITHOUT moves: slot s continues what slot s + 8 held, and the first update a slot receives
      // in a batch reads that value and writes the slot's own register (untied); the later ones are tied.  Only a slot
      // that receives nothing is copied; a new-born slot (the top 8) starts from its first update's two cells.
      T old[NACC];
#pragma unroll
      for (int s = 0; s < NACC; ++s) old[s] = acc[s];
      [&]<int... S>(std::integer_sequence<int, S...>) {
        (([&] {
           if constexpr (C::plan.first[S] == C::NONE) acc[S] = S + ROWS < NACC ? old[S + ROWS] : ident<T>(false);
         }()),
         ...);
      }(std::make_integer_sequence<int, NACC>{});
      // scatter: job (row pair p, cell pair k) reads {rowA, rowB} at columns x - dx and x + dx and updates the slots of output
      // rows 2p - dy and 2p + 1 - dy; an item of a mirror plan applies the same two cells to the slots of 2p + dy and 2p + 1 + dy
      // as well, low and high slot alternating so that no update reads the result of the one before it.  Groups of G items
      // in the plan's order, the next group's reads in flight while this one's min3 issue.
      T2 rd[2 * G][2];
      auto issue = [&]<int I>(std::integral_constant<int, I>) {
        constexpr int J = C::plan.item[I].j, p = J / N, k = J % N;
        constexpr int offl = (p * W + DY - C::dx(k)) * (int)sizeof(T2), offr = (p * W + DY + C::dx(k)) * (int)sizeof(T2);
        rd[I % (2 * G)][0] = lds_read2<offl>(lds_b, T());
        rd[I % (2 * G)][1] = lds_read2<offr>(lds_b, T());
      };
      auto update = [&]<int S, int I>(std::integral_constant<int, S>, std::integral_constant<int, I>, const T& l, const T& r) {
        static_assert(S >= 0 && S < NACC, "slot outside the ring");
        if constexpr (C::plan.first[S] != I) op3_acc<false>(acc[S], l, r);   // (tied)
        else if constexpr (S + ROWS < NACC) acc[S] = op3<false>(old[S + ROWS], l, r);
        else acc[S] = op2<false>(l, r);
      };
      auto apply = [&]<int I>(std::integral_constant<int, I> i) {
        constexpr int s = C::slot(C::plan.item[I].j), m = C::slot(C::mirror(C::plan.item[I].j));
        update(std::integral_constant<int, s>{}, i, rd[I % (2 * G)][0].x, rd[I % (2 * G)][1].x);
        if constexpr (C::plan.item[I].both) update(std::integral_constant<int, m>{}, i, rd[I % (2 * G)][0].x, rd[I % (2 * G)][1].x);
        update(std::integral_constant<int, s + 1>{}, i, rd[I % (2 * G)][0].y, rd[I % (2 * G)][1].y);
        if constexpr (C::plan.item[I].both) update(std::integral_constant<int, m + 1>{}, i, rd[I % (2 * G)][0].y, rd[I % (2 * G)][1].y);
      };
      auto issue_group = [&]<int Gi>(std::integral_constant<int, Gi>) {
        [&]<int... I>(std::integer_sequence<int, I...>) {
          (issue(std::integral_constant<int, Gi * G + I>{}), ...);
        }(std::make_integer_sequence<int, C::gsize(Gi)>{});
      };
      auto apply_group = [&]<int Gi>(std::integral_constant<int, Gi>) {
        [&]<int... I>(std::integer_sequence<int, I...>) {
          (apply(std::integral_constant<int, Gi * G + I>{}), ...);
        }(std::make_integer_sequence<int, C::gsize(Gi)>{});
      };
      issue_group(std::integral_constant<int, 0>{});
      [&]<int... Gi>(std::integer_sequence<int, Gi...>) {
        (([&] {
           if constexpr (Gi + 1 < C::NG) {
             issue_group(std::integral_constant<int, Gi + 1>{});
             lds_wait<2 * C::gsize(Gi + 1)>();
           } else {
             lds_wait<0>();
           }
           apply_group(std::integral_constant<int, Gi>{});
         }()),
         ...);
      }(std::make_integer_sequence<int, C::NG>{});
    }
    if (store) {
      if constexpr (C::LATE) cross_loads();
#pragma unroll
      for (int j = 0; j < ROWS; ++j) {
        T m = op3<false>(ec[j + 1], el[j], er[j]);
        m = op3<false>(m, ec[j], ec[j + 2]);
        if constexpr (N > 0) m = op2<false>(m, acc[j]);
        outv[j] = m;
      }
    }
  }
  if (o0 - ROWS >= ys) store_rows(o0 - ROWS);              // the last batch's rows
}

template <typename T, int R>
int inc_erode_launch(const IncEroArgs<T>& a_in, hipStream_t stream) {
  using C = IncEroCfg<R>;
  constexpr auto kern = inc_erode_kernel<T, R>;
  int resident;
  bool first;
  if (int rc = smrf_resident<kern>(C::TW, 0, resident, first)) return rc;   // (its LDS is static)
  if (first && smrf_sw().ring_debug)
    fprintf(stderr, "smrf inc erode: R=%d pairs=%d reach=%d LDS=%zu, %d workgroups/CU resident\n", R, C::N, C::DY,
            C::LDS_CELLS * 2 * sizeof(T), resident);
  IncEroArgs<T> a = a_in;
  const int strips = (a.cols + C::TW - 1) / C::TW;
  a.seg = smrf_seg_len(a.rows, strips, resident, smrf_sw().ring_rounds, 2 * C::DY + C::DELTA, C::ROWS, std::max(32, 4 * C::DY),
                       smrf_sw().seg_rule, a.seg);
  a.plain_tiles = smrf_sw().xcd_remap ? 0 : 1;
  dim3 grid(strips, (a.rows + a.seg - 1) / a.seg);
  hipLaunchKernelGGL(kern, grid, dim3(C::TW), 0, stream, a);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // namespace smrf
