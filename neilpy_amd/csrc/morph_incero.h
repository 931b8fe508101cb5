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
// receives nothing costs one move - and the ring turns by 8 slots per batch inside those updates (IncEroCfg::Plan).  The 8
// rows a batch completes take the cross of e_{R-1} (five loads per cell, issued before the batch's LDS phase and before
// the prefetch, so that the waits for them leave the prefetch in flight) and are stored one batch late.  No scratch.
#pragma once
#include "morph_ring.h"

namespace smrf {

#include "ero_inc.inc"
#include "ero_inc_adopt.inc"

#define SMRF_INCERO_MIN_RADIUS 16   // the first window after the first two-pass window of a default call (15)
#define SMRF_INCERO_MAX_RADIUS 64

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
  static constexpr int G = 4;                            // cell pairs per lookup group (two reads each), two groups in flight
  static constexpr int NJ = NP * N;                      // jobs per batch: job j = row pair j / N, cell pair j % N
  static constexpr int NG = (NJ + G - 1) / G;
  static constexpr int gsize(int g) { const int n = NJ - g * G; return n < 0 ? 0 : n > G ? G : n; }
  static constexpr int dy(int k) { return kEroInc[R].p[k].dy; }
  static constexpr int dx(int k) { return kEroInc[R].p[k].dx; }
  // job j = (row pair j / N, cell pair j % N) updates the ring slots slot(j) (row A of its pair) and slot(j) + 1 (row B)
  static constexpr int slot(int j) { return 2 * (j / N) - dy(j % N) + DY; }
  // A batch runs its jobs by ascending slot (seq[i] = the i-th job), so that slot s receives its first update - the one
  // that reads what slot s + ROWS held - before slot s + ROWS receives its own and overwrites that: the two values never
  // live at once, and the ring turns in place.  first[s] = the position in seq of the first job that updates slot s, NJ if
  // the batch leaves the slot alone.
  struct Plan { short seq[NJ > 0 ? NJ : 1], first[NACC]; };
  static constexpr Plan make_plan() {
    Plan pl{};
    int n = 0;
    for (int s = 0; s < NACC; ++s) {
      pl.first[s] = NJ;
      for (int j = 0; j < NJ; ++j)
        if (slot(j) == s) pl.seq[n++] = (short)j;
    }
    for (int i = NJ - 1; i >= 0; --i) pl.first[slot(pl.seq[i])] = pl.first[slot(pl.seq[i]) + 1] = (short)i;
    return pl;
  }
  static constexpr Plan plan = make_plan();
  // every job is run once, every slot a batch updates has exactly one first update, and slot s has it before slot s + ROWS
  // (tests/test_gpu_incero_overlap.py states the same in Python from ero_inc.inc)
  static constexpr bool plan_ok() {
    int seen[NJ > 0 ? NJ : 1] = {};
    for (int i = 0; i < NJ; ++i) ++seen[plan.seq[i]];
    for (int j = 0; j < NJ; ++j)
      if (seen[j] != 1) return false;
    for (int s = 0; s < NACC; ++s) {
      int firsts = 0, touches = 0;
      for (int i = 0; i < NJ; ++i)
        for (int h = 0; h < 2; ++h)
          if (slot(plan.seq[i]) + h == s) { ++touches; firsts += plan.first[s] == i; }
      if (firsts != (touches > 0)) return false;
      if (s + ROWS < NACC && plan.first[s] < NJ && plan.first[s + ROWS] < NJ && plan.first[s] >= plan.first[s + ROWS]) return false;
    }
    return true;
  }
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
    // the cross of e_{R-1} for the rows this batch completes: loads issued now, used after the LDS phase
    const bool store = o0 >= ys;
    T ec[ROWS + 2], el[ROWS], er[ROWS];
    if (store) {
      RowFold rfe(o0 - 1, a.rows);
#pragma unroll
      for (int j = 0; j < ROWS + 2; ++j) {
        const T* row = a.e_prev + (long long)rfe.at(j) * a.ld;
        ec[j] = row[xc];
        if (j >= 1 && j <= ROWS) { el[j - 1] = row[xl]; er[j - 1] = row[xr]; }
      }
    }
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
           if constexpr (C::plan.first[S] == C::NJ) acc[S] = S + ROWS < NACC ? old[S + ROWS] : ident<T>(false);
         }()),
         ...);
      }(std::make_integer_sequence<int, NACC>{});
      // scatter: job (row pair p, cell pair k) reads {rowA, rowB} at columns x - dx and x + dx and updates the slots of output
      // rows 2p - dy and 2p + 1 - dy.  Groups of G jobs in the plan's order, the next group's reads in flight while this one's
      // min3 issue.
      T2 rd[2 * G][2];
      auto issue = [&]<int I>(std::integral_constant<int, I>) {
        constexpr int J = C::plan.seq[I], p = J / N, k = J % N;
        constexpr int offl = (p * W + DY - C::dx(k)) * (int)sizeof(T2), offr = (p * W + DY + C::dx(k)) * (int)sizeof(T2);
        rd[I % (2 * G)][0] = lds_read2<offl>(lds_b, T());
        rd[I % (2 * G)][1] = lds_read2<offr>(lds_b, T());
      };
      auto update = [&]<int S, int I>(std::integral_constant<int, S>, std::integral_constant<int, I>, const T& l, const T& r) {
        static_assert(S >= 0 && S < NACC, "slot outside the ring");
        if constexpr (C::plan.first[S] != I) op3_acc<false>(acc[S], l, r);
        else if constexpr (S + ROWS < NACC) acc[S] = op3<false>(old[S + ROWS], l, r);
        else acc[S] = op2<false>(l, r);
      };
      auto apply = [&]<int I>(std::integral_constant<int, I> i) {
        constexpr int s = C::slot(C::plan.seq[I]);
        update(std::integral_constant<int, s>{}, i, rd[I % (2 * G)][0].x, rd[I % (2 * G)][1].x);
        update(std::integral_constant<int, s + 1>{}, i, rd[I % (2 * G)][0].y, rd[I % (2 * G)][1].y);
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
