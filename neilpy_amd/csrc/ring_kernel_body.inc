// The body of the single-pass ring kernels (morph_ring.h), included once per kernel: ring_kernel (CROSS = false) and
// ring_cross_kernel (CROSS = true).  Text, not a function: the kernel's arguments stay kernel arguments (a function taking the
// DiskArgs, however inlined, changed the generated code of every existing instance).  In scope: T, R, DIL, TW, NP, CROSS, `a`.
  static_assert(!CROSS || (DIL && sizeof(T) == 4), "cross on load: the fp32 dilation only");
  using C = RingCfg<T, R, TW, NP>;
  using T2 = typename Vec2<T>::type;
  constexpr int WP = C::WP, ROWS = C::ROWS, NLEV = C::NLEV;
  // fp64 with three row pairs per batch is NOT a validated configuration: a variant build that forced it gave wrong cells at
  // R = 57, 58, 62, 63, 64 (512 registers + 240-290 B of scratch per lane; tools/ab_equal.py, profiles/r05_f64_np.md) while
  // every shipped instance (<= 2 pairs) equals the oracle on every radius.  ring_tune.inc's fp64 caps keep it out.
  static_assert(sizeof(T) == 4 || NP <= 2, "fp64 ring instances are validated for at most two row pairs per batch");
  extern __shared__ __attribute__((aligned(16))) unsigned char smrf_lds[];
  T2* const L = reinterpret_cast<T2*>(smrf_lds);         // [NP][NLEV][WP] of {row A, row B}

  const int tid = threadIdx.x;
  int bx, by;   // the general branch: equal segments only (smrf_ring_plan's residency classes count on `by` growing with the dispatch id)
  smrf_xcd_tile(!SMRF_RING_XCD_REMAP || a.plain_tiles, [&] { return a.seg_cls == 0; }, bx, by);
#ifdef SMRF_RING_DBG_CLOCK   // timing experiment only: the shader clock this workgroup ran at, left in the output's first two cells
  const unsigned long long dbg_t0 = __builtin_amdgcn_s_memtime(), dbg_q0 = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef SMRF_RING_DBG_TS
  const unsigned long long dbg_ts0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int x0 = bx * TW;
  const int x = x0 + tid;
  int ys, ye;                                            // global output rows [ys, ye)
  if (a.seg_cls > 0) {                                   // segments of unequal length (smrf_ring_plan: residency classes)
    int cls = 0;
    for (int c = 1; c < a.seg_cls; ++c) cls += by >= a.seg_first[c] ? 1 : 0;
    ys = a.out_row0 + a.seg_row0[cls] + (by - a.seg_first[cls]) * a.seg_len[cls];
    ye = min(a.out_row0 + a.out_rows, ys + a.seg_len[cls]);
    if (ys >= ye) return;                                // (lengths are rounded up: a trailing segment may be empty)
  } else {
    ys = a.out_row0 + by * a.seg;
    ye = min(a.out_row0 + a.out_rows, ys + a.seg);
  }
  constexpr int NPOS = C::NPOS, W = C::W;
  // lane-owned staged cells: positions tid + i*TW of the TW+2R wide row; only the last can be absent
  const bool has_last = tid + (NPOS - 1) * TW < W;
  int cpos[NPOS];
#pragma unroll
  for (int i = 0; i < NPOS; ++i) cpos[i] = smrf_fold(x0 - R + tid + (tid + i * TW < W ? i * TW : 0), a.cols);
  const int last_in = a.in_rows - 1;
  // halo cells shared out over the waves (HaloCfg): this lane's halo cell and the column it is loaded from
  using H = HaloCfg<T, R, TW, NP>;
  constexpr bool BAL = H::OK;
  HaloLane hl;
  hl.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    const int h = (hl.wave % H::NH) * 64 + (tid & 63);
    hl.act = BAL && h < H::HW;
    hl.pos = hl.act ? TW + h : TW;
  }
  const int hcol = smrf_fold(x0 - R + hl.pos, a.cols);
  // CROSS: the side columns of the lane's staged cells (its own positions and its halo cell)
  int cposl[NPOS], cposr[NPOS], hcoll = 0, hcolr = 0;
  if constexpr (CROSS) {
#pragma unroll
    for (int i = 0; i < NPOS; ++i) { cposl[i] = smrf_fold(cpos[i] - 1, a.cols); cposr[i] = smrf_fold(cpos[i] + 1, a.cols); }
    hcoll = smrf_fold(hcol - 1, a.cols);
    hcolr = smrf_fold(hcol + 1, a.cols);
  }
  static_assert(TW == kRingTW, "the table is shared by the workgroup's four waves: workgroup barriers between the phases");
  auto phase_sync = [&]() { __syncthreads(); };
  const bool flag = a.mask != nullptr;
  const int xc = x < a.cols ? x : a.cols - 1;

  // ring: between pairs, slot s holds the partial result of output row (next input row) - R + s
  T acc[2 * R];
#pragma unroll
  for (int i = 0; i < 2 * R; ++i) acc[i] = ident<T>(DIL);

  T2 pf[NP][NPOS];                                       // next batch, this lane's staged cells
  T2 pfh[H::NJ];                                         // BAL: next batch, this lane's halo cell of its wave's jobs
  // CROSS: next batch, the cells of e_{R-1} the crosses of the lane's staged cells are made of (row 0 = the row above the
  // batch's first): per position ROWS + 2 centre cells and ROWS cells on either side; per halo job the same for its row pair
  constexpr int NPX = CROSS ? (BAL ? 1 : NPOS) : 1, NJX = CROSS ? H::NJ : 1;
  T pxc[NPX][ROWS + 2], pxl[NPX][ROWS], pxr[NPX][ROWS];
  T phc[NJX][4], phl[NJX][2], phr[NJX][2];
  T outv[ROWS], lastv[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) { outv[i] = T(0); lastv[i] = T(0); }

  // The row loop starts DELTA rows early so that the ROWS outputs a batch completes are either all
  // at or above ys or all below it (rows before ys - R only feed outputs that are never written).
  constexpr int DELTA = (ROWS - (2 * R) % ROWS) % ROWS;
  const int ystart = ys - R - DELTA;
  constexpr int UP = CROSS ? 1 : 0;                      // CROSS: rf tracks the row ABOVE the next batch's first (RowFold::at takes i >= 0)
  RowFold rf(ystart - UP, a.img_rows);                   // tracks the NEXT batch to prefetch
  // buffer addressing of the common cases (SMRF_RING_BUF): descriptors based at the first row of each plane this
  // workgroup touches there, byte offsets of the lane's columns; the host keeps a segment's span below 2 GiB (ring_launch_np)
  constexpr bool BUF = ring_buf_on<T, R, TW, NP>();
  constexpr bool RARE = C::INPLACE && SMRF_RING_RARE_OPAQUE(T, R);
  const int bi = max(0, ystart - UP - a.in_row0);                  // first band row of `in` a fast-path batch can start at
  const int bl = max(0, ys - 2 * R - DELTA - a.out_row0);          // ... of `last` (first batch: outputs of rows ystart - R ...)
  const int bo = ys - a.out_row0;                                  // ... of `out`, `mask`, `when`
  const unsigned rowb = (unsigned)a.ld * (unsigned)sizeof(T);     // bytes per row
  // (descriptors of planes a launch does not have are built from null pointers and never used)
  const smrf_rsrc_t rs_in = smrf_make_rsrc(a.in + (long long)bi * a.ld);
  const smrf_rsrc_t rs_out = smrf_make_rsrc(a.out + (long long)bo * a.ld);
  const smrf_rsrc_t rs_last = smrf_make_rsrc(flag ? a.last + (long long)bl * a.ld : nullptr);
  const smrf_rsrc_t rs_mask = smrf_make_rsrc(flag ? a.mask + (long long)bo * a.ld : nullptr);
  const smrf_rsrc_t rs_when = smrf_make_rsrc(flag && a.when != nullptr ? a.when + (long long)bo * a.ld : nullptr);
  unsigned cposb[NPOS], hcolb = 0, xb = 0, xcb = 0;
  if constexpr (BUF) {
#pragma unroll
    for (int i = 0; i < NPOS; ++i) cposb[i] = (unsigned)cpos[i] * (unsigned)sizeof(T);
    hcolb = (unsigned)hcol * (unsigned)sizeof(T);
    xb = (unsigned)x * (unsigned)sizeof(T);
    xcb = (unsigned)xc * (unsigned)sizeof(T);
  }
  // CROSS: a batch's cells of e_{R-1} from cell(k, column, its byte offset), k = 0 .. ROWS + 1 the rows from the one above the batch's first
  auto cross_fill = [&](auto&& cell) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
      const unsigned cb = (unsigned)cpos[i] * (unsigned)sizeof(T), lb = (unsigned)cposl[i] * (unsigned)sizeof(T), rb = (unsigned)cposr[i] * (unsigned)sizeof(T);
#pragma unroll
      for (int k = 0; k < ROWS + 2; ++k) pxc[i][k] = cell(k, cpos[i], cb);
#pragma unroll
      for (int k = 0; k < ROWS; ++k) { pxl[i][k] = cell(k + 1, cposl[i], lb); pxr[i][k] = cell(k + 1, cposr[i], rb); }
    }
    if constexpr (BAL) {
      const unsigned cb = (unsigned)hcol * (unsigned)sizeof(T), lb = (unsigned)hcoll * (unsigned)sizeof(T), rb = (unsigned)hcolr * (unsigned)sizeof(T);
#pragma unroll
      for (int j = 0; j < NJX; ++j) {
        const int q = hl.wave + H::WAVES * j;              // wave-job: row pair q / NH (inactive lanes load a valid cell)
        const int pq = q < H::NQ ? q / H::NH : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) phc[j][k] = cell(2 * pq + k, hcol, cb);
#pragma unroll
        for (int k = 0; k < 2; ++k) { phl[j][k] = cell(2 * pq + 1 + k, hcoll, lb); phr[j][k] = cell(2 * pq + 1 + k, hcolr, rb); }
      }
    }
  };
  // CROSS: the prefetched cells of e_{R-1} become the next batch's level 0 = e_R, the 5-point cross min3(min3(c, l, r), up, down) as
  // inc_erode_kernel takes it.  Between a batch's build phases and its consume phase (the loads were issued before the build), so
  // that the consume phase holds ROWS cells per position like the plain instance, not 3 ROWS + 2.
  auto cross_reduce = [&]() __attribute__((always_inline)) {
    if constexpr (CROSS) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
          pf[p][i].x = op3<false>(op3<false>(pxc[i][2 * p + 1], pxl[i][2 * p], pxr[i][2 * p]), pxc[i][2 * p], pxc[i][2 * p + 2]);
          pf[p][i].y = op3<false>(op3<false>(pxc[i][2 * p + 2], pxl[i][2 * p + 1], pxr[i][2 * p + 1]), pxc[i][2 * p + 1], pxc[i][2 * p + 3]);
        }
      }
      if constexpr (BAL) {
#pragma unroll
        for (int j = 0; j < NJX; ++j) {
          pfh[j].x = op3<false>(op3<false>(phc[j][1], phl[j][0], phr[j][0]), phc[j][0], phc[j][2]);
          pfh[j].y = op3<false>(op3<false>(phc[j][2], phl[j][1], phr[j][1]), phc[j][1], phc[j][3]);
        }
      }
    }
  };
  auto prefetch = [&]() {
    const int l0 = rf.p - a.in_row0;
    if constexpr (CROSS) {
      if (rf.p + ROWS + 2 <= rf.n && l0 >= 0 && l0 + ROWS + 1 <= last_in) {
        // common case: the ROWS + 2 rows from the one above the batch are consecutive rows of the raster, no reflection
        SMRF_MARK("prefetch");
        if constexpr (BUF) {
          const unsigned s0 = (unsigned)(l0 - bi) * rowb;
          cross_fill([&](int k, int, unsigned cb) { return smrf_buf_load(rs_in, cb, s0 + (unsigned)k * rowb, T()); });
        } else {
          const T* r0 = a.in + (long long)l0 * a.ld;
          cross_fill([&](int k, int c, unsigned) { return r0[(long long)k * a.ld + c]; });
        }
      } else {
        SMRF_MARK("rare");
        cross_fill([&](int k, int c, unsigned) {
          int l = rf.at(k) - a.in_row0;
          l = l < 0 ? 0 : (l > last_in ? last_in : l);     // only rows outside the segment's halo clamp
          return a.in[(long long)l * a.ld + smrf_rare<RARE>(c)];
        });
      }
      SMRF_MARK("prefetch");
      rf.advance(ROWS);
      return;
    }
    if (rf.p + ROWS <= rf.n && l0 >= 0 && l0 + ROWS - 1 <= last_in) {
      // common case: ROWS consecutive rows inside the band, no reflection: one address, row strides
      SMRF_MARK("prefetch");
      if constexpr (BUF) {
        const unsigned s0 = (unsigned)(l0 - bi) * rowb;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
          for (int i = 0; i < (BAL ? 1 : NPOS); ++i) {
            pf[p][i].x = smrf_buf_load(rs_in, cposb[i], s0 + (unsigned)(2 * p) * rowb, T());
            pf[p][i].y = smrf_buf_load(rs_in, cposb[i], s0 + (unsigned)(2 * p + 1) * rowb, T());
          }
        }
        if constexpr (BAL) {
#pragma unroll
          for (int j = 0; j < H::NJ; ++j) {
            const int q = hl.wave + H::WAVES * j;
            const int pq = q < H::NQ ? q / H::NH : 0;
            pfh[j].x = smrf_buf_load(rs_in, hcolb, s0 + (unsigned)(2 * pq) * rowb, T());
            pfh[j].y = smrf_buf_load(rs_in, hcolb, s0 + (unsigned)(2 * pq + 1) * rowb, T());
          }
        }
      } else {
      const T* r0 = a.in + (long long)l0 * a.ld;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int i = 0; i < (BAL ? 1 : NPOS); ++i) {
          pf[p][i].x = r0[(long long)(2 * p) * a.ld + cpos[i]];
          pf[p][i].y = r0[(long long)(2 * p + 1) * a.ld + cpos[i]];
        }
      }
      if constexpr (BAL) {
#pragma unroll
        for (int j = 0; j < H::NJ; ++j) {
          const int q = hl.wave + H::WAVES * j;            // wave-job: row pair q / NH (inactive lanes load a valid cell)
          const int pq = q < H::NQ ? q / H::NH : 0;
          pfh[j].x = r0[(long long)(2 * pq) * a.ld + hcol];
          pfh[j].y = r0[(long long)(2 * pq + 1) * a.ld + hcol];
        }
      }
      }
    } else {
      SMRF_MARK("rare");
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        int la = rf.at(2 * p) - a.in_row0;
        int lb = rf.at(2 * p + 1) - a.in_row0;
        la = la < 0 ? 0 : (la > last_in ? last_in : la);   // only rows outside the segment's halo clamp
        lb = lb < 0 ? 0 : (lb > last_in ? last_in : lb);
        const T* ra = a.in + (long long)la * a.ld;
        const T* rb = a.in + (long long)lb * a.ld;
#pragma unroll
        for (int i = 0; i < (BAL ? 1 : NPOS); ++i) { const int c = smrf_rare<RARE>(cpos[i]); pf[p][i].x = ra[c]; pf[p][i].y = rb[c]; }
      }
      if constexpr (BAL) {
#pragma unroll
        for (int j = 0; j < H::NJ; ++j) {
          const int q = hl.wave + H::WAVES * j;
          const int pq = q < H::NQ ? q / H::NH : 0;
          int la = rf.at(2 * pq) - a.in_row0;
          int lb = rf.at(2 * pq + 1) - a.in_row0;
          la = la < 0 ? 0 : (la > last_in ? last_in : la);
          lb = lb < 0 ? 0 : (lb > last_in ? last_in : lb);
          const int hc = smrf_rare<RARE>(hcol);
          pfh[j].x = a.in[(long long)la * a.ld + hc];
          pfh[j].y = a.in[(long long)lb * a.ld + hc];
        }
      }
    }
    SMRF_MARK("prefetch");
    rf.advance(ROWS);
  };
  // one completed output cell, general form: NaN rule, store, flag step (sparse or dense)
  auto emit = [&](int yo, long long off, T val, T lastval) {
    if (a.nan_aware) {
      // scipy: the first visited footprint element (offset (-R, 0)) decides NaN-ness
      const int ly = smrf_fold(yo - R, a.img_rows) - a.in_row0;
      const T first = a.in[(long long)ly * a.ld + smrf_rare<RARE>(x)];
      if (first != first) val = qnan<T>();
    }
    smrf_store_out(&a.out[off], val, a.nt);
    if (flag) smrf_flag_cell(a, off, lastval, val);
  };
  // the common case of a batch (all ROWS rows inside the segment, no NaN rule, sparse flags) as straight-line code per
  // (store kind, flag step): the uniform tests are made once per batch, not once per cell - scalar branches between
  // the VALU instructions of a kernel that runs at 2-3 waves per SIMD are not free (profiles/r02_issue_rate_ubench.md)
  auto emit_rows = [&]<bool NT, bool FLAG>(std::bool_constant<NT>, std::bool_constant<FLAG>, long long off0, int ro0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const long long off = off0 + (long long)i * a.ld;
      const unsigned so = (unsigned)(ro0 - bo + i) * rowb;   // BUF: row offset from the segment's first output row
      if constexpr (BUF) smrf_buf_store<NT>(rs_out, xb, so, outv[i]);
      else if constexpr (NT) __builtin_nontemporal_store(outv[i], &a.out[off]);
      else a.out[off] = outv[i];
      if constexpr (FLAG) {
        const T diff = lastv[i] - outv[i];                   // raster dtype
        bool hit;                                            // float64 comparison (NumPy 2); fp32: smrf_float_below
        if constexpr (sizeof(T) == 4) hit = diff > a.thr_lo;
        else hit = (double)diff > a.thr;
        if (hit) {
          if constexpr (BUF) {
            const unsigned sm = (unsigned)(ro0 - bo + i) * (unsigned)a.ld;
            smrf_buf_store_u8(rs_mask, (unsigned)x, sm, (uint8_t)1);
            if (a.when != nullptr) smrf_buf_store_u8(rs_when, (unsigned)x, sm, (uint8_t)a.widx);
          } else {
            a.mask[off] = 1;
            if (a.when != nullptr) a.when[off] = (uint8_t)a.widx;
          }
        }
      }
    }
  };
  // outputs of the batch whose first input row was yyb; written one iteration late so that no
  // store is younger than the prefetch loads the loop waits for
  auto epilogue = [&](int yyb) {
    const int yob = yyb - R;                               // first output row of the batch
    if (yob < ys || x >= a.cols) return;                   // (aligned: yob < ys means all rows are)
    const long long off0 = (long long)(yob - a.out_row0) * a.ld + x;
    if (yob + ROWS <= ye && !a.nan_aware && !a.dense) {
      const int ro0 = yob - a.out_row0;
      if (flag) {
        if (a.nt) { SMRF_MARK("epilogue:nt1:flag1"); emit_rows(std::true_type{}, std::true_type{}, off0, ro0); }
        else { SMRF_MARK("epilogue:nt0:flag1"); emit_rows(std::false_type{}, std::true_type{}, off0, ro0); }
      } else {
        if (a.nt) { SMRF_MARK("epilogue:nt1:flag0"); emit_rows(std::true_type{}, std::false_type{}, off0, ro0); }
        else { SMRF_MARK("epilogue:nt0:flag0"); emit_rows(std::false_type{}, std::false_type{}, off0, ro0); }
      }
      SMRF_MARK("epilogue");
    } else {
      SMRF_MARK("rare");
      const long long off0r = (long long)(yob - a.out_row0) * a.ld + smrf_rare<RARE>(x);
#pragma unroll
      for (int i = 0; i < ROWS; ++i)
        if (yob + i < ye) emit(yob + i, off0r + (long long)i * a.ld, outv[i], lastv[i]);
      SMRF_MARK("epilogue");
    }
  };
  auto load_last = [&](int yyb) {
    if (!flag) return;
    const int y0 = yyb - R - a.out_row0;
    if (y0 >= 0 && y0 + ROWS <= a.out_rows) {
      SMRF_MARK("last");
      if constexpr (BUF) {
        const unsigned s0 = (unsigned)(y0 - bl) * rowb;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) lastv[i] = smrf_buf_load(rs_last, xcb, s0 + (unsigned)i * rowb, T());
      } else {
      const T* l0 = a.last + (long long)y0 * a.ld + xc;
#pragma unroll
      for (int i = 0; i < ROWS; ++i) lastv[i] = l0[(long long)i * a.ld];
      }
    } else {
      SMRF_MARK("rare");
#pragma unroll
      for (int i = 0; i < ROWS; ++i) {
        int yo = y0 + i;
        yo = yo < 0 ? 0 : (yo >= a.out_rows ? a.out_rows - 1 : yo);
        lastv[i] = a.last[(long long)yo * a.ld + smrf_rare<RARE>(xc)];
      }
    }
    SMRF_MARK("last");
  };

  prefetch();
  cross_reduce();
  int par = 0;                                           // which level-0 copy this batch uses
  for (int yy0 = ystart; yy0 < ye + R; yy0 += ROWS, par ^= 1) {
    // (1) stage the prefetched rows into this batch's level-0 copy.  The other copy may still be
    //     read by a slower wave (its own cells of the previous batch); the higher levels are only
    //     written after the barrier below, which every wave reaches after its previous consume.
    SMRF_MARK("stage");
    T2 v[NP][NPOS];
    T2 vh[H::NJ];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
      for (int i = 0; i < (BAL ? 1 : NPOS); ++i) {
        v[p][i] = pf[p][i];
        if (i < NPOS - 1 || has_last)
          lds_write2((unsigned)(size_t)(__attribute__((address_space(3))) void*)(L + (p * NLEV + par) * WP + tid + i * TW), v[p][i]);
      }
    }
    if constexpr (BAL) {
#pragma unroll
      for (int j = 0; j < H::NJ; ++j) {
        vh[j] = pfh[j];
        const int q = hl.wave + H::WAVES * j;
        if (hl.act && q < H::NQ)
          lds_write2((unsigned)(size_t)(__attribute__((address_space(3))) void*)(L + ((q / H::NH) * NLEV + par) * WP + hl.pos), vh[j]);
      }
    }
    lds_wait<0>();                                         // the compiler does not count asm stores: complete them before the barrier
    phase_sync();
    SMRF_MARK("epilogue");
    if (yy0 > ystart) epilogue(yy0 - ROWS);
    SMRF_MARK("prefetch");
    if (yy0 + ROWS < ye + R) prefetch();
    SMRF_MARK("last");
    load_last(yy0);
    SMRF_MARK("build");

    if constexpr (BAL) {
      // ring_build_consume with the halo cells as wave-jobs: every wave builds its own 256 cells' worth of each row
      // pair plus its share of the halo, so the waves reach the phase barriers together
      __builtin_amdgcn_s_setprio(kRingBuildPrio);
      ring_base<T, R, DIL, TW, NP, 1, 0>(L, par, tid, true, v);
      SMRF_MARK("build:halo");
      ring_base_halo<T, R, DIL, TW, NP>(L, par, hl, vh);
      SMRF_MARK("build");
      phase_sync();
      if constexpr (C::J > C::JB) {
        ring_upper<T, R, DIL, TW, NP, 1, 0>(L, tid, true, v);
        ring_upper_halo<T, R, DIL, TW, NP>(L, hl, vh);
        phase_sync();
      }
      __builtin_amdgcn_s_setprio(0);
      cross_reduce();
      ring_consume<T, R, DIL, TW, NP>(L, par, tid, acc, outv);
    } else if constexpr (CROSS) {
      // ring_build_consume with the crosses of the next batch between the build phases and the consume phase
      __builtin_amdgcn_s_setprio(kRingBuildPrio);
      ring_base<T, R, DIL, TW, NP, NPOS, 0>(L, par, tid, has_last, v);
      phase_sync();
      if constexpr (C::J > C::JB) {
        ring_upper<T, R, DIL, TW, NP, NPOS, 0>(L, tid, has_last, v);
        phase_sync();
      }
      __builtin_amdgcn_s_setprio(0);
      cross_reduce();
      ring_consume<T, R, DIL, TW, NP>(L, par, tid, acc, outv);
    } else {
      ring_build_consume<T, R, DIL, TW, NP, NPOS, 0>(L, par, tid, has_last, v, acc, outv, phase_sync);
    }
  }
  SMRF_MARK("tail");
  {
    const int nb = (ye + R - ystart + ROWS - 1) / ROWS;
    epilogue(ystart + (nb - 1) * ROWS);
  }
#ifdef SMRF_RING_DBG_TS   // timing experiment only (tools/experiments/ring_tails.py): when and where this workgroup ran, left in
  if (tid == 0 && x0 + 6 <= a.cols) {   // the first cells of its segment's first row (the RESULT IS WRONG there)
    __threadfence();
    unsigned xcc, hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    T* const o = a.out + (long long)(ys - a.out_row0) * a.ld + x0;
    o[0] = (T)(float)(dbg_ts0 & 0x7fffff);
    o[1] = (T)(float)(__builtin_amdgcn_s_memrealtime() & 0x7fffff);
    o[2] = (T)(float)(xcc & 0xf);
    o[3] = (T)(float)(hwid & 0xffff);
    o[4] = (T)(float)(blockIdx.y * gridDim.x + blockIdx.x);
    o[5] = (T)(float)(ye - ys);
  }
#endif
#ifdef SMRF_RING_DBG_CLOCK
  if (bx == gridDim.x / 2 && by == gridDim.y / 2 && tid == 0) {
    __threadfence();
    a.out[0] = (T)(float)(__builtin_amdgcn_s_memtime() - dbg_t0);
    a.out[1] = (T)(float)(__builtin_amdgcn_s_memrealtime() - dbg_q0);
  }
#endif
