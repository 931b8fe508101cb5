// Shared host/device helpers of libsmrf_hip (gfx950 only; no other backend is supported).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>

#include "smrf_hip.h"

#define SMRF_HIDDEN __attribute__((visibility("hidden")))

SMRF_HIDDEN int smrf_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define SMRF_HIP_CHECK(expr)                                                                  \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return smrf_fail(SMRF_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                       __FILE__, __LINE__);                                                   \
  } while (0)

#define SMRF_LAUNCH_CHECK() SMRF_HIP_CHECK(hipGetLastError())

// scipy.ndimage mode='reflect' (d c b a | a b c d | d c b a): period 2n fold, any i, n >= 1
__host__ __device__ inline int smrf_fold(int i, int n) {
  const int p2 = 2 * n;
  int p = i % p2;
  if (p < 0) p += p2;
  return p < n ? p : p2 - 1 - p;
}

// XCD-aware tile placement of the strip kernels (ring, fused opening, incremental erosion): which tile (bx, by) = (strip,
// row segment) this workgroup takes.  Workgroups are dealt round-robin over the 8 XCDs in dispatch order (x fastest), each
// XCD with its own L2.  The tile is remapped so that an XCD owns a contiguous range of strips (all their segments):
// neighbouring strips share their halo columns, which then hit the same L2.  Placement only, any mapping is correct
// (MI355X_MICROARCH: workgroup dispatch, XCD placement).  plain: workgroup (x, y) takes tile (x, y).  general_allowed: a
// callable, asked only where the second branch is reached (a kernel argument it reads is loaded there and nowhere else).
template <typename F>
__device__ __forceinline__ void smrf_xcd_tile(const bool plain, F&& general_allowed, int& bx, int& by) {
  bx = blockIdx.x;
  by = blockIdx.y;
  if (plain) {
  } else if ((gridDim.x & 7) == 0) {
    const int id = blockIdx.y * gridDim.x + blockIdx.x, per = gridDim.x >> 3;
    const int xcd = id & 7, slot = id >> 3;
    bx = xcd * per + slot % per;
    by = slot / per;
  } else if (gridDim.x > 8 && general_allowed()) {
    // any other strip count (round 5): an XCD owns a contiguous range of the tiles taken strip by strip (a strip's segments
    // together), i.e. strips / 8 neighbouring strips and parts of the two at its ends.  Without it the halo columns of a
    // raster of arbitrary width came from HBM again: 8193 columns fetched 5.6-7.3 B per cell and erosion pass against
    // 4.7-5.3 at 8192 (profiles/r05_segment_balance.md section 5).  XCD x gets ceil((total - x) / 8) of the workgroups.
    const int total = gridDim.x * gridDim.y, id = blockIdx.y * gridDim.x + blockIdx.x;
    const int xcd = id & 7, slot = id >> 3, q = total >> 3, rem = total & 7;
    const int t = xcd * q + (xcd < rem ? xcd : rem) + slot;
    bx = t / (int)gridDim.y;
    by = t % (int)gridDim.y;
  }
}

// The SMRF_* environment switches (developer A/B runs; the parity tests force every launch variant through them), read
// once by core.hip - smrf_switches_reload() of the C ABI reads them again.  -1 / 0 = "by the library's own rule".
struct SmrfSwitches {
  int fused;          // SMRF_FUSED: 0 never, 1 by rule, 2 every radius that has a fused / chained kernel whatever the raster size
  int chain;          // SMRF_CHAIN: 0 = no chained / table-free launches
  int nan_ride;       // SMRF_NAN_RIDE: 0 = always a separate NaN count pass
  int nt;             // SMRF_NT: -1 by plane size, 0 / 1 forced
  int ring_seg;       // SMRF_RING_SEG: output rows per workgroup (0 = from the occupancy)
  int ring_dual;      // SMRF_RING_DUAL: -1 by segment length, 0 shifting ring, 1 in-place ring
  int ring_rounds, fused_rounds, chain_rounds;   // workgroups per resident slot
  int seg_rule;       // SMRF_SEG_RULE: how a launch is cut into row segments (smrf_pick_nseg): 0 = by the cost model (default);
                      // 2 = one full round, rounds x resident x 256 / strips rounded down, segments >= 4R; 1 = rounded to nearest
                      // (rounds 1-4's rule)
  int xcd_remap;      // SMRF_XCD_REMAP=0: no XCD-aware tile placement in the ring kernels (A/B runs)
  int ring_slope;     // SMRF_RING_SLOPE: permille of segment length per residency class (-1 = the library's rule, 0 = equal segments)
  int ring_debug;     // SMRF_RING_DEBUG: print each instance's geometry once
  int ero_inc;        // SMRF_ERO_INC: window R's erosion from window R-1's (morph_incero.h): 0 never, 1 where ero_inc_adopt.inc says
                      // it wins (default), 2 every eligible window
  int dil_cross;      // SMRF_DIL_CROSS: a rim-free window's erosion taken inside its dilation pass (morph_ring.h, cross on load): 0 never,
                      // 1 where dil_cross_adopt.inc says it wins (default), 2 every eligible window
};
SMRF_HIDDEN const SmrfSwitches& smrf_sw();

// workgroups of 256 threads of a grid-stride loop over n items: one per 256 items, at least 1 and at most cap
inline int smrf_blocks(long long n, int cap) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap)); }

// a byte count rounded up to the 256-byte granule every part of a workspace starts on
inline size_t smrf_up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// integer floor(sqrt(v)), v >= 0
__host__ __device__ constexpr int smrf_isqrt(int v) {
  int r = 0;
  while ((long long)(r + 1) * (r + 1) <= v) ++r;
  return r;
}

// largest float <= t.  The flag step compares the raster dtype's difference with the float64 threshold in float64
// (neilpy.py:1671 under NumPy 2).  For a float `diff`: diff > t implies diff > thr_lo (thr_lo <= t); and diff > thr_lo
// implies diff >= the next float above thr_lo, which lies above t by the choice of thr_lo.  So `diff > thr_lo` is the same
// predicate, in one fp32 instruction instead of a conversion and a float64 compare (NaN: false either way).
inline float smrf_float_below(double t) {
  float f = (float)t;
  if ((double)f > t) f = __builtin_nextafterf(f, -__builtin_inff());
  return f;
}

#include "seg_rule.h"   // smrf_seg_len, smrf_ring_plan: how a launch is cut into row segments (plain C++: tests/test_host_logic.py compiles it)
#include "pf_route.h"   // smrf_pf_route: which launch every progressive_filter window takes, with smrf_fused_radius, the chain patterns and
                        // the incremental erosion's radii (plain C++: tests/test_pf_route_host.py compiles it)

// Workgroups of `Kern` (`block` threads, `lds` bytes of dynamic LDS) one CU really holds (registers + LDS), asked once per
// kernel and device - the attribute that allows more than 48 KB of dynamic LDS is per device too - and at least 1.
// `first`: this call asked (the launchers print their SMRF_RING_DEBUG geometry line then).
template <auto Kern>
int smrf_resident(int block, size_t lds, int& resident, bool& first) {
  static int resident_of[64] = {0};
  int dev = 0;
  SMRF_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return smrf_fail(SMRF_E_UNSUPPORTED, "device index %d out of range", dev);
  resident = __atomic_load_n(&resident_of[dev], __ATOMIC_ACQUIRE);   // host threads may launch one kernel at once
  first = resident == 0;
  if (first) {
    const void* const kern = reinterpret_cast<const void*>(Kern);
    if (lds > 48 * 1024) SMRF_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int nb = 0;
    SMRF_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, block, lds));
    resident = std::max(1, nb);
    __atomic_store_n(&resident_of[dev], resident, __ATOMIC_RELEASE);
  }
  return SMRF_OK;
}

// arguments of one disk erosion / dilation pass over a row band (see smrf_hip.h)
template <typename T>
struct DiskArgs {
  const T* in;        // first row held = global row in_row0
  T* out;             // first row = global row out_row0
  const T* last;      // flag step only (NULL otherwise), first row = out_row0
  uint8_t* mask;      // flag step only
  uint8_t* when;      // flag step only, may be NULL
  double thr;
  float thr_lo;       // largest float <= thr: for fp32 rasters `diff > thr_lo` decides exactly as `(double)diff > thr`
  int widx;
  int img_rows, cols;
  long long ld;
  int in_row0, in_rows, out_row0, out_rows;
  int radius;
  int nan_aware;
  int seg;            // output rows per workgroup (ring kernels)
  int nt;             // output cells as non-temporal (streaming) stores: planes far larger than the caches
  int dense;          // flag step writes EVERY mask / when byte (0 included): the planes need no clearing first
  // segments of unequal length (ring kernels, round 5): seg_cls = number of classes (0: every segment is `seg` rows); class c
  // holds the segments seg_first[c] .. seg_first[c + 1] - 1, each seg_len[c] rows, the first at out_row0 + seg_row0[c].
  // Filled by ring_launch_np from smrf_ring_plan (seg_rule.h).
  int seg_cls;
  int seg_first[8], seg_row0[8], seg_len[8];
  int plain_tiles;    // 1: workgroup (x, y) takes tile (x, y) (SMRF_XCD_REMAP=0, A/B runs); 0: the XCD-aware placement of the kernel
};

// ring-kernel dispatchers, one per (dtype, radius % SMRF_RING_PARTS); defined in ring_part.hip.
// mode: erosion, dilation (+ flag step when mask != NULL), or the fused opening + flag of morph_fused.h (in = last)
// SMRF_RING_DILATE_CROSS: the dilation + flag step whose `in` is e_{R-1} and whose loads take the 5-point cross (fp32, the radii of
// smrf_dil_cross_has, whole rasters without NaN)
enum { SMRF_RING_ERODE = 0, SMRF_RING_DILATE = 1, SMRF_RING_FUSED_OPEN = 2, SMRF_RING_DILATE_CROSS = 3 };
// incremental erosion of progressive_filter's consecutive windows (morph_incero.h, defined in incero.hip); which radii have an
// instance and which the default routing adopts: pf_route.h
SMRF_HIDDEN int smrf_inc_erode_f32(const float* e_prev, const float* last, float* out, int rows, int cols, long long ld,
                                   int radius, int nt, hipStream_t s);
#define SMRF_RING_PARTS 8
#define SMRF_RING_DECL(P)                                                                     \
  SMRF_HIDDEN int smrf_ring_f32_p##P(const DiskArgs<float>&, int mode, hipStream_t);          \
  SMRF_HIDDEN int smrf_ring_f64_p##P(const DiskArgs<double>&, int mode, hipStream_t);
SMRF_RING_DECL(0) SMRF_RING_DECL(1) SMRF_RING_DECL(2) SMRF_RING_DECL(3)
SMRF_RING_DECL(4) SMRF_RING_DECL(5) SMRF_RING_DECL(6) SMRF_RING_DECL(7)
#undef SMRF_RING_DECL
