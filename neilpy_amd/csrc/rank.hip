// Rank filters of a raster by an arbitrary flat footprint: scipy.ndimage.rank_filter / median_filter /
// percentile_filter / minimum_filter / maximum_filter with footprint=, modes 'reflect' and 'nearest'.  Host side:
// neilpy_amd/rank.py; C ABI: include/smrf_rank.h; contract: DESIGN.md section 20.
//
// The plan is the erosion's of morphology.plan: the members' (drow, dcol) offsets.  One launch, one thread per cell, 64
// lanes along a raster row, 8 rows per workgroup.  The result of a cell is the element at position `rank` of its n
// samples sorted ascending.  Selection is comparison only, on order-preserving unsigned keys (float_key.h), so every path
// below gives the same bits:
//
// Sample source.  TILE: the tile plus the halo of the members' bounding box is staged once as keys in LDS, the border
// rule applied while staging, and behind it every member's offset in the tile (clamped to the tile whatever the plan
// holds); a member is then two LDS reads, its offset - the same address in every lane - and the key there, and no scalar
// arithmetic.  GLOBAL: every sample is read from global memory through border(), for any footprint and any raster.
//
// Selection.  BISECT: a radix select on the key from the first bit in which the cell's least and largest key differ.
// COUNT: the stable-sort position of SMRF_RANK_COUNT_BLOCK candidates at a time by one sweep over the members, until
// every lane of the wave has found the member at position `rank`.  Both are written once, in float_key.h, over a
// callable that returns member j's key; the CPU tests run the same text.
#include "float_key.h"
#include "raster_stencil.h"
#include "smrf_rank.h"

namespace {

constexpr int TX = 64, TY = 8, NT = TX * TY;
constexpr int MAX_EXTENT = 1 << 20;     // footprint rows / columns the offsets' arithmetic is checked for
constexpr int MAX_AXIS = 1 << 30;       // raster rows / columns: 2 n of the reflect stays an int
enum { HEAD_NTAPS = 0, HEAD_NRUNS, HEAD_R_LO, HEAD_C_LO, HEAD_BH, HEAD_BW };
enum { METHOD_COUNT = SMRF_RANK_PATH_COUNT, METHOD_BISECT = SMRF_RANK_PATH_BISECT };
constexpr int SOURCE_FLAGS = SMRF_RANK_IMPL_GLOBAL | SMRF_RANK_IMPL_TILE;

struct Tap {
  int drow, dcol;
};
static_assert(sizeof(Tap) == 8, "the host packs the plan as int32 records");

template <typename T>
struct RankArgs {
  const T* in;
  T* out;
  int rows, cols;
  const Tap* taps;
  int ntaps, rank;
  int r_lo, c_lo, bh, bw;  // least row / column offset of a member, rows and columns of the members' bounding box
  int nan_aware;
};

template <int MODE>
__device__ inline int border(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if constexpr (MODE == SMRF_RANK_NEAREST) return i < 0 ? 0 : n - 1;
  else return smrf_fold(i, n);
}

// a cell index plus an offset of the plan, wrapping instead of overflowing: border() takes any int
__device__ inline int shifted(int i, int d) { return (int)((unsigned)i + (unsigned)d); }

template <typename T, int MODE, bool TILE, int METHOD>
__global__ __launch_bounds__(NT) void rank_kernel(RankArgs<T> a) {
  using K = typename SmrfKey<T>::type;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  K* const tile = reinterpret_cast<K*>(smem_raw);
  const int rows = a.rows, cols = a.cols;
  const int lx = threadIdx.x, ly = threadIdx.y;
  const int r0 = blockIdx.y * TY, c0 = blockIdx.x * TX;
  const int r = r0 + ly, c = c0 + lx;
  const bool live = r < rows && c < cols;
  const int rc = min(r, rows - 1), cc = min(c, cols - 1);   // a lane off the raster computes a cell it never writes
  const T* __restrict__ in = a.in;
  const Tap* __restrict__ taps = a.taps;
  const bool nan_last = a.nan_aware != 0;
  const int n = a.ntaps, rank = a.rank;
  const int r_lo = a.r_lo, c_lo = a.c_lo, bh = a.bh, bw = a.bw;
  const int LW = TX + bw - 1;

  const int TH = TY + bh - 1;
  int* const off = reinterpret_cast<int*>(tile + (TILE ? TH * LW : 0));   // behind the keys: every member's offset in the tile
  if constexpr (TILE) {
    for (int tr = ly; tr < TH; tr += TY) {
      const T* row = in + (long long)border<MODE>(r0 + r_lo + tr, rows) * cols;
      for (int tc = lx; tc < LW; tc += TX) tile[tr * LW + tc] = smrf_key<T>(row[border<MODE>(c0 + c_lo + tc, cols)], nan_last);
    }
    for (int j = ly * TX + lx; j < n; j += NT) {
      const Tap t = taps[j];
      off[j] = min(max(t.drow - r_lo, 0), bh - 1) * LW + min(max(t.dcol - c_lo, 0), bw - 1);
    }
    __syncthreads();
  }
  const K* const mine = tile + ly * LW + lx;
  auto at = [&](int j) -> K {
    if constexpr (TILE) {
      return mine[off[j]];
    } else {
      const Tap t = taps[j];
      return smrf_key<T>(in[(long long)border<MODE>(shifted(rc, t.drow), rows) * cols + border<MODE>(shifted(cc, t.dcol), cols)],
                         nan_last);
    }
  };
  K res;
  if constexpr (METHOD == METHOD_BISECT) res = smrf_select_bisect<K>(n, rank, at);
  else res = smrf_select_count<K, SMRF_RANK_COUNT_BLOCK>(n, rank, at, [](bool found) { return __all(found) != 0; });
  if (live) a.out[(long long)rc * cols + cc] = smrf_unkey<T>(res);
}

// the part of morphology.plan's head this family reads, checked
struct Head {
  int ntaps, r_lo, c_lo, bh, bw;
  size_t lds_bytes(int elem) const { return (size_t)(TY + bh - 1) * (TX + bw - 1) * elem + (size_t)ntaps * sizeof(int); }
};

int read_head(const int* h, Head& H) {
  if (!h) return smrf_fail(SMRF_E_ARG, "null plan");
  H = Head{h[HEAD_NTAPS], h[HEAD_R_LO], h[HEAD_C_LO], h[HEAD_BH], h[HEAD_BW]};
  if (H.bh < 1 || H.bw < 1 || H.bh > MAX_EXTENT || H.bw > MAX_EXTENT || H.r_lo < -MAX_EXTENT || H.r_lo > MAX_EXTENT ||
      H.c_lo < -MAX_EXTENT || H.c_lo > MAX_EXTENT)
    return smrf_fail(SMRF_E_ARG, "footprint box of %d x %d at (%d, %d)", H.bh, H.bw, H.r_lo, H.c_lo);
  if (H.ntaps < 1 || H.ntaps > (long long)H.bh * H.bw)
    return smrf_fail(SMRF_E_ARG, "plan of %d taps in a box of %d x %d", H.ntaps, H.bh, H.bw);
  return SMRF_OK;
}

int count_max_taps(int elem) { return elem == 4 ? SMRF_RANK_COUNT_MAX_TAPS_F32 : SMRF_RANK_COUNT_MAX_TAPS_F64; }

// SMRF_RANK_PATH_* method | source, negative = refused
int pick_path(const Head& H, int elem, int impl) {
  if (elem != 4 && elem != 8) return smrf_fail(SMRF_E_ARG, "element size %d", elem);
  const int method = impl & ~SOURCE_FLAGS, source = impl & SOURCE_FLAGS;
  if (impl < 0 || method > SMRF_RANK_IMPL_BISECT || source == SOURCE_FLAGS) return smrf_fail(SMRF_E_ARG, "unknown impl %d", impl);
  const bool fits = H.lds_bytes(elem) <= SMRF_RANK_TILE_BYTES;
  if (source == SMRF_RANK_IMPL_TILE && !fits)
    return smrf_fail(SMRF_E_UNSUPPORTED, "the tile of a %d x %d footprint takes %zu bytes of LDS, %d allowed", H.bh, H.bw,
                     H.lds_bytes(elem), SMRF_RANK_TILE_BYTES);
  const bool count = method == SMRF_RANK_IMPL_AUTO ? H.ntaps <= count_max_taps(elem) : method == SMRF_RANK_IMPL_COUNT;
  const bool tile = source == SMRF_RANK_IMPL_GLOBAL ? false : fits;
  return (count ? SMRF_RANK_PATH_COUNT : SMRF_RANK_PATH_BISECT) | (tile ? SMRF_RANK_PATH_TILE : SMRF_RANK_PATH_GLOBAL);
}

template <typename T, int MODE, bool TILE>
hipError_t launch(const RankArgs<T>& a, bool count, size_t lds, dim3 grid, hipStream_t st) {
  if (count)
    hipLaunchKernelGGL((rank_kernel<T, MODE, TILE, METHOD_COUNT>), grid, dim3(TX, TY), lds, st, a);
  else
    hipLaunchKernelGGL((rank_kernel<T, MODE, TILE, METHOD_BISECT>), grid, dim3(TX, TY), lds, st, a);
  return hipGetLastError();
}

template <typename T, int MODE>
hipError_t launch_source(const RankArgs<T>& a, bool tile, bool count, size_t lds, dim3 grid, hipStream_t st) {
  return tile ? launch<T, MODE, true>(a, count, lds, grid, st) : launch<T, MODE, false>(a, count, 0, grid, st);
}

template <typename T>
int rank_filter(const T* d_in, T* d_out, int rows, int cols, const void* d_plan, const int* h_head, int rank, int mode,
                int nan_aware, int impl, void* stream) {
  if (int rc = smrf::check_size(rows, cols)) return rc;
  if (rows > MAX_AXIS || cols > MAX_AXIS) return smrf_fail(SMRF_E_UNSUPPORTED, "raster of %d x %d", rows, cols);
  if (mode != SMRF_RANK_REFLECT && mode != SMRF_RANK_NEAREST) return smrf_fail(SMRF_E_ARG, "unknown mode %d", mode);
  Head H;
  if (int rc = read_head(h_head, H)) return rc;
  const int path = pick_path(H, (int)sizeof(T), impl);
  if (path < 0) return path;
  if (rank < 0 || rank >= H.ntaps) return smrf_fail(SMRF_E_ARG, "rank %d of %d members", rank, H.ntaps);
  if (smrf::empty_raster(rows, cols)) return SMRF_OK;
  if (!d_in || !d_out || !d_plan) return smrf_fail(SMRF_E_ARG, "null pointer");
  unsigned gy = 0;
  if (int rc = smrf::grid_rows(rows, TY, gy)) return rc;
  RankArgs<T> a{d_in, d_out, rows, cols, static_cast<const Tap*>(d_plan), H.ntaps, rank, H.r_lo, H.c_lo, H.bh, H.bw,
                nan_aware ? 1 : 0};
  const dim3 grid((cols + TX - 1) / TX, gy);
  const bool tile = !(path & SMRF_RANK_PATH_GLOBAL), count = !(path & SMRF_RANK_PATH_BISECT);
  const size_t lds = H.lds_bytes((int)sizeof(T));
  const hipStream_t st = (hipStream_t)stream;
  SMRF_HIP_CHECK(mode == SMRF_RANK_REFLECT ? (launch_source<T, SMRF_RANK_REFLECT>(a, tile, count, lds, grid, st))
                                           : (launch_source<T, SMRF_RANK_NEAREST>(a, tile, count, lds, grid, st)));
  return SMRF_OK;
}

}  // namespace

extern "C" {

int smrf_rank_tile_bytes(void) { return SMRF_RANK_TILE_BYTES; }

int smrf_rank_count_max_taps(int elem_size) {
  if (elem_size != 4 && elem_size != 8) return smrf_fail(SMRF_E_ARG, "element size %d", elem_size);
  return count_max_taps(elem_size);
}

int smrf_rank_path(const int* h_head, int elem_size, int impl) {
  Head H;
  if (int rc = read_head(h_head, H)) return rc;
  return pick_path(H, elem_size, impl);
}

int smrf_rank_filter_f32(const float* d_in, float* d_out, int rows, int cols, const void* d_plan, const int* h_head, int rank,
                         int mode, int nan_aware, int impl, void* stream) {
  return rank_filter<float>(d_in, d_out, rows, cols, d_plan, h_head, rank, mode, nan_aware, impl, stream);
}

int smrf_rank_filter_f64(const double* d_in, double* d_out, int rows, int cols, const void* d_plan, const int* h_head, int rank,
                         int mode, int nan_aware, int impl, void* stream) {
  return rank_filter<double>(d_in, d_out, rows, cols, d_plan, h_head, rank, mode, nan_aware, impl, stream);
}

}  // extern "C"
