// Grey erosion / dilation of a raster by an arbitrary flat footprint (scipy.ndimage.grey_erosion / grey_dilation with
// footprint=, modes 'reflect' and 'nearest'), with the subtractions of the top-hats and the morphological gradient as
// store epilogues.  Host side: neilpy_amd/morphology.py; contract: DESIGN.md section 19.
//
// The host turns the footprint into a plan (morphology.plan): the members' (drow, dcol) offsets in ndimage's visiting
// order, for a dilation already mirrored about the centre, and per footprint row the maximal runs of consecutive members.
// One thread per cell, 64 lanes along a raster row, 8 rows per workgroup.  Every global index goes through border():
// the period-2n reflect or the clamp, valid for any offset, so no sample is read off the raster whatever the plan holds.
//
// Taps path (the reference path): res = the first visited sample, then `if (v < res) res = v` (`>` for a dilation) per
// further member - ndimage's loop, so also its NaN rule: the result is NaN iff the first visited sample is.  The offset
// table is indexed by the loop counter alone: scalar loads.
//
// Runs path: the tile plus the halo of the members' bounding box is staged in LDS with the border rule applied while
// staging.  For every level k up to the largest floor(log2(run length)) a plane H_k[x] = op(H_{k-1}[x],
// H_{k-1}[x + 2^(k-1)]) is built from the one below; the host gives every level an LDS slot, and a level no run uses is
// overwritten once the next one stands.  A run of length L at level k is op(H_k[x0], H_k[x0 + L - 2^k]): two LDS reads.
// op is the NaN-ignoring fmin / fmax; with nan_aware the first visited sample is read once more and a NaN there makes
// the result NaN - ndimage's rule again.  min and max are exact, so the grouping changes no value: both paths agree.
#include "raster_stencil.h"

namespace {

constexpr int TX = 64, TY = 8, NT = TX * TY;
constexpr int MAX_LEVELS = 16;          // slots of the plan's head
constexpr int MAX_EXTENT = 1 << 20;     // footprint rows / columns the offsets' arithmetic is checked for
constexpr int MAX_AXIS = 1 << 30;       // raster rows / columns: 2 n of the reflect stays an int
enum { OP_MIN = 0, OP_MAX = 1, OP_BOTH = 2 };
enum { HEAD_NTAPS = 0, HEAD_NRUNS, HEAD_R_LO, HEAD_C_LO, HEAD_BH, HEAD_BW, HEAD_MAXLEVEL, HEAD_NPLANES, HEAD_SLOT0 };

struct Tap {
  int drow, dcol;
};
struct Run {
  int trow, tcol, tcol2, slot;   // tile row and the two tile columns of the run's reads, LDS slot of its level
};
static_assert(sizeof(Tap) == 8 && sizeof(Run) == 16, "the host packs the plan as int32 records");

template <typename T>
struct FpArgs {
  const T* in;
  const T* sub;
  T* out;
  int rows, cols;
  const Tap* taps;
  int ntaps;
  const Run* runs;
  int nruns;
  int r_lo, c_lo;          // least row / column offset of a member
  int th, lw;              // rows and columns of an LDS plane: TY + bh - 1, TX + bw - 1
  int maxlevel;
  int nplanes;             // slots of one set of planes (OP_BOTH holds two sets, the max set behind the min set)
  unsigned long long slots;   // 4 bits per level: its slot
  int nan_aware, epilogue;
};

template <int MODE>
__device__ inline int border(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if constexpr (MODE == SMRF_FOOTPRINT_NEAREST) return i < 0 ? 0 : n - 1;
  else return smrf_fold(i, n);
}

__device__ inline float nmin(float a, float b) { return __builtin_fminf(a, b); }
__device__ inline double nmin(double a, double b) { return __builtin_fmin(a, b); }
__device__ inline float nmax(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ inline double nmax(double a, double b) { return __builtin_fmax(a, b); }

template <typename T, int OP>
__device__ inline void store(const FpArgs<T>& a, bool live, long long idx, T lo, T hi) {
  if (!live) return;
  T res = OP == OP_BOTH ? hi - lo : (OP == OP_MIN ? lo : hi);
  if (a.epilogue == SMRF_FOOTPRINT_SUB_MINUS) res = a.sub[idx] - res;
  else if (a.epilogue == SMRF_FOOTPRINT_MINUS_SUB) res = res - a.sub[idx];
  a.out[idx] = res;
}

template <typename T, int MODE, int OP>
__global__ __launch_bounds__(NT) void footprint_taps_kernel(FpArgs<T> a) {
  const int rows = a.rows, cols = a.cols;
  const int r = blockIdx.y * TY + threadIdx.y, c = blockIdx.x * TX + threadIdx.x;
  const bool live = r < rows && c < cols;
  const int rc = min(r, rows - 1), cc = min(c, cols - 1);   // a lane off the raster computes a cell it never writes
  const T* __restrict__ in = a.in;
  const Tap* __restrict__ taps = a.taps;
  auto sample = [&](const Tap t) -> T {
    return in[(long long)border<MODE>(rc + t.drow, rows) * cols + border<MODE>(cc + t.dcol, cols)];
  };
  T lo = sample(taps[0]), hi = lo;
  const int ntaps = a.ntaps;
#pragma unroll 4
  for (int i = 1; i < ntaps; ++i) {
    const T v = sample(taps[i]);
    if constexpr (OP != OP_MAX) lo = v < lo ? v : lo;
    if constexpr (OP != OP_MIN) hi = v > hi ? v : hi;
  }
  store<T, OP>(a, live, (long long)rc * cols + cc, lo, hi);
}

template <typename T, int MODE, int OP>
__global__ __launch_bounds__(NT) void footprint_runs_kernel(FpArgs<T> a) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* const planes = reinterpret_cast<T*>(smem_raw);
  const int rows = a.rows, cols = a.cols;
  const int lx = threadIdx.x, ly = threadIdx.y;
  const int r0 = blockIdx.y * TY, c0 = blockIdx.x * TX;
  const int TH = a.th, LW = a.lw, n = TH * LW;
  const int hi_set = OP == OP_BOTH ? a.nplanes * n : 0;     // where the max planes start
  const unsigned long long slots = a.slots;
  auto slot = [&](int k) -> int { return (int)((slots >> (4 * k)) & 15); };
  const T* __restrict__ in = a.in;

  {
    T* p0 = planes + slot(0) * n;
    for (int tr = ly; tr < TH; tr += TY) {
      const T* row = in + (long long)border<MODE>(r0 + a.r_lo + tr, rows) * cols;
      for (int tc = lx; tc < LW; tc += TX) {
        const T v = row[border<MODE>(c0 + a.c_lo + tc, cols)];
        p0[tr * LW + tc] = v;
        if constexpr (OP == OP_BOTH) p0[hi_set + tr * LW + tc] = v;
      }
    }
  }
  __syncthreads();
  for (int k = 1; k <= a.maxlevel; ++k) {
    const int half = 1 << (k - 1);
    const T* src = planes + slot(k - 1) * n;
    T* dst = planes + slot(k) * n;          // never the source, never a level a run still reads (the host's slots)
    for (int tr = ly; tr < TH; tr += TY)
      for (int tc = lx; tc < LW; tc += TX) {
        const int i = tr * LW + tc;
        const bool pair = tc + half < LW;   // past it the plane's cell stands for no run
        if constexpr (OP != OP_MAX) {
          T v = src[i];
          if (pair) v = nmin(v, src[i + half]);
          dst[i] = v;
        }
        if constexpr (OP != OP_MIN) {
          T v = src[hi_set + i];
          if (pair) v = nmax(v, src[hi_set + i + half]);
          dst[hi_set + i] = v;
        }
      }
    __syncthreads();
  }

  const Run* __restrict__ runs = a.runs;
  const int nruns = a.nruns;
  T lo = 0, hi = 0;
#pragma unroll 2
  for (int i = 0; i < nruns; ++i) {
    const Run q = runs[i];
    const T* p = planes + q.slot * n + (ly + q.trow) * LW + lx;
    if constexpr (OP != OP_MAX) {
      T v = p[q.tcol];
      if (q.tcol2 != q.tcol) v = nmin(v, p[q.tcol2]);
      lo = i ? nmin(lo, v) : v;
    }
    if constexpr (OP != OP_MIN) {
      T v = p[hi_set + q.tcol];
      if (q.tcol2 != q.tcol) v = nmax(v, p[hi_set + q.tcol2]);
      hi = i ? nmax(hi, v) : v;
    }
  }
  const int r = r0 + ly, c = c0 + lx;
  const bool live = r < rows && c < cols;
  const int rc = min(r, rows - 1), cc = min(c, cols - 1);
  if (a.nan_aware) {
    const Tap t = a.taps[0];
    const T first = in[(long long)border<MODE>(rc + t.drow, rows) * cols + border<MODE>(cc + t.dcol, cols)];
    if (first != first) lo = hi = first;
  }
  store<T, OP>(a, live, (long long)rc * cols + cc, lo, hi);
}

// the plan's head as the host sends it, checked; what the LDS planes of the runs path take
struct Head {
  int ntaps, nruns, r_lo, c_lo, bh, bw, maxlevel, nplanes;
  unsigned long long slots;
  size_t lds_bytes(int elem, int epilogue) const {
    return (size_t)(epilogue == SMRF_FOOTPRINT_GRADIENT ? 2 : 1) * nplanes * (TY + bh - 1) * (TX + bw - 1) * elem;
  }
};

int read_head(const int* h, Head& H) {
  if (!h) return smrf_fail(SMRF_E_ARG, "null plan");
  H = Head{h[HEAD_NTAPS], h[HEAD_NRUNS], h[HEAD_R_LO], h[HEAD_C_LO], h[HEAD_BH], h[HEAD_BW], h[HEAD_MAXLEVEL],
           h[HEAD_NPLANES], 0};
  if (H.ntaps < 1 || H.nruns < 1 || H.nruns > H.ntaps) return smrf_fail(SMRF_E_ARG, "plan of %d taps in %d runs", H.ntaps, H.nruns);
  if (H.bh < 1 || H.bw < 1 || H.bh > MAX_EXTENT || H.bw > MAX_EXTENT || H.r_lo < -MAX_EXTENT || H.r_lo > MAX_EXTENT ||
      H.c_lo < -MAX_EXTENT || H.c_lo > MAX_EXTENT)
    return smrf_fail(SMRF_E_ARG, "footprint box of %d x %d at (%d, %d)", H.bh, H.bw, H.r_lo, H.c_lo);
  if (H.maxlevel < 0 || H.maxlevel >= MAX_LEVELS || (1LL << H.maxlevel) > H.bw || H.nplanes < 1 || H.nplanes > MAX_LEVELS)
    return smrf_fail(SMRF_E_ARG, "plan with top level %d in %d planes", H.maxlevel, H.nplanes);
  for (int k = 0; k <= H.maxlevel; ++k) {
    const int s = h[HEAD_SLOT0 + k];
    if (s < 0 || s >= H.nplanes || (k && s == h[HEAD_SLOT0 + k - 1])) return smrf_fail(SMRF_E_ARG, "level %d in slot %d", k, s);
    H.slots |= (unsigned long long)s << (4 * k);
  }
  return SMRF_OK;
}

// 0 = taps, 1 = runs, negative = refused
int pick_path(const Head& H, int elem, int epilogue, int impl) {
  if (elem != 4 && elem != 8) return smrf_fail(SMRF_E_ARG, "element size %d", elem);
  if (epilogue < SMRF_FOOTPRINT_STORE || epilogue > SMRF_FOOTPRINT_GRADIENT) return smrf_fail(SMRF_E_ARG, "unknown epilogue %d", epilogue);
  if (impl < SMRF_FOOTPRINT_IMPL_AUTO || impl > SMRF_FOOTPRINT_IMPL_TAPS) return smrf_fail(SMRF_E_ARG, "unknown impl %d", impl);
  const bool fits = H.lds_bytes(elem, epilogue) <= SMRF_FOOTPRINT_TILE_BYTES;
  if (impl == SMRF_FOOTPRINT_IMPL_RUNS && !fits)
    return smrf_fail(SMRF_E_UNSUPPORTED, "the planes of a %d x %d footprint take %zu bytes of LDS, %d allowed", H.bh, H.bw,
                     H.lds_bytes(elem, epilogue), SMRF_FOOTPRINT_TILE_BYTES);
  if (impl == SMRF_FOOTPRINT_IMPL_AUTO) return fits && H.ntaps >= SMRF_FOOTPRINT_RUNS_MIN_TAPS;
  return impl == SMRF_FOOTPRINT_IMPL_RUNS;
}

template <typename T, int MODE, int OP>
hipError_t launch(const FpArgs<T>& a, bool runs, size_t lds, dim3 grid, hipStream_t st) {
  if (runs)
    hipLaunchKernelGGL((footprint_runs_kernel<T, MODE, OP>), grid, dim3(TX, TY), lds, st, a);
  else
    hipLaunchKernelGGL((footprint_taps_kernel<T, MODE, OP>), grid, dim3(TX, TY), 0, st, a);
  return hipGetLastError();
}

template <typename T, int MODE>
hipError_t launch_op(int op, const FpArgs<T>& a, bool runs, size_t lds, dim3 grid, hipStream_t st) {
  switch (op) {
    case OP_MIN: return launch<T, MODE, OP_MIN>(a, runs, lds, grid, st);
    case OP_MAX: return launch<T, MODE, OP_MAX>(a, runs, lds, grid, st);
    default: return launch<T, MODE, OP_BOTH>(a, runs, lds, grid, st);
  }
}

template <typename T>
int footprint_filter(const T* d_in, const T* d_sub, T* d_out, int rows, int cols, const void* d_plan, const int* h_head,
                     int is_dilate, int mode, int nan_aware, int impl, int epilogue, void* stream) {
  if (int rc = smrf::check_size(rows, cols)) return rc;
  if (rows > MAX_AXIS || cols > MAX_AXIS) return smrf_fail(SMRF_E_UNSUPPORTED, "raster of %d x %d", rows, cols);
  if (mode != SMRF_FOOTPRINT_REFLECT && mode != SMRF_FOOTPRINT_NEAREST) return smrf_fail(SMRF_E_ARG, "unknown mode %d", mode);
  Head H;
  if (int rc = read_head(h_head, H)) return rc;
  const int path = pick_path(H, (int)sizeof(T), epilogue, impl);
  if (path < 0) return path;
  if (smrf::empty_raster(rows, cols)) return SMRF_OK;
  if (!d_in || !d_out || !d_plan) return smrf_fail(SMRF_E_ARG, "null pointer");
  const bool needs_sub = epilogue == SMRF_FOOTPRINT_SUB_MINUS || epilogue == SMRF_FOOTPRINT_MINUS_SUB;
  if (needs_sub && !d_sub) return smrf_fail(SMRF_E_ARG, "epilogue %d without d_sub", epilogue);
  unsigned gy = 0;
  if (int rc = smrf::grid_rows(rows, TY, gy)) return rc;
  const Tap* taps = static_cast<const Tap*>(d_plan);
  FpArgs<T> a{d_in, needs_sub ? d_sub : nullptr, d_out, rows, cols, taps, H.ntaps,
              reinterpret_cast<const Run*>(taps + H.ntaps), H.nruns, H.r_lo, H.c_lo, TY + H.bh - 1, TX + H.bw - 1,
              H.maxlevel, H.nplanes, H.slots, nan_aware ? 1 : 0, epilogue};
  const dim3 grid((cols + TX - 1) / TX, gy);
  const int op = epilogue == SMRF_FOOTPRINT_GRADIENT ? OP_BOTH : (is_dilate ? OP_MAX : OP_MIN);
  const size_t lds = H.lds_bytes((int)sizeof(T), epilogue);
  const hipStream_t st = (hipStream_t)stream;
  SMRF_HIP_CHECK(mode == SMRF_FOOTPRINT_REFLECT ? (launch_op<T, SMRF_FOOTPRINT_REFLECT>(op, a, path == 1, lds, grid, st))
                                                : (launch_op<T, SMRF_FOOTPRINT_NEAREST>(op, a, path == 1, lds, grid, st)));
  return SMRF_OK;
}

}  // namespace

extern "C" {

int smrf_footprint_tile_bytes(void) { return SMRF_FOOTPRINT_TILE_BYTES; }

int smrf_footprint_path(const int* h_head, int elem_size, int epilogue, int impl) {
  Head H;
  if (int rc = read_head(h_head, H)) return rc;
  return pick_path(H, elem_size, epilogue, impl);
}

int smrf_footprint_filter_f32(const float* d_in, const float* d_sub, float* d_out, int rows, int cols, const void* d_plan,
                              const int* h_head, int is_dilate, int mode, int nan_aware, int impl, int epilogue,
                              void* stream) {
  return footprint_filter<float>(d_in, d_sub, d_out, rows, cols, d_plan, h_head, is_dilate, mode, nan_aware, impl, epilogue,
                                 stream);
}

int smrf_footprint_filter_f64(const double* d_in, const double* d_sub, double* d_out, int rows, int cols,
                              const void* d_plan, const int* h_head, int is_dilate, int mode, int nan_aware, int impl,
                              int epilogue, void* stream) {
  return footprint_filter<double>(d_in, d_sub, d_out, rows, cols, d_plan, h_head, is_dilate, mode, nan_aware, impl,
                                  epilogue, stream);
}

}  // extern "C"
