// Weighted focal sums of neilpy's convolution family (neilpy/neilpy.py:2039-2124): std, topographic_position_index and
// reduce_peaks, each scipy.ndimage.convolve(X, w, mode='nearest') plus cell-wise arithmetic, from one templated kernel.
//
// The host compacts w (KH x KW) into its non-zero taps (drow, dcol, weight) in ndimage's order: s = KH-1 .. 0 outer,
// t = KW-1 .. 0 inner, drow = KH/2 - s, dcol = KW/2 - t.  One thread per cell, 64 lanes along a raster row, 8 rows per
// workgroup.  Per tap the thread adds fp64(X[clamp(r + drow), clamp(c + dcol)]) * weight to an fp64 accumulator: one
// multiply, one add (the build has -ffp-contract=off), and the sum is rounded to the raster's dtype at the end.  That is
// ndimage's arithmetic in ndimage's order, so the bits are ndimage's.  Every lane reads the same
// tap at the same time: the tap table is read-only and indexed by the loop counter alone, which makes the reads scalar
// loads.
//
// Tiled path: the workgroup's 64 x 8 cells plus a halo of (KH/2, KW/2) cells, edge-clamped, are staged in LDS once;
// taps inside the halo read LDS and any other tap reads global memory (only when the path is forced on a kernel whose
// halo exceeds the cap).  Direct path: every sample reads global memory with clamped indices.  The arithmetic is the
// same code in both, so both give the same bits.
#include <algorithm>
#include <cmath>

#include "raster_stencil.h"

namespace {

constexpr int TX = 64, TY = 8, NT = TX * TY;
constexpr int RED_THREADS = 256;      // the reduction kernels' workgroup
constexpr int MINMAX_BLOCKS = 1024;   // most workgroups of the min / max pass
constexpr int WS_HEAD = 4;            // doubles in front of the partials: TPI (sum conv(X*X), sum result, sd, -), min / max (lo, hi)

struct Tap {
  int drow, dcol;
  double w;
};
static_assert(sizeof(Tap) == 16, "the host packs taps as (int32, int32, float64)");

template <typename T>
struct FocalArgs {
  const T* X;
  const T* sub;       // not NULL: the raster is X - sub, formed in T (reduce_peaks' Z - M)
  int rows, cols;
  const Tap* taps;
  int ntaps;
  int hr, hc;         // tiled path: halo rows / columns held in LDS on each side
  double S;           // STD: np.sum(strel)
  void* out0;
  void* out1;
  double* part;       // TPI: two partial sums per workgroup
};

// fixed-order sum of one value per thread over the workgroup: a shuffle tree inside each wave of 64, then the waves in
// ascending order.  buf holds one double per wave.
template <int NTHREADS>
__device__ inline double block_sum(double* buf, int tid, double v) {
  for (int s = 32; s > 0; s >>= 1) v = v + __shfl_down(v, s, 64);
  if ((tid & 63) == 0) buf[tid >> 6] = v;
  __syncthreads();
  double t = buf[0];
  for (int w = 1; w < NTHREADS / 64; ++w) t = t + buf[w];
  __syncthreads();
  return t;
}

template <typename T, int MODE, bool LDS>
__global__ __launch_bounds__(NT) void focal_kernel(FocalArgs<T> a) {
  extern __shared__ __align__(8) unsigned char smem_raw[];
  __shared__ double red[NT / 64];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const int lx = threadIdx.x, ly = threadIdx.y;
  const int c0 = blockIdx.x * TX, r0 = blockIdx.y * TY;
  const int rows = a.rows, cols = a.cols;
  const int HR = LDS ? a.hr : 0, HC = LDS ? a.hc : 0;
  const int LW = TX + 2 * HC;
  const T* __restrict__ X = a.X;
  const T* __restrict__ sub = a.sub;
  auto cell = [&](long long i) -> T { return sub ? (T)(X[i] - sub[i]) : X[i]; };
  if constexpr (LDS) {
    const int n = LW * (TY + 2 * HR);
    for (int i = ly * TX + lx; i < n; i += NT) {
      const int tr = i / LW, tc = i - tr * LW;
      const int gr = min(max(r0 - HR + tr, 0), rows - 1), gc = min(max(c0 - HC + tc, 0), cols - 1);
      tile[i] = cell((long long)gr * cols + gc);
    }
    __syncthreads();
  }
  const int r = r0 + ly, c = c0 + lx;
  const bool live = r < rows && c < cols;
  const int rc = min(r, rows - 1), cc = min(c, cols - 1);   // a lane off the raster computes a cell it never writes
  const long long idx = (long long)rc * cols + cc;
  const Tap* __restrict__ taps = a.taps;
  const int ntaps = a.ntaps;
  const T* base = tile + (ly + HR) * LW + (lx + HC);

  double acc = 0.0;
  [[maybe_unused]] double acc2 = 0.0;
#pragma unroll 4
  for (int i = 0; i < ntaps; ++i) {
    const Tap t = taps[i];
    T v;
    bool lds = false;
    if constexpr (LDS) lds = t.drow >= -HR && t.drow <= HR && t.dcol >= -HC && t.dcol <= HC;   // wave-uniform
    if (lds) {
      v = base[t.drow * LW + t.dcol];
    } else {
      const int sr = min(max(rc + t.drow, 0), rows - 1), sc = min(max(cc + t.dcol, 0), cols - 1);
      v = cell((long long)sr * cols + sc);
    }
    acc = acc + (double)v * t.w;
    if constexpr (MODE != SMRF_FOCAL_SUM) {
      const T sq = v * v;              // X**2 in the raster's dtype
      acc2 = acc2 + (double)sq * t.w;
    }
  }
  const T sum = (T)acc;
  [[maybe_unused]] const T sum2 = (T)acc2;

  if constexpr (MODE == SMRF_FOCAL_SUM) {
    if (live) static_cast<T*>(a.out0)[idx] = sum;
  } else if constexpr (MODE == SMRF_FOCAL_SUM_SQ) {
    if (live) {
      static_cast<T*>(a.out0)[idx] = sum;
      static_cast<T*>(a.out1)[idx] = sum2;
    }
  } else if constexpr (MODE == SMRF_FOCAL_STD) {
    // std()'s tail, neilpy.py:2042-2045, in float64 as NumPy promotes it
    const double xs = (double)sum, xss = (double)sum2, S = a.S;
    const double xm = xs / S;
    double v = ((xss - (2.0 * xm) * xs) + S * (xm * xm)) / S;
    if (v < 0.0) v = 0.0;
    if (live) static_cast<double*>(a.out0)[idx] = sqrt(v);
  } else {
    const T x = LDS ? base[0] : cell(idx);
    const T res = x - sum;
    if (live) static_cast<T*>(a.out0)[idx] = res;
    const int tid = ly * TX + lx;
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    const double s2 = block_sum<NT>(red, tid, live ? (double)sum2 : 0.0);
    const double s1 = block_sum<NT>(red, tid, live ? (double)res : 0.0);
    if (tid == 0) {
      a.part[2 * (long long)wg] = s2;
      a.part[2 * (long long)wg + 1] = s1;
    }
  }
}

// TPI: the two sums over all workgroups in a fixed order, and sd = sqrt(mean(conv(X*X)) - mean(result)**2) in T
template <typename T>
__global__ __launch_bounds__(RED_THREADS) void tpi_reduce_kernel(const double* part, long long nwg, double cells,
                                                                  double* head) {
  __shared__ double red[RED_THREADS / 64];
  const int tid = threadIdx.x;
  double v0 = 0.0, v1 = 0.0;
  for (long long i = tid; i < nwg; i += RED_THREADS) {
    v0 = v0 + part[2 * i];
    v1 = v1 + part[2 * i + 1];
  }
  const double s[2] = {block_sum<RED_THREADS>(red, tid, v0), block_sum<RED_THREADS>(red, tid, v1)};
  if (tid == 0) {
    const T m2 = (T)(s[0] / cells), m = (T)(s[1] / cells);
    const T var = m2 - m * m;
    head[0] = s[0];
    head[1] = s[1];
    head[2] = (double)(T)sqrt(var);
  }
}

template <typename T>
__global__ void divide_kernel(T* io, long long n, const double* sd) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) io[i] = io[i] / (T)sd[0];
}

// NaN-ignoring minimum and maximum (np.nanmin / np.nanmax); NaN when every cell is NaN
__device__ inline void minmax_block(double* red, int tid, double& lo, double& hi) {
  red[tid] = lo;
  __syncthreads();
  for (int s = RED_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmin(red[tid], red[tid + s]);
    __syncthreads();
  }
  lo = red[0];
  __syncthreads();
  red[tid] = hi;
  __syncthreads();
  for (int s = RED_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  hi = red[0];
  __syncthreads();
}

__global__ __launch_bounds__(RED_THREADS) void minmax_kernel(const double* x, long long n, double* part) {
  __shared__ double red[RED_THREADS];
  const int tid = threadIdx.x;
  double lo = NAN, hi = NAN;
  for (long long i = (long long)blockIdx.x * RED_THREADS + tid; i < n; i += (long long)gridDim.x * RED_THREADS) {
    const double v = x[i];
    lo = fmin(lo, v);   // fmin / fmax return the other operand when one is NaN
    hi = fmax(hi, v);
  }
  minmax_block(red, tid, lo, hi);
  if (tid == 0) {
    part[2 * blockIdx.x] = lo;
    part[2 * blockIdx.x + 1] = hi;
  }
}

__global__ __launch_bounds__(RED_THREADS) void minmax_final_kernel(const double* part, int nblocks, double* head) {
  __shared__ double red[RED_THREADS];
  const int tid = threadIdx.x;
  double lo = NAN, hi = NAN;
  for (int i = tid; i < nblocks; i += RED_THREADS) {
    lo = fmin(lo, part[2 * i]);
    hi = fmax(hi, part[2 * i + 1]);
  }
  minmax_block(red, tid, lo, hi);
  if (tid == 0) {
    head[0] = lo;
    head[1] = hi;
  }
}

// reduce_peaks' tail, neilpy.py:2082-2085: V = (1 - normalize(STD))**blend_rate, MIX = (1 - V)*M + V*Z.  normalize is
// np.interp over the knots (lo, 0), (hi, 1): its own formula slope*(x - lo) + 0 between the knots, the knot values at them
template <typename T>
__global__ void mix_kernel(const T* Z, const T* M, const double* STD, const double* lohi, double blend, double* out,
                           long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double lo = lohi[0], hi = lohi[1];
  const double x = STD[i];
  double u;
  if (x != x) u = x;
  else if (x == hi) u = 1.0;
  else if (x == lo) u = 0.0;
  else u = (1.0 / (hi - lo)) * (x - lo) + 0.0;
  const double b = 1.0 - u;
  double V;
  if (blend == 2.0) V = b * b;            // NumPy's ** takes these exponents as square, identity, sqrt and reciprocal
  else if (blend == 1.0) V = b;
  else if (blend == 0.5) V = sqrt(b);
  else if (blend == -1.0) V = 1.0 / b;
  else V = pow(b, blend);
  out[i] = (1.0 - V) * (double)M[i] + V * (double)Z[i];
}

inline size_t tile_bytes(int hr, int hc, size_t elem) { return (size_t)(TX + 2 * hc) * (TY + 2 * hr) * elem; }

inline long long n_workgroups(int rows, int cols) {
  return (long long)((cols + TX - 1) / TX) * ((rows + TY - 1) / TY);
}

template <typename T, int MODE>
hipError_t launch_mode(const FocalArgs<T>& a, bool tiled, unsigned gy, hipStream_t st) {
  const dim3 grid((a.cols + TX - 1) / TX, gy), block(TX, TY);
  if (tiled)
    hipLaunchKernelGGL((focal_kernel<T, MODE, true>), grid, block, tile_bytes(a.hr, a.hc, sizeof(T)), st, a);
  else
    hipLaunchKernelGGL((focal_kernel<T, MODE, false>), grid, block, 0, st, a);
  return hipGetLastError();
}

template <typename T>
int focal(const T* d_X, const T* d_sub, int rows, int cols, int mode, const void* d_taps, int ntaps, int kh, int kw,
          double S, void* d_out0, void* d_out1, void* d_ws, size_t ws_bytes, int impl, void* stream) {
  if (int rc = smrf::check_size(rows, cols, ntaps)) return rc;
  if (kh < 1 || kw < 1) return smrf_fail(SMRF_E_ARG, "kernel of %d x %d", kh, kw);
  if (mode < SMRF_FOCAL_SUM || mode > SMRF_FOCAL_TPI) return smrf_fail(SMRF_E_ARG, "unknown mode %d", mode);
  if (impl < SMRF_FOCAL_IMPL_AUTO || impl > SMRF_FOCAL_IMPL_DIRECT) return smrf_fail(SMRF_E_ARG, "unknown impl %d", impl);
  if (smrf::empty_raster(rows, cols)) return SMRF_OK;
  if (!d_X || !d_out0 || (ntaps > 0 && !d_taps)) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (mode == SMRF_FOCAL_SUM_SQ && !d_out1) return smrf_fail(SMRF_E_ARG, "null output");
  unsigned gy = 0;
  if (int rc = smrf::grid_rows(rows, TY, gy)) return rc;
  const long long nwg = n_workgroups(rows, cols);
  if (mode == SMRF_FOCAL_TPI && (!d_ws || ws_bytes < smrf_focal_workspace_bytes(rows, cols)))
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes, %zu needed", ws_bytes,
                     smrf_focal_workspace_bytes(rows, cols));
  double* head = static_cast<double*>(d_ws);
  FocalArgs<T> a{d_X, d_sub, rows, cols, static_cast<const Tap*>(d_taps), ntaps, 0, 0, S, d_out0, d_out1,
                 head ? head + WS_HEAD : nullptr};
  const bool fits = smrf_focal_fits_tile(kh, kw, (int)sizeof(T)) != 0;
  const bool tiled = impl == SMRF_FOCAL_IMPL_TILED || (impl == SMRF_FOCAL_IMPL_AUTO && fits && rows >= TY && cols >= TX);
  if (tiled) {
    // a forced tiled launch of a kernel beyond the cap keeps the largest common halo that fits
    int h = std::max(kh / 2, kw / 2);
    while (tile_bytes(std::min(kh / 2, h), std::min(kw / 2, h), sizeof(T)) > SMRF_FOCAL_TILE_BYTES) --h;
    a.hr = std::min(kh / 2, h);
    a.hc = std::min(kw / 2, h);
  }
  const hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  switch (mode) {
    case SMRF_FOCAL_SUM: e = launch_mode<T, SMRF_FOCAL_SUM>(a, tiled, gy, st); break;
    case SMRF_FOCAL_SUM_SQ: e = launch_mode<T, SMRF_FOCAL_SUM_SQ>(a, tiled, gy, st); break;
    case SMRF_FOCAL_STD: e = launch_mode<T, SMRF_FOCAL_STD>(a, tiled, gy, st); break;
    default: e = launch_mode<T, SMRF_FOCAL_TPI>(a, tiled, gy, st); break;
  }
  SMRF_HIP_CHECK(e);
  if (mode == SMRF_FOCAL_TPI) {
    hipLaunchKernelGGL((tpi_reduce_kernel<T>), dim3(1), dim3(RED_THREADS), 0, st, head + WS_HEAD, nwg,
                       (double)((long long)rows * cols), head);
    SMRF_LAUNCH_CHECK();
  }
  return SMRF_OK;
}

template <typename T>
int focal_divide(T* d_io, int64_t n, const double* d_sd, void* stream) {
  if (n < 0) return smrf_fail(SMRF_E_ARG, "negative size");
  if (n == 0) return SMRF_OK;
  if (!d_io || !d_sd) return smrf_fail(SMRF_E_ARG, "null pointer");
  hipLaunchKernelGGL((divide_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_io,
                     (long long)n, d_sd);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

template <typename T>
int focal_mix(const T* d_Z, const T* d_M, const double* d_STD, const double* d_lohi, double blend_rate, double* d_out,
              int64_t n, void* stream) {
  if (n < 0) return smrf_fail(SMRF_E_ARG, "negative size");
  if (n == 0) return SMRF_OK;
  if (!d_Z || !d_M || !d_STD || !d_lohi || !d_out) return smrf_fail(SMRF_E_ARG, "null pointer");
  hipLaunchKernelGGL((mix_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_Z, d_M,
                     d_STD, d_lohi, blend_rate, d_out, (long long)n);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // namespace

extern "C" {

int smrf_focal_fits_tile(int kh, int kw, int elem_size) {
  if (kh < 1 || kw < 1 || (elem_size != 4 && elem_size != 8)) return 0;
  return tile_bytes(kh / 2, kw / 2, (size_t)elem_size) <= SMRF_FOCAL_TILE_BYTES ? 1 : 0;
}

size_t smrf_focal_workspace_bytes(int rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  return (size_t)(WS_HEAD + 2 * std::max<long long>(n_workgroups(rows, cols), MINMAX_BLOCKS)) * sizeof(double);
}

int smrf_focal_f32(const float* d_X, const float* d_sub, int rows, int cols, int mode, const void* d_taps, int ntaps,
                   int kh, int kw, double S, void* d_out0, void* d_out1, void* d_workspace, size_t workspace_bytes,
                   int impl, void* stream) {
  return focal<float>(d_X, d_sub, rows, cols, mode, d_taps, ntaps, kh, kw, S, d_out0, d_out1, d_workspace,
                      workspace_bytes, impl, stream);
}

int smrf_focal_f64(const double* d_X, const double* d_sub, int rows, int cols, int mode, const void* d_taps, int ntaps,
                   int kh, int kw, double S, void* d_out0, void* d_out1, void* d_workspace, size_t workspace_bytes,
                   int impl, void* stream) {
  return focal<double>(d_X, d_sub, rows, cols, mode, d_taps, ntaps, kh, kw, S, d_out0, d_out1, d_workspace,
                       workspace_bytes, impl, stream);
}

int smrf_focal_divide_f32(float* d_io, int64_t n, const double* d_sd, void* stream) {
  return focal_divide<float>(d_io, n, d_sd, stream);
}

int smrf_focal_divide_f64(double* d_io, int64_t n, const double* d_sd, void* stream) {
  return focal_divide<double>(d_io, n, d_sd, stream);
}

int smrf_focal_minmax_f64(const double* d_x, int64_t n, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (n < 0) return smrf_fail(SMRF_E_ARG, "negative size");
  if (n == 0) return SMRF_OK;
  if (!d_x || !d_workspace) return smrf_fail(SMRF_E_ARG, "null pointer");
  const int nblocks = (int)std::min<long long>(MINMAX_BLOCKS, (n + RED_THREADS * 8 - 1) / (RED_THREADS * 8));
  if (workspace_bytes < (size_t)(WS_HEAD + 2 * nblocks) * sizeof(double))
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes is too small", workspace_bytes);
  double* head = static_cast<double*>(d_workspace);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(minmax_kernel, dim3(nblocks), dim3(RED_THREADS), 0, st, d_x, (long long)n, head + WS_HEAD);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(RED_THREADS), 0, st, head + WS_HEAD, nblocks, head);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

int smrf_focal_mix_f32(const float* d_Z, const float* d_M, const double* d_STD, const double* d_lohi, double blend_rate,
                       double* d_out, int64_t n, void* stream) {
  return focal_mix<float>(d_Z, d_M, d_STD, d_lohi, blend_rate, d_out, n, stream);
}

int smrf_focal_mix_f64(const double* d_Z, const double* d_M, const double* d_STD, const double* d_lohi,
                       double blend_rate, double* d_out, int64_t n, void* stream) {
  return focal_mix<double>(d_Z, d_M, d_STD, d_lohi, blend_rate, d_out, n, stream);
}

}  // extern "C"
