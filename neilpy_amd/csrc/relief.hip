// Relief colouring and raster statistics of neilpy (neilpy/neilpy.py:1848-2031): raster_stats (this package's own
// primitive: NaN-ignoring count, min, max, mean, sum of squares and exact median), normalize (np.interp over knots),
// colortable_shade / swiss_shading (hillshade x elevation -> a 256 x 256 colour table) and Brassel's atmospheric
// perspective.  The arithmetic contract is DESIGN.md section 16 (tests/relief_numpy.py).
//
// Moments: the reduction pattern of cloud_reduce.h - smrf_blocks(n, CLOUD_PARTS) workgroups of 256 threads, a
// grid-stride chain per thread in index order, a 64-lane __shfl_down tree (offsets 32 .. 1), lane 0 of the four waves
// into LDS, thread 0 folding them as (w0, w1), (w2, w3), and the host folding the partial rows in workgroup order.  The
// sums are float64 additions in exactly that order (no float atomics), so tests replay them bit for bit.
//
// Median: a radix select on an order-preserving integer key, SELECT_BITS per pass (select_plan.h).  A pass is one
// histogram kernel (digit counts in LDS with integer atomics, flushed to a global row with integer atomics) and one
// single-workgroup kernel that walks the row with select_plan.h's select_step(); the state stays on the device, and
// the median joins the partial rows in the one device-to-host copy of the call.
#include <cmath>

#include "cloud_reduce.h"
#include "raster_stencil.h"
#include "select_plan.h"

namespace smrf {

// ------------------------------------------------------------------------------------------
// moments
// ------------------------------------------------------------------------------------------
constexpr int MOM_STRIDE = 5;   // a partial row: min, max, NaN cells, sum, sum of squares
constexpr int MOM_UNROLL = 4;   // loads in flight per thread; the additions keep the index order

template <typename T>
__device__ inline double squared(T x) {
  if constexpr (std::is_floating_point_v<T>) return (double)(T)(x * x);   // X**2 in the raster's dtype, then widened
  else return (double)x * (double)x;
}

template <typename T>
__global__ __launch_bounds__(256) void moments_kernel(const T* __restrict__ X, long long n, double* __restrict__ part) {
  double lo = INFINITY, hi = -INFINITY, sum = 0.0, sq = 0.0;
  unsigned long long nan = 0;
  const long long G = (long long)gridDim.x * 256;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += MOM_UNROLL * G) {
    T x[MOM_UNROLL];
    bool in[MOM_UNROLL];
#pragma unroll
    for (int u = 0; u < MOM_UNROLL; ++u) {
      in[u] = i + u * G < n;
      x[u] = in[u] ? X[i + u * G] : T(0);
    }
#pragma unroll
    for (int u = 0; u < MOM_UNROLL; ++u) {
      if (!in[u]) continue;
      if (x[u] != x[u]) { ++nan; continue; }
      const double v = (double)x[u];
      lo = fmin(lo, v);
      hi = fmax(hi, v);
      sum = sum + v;
      sq = sq + squared<T>(x[u]);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_down(lo, o, 64));
    hi = fmax(hi, __shfl_down(hi, o, 64));
    sum = sum + __shfl_down(sum, o, 64);
    sq = sq + __shfl_down(sq, o, 64);
    nan += __shfl_down(nan, o, 64);
  }
  __shared__ double s[4][4];
  __shared__ unsigned long long snan[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s[0][w] = lo; s[1][w] = hi; s[2][w] = sum; s[3][w] = sq;
    snan[w] = nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + (long long)blockIdx.x * MOM_STRIDE;
    o[0] = fmin(fmin(s[0][0], s[0][1]), fmin(s[0][2], s[0][3]));
    o[1] = fmax(fmax(s[1][0], s[1][1]), fmax(s[1][2], s[1][3]));
    o[2] = (double)(snan[0] + snan[1] + snan[2] + snan[3]);   // < 2^53: exact
    o[3] = (s[2][0] + s[2][1]) + (s[2][2] + s[2][3]);
    o[4] = (s[3][0] + s[3][1]) + (s[3][2] + s[3][3]);
  }
}

// ------------------------------------------------------------------------------------------
// median: radix select
// ------------------------------------------------------------------------------------------
template <typename T>
struct KeyOf;
template <>
struct KeyOf<float> {
  using type = uint32_t;
  static constexpr int bits = 32;
};
template <>
struct KeyOf<double> {
  using type = uint64_t;
  static constexpr int bits = 64;
};

// a < b as floats  <=>  key(a) < key(b) as unsigned integers (-0 below +0; NaN never gets here)
template <typename T>
__device__ inline typename KeyOf<T>::type to_key(T x) {
  using Key = typename KeyOf<T>::type;
  constexpr Key top = (Key)1 << (KeyOf<T>::bits - 1);
  Key u;
  __builtin_memcpy(&u, &x, sizeof(u));
  return (u & top) ? (Key)~u : (Key)(u | top);
}
template <typename T>
__device__ inline T from_key(typename KeyOf<T>::type k) {
  using Key = typename KeyOf<T>::type;
  constexpr Key top = (Key)1 << (KeyOf<T>::bits - 1);
  const Key u = (k & top) ? (Key)(k ^ top) : (Key)~k;
  T x;
  __builtin_memcpy(&x, &u, sizeof(x));
  return x;
}

// one rank's share of a histogram pass: equal digits in a thread's consecutive cells are counted in a register and
// reach LDS as one atomic (the top digits of a terrain raster fall into a handful of buckets)
struct DigitRun {
  int digit = -1;
  unsigned count = 0;
  __device__ inline void add(unsigned* row, int d) {
    if (d == digit) { ++count; return; }
    flush(row);
    digit = d;
    count = 1;
  }
  __device__ inline void flush(unsigned* row) {
    if (count) atomicAdd(&row[digit], count);
    count = 0;
  }
};

constexpr int SEL_UNROLL = 4;

template <typename T>
__global__ __launch_bounds__(256) void select_hist_kernel(const T* __restrict__ X, long long n, int pass,
                                                          const SelectState* __restrict__ st,
                                                          unsigned long long* __restrict__ hist) {
  using Key = typename KeyOf<T>::type;
  constexpr int KB = KeyOf<T>::bits;
  __shared__ unsigned h[2 * SELECT_BUCKETS];
  for (int b = threadIdx.x; b < 2 * SELECT_BUCKETS; b += 256) h[b] = 0;
  __syncthreads();
  const int lo = select_lo(KB, pass), hi = select_hi(KB, pass);
  const Key mask = (Key)(((Key)1 << (hi - lo)) - 1);
  const bool first = pass == 0;   // nothing above the top digit (and no shift by the key's width)
  Key p0 = 0, p1 = 0;
  if (!first) {
    p0 = (Key)st->prefix[0] >> hi;
    p1 = (Key)st->prefix[1] >> hi;
  }
  const bool split = p0 != p1;
  DigitRun r0, r1;
  const long long G = (long long)gridDim.x * 256;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += SEL_UNROLL * G) {
    T x[SEL_UNROLL];
#pragma unroll
    for (int u = 0; u < SEL_UNROLL; ++u) x[u] = i + u * G < n ? X[i + u * G] : (T)NAN;
#pragma unroll
    for (int u = 0; u < SEL_UNROLL; ++u) {
      if (x[u] != x[u]) continue;
      const Key k = to_key<T>(x[u]);
      const Key up = first ? (Key)0 : (Key)(k >> hi);
      const int d = (int)((k >> lo) & mask);
      if (up == p0) r0.add(h, d);
      if (split && up == p1) r1.add(h + SELECT_BUCKETS, d);
    }
  }
  r0.flush(h);
  r1.flush(h + SELECT_BUCKETS);
  __syncthreads();
  for (int b = threadIdx.x; b < (split ? 2 : 1) * SELECT_BUCKETS; b += 256)
    if (h[b]) atomicAdd(&hist[b], (unsigned long long)h[b]);
}

// the walk of one pass; after the last one the two keys are whole and the median goes to *result
template <typename T>
__global__ __launch_bounds__(256) void select_walk_kernel(int pass, const unsigned long long* __restrict__ hist,
                                                          SelectState* __restrict__ st, double* __restrict__ result) {
  using Key = typename KeyOf<T>::type;
  constexpr int KB = KeyOf<T>::bits;
  __shared__ unsigned long long rows[2 * SELECT_BUCKETS];
  for (int b = threadIdx.x; b < 2 * SELECT_BUCKETS; b += 256) rows[b] = hist[b];
  __syncthreads();
  if (threadIdx.x != 0) return;
  SelectState s;
  if (pass == 0) select_begin(s, select_total(rows));
  else s = *st;
  select_step(rows, select_lo(KB, pass), s);
  *st = s;
  if (pass == select_passes(KB) - 1) {
    const T a = from_key<T>((Key)s.prefix[0]), b = from_key<T>((Key)s.prefix[1]);
    // np.nanmedian: the middle value, or the mean of the two middle ones in the raster's dtype
    const T m = (s.count & 1) ? a : (T)((a + b) / T(2));
    *result = s.count ? (double)m : (double)NAN;
  }
}

// workspace: [partial rows, CLOUD_PARTS x MOM_STRIDE doubles][the median, one granule][SelectState, one granule]
// [histograms, one [2][SELECT_BUCKETS] of 64-bit counts per pass]
constexpr size_t STATS_PART_BYTES = (size_t)CLOUD_PARTS * MOM_STRIDE * sizeof(double);   // a multiple of 256
constexpr size_t STATS_HIST_BYTES = (size_t)2 * SELECT_BUCKETS * sizeof(unsigned long long);
constexpr size_t stats_bytes(int key_bits) {
  return STATS_PART_BYTES + 256 + 256 + (key_bits ? (size_t)select_passes(key_bits) * STATS_HIST_BYTES : 0);
}

inline double* stats_host_rows() {
  static thread_local double rows[CLOUD_PARTS * MOM_STRIDE + 32];
  return rows;
}

template <typename T>
int raster_stats(const T* d_X, int64_t n, int what, double* h_out, void* d_workspace, size_t workspace_bytes,
                 void* stream) {
  if (n < 0) return smrf_fail(SMRF_E_ARG, "negative size");
  if (!h_out) return smrf_fail(SMRF_E_ARG, "null result row");
  if (what & ~(SMRF_STATS_MOMENTS | SMRF_STATS_MEDIAN) || !what) return smrf_fail(SMRF_E_ARG, "unknown statistics %d", what);
  constexpr bool can_select = std::is_floating_point_v<T>;
  if ((what & SMRF_STATS_MEDIAN) && !can_select) return smrf_fail(SMRF_E_UNSUPPORTED, "no median of a uint8 raster");
  for (int k = 0; k < SMRF_STATS_ROW; ++k) h_out[k] = NAN;
  h_out[SMRF_STATS_COUNT] = h_out[SMRF_STATS_NAN] = 0.0;
  if (n == 0) return SMRF_OK;
  if (int rc = check_raster_ptr(d_X)) return rc;
  size_t need = stats_bytes(0);
  if constexpr (can_select) need = stats_bytes((what & SMRF_STATS_MEDIAN) ? KeyOf<T>::bits : 0);
  if (!d_workspace || workspace_bytes < need)
    return smrf_fail(SMRF_E_WORKSPACE, "statistics workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  const int blocks = smrf_blocks(n, CLOUD_PARTS);
  char* ws = (char*)d_workspace;
  double* part = (double*)ws;
  double* d_median = (double*)(ws + STATS_PART_BYTES);
  if (what & SMRF_STATS_MOMENTS) {
    hipLaunchKernelGGL((moments_kernel<T>), dim3(blocks), dim3(256), 0, st, d_X, (long long)n, part);
    SMRF_LAUNCH_CHECK();
  }
  if constexpr (can_select) {
    if (what & SMRF_STATS_MEDIAN) {
      constexpr int KB = KeyOf<T>::bits;
      SelectState* state = (SelectState*)(ws + STATS_PART_BYTES + 256);
      unsigned long long* hist = (unsigned long long*)(ws + STATS_PART_BYTES + 512);
      SMRF_HIP_CHECK(hipMemsetAsync(hist, 0, select_passes(KB) * STATS_HIST_BYTES, st));
      for (int p = 0; p < select_passes(KB); ++p) {
        unsigned long long* hp = hist + (size_t)p * 2 * SELECT_BUCKETS;
        hipLaunchKernelGGL((select_hist_kernel<T>), dim3(blocks), dim3(256), 0, st, d_X, (long long)n, p, state, hp);
        SMRF_LAUNCH_CHECK();
        hipLaunchKernelGGL((select_walk_kernel<T>), dim3(1), dim3(256), 0, st, p, hp, state, d_median);
        SMRF_LAUNCH_CHECK();
      }
    }
  }
  // one copy: the partial rows the moments wrote and the median behind them
  double* host = stats_host_rows();
  const bool mom = what & SMRF_STATS_MOMENTS;
  const size_t first = mom ? 0 : STATS_PART_BYTES;
  const size_t last = (what & SMRF_STATS_MEDIAN) ? STATS_PART_BYTES + sizeof(double) : (size_t)blocks * MOM_STRIDE * sizeof(double);
  // between the rows written and the median lie rows nobody wrote: copied only when both are asked, never read
  SMRF_HIP_CHECK(hipMemcpyAsync((char*)host + first, ws + first, last - first, hipMemcpyDeviceToHost, st));
  SMRF_HIP_CHECK(hipStreamSynchronize(st));
  if (mom) {
    double lo = INFINITY, hi = -INFINITY, nan = 0.0, sum = 0.0, sq = 0.0;
    for (int b = 0; b < blocks; ++b) {
      const double* p = host + b * MOM_STRIDE;
      lo = std::min(lo, p[0]);
      hi = std::max(hi, p[1]);
      nan += p[2];
      sum = sum + p[3];
      sq = sq + p[4];
    }
    const double count = (double)n - nan;
    h_out[SMRF_STATS_COUNT] = count;
    h_out[SMRF_STATS_NAN] = nan;
    if (count > 0.0) {
      h_out[SMRF_STATS_MIN] = lo;
      h_out[SMRF_STATS_MAX] = hi;
      h_out[SMRF_STATS_MEAN] = sum / count;
      h_out[SMRF_STATS_SUM_SQ] = sq;
    }
  }
  if (what & SMRF_STATS_MEDIAN) h_out[SMRF_STATS_MEDIAN_AT] = host[CLOUD_PARTS * MOM_STRIDE];
  return SMRF_OK;
}

// ------------------------------------------------------------------------------------------
// np.interp of one value over n >= 2 knots (numpy's arr_interp, line for line): float64, no FMA
// ------------------------------------------------------------------------------------------
template <typename P>
__device__ inline double interp_cell(double x, P xp, P fp, int n) {
  if (x != x) return x;
  if (x > xp[n - 1]) return fp[n - 1];
  if (x < xp[0]) return fp[0];
  int j = 0;
  for (int k = 1; k < n; ++k) j = xp[k] <= x ? k : j;   // the last knot at or below x
  if (j == n - 1 || xp[j] == x) return fp[j];
  const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
  double r = slope * (x - xp[j]) + fp[j];
  if (r != r) {   // a NaN in one direction (an infinite knot): the other one
    r = slope * (x - xp[j + 1]) + fp[j + 1];
    if (r != r && fp[j] == fp[j + 1]) r = fp[j];
  }
  return r;
}

template <typename T>
__global__ __launch_bounds__(256) void normalize_kernel(const T* __restrict__ X, long long n,
                                                        const double* __restrict__ knots, int n_knots,
                                                        double* __restrict__ out) {
  const double* xp = knots;
  const double* fp = knots + n_knots;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    out[i] = interp_cell((double)X[i], xp, fp, n_knots);
}

constexpr int STREAM_BLOCKS = 1 << 16;   // grid-stride cap of the element-wise kernels

template <typename T>
int normalize(const T* d_X, int64_t n, const double* d_knots, int n_knots, double* d_out, void* stream) {
  if (n < 0) return smrf_fail(SMRF_E_ARG, "negative size");
  if (n_knots < 2) return smrf_fail(SMRF_E_ARG, "normalize needs at least 2 knots (%d)", n_knots);
  if (n == 0) return SMRF_OK;
  if (!d_X || !d_knots || !d_out) return smrf_fail(SMRF_E_ARG, "null pointer");
  hipLaunchKernelGGL((normalize_kernel<T>), dim3(smrf_blocks(n, STREAM_BLOCKS)), dim3(256), 0, (hipStream_t)stream,
                     d_X, (long long)n, d_knots, n_knots, d_out);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

// ------------------------------------------------------------------------------------------
// float -> uint8 as NumPy's astype gives it on x86: through a signed 32-bit truncation, of which the low byte is kept;
// NaN and everything outside int32 become 0x80000000, low byte 0
// ------------------------------------------------------------------------------------------
__device__ inline uint8_t wrap_u8(double v) {
  if (!(fabs(v) < 2147483648.0)) return 0;
  return (uint8_t)((unsigned)(int)v & 255u);
}

// ------------------------------------------------------------------------------------------
// colortable_shade: the streaming layout of surface.hip (a wave on 64 columns, a thread walking a strip of rows with a
// 3 x 3 register window, so the raster comes from HBM once), the shade of raster_stencil.h's hillshade_cell, the
// table index in T, one gather from the packed table (R | G << 8 | B << 16, 256 KB: it lives in L2) and three bytes out
// ------------------------------------------------------------------------------------------
constexpr int CX = 64, CY = 4, CR = 32;

#ifndef SMRF_RELIEF_RGB3_LUT
#define SMRF_RELIEF_RGB3_LUT 0   // 1 (A/B builds of tools/relief_bench.py): the table as 3 bytes per entry, three gathers
#endif

template <typename T>
struct ColorArgs {
  const T* Z;
  int rows, cols;
  T zmin, zmax;
  double spacing;
  double ang[3];
  const uint32_t* lut;
  uint8_t* rgb;
};

template <typename T>
__global__ __launch_bounds__(CX* CY) void colortable_kernel(ColorArgs<T> a) {
  const int c = blockIdx.x * CX + threadIdx.x;
  const int r0 = (blockIdx.y * CY + threadIdx.y) * CR;
  const int rows = a.rows, cols = a.cols;
  if (c >= cols || r0 >= rows) return;
  const int r1 = min(r0 + CR, rows);
  const int cl = c > 0 ? c - 1 : 0, cr = c + 1 < cols ? c + 1 : c;
  const bool ex = c == 0 || c == cols - 1;
  const T* __restrict__ Z = a.Z;
  const T range = a.zmax - a.zmin;
  const double ang[3] = {a.ang[0], a.ang[1], a.ang[2]};
  T up = Z[(long long)(r0 > 0 ? r0 - 1 : 0) * cols + c];
  const T* p = Z + (long long)r0 * cols;
  T lf = p[cl], X = p[c], rt = p[cr];
  long long idx = (long long)r0 * cols + c;
  for (int r = r0; r < r1; ++r, idx += cols) {
    const T* q = Z + (long long)(r + 1 < rows ? r + 1 : r) * cols;
    const T nl = q[cl], dn = q[c], nr = q[cr];
    double H;
    const int shade = hillshade_cell<T>(dn - up, rt - lf, r == 0 || r == rows - 1, ex, a.spacing, ang, 1, H) & 255;
    // zi = uint8(round(255 * (Z - min) / (max - min))) in T, half-even; NaN (a NaN or constant raster) -> 0
    const T v = rint((T(255) * (X - a.zmin)) / range);
    const int zi = wrap_u8((double)v);
    uint8_t* o = a.rgb + idx * 3;
#if SMRF_RELIEF_RGB3_LUT
    const uint8_t* e = (const uint8_t*)a.lut + 3 * (zi << 8 | shade);
    o[0] = e[0];
    o[1] = e[1];
    o[2] = e[2];
#else
    const uint32_t e = a.lut[zi << 8 | shade];
    o[0] = (uint8_t)e;
    o[1] = (uint8_t)(e >> 8);
    o[2] = (uint8_t)(e >> 16);
#endif
    up = X;
    lf = nl;
    X = dn;
    rt = nr;
  }
}

template <typename T>
int colortable(const T* d_Z, int rows, int cols, double zmin, double zmax, double spacing, const double* h_angle,
               const uint32_t* d_lut, uint8_t* d_rgb, void* stream) {
  if (int rc = check_size(rows, cols)) return rc;
  if (empty_raster(rows, cols)) return SMRF_OK;
  if (int rc = check_raster_ptr(d_Z)) return rc;
  if (rows < 2 || cols < 2)
    return smrf_fail(SMRF_E_ARG, "np.gradient needs at least 2 cells per axis (%d x %d)", rows, cols);
  if (!h_angle || !d_lut || !d_rgb) return smrf_fail(SMRF_E_ARG, "null pointer");
  unsigned gy = 0;
  if (int rc = grid_rows(rows, CY * CR, gy)) return rc;
  ColorArgs<T> a{d_Z, rows, cols, (T)zmin, (T)zmax, spacing, {h_angle[0], h_angle[1], h_angle[2]}, d_lut, d_rgb};
  hipLaunchKernelGGL((colortable_kernel<T>), dim3((cols + CX - 1) / CX, gy), dim3(CX, CY), 0, (hipStream_t)stream, a);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

// ------------------------------------------------------------------------------------------
// brassel_atmospheric_perspective: one element-wise kernel; TH = the shade's dtype, T = the elevation's
// ------------------------------------------------------------------------------------------
template <typename T>
struct BrasselArgs {
  const void* H;
  const T* Z;
  long long n;
  int options;
  double flat, zmid, logk, c2;
  T zmin, zmax;
  void* out;
};

template <typename TH, typename T>
__global__ __launch_bounds__(256) void brassel_kernel(BrasselArgs<T> a) {
  const bool was_int = a.options & SMRF_BRASSEL_WAS_INT, use_mid = a.options & SMRF_BRASSEL_ZMID;
  const bool reverse = a.options & SMRF_BRASSEL_REVERSE;
  const TH* __restrict__ Hs = (const TH*)a.H;
  const T mid = (a.zmax + a.zmin) / T(2), half = (a.zmax - a.zmin) / T(2);
  const double xp[3] = {(double)a.zmin, a.zmid, (double)a.zmax}, fp[3] = {-1.0, 0.0, 1.0};
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < a.n; i += (long long)gridDim.x * 256) {
    const T z = a.Z[i];
    // Zstar and the tonal term (C2 * (Zstar - 1)) / 2, in T without a midpoint and in float64 (np.interp) with one
    double zstar, tone;
    if (use_mid) {
      zstar = interp_cell((double)z, xp, fp, 3);
      if (reverse) zstar = -zstar;
      tone = (a.c2 * (zstar - 1.0)) / 2.0;
    } else {
      T zs = (z - mid) / half;
      if (reverse) zs = -zs;
      zstar = (double)zs;
      tone = (double)(((T)a.c2 * (zs - T(1))) / T(2));
    }
    const double ex = pow(2.718281828459045, zstar * a.logk);   // np.e ** (Zstar * np.log(k))
    double d;   // H - flat: float64 once H was divided by 255, else in H's dtype
    if (was_int) d = (double)Hs[i] / 255.0 - a.flat;
    else if constexpr (std::is_same_v<TH, float>) d = (double)(Hs[i] - (float)a.flat);
    else d = (double)Hs[i] - a.flat;
    double hn = (d * ex) + a.flat;
    if (hn < 0.0) hn = 0.0;
    if (hn > 1.0) hn = 1.0;
    if (a.c2 != 0.0) hn = hn + tone;
    if (was_int) static_cast<uint8_t*>(a.out)[i] = wrap_u8(rint(255.0 * hn));
    else static_cast<double*>(a.out)[i] = hn;
  }
}

template <typename T>
int brassel(const void* d_H, int h_type, const T* d_Z, int64_t n, int options, double flat, double zmin, double zmax,
            double zmid, double logk, double c2, void* d_out, void* stream) {
  if (n < 0) return smrf_fail(SMRF_E_ARG, "negative size");
  if (h_type < SMRF_SHADE_U8 || h_type > SMRF_SHADE_F64) return smrf_fail(SMRF_E_ARG, "unknown shade type %d", h_type);
  if (n == 0) return SMRF_OK;
  if (!d_H || !d_Z || !d_out) return smrf_fail(SMRF_E_ARG, "null pointer");
  BrasselArgs<T> a{d_H, d_Z, (long long)n, options, flat, zmid, logk, c2, (T)zmin, (T)zmax, d_out};
  const dim3 grid(smrf_blocks(n, STREAM_BLOCKS)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (h_type == SMRF_SHADE_U8) hipLaunchKernelGGL((brassel_kernel<uint8_t, T>), grid, block, 0, st, a);
  else if (h_type == SMRF_SHADE_F32) hipLaunchKernelGGL((brassel_kernel<float, T>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((brassel_kernel<double, T>), grid, block, 0, st, a);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // namespace smrf

extern "C" {

size_t smrf_raster_stats_workspace_bytes(int elem_size, int what) {
  const bool median = what & SMRF_STATS_MEDIAN;
  return smrf::stats_bytes(!median ? 0 : elem_size == 4 ? 32 : 64);
}

int smrf_raster_stats_f32(const float* d_X, int64_t n, int what, double* h_out, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
  return smrf::raster_stats<float>(d_X, n, what, h_out, d_workspace, workspace_bytes, stream);
}
int smrf_raster_stats_f64(const double* d_X, int64_t n, int what, double* h_out, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
  return smrf::raster_stats<double>(d_X, n, what, h_out, d_workspace, workspace_bytes, stream);
}
int smrf_raster_stats_u8(const uint8_t* d_X, int64_t n, int what, double* h_out, void* d_workspace,
                         size_t workspace_bytes, void* stream) {
  return smrf::raster_stats<uint8_t>(d_X, n, what, h_out, d_workspace, workspace_bytes, stream);
}

int smrf_normalize_f32(const float* d_X, int64_t n, const double* d_knots, int n_knots, double* d_out, void* stream) {
  return smrf::normalize<float>(d_X, n, d_knots, n_knots, d_out, stream);
}
int smrf_normalize_f64(const double* d_X, int64_t n, const double* d_knots, int n_knots, double* d_out, void* stream) {
  return smrf::normalize<double>(d_X, n, d_knots, n_knots, d_out, stream);
}

int smrf_colortable_f32(const float* d_Z, int rows, int cols, double zmin, double zmax, double spacing,
                        const double* h_angle, const uint32_t* d_lut, uint8_t* d_rgb, void* stream) {
  return smrf::colortable<float>(d_Z, rows, cols, zmin, zmax, spacing, h_angle, d_lut, d_rgb, stream);
}
int smrf_colortable_f64(const double* d_Z, int rows, int cols, double zmin, double zmax, double spacing,
                        const double* h_angle, const uint32_t* d_lut, uint8_t* d_rgb, void* stream) {
  return smrf::colortable<double>(d_Z, rows, cols, zmin, zmax, spacing, h_angle, d_lut, d_rgb, stream);
}

int smrf_brassel_f32(const void* d_H, int h_type, const float* d_Z, int64_t n, int options, double flat, double zmin,
                     double zmax, double zmid, double logk, double c2, void* d_out, void* stream) {
  return smrf::brassel<float>(d_H, h_type, d_Z, n, options, flat, zmin, zmax, zmid, logk, c2, d_out, stream);
}
int smrf_brassel_f64(const void* d_H, int h_type, const double* d_Z, int64_t n, int options, double flat, double zmin,
                     double zmax, double zmid, double logk, double c2, void* d_out, void* stream) {
  return smrf::brassel<double>(d_H, h_type, d_Z, n, options, flat, zmin, zmax, zmid, logk, c2, d_out, stream);
}

}  // extern "C"
