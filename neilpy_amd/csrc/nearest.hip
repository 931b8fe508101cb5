// Nearest-source infill (neilpy.py:1277, inpaint_nearest) as an exact Euclidean feature transform: every cell of a
// raster learns its nearest finite cell, ties to the lowest (row, column).  DESIGN.md section 11 is the contract.
//
// Separable and integer throughout.
//   pass 1, columns   nearest_mask_kernel packs isfinite() of 32 rows x 1 column into one word (the raster is read once,
//                     a wave covers 64 consecutive columns of a row); nearest_carry_kernel walks the words of a column
//                     down and up, one thread per column, and leaves for every 32-row strip the nearest source row above
//                     and below it.  g(r, c) = signed row offset of column c's nearest source to row r (upper on a tie)
//                     follows from two words and two carries, so the g plane itself is never stored.
//   pass 2, rows      nearest_envelope_kernel: one thread per (row, segment of NSEG columns) builds the lower envelope
//                     of the parabolas (c - c')^2 + g(r, c')^2 of its segment with the stack scan of Felzenszwalb and
//                     Huttenlocher / Meijster, every crossing an integer floor division and an exact tie decided by
//                     (source row, source column).  A wave takes 64 rows; the g values of a 64 x 64 tile are formed
//                     with a lane per column (coalesced words) and read back with a lane per row through LDS - the
//                     tile transpose.  nearest_lookup_kernel: one thread per cell; a hole binary-searches the envelope
//                     of its own segment, then of the segments left and right while their nearest column could still
//                     win or tie, and copies the winner's bits.
// Sources are never written, so in == out is safe: a hole only reads source cells.
#include <climits>

#include "raster_stencil.h"

namespace smrf {

constexpr int NSTRIP = 32;        // rows per mask word
constexpr int NTILE = 64;         // rows per wave and columns per LDS tile of the envelope scan
constexpr int NSEG = 1024;        // columns per envelope segment
constexpr int NONE = INT_MIN;     // g: no source in this column
constexpr int NMAX = 46341;       // 2 * (NMAX - 1)^2 < 2^32: squared distances fit uint32_t

struct NearestWs {
  uint32_t* mask;   // [strips][cols] bit i = row 32 s + i is a source
  int* up;          // [strips][cols] nearest source row above strip s, -1 if none
  int* dn;          // [strips][cols] nearest source row below strip s, -1 if none
  int* cnt;         // [rows][nseg]   envelope entries of the segment
  int2* sg;         // [rows][cols]   envelope entry: x = source column, y = g; segment j at column j * NSEG
  int* z;           // [rows][cols]   first column the entry wins from
};

inline size_t nearest_layout(int rows, int cols, char* base, NearestWs* w) {
  const size_t strips = (rows + NSTRIP - 1) / NSTRIP, nseg = (cols + NSEG - 1) / NSEG;
  const size_t plane = smrf_up256(strips * (size_t)cols * 4), cells = (size_t)rows * cols;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += smrf_up256(bytes);
    return p;
  };
  uint32_t* mask = (uint32_t*)take(plane);
  int* up = (int*)take(plane);
  int* dn = (int*)take(plane);
  int* cnt = (int*)take((size_t)rows * nseg * 4);
  int2* sg = (int2*)take(cells * 8);
  int* z = (int*)take(cells * 4);
  if (w) *w = NearestWs{mask, up, dn, cnt, sg, z};
  return off;
}

// ---------------------------------------------------------------------------------------------------------------
// pass 1
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void nearest_mask_kernel(const T* in, uint32_t* mask, int rows, int cols) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int s = blockIdx.y * 4 + threadIdx.y;
  const int r0 = s * NSTRIP;
  if (c >= cols || r0 >= rows) return;
  const int n = min(NSTRIP, rows - r0);
  const T* p = in + (long long)r0 * cols + c;
  uint32_t m = 0;
  for (int i = 0; i < n; ++i, p += cols) m |= (uint32_t)(isfinite(*p) ? 1u : 0u) << i;
  mask[(long long)s * cols + c] = m;
}

__global__ __launch_bounds__(64) void nearest_carry_kernel(const uint32_t* mask, int* up, int* dn, int strips, int cols) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= cols) return;
  int last = -1;
  for (int s = 0; s < strips; ++s) {
    const long long i = (long long)s * cols + c;
    up[i] = last;
    const uint32_t m = mask[i];
    if (m) last = s * NSTRIP + 31 - __clz(m);
  }
  last = -1;
  for (int s = strips - 1; s >= 0; --s) {
    const long long i = (long long)s * cols + c;
    dn[i] = last;
    const uint32_t m = mask[i];
    if (m) last = s * NSTRIP + __ffs(m) - 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// pass 2
// ---------------------------------------------------------------------------------------------------------------
// Parabolas a < b (columns) with row offsets ga, gb: the first integer column from which b beats a in the order
// (distance, source row, source column).  They meet at x = ((b^2 - a^2) + (gb^2 - ga^2)) / (2 (b - a)); left of x the
// parabola a is lower, right of it b; on an integer x they tie and the lower source row wins, a on equal rows (a < b).
__device__ inline long long first_win(int a, int ga, int b, int gb) {
  const long long num = (long long)(b - a) * (b + a) + (long long)(gb - ga) * ((long long)gb + ga);
  const long long den = 2LL * (b - a);
  // |num| < 2^34 and den < 2^17 are exact doubles, so the rounded quotient's floor is off by one at most
  long long q = (long long)floor((double)num / (double)den);
  long long rem = num - q * den;
  if (rem < 0) {
    --q;
    rem += den;
  } else if (rem >= den) {
    ++q;
    rem -= den;
  }
  const bool a_keeps_x = rem != 0 || ga <= gb;   // a non-integer x: a wins up to floor(x)
  return a_keeps_x ? q + 1 : q;
}

__global__ __launch_bounds__(NTILE) void nearest_envelope_kernel(NearestWs w, int rows, int cols, int strips, int nseg) {
  __shared__ int tile[NTILE][NTILE + 1];
  const int lane = threadIdx.x;
  const int seg = blockIdx.x;
  const int rb = blockIdx.y * NTILE;           // a multiple of 64: strips 2 * blockIdx.y and the next
  const int r = rb + lane;
  const int c0 = seg * NSEG, c1 = min(cols, c0 + NSEG);
  const int s0 = 2 * blockIdx.y, s1 = s0 + 1;
  const long long base = (long long)(r < rows ? r : 0) * cols + c0;
  int2* sg = w.sg + base;
  int* z = w.z + base;
  int n = 0, ts = 0, tg = 0, tz = 0;           // entries on the stack and the top one, kept in registers

  for (int cc = c0; cc < c1; cc += NTILE) {
    const int cw = min(NTILE, c1 - cc);
    // lane = column: g of 64 rows from two mask words and the carries above and below them
    if (lane < cw) {
      const int c = cc + lane;
      const long long i0 = (long long)s0 * cols + c;
      unsigned long long m = w.mask[i0];
      int below = w.dn[i0];
      if (s1 < strips) {
        m |= (unsigned long long)w.mask[i0 + cols] << 32;
        below = w.dn[i0 + cols];
      }
      int above = w.up[i0];
      for (int i = 0; i < NTILE; ++i) {       // down: distance to the nearest source at or above
        if ((m >> i) & 1) above = rb + i;
        tile[i][lane] = above >= 0 ? rb + i - above : -1;
      }
      for (int i = NTILE - 1; i >= 0; --i) {  // up: distance at or below; the upper source takes a tie
        if ((m >> i) & 1) below = rb + i;
        const int du = tile[i][lane];
        const int dd = below >= 0 ? below - (rb + i) : -1;
        int g = NONE;
        if (du >= 0 && (dd < 0 || du <= dd)) g = -du;
        else if (dd >= 0) g = dd;
        tile[i][lane] = g;
      }
    }
    __syncthreads();
    // lane = row: push the tile's columns onto the row's envelope
    if (r < rows) {
      for (int j = 0; j < cw; ++j) {
        const int g = tile[lane][j];
        if (g == NONE) continue;
        const int u = cc + j;
        long long wcol = 0;
        while (n > 0) {
          wcol = first_win(ts, tg, u, g);
          if (wcol > tz) break;
          --n;                                 // the top never wins: u beats it where it would start
          if (n > 0) {
            const int2 e = sg[n - 1];
            ts = e.x;
            tg = e.y;
            tz = z[n - 1];
          }
        }
        if (n == 0) wcol = 0;
        if (wcol >= cols) continue;            // u wins only beyond the raster
        ts = u;
        tg = g;
        tz = (int)wcol;
        sg[n] = make_int2(ts, tg);
        z[n] = tz;
        ++n;
      }
    }
    __syncthreads();
  }
  if (r < rows) w.cnt[(long long)r * nseg + seg] = n;
}

template <typename T>
struct LookupArgs {
  const T* in;
  T* out;
  long long* index;
  uint32_t* dist2;
  int rows, cols, nseg;
};

template <typename T>
__global__ __launch_bounds__(256) void nearest_lookup_kernel(LookupArgs<T> a, NearestWs w) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y;
  if (c >= a.cols) return;
  const long long idx = (long long)r * a.cols + c;
  const T v = a.in[idx];
  if (isfinite(v)) {
    if (a.out && a.out != a.in) a.out[idx] = v;
    if (a.index) a.index[idx] = idx;
    if (a.dist2) a.dist2[idx] = 0u;
    return;
  }
  unsigned long long best = ~0ULL;
  int brow = -1, bcol = -1;
  // the envelope of segment j at column c: the last entry whose first column is <= c
  auto probe = [&](int j) {
    const int n = w.cnt[(long long)r * a.nseg + j];
    if (n == 0) return;
    const long long base = (long long)r * a.cols + (long long)j * NSEG;
    const int* z = w.z + base;
    int lo = 0, hi = n - 1;                    // z[0] = 0 <= c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (z[mid] <= c) lo = mid;
      else hi = mid - 1;
    }
    const int2 e = w.sg[base + lo];
    const long long dc = c - e.x, dr = e.y;
    const unsigned long long d = (unsigned long long)(dc * dc + dr * dr);
    const int row = r + e.y;
    if (d < best || (d == best && (row < brow || (row == brow && e.x < bcol)))) {
      best = d;
      brow = row;
      bcol = e.x;
    }
  };
  const int j0 = c / NSEG;
  probe(j0);
  for (int j = j0 - 1; j >= 0; --j) {          // leftwards while the segment's nearest column can still win or tie
    const long long gap = c - ((long long)(j + 1) * NSEG - 1);
    if ((unsigned long long)(gap * gap) > best) break;
    probe(j);
  }
  for (int j = j0 + 1; j < a.nseg; ++j) {
    const long long gap = (long long)j * NSEG - c;
    if ((unsigned long long)(gap * gap) > best) break;
    probe(j);
  }
  if (brow < 0) {                              // no source in the raster: the hole stays
    if (a.out && a.out != a.in) a.out[idx] = v;
    if (a.index) a.index[idx] = -1;
    if (a.dist2) a.dist2[idx] = 0xFFFFFFFFu;
    return;
  }
  const long long src = (long long)brow * a.cols + bcol;
  if (a.out) a.out[idx] = a.in[src];
  if (a.index) a.index[idx] = src;
  if (a.dist2) a.dist2[idx] = (uint32_t)best;
}

__global__ __launch_bounds__(256) void nearest_planes_kernel(const long long* index, const uint32_t* dist2, long long n,
                                                             int cols, double* dist, long long* row, long long* col) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (dist) {
    const uint32_t d = dist2[i];
    dist[i] = d == 0xFFFFFFFFu ? __builtin_inf() : sqrt((double)d);
  }
  if (row) {
    const long long s = index[i];
    row[i] = s < 0 ? -1 : s / cols;
    col[i] = s < 0 ? -1 : s % cols;
  }
}

template <typename T>
int nearest(const T* d_in, T* d_out, int64_t* d_index, uint32_t* d_dist2, int rows, int cols, void* d_ws, size_t ws_bytes,
            void* stream) {
  if (int rc = check_size(rows, cols)) return rc;
  if (empty_raster(rows, cols)) return SMRF_OK;
  if (rows > NMAX || cols > NMAX)
    return smrf_fail(SMRF_E_ARG, "%d x %d: squared distances beyond %d cells per axis do not fit 32 bits", rows, cols, NMAX);
  if (int rc = check_raster_ptr(d_in)) return rc;
  if (!d_out && !d_index && !d_dist2) return smrf_fail(SMRF_E_ARG, "null output");
  if (!d_ws || ws_bytes < nearest_layout(rows, cols, nullptr, nullptr))
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes, %zu needed", ws_bytes,
                     nearest_layout(rows, cols, nullptr, nullptr));
  NearestWs w;
  nearest_layout(rows, cols, (char*)d_ws, &w);
  const hipStream_t st = (hipStream_t)stream;
  const int strips = (rows + NSTRIP - 1) / NSTRIP, nseg = (cols + NSEG - 1) / NSEG;
  hipLaunchKernelGGL((nearest_mask_kernel<T>), dim3((cols + 63) / 64, (strips + 3) / 4), dim3(64, 4), 0, st, d_in, w.mask,
                     rows, cols);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(nearest_carry_kernel, dim3((cols + 63) / 64), dim3(64), 0, st, w.mask, w.up, w.dn, strips, cols);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(nearest_envelope_kernel, dim3(nseg, (rows + NTILE - 1) / NTILE), dim3(NTILE), 0, st, w, rows, cols,
                     strips, nseg);
  SMRF_LAUNCH_CHECK();
  const LookupArgs<T> a{d_in, d_out, (long long*)d_index, d_dist2, rows, cols, nseg};
  hipLaunchKernelGGL((nearest_lookup_kernel<T>), dim3((cols + 255) / 256, rows), dim3(256), 0, st, a, w);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // namespace smrf

extern "C" {

size_t smrf_nearest_workspace_bytes(int rows, int cols, int elem_size) {
  (void)elem_size;   // the workspace holds integers only
  if (rows <= 0 || cols <= 0) return 0;
  return smrf::nearest_layout(rows, cols, nullptr, nullptr);
}

int smrf_nearest_f32(const float* d_in, float* d_out, int64_t* d_src_index, uint32_t* d_dist2, int rows, int cols,
                     void* d_workspace, size_t workspace_bytes, void* stream) {
  return smrf::nearest<float>(d_in, d_out, d_src_index, d_dist2, rows, cols, d_workspace, workspace_bytes, stream);
}

int smrf_nearest_f64(const double* d_in, double* d_out, int64_t* d_src_index, uint32_t* d_dist2, int rows, int cols,
                     void* d_workspace, size_t workspace_bytes, void* stream) {
  return smrf::nearest<double>(d_in, d_out, d_src_index, d_dist2, rows, cols, d_workspace, workspace_bytes, stream);
}

int smrf_nearest_planes(const int64_t* d_src_index, const uint32_t* d_dist2, int64_t n, int cols, double* d_dist,
                        int64_t* d_row, int64_t* d_col, void* stream) {
  if (n < 0 || cols < 1) return smrf_fail(SMRF_E_ARG, "bad size");
  if (n == 0) return SMRF_OK;
  if ((d_dist && !d_dist2) || ((d_row || d_col) && (!d_src_index || !d_row || !d_col)))
    return smrf_fail(SMRF_E_ARG, "null plane");
  hipLaunchKernelGGL(smrf::nearest_planes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)d_src_index, d_dist2, (long long)n, cols, d_dist, (long long*)d_row,
                     (long long*)d_col);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // extern "C"
