// The multi-scale tools of neilpy built on ashift(surface, direction, n): scaled_morphometry (neilpy/neilpy.py:2472),
// vip_score (:1832, with triangle_height :1818) and ashift itself (:1290).
//
// One sampling rule for every neighbour, ashift's: the sample at offset (dr, dc) of cell (r, c) is Z[r + dr, c + dc]
// where that row AND that column are on the raster, otherwise Z[r, c].  A stride n >= rows (or cols) makes every sample
// along that axis the cell itself.
//
// Layout: a wave covers 64 consecutive columns of a row; a thread walks a short strip of MR rows down its column.  The
// rows r - n, r, r + n are each read coalesced at the columns c - n, c, c + n; the ninefold reuse of a cell is left to
// L2 and the memory-side cache (a register window as in surface.hip only works at n = 1).  Every address is formed in
// 64 bits and lies on the raster: an off-raster offset is replaced by 0 before the load, and the loaded value by the
// cell afterwards.  Row addresses advance by `cols` per step: no per-cell division.
//
// Arithmetic follows DESIGN.md section 13 (tests/morphometry_numpy.py) operation by operation in the reference's order.
// The library builds with -ffp-contract=off and fp32 divide and sqrt stay correctly rounded, so every output that needs
// no transcendental function gives the reference's bits.
#include "raster_stencil.h"

namespace smrf {

constexpr int MX = 64, MY = 4;   // 64 columns x 4 strips per workgroup
constexpr int MR = 4;            // rows per strip

// Column offsets and their validity are the thread's; row offsets the step's.  p = &Z[r, 0].
template <typename T>
__device__ inline Ring<T> ring_at(const T* __restrict__ p, long long c, long long up, long long dn, long long lf,
                                  long long rt, bool uok, bool dok, bool lok, bool rok) {
  Ring<T> g;
  const T* pu = p - up;   // up, dn: n * cols where the row is on the raster, else 0
  const T* pd = p + dn;
  const long long cl = c - lf, cr = c + rt;   // lf, rt: n where the column is on the raster, else 0
  g.X = p[c];
  g.z1 = pu[cl]; g.z2 = pu[c]; g.z3 = pu[cr];
  g.z4 = p[cl];                g.z6 = p[cr];
  g.z7 = pd[cl]; g.z8 = pd[c]; g.z9 = pd[cr];
  if (!(uok && lok)) g.z1 = g.X;
  if (!uok) g.z2 = g.X;
  if (!(uok && rok)) g.z3 = g.X;
  if (!lok) g.z4 = g.X;
  if (!rok) g.z6 = g.X;
  if (!(dok && lok)) g.z7 = g.X;
  if (!dok) g.z8 = g.X;
  if (!(dok && rok)) g.z9 = g.X;
  return g;
}

// np.mod(a, 360): C fmod, then the sign of the divisor
template <typename T>
__device__ inline T mod360(T a) {
  T m = fmod(a, T(360));
  if (m != T(0)) {
    if (m < T(0)) m = m + T(360);
  } else {
    m = T(0);
  }
  return m;
}

template <typename T>
struct MorphArgs {
  const T* Z;
  int rows, cols, n;
  double d0, d1, d2, d3;   // 6L^2, 3L^2, 4L^2, 6L
  T* out[8];               // A, S, K, K_profile, K_cross, K_long, K_tan, K_plan
};

template <typename T>
__device__ inline void morph_cell(const MorphArgs<T>& a, const Ring<T>& g, long long idx) {
  // the quadratic shared with evans_curvature (raster_stencil.h); the divisors are converted once, up front
  const T L2x6 = (T)a.d0, L2x3 = (T)a.d1, L2x4 = (T)a.d2, Lx6 = (T)a.d3;
  Evans<T> q;
  q.set_AB(g, L2x6, L2x3);
  if (a.out[2]) a.out[2][idx] = q.K();
  if (!(a.out[0] || a.out[1] || a.out[3] || a.out[4] || a.out[5] || a.out[6] || a.out[7])) return;
  q.set_DE(g, Lx6);
  if (a.out[0]) a.out[0][idx] = mod360(T(270) - atan2(q.E, q.D) * Consts<T>::rad2deg);
  q.set_S2();
  if (a.out[1]) a.out[1][idx] = atan(sqrt(q.S2)) * Consts<T>::rad2deg;
  if (!(a.out[3] || a.out[4] || a.out[5] || a.out[6] || a.out[7])) return;
  q.set_C(g, L2x4);
  // no NaN repair: 0 / 0 on flats propagates
  if (a.out[3]) a.out[3][idx] = q.K_profile();
  if (a.out[4]) a.out[4][idx] = q.K_cross();
  if (a.out[5]) a.out[5][idx] = q.K_long();
  if (a.out[6]) a.out[6][idx] = q.K_tan();
  if (a.out[7]) a.out[7][idx] = q.K_plan();
}

template <typename T>
struct VipArgs {
  const T* Z;
  int rows, cols;
  double x[2], b2[2];   // [0] diagonal, [1] axis: x = dlist[d % 2] * cellsize, b2 = (2x)**2 as the host's pow gives it
  double* out;
};

// triangle_height summed over the four lines through the cell, divided by 4
template <typename T>
__device__ inline void vip_cell(const VipArgs<T>& a, const Ring<T>& g, long long idx) {
  const T zd[4] = {g.z1, g.z2, g.z3, g.z6};   // directions 0..3
  const T ze[4] = {g.z9, g.z8, g.z7, g.z4};   // directions 4..7, the opposite ends
  double acc = 0.0;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const double x = a.x[d & 1], b2 = a.b2[d & 1];
    const double h0 = (double)(T)(zd[d] - g.X);   // the differences are formed in T, then widened
    const double h1 = (double)(T)(ze[d] - g.X);
    const double cp = fabs(((-x) * h1) - (h0 * x));
    const double dh = h1 - h0;
    const double base = sqrt(b2 + dh * dh);
    acc = acc + cp / base;
  }
  a.out[idx] = acc / 4.0;
}

template <typename T>
struct ShiftArgs {
  const T* Z;
  int rows, cols;
  long long dr, dc;   // the tap, in cells: each 0 or +-n
  T* out;
};

// The strip walk shared by the three kernels: F(ring, flat index) per cell.
template <typename T, typename F>
__device__ inline void walk(const T* __restrict__ Z, int rows, int cols, long long n, F&& f) {
  const int c = blockIdx.x * MX + threadIdx.x;
  const int r0 = (blockIdx.y * MY + threadIdx.y) * MR;
  if (c >= cols || r0 >= rows) return;
  const int r1 = min(r0 + MR, rows);
  const bool lok = c - n >= 0, rok = c + n < cols;
  const long long lf = lok ? n : 0, rt = rok ? n : 0;
  const long long step = n * cols;
  long long idx = (long long)r0 * cols;
  for (int r = r0; r < r1; ++r, idx += cols) {
    const bool uok = r - n >= 0, dok = r + n < rows;
    const Ring<T> g = ring_at<T>(Z + idx, c, uok ? step : 0, dok ? step : 0, lf, rt, uok, dok, lok, rok);
    f(g, idx + c);
  }
}

template <typename T>
__global__ __launch_bounds__(MX* MY) void morphometry_kernel(MorphArgs<T> a) {
  walk<T>(a.Z, a.rows, a.cols, a.n, [&](const Ring<T>& g, long long idx) { morph_cell<T>(a, g, idx); });
}

template <typename T>
__global__ __launch_bounds__(MX* MY) void vip_kernel(VipArgs<T> a) {
  walk<T>(a.Z, a.rows, a.cols, 1, [&](const Ring<T>& g, long long idx) { vip_cell<T>(a, g, idx); });
}

template <typename T>
__global__ __launch_bounds__(MX* MY) void ashift_kernel(ShiftArgs<T> a) {
  const int c = blockIdx.x * MX + threadIdx.x;
  const int r0 = (blockIdx.y * MY + threadIdx.y) * MR;
  if (c >= a.cols || r0 >= a.rows) return;
  const int r1 = min(r0 + MR, a.rows);
  const long long cc = c + a.dc;
  const bool cok = cc >= 0 && cc < a.cols;
  long long idx = (long long)r0 * a.cols + c;
  for (int r = r0; r < r1; ++r, idx += a.cols) {
    const long long rr = r + a.dr;
    const bool ok = cok && rr >= 0 && rr < a.rows;
    a.out[idx] = a.Z[ok ? rr * a.cols + cc : idx];
  }
}

static int grid_of(int rows, int cols, dim3& grid) {
  unsigned gy = 0;
  if (int rc = grid_rows(rows, MY * MR, gy)) return rc;
  grid = dim3((cols + MX - 1) / MX, gy);
  return SMRF_OK;
}

static int check_raster(const void* d_Z, int rows, int cols, bool& empty) {
  if (int rc = check_size(rows, cols)) return rc;
  empty = empty_raster(rows, cols);
  return empty ? SMRF_OK : check_raster_ptr(d_Z);
}

template <typename T>
int morphometry(const T* d_Z, int rows, int cols, int n, double d0, double d1, double d2, double d3, T* d_A, T* d_S,
                T* d_K, T* d_K_profile, T* d_K_cross, T* d_K_long, T* d_K_tan, T* d_K_plan, void* stream) {
  bool empty = false;
  if (int rc = check_raster(d_Z, rows, cols, empty)) return rc;
  if (n < 1) return smrf_fail(SMRF_E_ARG, "lookup distance %d: must be >= 1", n);
  MorphArgs<T> a{d_Z, rows, cols, n, d0, d1, d2, d3, {d_A, d_S, d_K, d_K_profile, d_K_cross, d_K_long, d_K_tan, d_K_plan}};
  bool any = false;
  for (T* p : a.out) any = any || p;
  if (empty || !any) return SMRF_OK;
  dim3 grid;
  if (int rc = grid_of(rows, cols, grid)) return rc;
  hipLaunchKernelGGL(morphometry_kernel<T>, grid, dim3(MX, MY), 0, (hipStream_t)stream, a);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

template <typename T>
int vip(const T* d_Z, int rows, int cols, double x_diag, double x_axis, double b2_diag, double b2_axis, double* d_out,
        void* stream) {
  bool empty = false;
  if (int rc = check_raster(d_Z, rows, cols, empty)) return rc;
  if (empty) return SMRF_OK;
  if (!d_out) return smrf_fail(SMRF_E_ARG, "null output");
  VipArgs<T> a{d_Z, rows, cols, {x_diag, x_axis}, {b2_diag, b2_axis}, d_out};
  dim3 grid;
  if (int rc = grid_of(rows, cols, grid)) return rc;
  hipLaunchKernelGGL(vip_kernel<T>, grid, dim3(MX, MY), 0, (hipStream_t)stream, a);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

template <typename T>
int ashift(const T* d_Z, int rows, int cols, int direction, int n, T* d_out, void* stream) {
  bool empty = false;
  if (int rc = check_raster(d_Z, rows, cols, empty)) return rc;
  if (n < 1) return smrf_fail(SMRF_E_ARG, "shift %d: must be >= 1", n);
  if (empty) return SMRF_OK;
  if (!d_out) return smrf_fail(SMRF_E_ARG, "null output");
  if (d_out == d_Z) return smrf_fail(SMRF_E_ARG, "ashift cannot run in place");
  // any direction but the eight of the table leaves the raster as it is
  const bool known = direction >= 0 && direction < 8;
  ShiftArgs<T> a{d_Z, rows, cols, known ? (long long)kDR[direction] * n : 0, known ? (long long)kDC[direction] * n : 0, d_out};
  dim3 grid;
  if (int rc = grid_of(rows, cols, grid)) return rc;
  hipLaunchKernelGGL(ashift_kernel<T>, grid, dim3(MX, MY), 0, (hipStream_t)stream, a);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // namespace smrf

extern "C" {

int smrf_morphometry_f32(const float* d_Z, int rows, int cols, int n, double d0, double d1, double d2, double d3,
                         float* d_A, float* d_S, float* d_K, float* d_K_profile, float* d_K_cross, float* d_K_long,
                         float* d_K_tan, float* d_K_plan, void* stream) {
  return smrf::morphometry<float>(d_Z, rows, cols, n, d0, d1, d2, d3, d_A, d_S, d_K, d_K_profile, d_K_cross, d_K_long,
                                  d_K_tan, d_K_plan, stream);
}

int smrf_morphometry_f64(const double* d_Z, int rows, int cols, int n, double d0, double d1, double d2, double d3,
                         double* d_A, double* d_S, double* d_K, double* d_K_profile, double* d_K_cross,
                         double* d_K_long, double* d_K_tan, double* d_K_plan, void* stream) {
  return smrf::morphometry<double>(d_Z, rows, cols, n, d0, d1, d2, d3, d_A, d_S, d_K, d_K_profile, d_K_cross, d_K_long,
                                   d_K_tan, d_K_plan, stream);
}

int smrf_vip_f32(const float* d_Z, int rows, int cols, double x_diag, double x_axis, double b2_diag, double b2_axis,
                 double* d_out, void* stream) {
  return smrf::vip<float>(d_Z, rows, cols, x_diag, x_axis, b2_diag, b2_axis, d_out, stream);
}

int smrf_vip_f64(const double* d_Z, int rows, int cols, double x_diag, double x_axis, double b2_diag, double b2_axis,
                 double* d_out, void* stream) {
  return smrf::vip<double>(d_Z, rows, cols, x_diag, x_axis, b2_diag, b2_axis, d_out, stream);
}

int smrf_ashift_f32(const float* d_Z, int rows, int cols, int direction, int n, float* d_out, void* stream) {
  return smrf::ashift<float>(d_Z, rows, cols, direction, n, d_out, stream);
}

int smrf_ashift_f64(const double* d_Z, int rows, int cols, int direction, int n, double* d_out, void* stream) {
  return smrf::ashift<double>(d_Z, rows, cols, direction, n, d_out, stream);
}

}  // extern "C"
