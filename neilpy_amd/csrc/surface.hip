// Local surface derivatives of neilpy (neilpy/neilpy.py:434-871): slope, aspect, hillshade / multiple_illumination,
// esri_slope, curvature and the ESRI, Zevenbergen-Thorne, Evans and Wilson-Gallant curvatures, all 3 x 3 stencils
// from one templated kernel, smrf::surface_kernel<T, MODE>.
//
// Streaming layout: a wave covers 64 consecutive columns of a raster row; each thread walks a strip of SR rows down
// its column and keeps a 3 x 3 register window (rows r-1, r, r+1 at columns c-1, c, c+1, each index clamped to the
// raster), so every row is read from HBM once per strip; the left / right loads of a row hit the lines the
// neighbouring lanes fetched.  Row addresses advance by `cols` per step: no per-cell division.  The clamped window is
// ndimage's 'reflect' rule for a 3 x 3 footprint; the np.gradient rule and ashift's rule (an off-raster neighbour is
// the cell itself) are derived from it with the cell's border flags.
//
// Arithmetic follows the restatement of DESIGN.md section 10 (tests/surface_numpy.py) operation by operation, in T
// unless NumPy computes a step in float64 (hillshade's illumination, esri_slope's window sums, laplace's lines).
// The library builds with -ffp-contract=off, and fp32 divide and sqrt stay correctly rounded, so every output that
// needs no transcendental function gives the reference's bits.
#include <cmath>

#include "raster_stencil.h"

namespace smrf {

constexpr int SX = 64, SY = 4;   // 64 columns x 4 strips per workgroup
constexpr int SR = 32;           // rows per strip

template <typename T>
struct SurfArgs {
  const T* Z;
  int rows, cols;
  int opts;
  double p0, p1, p2, p3;
  const double* ang;   // [n_ang][3]: cos zenith, sin zenith, azimuth (radians)
  int n_ang;
  void* out[6];
};

template <typename T>
__device__ inline void put(void* p, long long i, T v) {
  if (p) static_cast<T*>(p)[i] = v;
}

template <typename T>
__device__ inline T zero_nan(T v) { return v != v ? T(0) : v; }

// the 3 x 3 neighbourhood of one cell: n[i][j] = Z[clamp(r + i - 1), clamp(c + j - 1)]
template <typename T>
struct Win {
  T n[3][3];
};

// ashift's neighbour: the cell itself where the row or the column is off the raster
template <typename T>
__device__ inline T ash(const Win<T>& w, int i, int j, bool top, bool bot, bool lft, bool rgt) {
  const bool off = (i == 0 && top) || (i == 2 && bot) || (j == 0 && lft) || (j == 2 && rgt);
  return off ? w.n[1][1] : w.n[i][j];
}

template <typename T, int MODE>
__device__ inline void cell(const SurfArgs<T>& a, const Win<T>& w, long long idx, bool top, bool bot, bool lft,
                            bool rgt) {
  using K = Consts<T>;
  const T X = w.n[1][1];
  if constexpr (MODE == SMRF_SURFACE_SLOPE || MODE == SMRF_SURFACE_ASPECT || MODE == SMRF_SURFACE_HILLSHADE) {
    // np.gradient: central differences inside, one-sided at the borders (rows, cols >= 2)
    const T dy = w.n[2][1] - w.n[0][1];
    const T dx = w.n[1][2] - w.n[1][0];
    const bool ey = top || bot, ex = lft || rgt;
    if constexpr (MODE == SMRF_SURFACE_HILLSHADE) {
      double H;
      const int best = hillshade_cell<T>(dy, dx, ey, ex, a.p0, a.ang, a.n_ang, H);   // raster_stencil.h
      put<uint8_t>(a.out[0], idx, (uint8_t)best);
      put<double>(a.out[1], idx, H);
      return;
    } else if constexpr (MODE == SMRF_SURFACE_ASPECT) {
      T gy, gx;
      T A = aspect_radians<T>(dy, dx, ey, ex, gy, gx);
      if (a.opts & SMRF_SURFACE_OPT_DEGREES) A = A * K::rad2deg;
      if (gx == T(0) && gy == T(0)) A = (T)a.p0;   // flat_as
      put<T>(a.out[0], idx, A);
      return;
    } else {
      const T h = (T)a.p0, h2 = (T)(2.0 * a.p0);
      const T gy = ey ? dy / h : dy / h2;
      const T gx = ex ? dx / h : dx / h2;
      T S = sqrt(gx * gx + gy * gy);
      if (a.opts & (SMRF_SURFACE_OPT_RADIANS | SMRF_SURFACE_OPT_DEGREES)) {
        S = atan(S);
        if (a.opts & SMRF_SURFACE_OPT_DEGREES) S = S * K::rad2deg;
      }
      put<T>(a.out[0], idx, S);
    }
  } else if constexpr (MODE == SMRF_SURFACE_HORN) {
    // generic_filter's callback runs in float64 on the clamped window; its result is stored in T
    double n[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) n[i][j] = (double)w.n[i][j];
    auto ws = [](double p, double q, double r) { return (p * 1.0 + q * 2.0) + r * 1.0; };
    const double dzdx = (ws(n[0][2], n[1][2], n[2][2]) - ws(n[0][0], n[1][0], n[2][0])) / 8.0;
    const double dzdy = (ws(n[2][0], n[2][1], n[2][2]) - ws(n[0][0], n[0][1], n[0][2])) / 8.0;
    T S = (T)sqrt(dzdx * dzdx + dzdy * dzdy);
    S = S / (T)a.p0;           // cellsize (x / 1 is x)
    S = (T)a.p1 * S;           // z_factor
    if (a.opts & SMRF_SURFACE_OPT_DEGREES) S = atan(S) * K::rad2deg;
    put<T>(a.out[0], idx, S);
  } else if constexpr (MODE == SMRF_SURFACE_LAPLACE) {
    // laplace(X / cellsize): one correlate1d per axis in float64, each stored in T, summed in T
    const T cs = (T)a.p0;
    const double c = (double)(X / cs);
    const double u = (double)(w.n[0][1] / cs), d = (double)(w.n[2][1] / cs);
    const double l = (double)(w.n[1][0] / cs), r = (double)(w.n[1][2] / cs);
    const T lap = (T)(c * -2.0 + (u + d)) + (T)(c * -2.0 + (l + r));
    put<T>(a.out[0], idx, T(-100) * lap);
  } else {
    // ashift's ring from the window
    Ring<T> g{ash(w, 0, 0, top, bot, lft, rgt), ash(w, 0, 1, top, bot, lft, rgt), ash(w, 0, 2, top, bot, lft, rgt),
              ash(w, 1, 0, top, bot, lft, rgt), X, ash(w, 1, 2, top, bot, lft, rgt),
              ash(w, 2, 0, top, bot, lft, rgt), ash(w, 2, 1, top, bot, lft, rgt), ash(w, 2, 2, top, bot, lft, rgt)};
    const T X2 = T(2) * X;
    if constexpr (MODE == SMRF_SURFACE_ESRI) {
      // a NaN neighbour is the cell itself
      auto self = [X](T& z) { z = z != z ? X : z; };
      self(g.z1); self(g.z2); self(g.z3); self(g.z4); self(g.z6); self(g.z7); self(g.z8); self(g.z9);
    } else if constexpr (MODE == SMRF_SURFACE_ZT || MODE == SMRF_SURFACE_EVANS) {
      // a NaN neighbour is 2X - the opposite one, filled in this order (later fills see earlier ones)
      if (g.z1 != g.z1) g.z1 = X2 - g.z9;
      if (g.z2 != g.z2) g.z2 = X2 - g.z8;
      if (g.z3 != g.z3) g.z3 = X2 - g.z7;
      if (g.z4 != g.z4) g.z4 = X2 - g.z6;
      if (g.z6 != g.z6) g.z6 = X2 - g.z4;
      if (g.z7 != g.z7) g.z7 = X2 - g.z3;
      if (g.z8 != g.z8) g.z8 = X2 - g.z2;
      if (g.z9 != g.z9) g.z9 = X2 - g.z1;
    }
    if constexpr (MODE == SMRF_SURFACE_ESRI || MODE == SMRF_SURFACE_ZT) {
      const T L2 = (T)a.p0, L2x4 = (T)a.p1, Lx2 = (T)a.p2;
      const T D = (((g.z4 + g.z6) / T(2)) - X) / L2;
      const T E = (((g.z2 + g.z8) / T(2)) - X) / L2;
      const T F = (-g.z1 + g.z3 + g.z7 - g.z9) / L2x4;
      const T G = (-g.z4 + g.z6) / Lx2;
      const T H = (g.z2 - g.z8) / Lx2;
      const T GG = G * G, HH = H * H;
      if constexpr (MODE == SMRF_SURFACE_ESRI) {
        put<T>(a.out[0], idx, T(-200) * (D + E));
        if (a.out[1]) put<T>(a.out[1], idx, zero_nan(T(200) * (D * HH + E * GG - F * G * H) / (GG + HH)));
        if (a.out[2]) put<T>(a.out[2], idx, zero_nan(T(-200) * (D * GG + E * HH + F * G * H) / (GG + HH)));
      } else {
        const T P = GG + HH;
        const T Q = GG + HH + T(1);
        put<T>(a.out[0], idx, T(2) * (D + E));
        if (a.out[1]) put<T>(a.out[1], idx, (D * GG + T(2) * F * G * H + E * HH) / (P * (T)pow(Q, T(1.5))));
        if (a.out[2]) put<T>(a.out[2], idx, -(D * (E * E) - T(2) * F * G * H + E * GG) / (T)pow(P, T(1.5)));
        if (a.out[3]) put<T>(a.out[3], idx, -(D * HH - T(2) * F * G * H + E * GG) / (P * sqrt(Q)));
        if (a.out[4]) put<T>(a.out[4], idx, zero_nan(T(-2) * (D * GG + E * HH + F * G * H) / P));
        if (a.out[5]) put<T>(a.out[5], idx, zero_nan(T(2) * (D * HH + E * GG - F * G * H) / P));
      }
    } else if constexpr (MODE == SMRF_SURFACE_EVANS) {
      // the quadratic shared with scaled_morphometry (raster_stencil.h), here on the NaN-filled ring
      const T L2x6 = (T)a.p0, L2x3 = (T)a.p1, L2x4 = (T)a.p2, Lx6 = (T)a.p3;
      Evans<T> q;
      q.set_AB(g, L2x6, L2x3);
      q.set_C(g, L2x4);
      q.set_DE(g, Lx6);
      q.set_S2();
      // Evans sets NaN to 0 in its five ratios where X is finite
      const bool fin = X - X == T(0);
      auto fix = [fin](T v) { return (v != v && fin) ? T(0) : v; };
      put<T>(a.out[0], idx, q.K());
      if (a.out[1]) put<T>(a.out[1], idx, fix(q.K_profile()));
      if (a.out[2]) put<T>(a.out[2], idx, fix(q.K_plan()));
      if (a.out[3]) put<T>(a.out[3], idx, fix(q.K_tan()));
      if (a.out[4]) put<T>(a.out[4], idx, fix(q.K_long()));
      if (a.out[5]) put<T>(a.out[5], idx, fix(q.K_cross()));
    } else {
      // Wilson-Gallant numbering: Z1 upper right, clockwise to Z6 left; Z7 = Z8 = X (the reference's ashift(X, 8)
      // and ashift(X, 9) do not move), Z9 = X
      T w1 = g.z3, w2 = g.z6, w3 = g.z9, w4 = g.z8, w5 = g.z7, w6 = g.z4, w7 = X, w8 = X;
      if (w1 != w1) w1 = X2 - w5;
      if (w2 != w2) w2 = X2 - w6;
      if (w3 != w3) w3 = X2 - w7;
      if (w4 != w4) w4 = X2 - w8;
      if (w5 != w5) w5 = X2 - w1;
      if (w6 != w6) w6 = X2 - w2;
      if (w7 != w7) w7 = X2 - w3;
      if (w8 != w8) w8 = X2 - w4;
      const T Hx2 = (T)a.p0, H2 = (T)a.p1;
      const T ZX = (w2 - w6) / Hx2;
      const T ZY = (w8 - w4) / Hx2;
      const T ZXX = (w2 - X2 + w6) / H2;
      const T ZYY = (w8 - X2 + w4) / H2;
      const T ZXY = (-w7 + w1 + w5 - w3) / T(4) * H2;   // the reference multiplies by H**2
      const T P = ZX * ZX + ZY * ZY;
      const T Q = P + T(1);
      const T num = ZXX * (ZX * ZX) + T(2) * ZXY * ZX * ZY + ZYY * (ZY * ZY);
      put<T>(a.out[0], idx, ZXX * ZXX + T(2) * (ZXY * ZXY) + ZYY * ZYY);
      if (a.out[1]) put<T>(a.out[1], idx, num / (P * (T)pow(Q, T(1.5))));
      if (a.out[2]) put<T>(a.out[2], idx, (ZXX * (ZY * ZY) - T(2) * ZXY * ZX * ZY + ZYY * (ZX * ZX)) / (T)pow(P, T(1.5)));
      if (a.out[3]) put<T>(a.out[3], idx, num / (P * sqrt(Q)));   // the same numerator as Kp, as the reference
    }
  }
}

template <typename T, int MODE>
__global__ __launch_bounds__(SX* SY) void surface_kernel(SurfArgs<T> a) {
  const int c = blockIdx.x * SX + threadIdx.x;
  const int r0 = (blockIdx.y * SY + threadIdx.y) * SR;
  const int rows = a.rows, cols = a.cols;
  if (c >= cols || r0 >= rows) return;
  const int r1 = min(r0 + SR, rows);
  const int cl = c > 0 ? c - 1 : 0, cr = c + 1 < cols ? c + 1 : c;
  const bool lft = c == 0, rgt = c == cols - 1;
  const T* __restrict__ Z = a.Z;
  auto load = [&](int rr, T (&v)[3]) {
    const T* p = Z + (long long)rr * cols;
    v[0] = p[cl];
    v[1] = p[c];
    v[2] = p[cr];
  };
  Win<T> w;
  load(r0 > 0 ? r0 - 1 : 0, w.n[0]);
  load(r0, w.n[1]);
  long long idx = (long long)r0 * cols + c;
  for (int r = r0; r < r1; ++r, idx += cols) {
    load(r + 1 < rows ? r + 1 : r, w.n[2]);
    cell<T, MODE>(a, w, idx, r == 0, r == rows - 1, lft, rgt);
    for (int j = 0; j < 3; ++j) {
      w.n[0][j] = w.n[1][j];
      w.n[1][j] = w.n[2][j];
    }
  }
}

template <typename T, int MODE>
hipError_t launch_surface(const SurfArgs<T>& a, unsigned gy, hipStream_t st) {
  const dim3 grid((a.cols + SX - 1) / SX, gy), block(SX, SY);
  hipLaunchKernelGGL((surface_kernel<T, MODE>), grid, block, 0, st, a);
  return hipGetLastError();
}

template <typename T>
int surface(const T* d_Z, int rows, int cols, int mode, int options, double p0, double p1, double p2, double p3,
            const double* d_angles, int n_angles, void* d_out0, void* d_out1, void* d_out2, void* d_out3,
            void* d_out4, void* d_out5, void* stream) {
  if (int rc = check_size(rows, cols)) return rc;
  if (mode < SMRF_SURFACE_SLOPE || mode > SMRF_SURFACE_WG) return smrf_fail(SMRF_E_ARG, "unknown mode %d", mode);
  if (empty_raster(rows, cols)) return SMRF_OK;
  if (int rc = check_raster_ptr(d_Z)) return rc;
  const bool gradient = mode == SMRF_SURFACE_SLOPE || mode == SMRF_SURFACE_ASPECT || mode == SMRF_SURFACE_HILLSHADE;
  if (gradient && (rows < 2 || cols < 2))
    return smrf_fail(SMRF_E_ARG, "np.gradient needs at least 2 cells per axis (%d x %d)", rows, cols);
  void* outs[6] = {d_out0, d_out1, d_out2, d_out3, d_out4, d_out5};
  const int n_out[] = {1, 1, 2, 1, 1, 3, 6, 6, 4};
  for (int k = n_out[mode]; k < 6; ++k)
    if (outs[k]) return smrf_fail(SMRF_E_ARG, "mode %d has %d outputs, output %d is set", mode, n_out[mode], k);
  if (mode == SMRF_SURFACE_HILLSHADE) {
    if (n_angles < 1 || !d_angles) return smrf_fail(SMRF_E_ARG, "hillshade needs a non-empty angle table");
    if (d_out1 && n_angles != 1) return smrf_fail(SMRF_E_ARG, "the float64 hillshade takes exactly one angle");
    if (!d_out0 && !d_out1) return smrf_fail(SMRF_E_ARG, "null output");
  } else if (!d_out0) {
    return smrf_fail(SMRF_E_ARG, "null output");
  }
  unsigned gy = 0;
  if (int rc = grid_rows(rows, SY * SR, gy)) return rc;
  SurfArgs<T> a{d_Z, rows, cols, options, p0, p1, p2, p3, d_angles, n_angles, {}};
  for (int k = 0; k < 6; ++k) a.out[k] = outs[k];
  const hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  switch (mode) {
    case SMRF_SURFACE_SLOPE: e = launch_surface<T, SMRF_SURFACE_SLOPE>(a, gy, st); break;
    case SMRF_SURFACE_ASPECT: e = launch_surface<T, SMRF_SURFACE_ASPECT>(a, gy, st); break;
    case SMRF_SURFACE_HILLSHADE: e = launch_surface<T, SMRF_SURFACE_HILLSHADE>(a, gy, st); break;
    case SMRF_SURFACE_HORN: e = launch_surface<T, SMRF_SURFACE_HORN>(a, gy, st); break;
    case SMRF_SURFACE_LAPLACE: e = launch_surface<T, SMRF_SURFACE_LAPLACE>(a, gy, st); break;
    case SMRF_SURFACE_ESRI: e = launch_surface<T, SMRF_SURFACE_ESRI>(a, gy, st); break;
    case SMRF_SURFACE_ZT: e = launch_surface<T, SMRF_SURFACE_ZT>(a, gy, st); break;
    case SMRF_SURFACE_EVANS: e = launch_surface<T, SMRF_SURFACE_EVANS>(a, gy, st); break;
    default: e = launch_surface<T, SMRF_SURFACE_WG>(a, gy, st); break;
  }
  SMRF_HIP_CHECK(e);
  return SMRF_OK;
}

}  // namespace smrf

extern "C" {

int smrf_surface_f32(const float* d_Z, int rows, int cols, int mode, int options, double p0, double p1, double p2,
                     double p3, const double* d_angles, int n_angles, void* d_out0, void* d_out1, void* d_out2,
                     void* d_out3, void* d_out4, void* d_out5, void* stream) {
  return smrf::surface<float>(d_Z, rows, cols, mode, options, p0, p1, p2, p3, d_angles, n_angles, d_out0, d_out1,
                              d_out2, d_out3, d_out4, d_out5, stream);
}

int smrf_surface_f64(const double* d_Z, int rows, int cols, int mode, int options, double p0, double p1, double p2,
                     double p3, const double* d_angles, int n_angles, void* d_out0, void* d_out1, void* d_out2,
                     void* d_out3, void* d_out4, void* d_out5, void* stream) {
  return smrf::surface<double>(d_Z, rows, cols, mode, options, p0, p1, p2, p3, d_angles, n_angles, d_out0, d_out1,
                               d_out2, d_out3, d_out4, d_out5, stream);
}

}  // extern "C"
