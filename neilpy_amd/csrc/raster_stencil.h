// What the raster stencil families (surface, morphometry, terrain, focal, nearest) share: the angle constants, the nine
// samples of a 3 x 3 ring, Evans' quadratic through them, ashift's direction table and the argument checks every entry
// point makes.  Device arithmetic is written operation for operation as DESIGN.md sections 10 and 13 state it: the
// library builds with -ffp-contract=off and the order of the additions is part of the contract.
#pragma once
#include <cmath>

#include "smrf_common.h"

namespace smrf {

template <typename T>
struct Consts;
template <>
struct Consts<float> {
  static constexpr float rad2deg = 180.0f / 3.14159265358979323846f;   // np.rad2deg on float32: 180f / float(pi)
  static constexpr float half_pi = (float)(3.14159265358979323846 / 2);
  static constexpr float two_pi = (float)(2 * 3.14159265358979323846);
};
template <>
struct Consts<double> {
  static constexpr double rad2deg = 180.0 / 3.14159265358979323846;   // np.rad2deg multiplies by 180 / pi
  static constexpr double half_pi = 3.14159265358979323846 / 2;       // np.pi / 2
  static constexpr double two_pi = 2 * 3.14159265358979323846;
};

// ashift's directions (neilpy.py:1290-1307): clockwise from the upper left, (row, column) offsets
constexpr int kDR[8] = {-1, -1, -1, 0, 1, 1, 1, 0};
constexpr int kDC[8] = {-1, 0, 1, 1, 1, 0, -1, -1};

// the nine samples of one cell, z1..z9 in reading order (z5 = X)
template <typename T>
struct Ring {
  T z1, z2, z3, z4, X, z6, z7, z8, z9;
};

// Evans' quadratic (Wood 1991) through a ring, z = A x^2 + B y^2 + C x y + D x + E y + F, and its curvatures.  The
// divisors 6L^2, 3L^2, 4L^2 and 6L come in T.  The members are filled in steps so that a caller computes only what its
// outputs need: K needs set_AB; aspect set_DE; slope set_S2 as well; the five ratio curvatures all four.  No NaN repair
// here: on a flat the ratios are 0 / 0, and what becomes of that is the caller's rule.
template <typename T>
struct Evans {
  T A, B, C, D, E, DD, EE, S2;
  __device__ inline void set_AB(const Ring<T>& g, T L2x6, T L2x3) {
    const T X = g.X;
    A = (g.z1 + g.z3 + g.z4 + g.z6 + g.z7 + g.z9) / L2x6 - (g.z2 + X + g.z8) / L2x3;
    B = (g.z1 + g.z2 + g.z3 + g.z7 + g.z8 + g.z9) / L2x6 - (g.z4 + X + g.z6) / L2x3;
  }
  __device__ inline void set_DE(const Ring<T>& g, T Lx6) {
    D = (g.z3 + g.z6 + g.z9 - g.z1 - g.z4 - g.z7) / Lx6;
    E = (g.z1 + g.z2 + g.z3 - g.z7 - g.z8 - g.z9) / Lx6;
  }
  __device__ inline void set_S2() { DD = D * D, EE = E * E, S2 = DD + EE; }
  __device__ inline void set_C(const Ring<T>& g, T L2x4) { C = (g.z3 + g.z7 - g.z1 - g.z9) / L2x4; }
  __device__ inline T K() const { return T(-2) * (A + B); }
  __device__ inline T K_profile() const { return -(A * DD + T(2) * C * D * E + B * EE) / (S2 * (T)pow(S2 + T(1), T(1.5))); }
  __device__ inline T K_plan() const { return -(A * EE - T(2) * C * D * E + B * DD) / (T)pow(S2, T(1.5)); }
  __device__ inline T K_tan() const { return -(A * EE - T(2) * C * D * E + B * DD) / (S2 * sqrt(S2 + T(1))); }
  __device__ inline T K_long() const { return T(-2) * (A * DD + B * EE + C * D * E) / S2; }
  __device__ inline T K_cross() const { return T(-2) * (B * DD + A * EE - C * D * E) / S2; }
};

// np.gradient's aspect of one cell, clockwise from north in radians in [0, 2 pi): dy, dx = the differences of the cell's
// vertical and horizontal neighbours (central inside, one-sided where ey / ex say the cell is on a border), at unit
// spacing whatever the cellsize.  gy, gx = the gradient (both 0 on a flat; what becomes of A there is the caller's rule).
template <typename T>
__device__ inline T aspect_radians(T dy, T dx, bool ey, bool ex, T& gy, T& gx) {
  using K = Consts<T>;
  gy = ey ? dy / T(1) : dy / T(2);
  gx = ex ? dx / T(1) : dx / T(2);
  T A = K::half_pi - atan2(gy, -gx);
  if (A < T(0)) A = A + K::two_pi;
  return A;
}

// hillshade of one cell: slope and aspect in T from the same differences, the illumination in
// float64 over a table of n_ang rows (cos zenith, sin zenith, azimuth).  Returns the largest uint8 shade round(255 H)
// over the rows (NaN -> 0); H = the last row's float shade.  hillshade, multiple_illumination (surface.hip) and
// colortable_shade (relief.hip) all shade through this one function, spacing = cellsize / z_factor.
template <typename T>
__device__ inline int hillshade_cell(T dy, T dx, bool ey, bool ex, double spacing, const double* ang, int n_ang,
                                     double& H) {
  T gy, gx;
  T A = aspect_radians<T>(dy, dx, ey, ex, gy, gx);
  if (gx == T(0) && gy == T(0)) A = T(0);
  const T h = (T)spacing, h2 = (T)(2.0 * spacing);
  const T sy = ey ? dy / h : dy / h2;
  const T sx = ex ? dx / h : dx / h2;
  const T S = atan(sqrt(sx * sx + sy * sy));
  const double cs = (double)cos(S), sn = (double)sin(S), Ad = (double)A;
  int best = 0;
  H = 0.0;
  for (int k = 0; k < n_ang; ++k) {
    const double* g = ang + 3 * k;
    H = (g[0] * cs) + (g[1] * sn * cos(g[2] - Ad));
    if (H < 0.0) H = 0.0;
    const double v = rint(255.0 * H);
    const int u = v != v ? 0 : (int)v;   // NaN -> 0, as the x86 conversion gives
    best = u > best ? u : best;
  }
  return best;
}

// ---- host: the checks of every raster entry point, with the status codes and texts callers read from smrf_last_error()
inline int check_size(int rows, int cols, int count = 0) {
  return (rows < 0 || cols < 0 || count < 0) ? smrf_fail(SMRF_E_ARG, "negative size") : SMRF_OK;
}
// an empty raster is SMRF_OK with nothing launched
inline bool empty_raster(int rows, int cols) { return (long long)rows * cols == 0; }
inline int check_raster_ptr(const void* d_Z) { return d_Z ? SMRF_OK : smrf_fail(SMRF_E_ARG, "null raster"); }
// grid.y for `rows_per_wg` rows per workgroup, within the launch limit of 65535
inline int grid_rows(int rows, int rows_per_wg, unsigned& gy) {
  const long long n = ((long long)rows + rows_per_wg - 1) / rows_per_wg;
  if (n > 65535) return smrf_fail(SMRF_E_ARG, "%d rows exceed the launch grid", rows);
  gy = (unsigned)n;
  return SMRF_OK;
}

}  // namespace smrf
