// Terrain ray marches of neilpy's openness family (neilpy/neilpy.py:1290-1653): openness, skyview_factor,
// count_openness / geomorphons and ternary_pattern_from_openness, all from one templated kernel.
//
// One thread per cell, 64 lanes along a raster row, 8 rows per workgroup.  For every direction d the thread walks
// the step list k_0 < k_1 < ... (1..L, or progressive_window's list under fast=True) and keeps the largest and
// smallest slope t = fp64(Z[sample] - Z[cell]) / D(d, k) with NaN ignored; the reference's per-sample angle
// pi/2 - arctan(t) is monotone in t, so one arctan per direction and sign gives the same minimum.
//
// Tiled path: the workgroup's 64 x 8 cells plus a halo of H = min(largest step, cap) cells are staged in LDS once,
// steps k <= H read LDS and larger steps read global memory.  Direct path: every sample reads global memory.  The
// arithmetic is the same code in both, so both give the same bits.
#include <algorithm>
#include <utility>

#include "raster_stencil.h"

namespace {

constexpr int TX = 64, TY = 8;
using smrf::kDC, smrf::kDR;
constexpr double kHalfPi = smrf::Consts<double>::half_pi, kRad2Deg = smrf::Consts<double>::rad2deg;

template <typename T>
struct RayArgs {
  const T* Z;
  int rows, cols;
  const int* steps;          // nsteps ascending step lengths
  const uint8_t* flags;      // per step: bit 0 main march, bit 1 the enhance march (a prefix; count mode only)
  const double* dist;        // [2][nsteps]: D for even d (diagonal), then for odd d
  int nsteps, halo;          // tiled path: steps k <= halo read the LDS tile
  const int* nbr;            // openness: the neighbors list
  int n_nbr, dir_mask;
  double thr;
  int opts;
  const void* lut;
  void* out0;
  void* out1;
  void* out2;
};

// a[d] for a workgroup-uniform d, as a branch on d (an indexed read would put a[] in scratch)
__device__ inline double pick(const double (&a)[8], int d) {
  switch (d) {
    case 0: return a[0];
    case 1: return a[1];
    case 2: return a[2];
    case 3: return a[3];
    case 4: return a[4];
    case 5: return a[5];
    case 6: return a[6];
    default: return a[7];
  }
}

// openness angle of a direction from its largest slope (+inf when every sample was NaN)
__device__ inline double open_angle(double tmax) { return tmax != tmax ? INFINITY : kHalfPi - atan(tmax); }

template <typename T, int MODE, bool LDS>
__global__ __launch_bounds__(TX* TY) void rays_kernel(RayArgs<T> a) {
  extern __shared__ __align__(8) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const int lx = threadIdx.x, ly = threadIdx.y;
  const int c0 = blockIdx.x * TX, r0 = blockIdx.y * TY;
  const int rows = a.rows, cols = a.cols;
  const int H = LDS ? a.halo : 0;
  const int LW = TX + 2 * H;
  if constexpr (LDS) {
    const int n = LW * (TY + 2 * H);
    for (int i = ly * TX + lx; i < n; i += TX * TY) {
      const int tr = i / LW, tc = i - tr * LW;
      const int gr = r0 - H + tr, gc = c0 - H + tc;
      T v = 0;
      if (gr >= 0 && gr < rows && gc >= 0 && gc < cols) v = a.Z[(long long)gr * cols + gc];
      tile[i] = v;
    }
    __syncthreads();
  }
  const int r = r0 + ly, c = c0 + lx;
  if (r >= rows || c >= cols) return;
  const long long idx = (long long)r * cols + c;
  const T z = a.Z[idx];
  const int nsteps = a.nsteps;
  const int* __restrict__ steps = a.steps;
  int n_lds = 0;                 // the steps are ascending: those within the halo come first
  if constexpr (LDS)
    while (n_lds < nsteps && steps[n_lds] <= H) ++n_lds;
  const uint8_t* __restrict__ flags = a.flags;
  int n_small = 0;               // count mode with enhance: the enhance march is a prefix of the steps
  if constexpr (MODE == 2)
    if (a.opts & 2)
      while (n_small < nsteps && (flags[n_small] & 2)) ++n_small;

  double acc[8];          // MODE 0: per-direction angle
  double sky = 0.0;       // MODE 1
  int npos = 0, nneg = 0, spos = 0, sneg = 0;   // MODE 2
  long long code = 0, pw = 1;                   // MODE 3
  // one body per direction with d a compile-time constant (acc[] stays in registers)
  auto direction = [&]<int d>(std::integral_constant<int, d>) {
    acc[d] = 0.0;
    if (!((a.dir_mask >> d) & 1)) {
      pw *= 3;
      return;
    }
    constexpr int dr = kDR[d], dc = kDC[d];
    int kin = 1 << 30;   // steps that stay on the raster
    if (dr < 0) kin = min(kin, r);
    if (dr > 0) kin = min(kin, rows - 1 - r);
    if (dc < 0) kin = min(kin, c);
    if (dc > 0) kin = min(kin, cols - 1 - c);
    const double* __restrict__ D = a.dist + ((d & 1) ? nsteps : 0);
    double tmax = NAN, tmin = NAN, smax = NAN, smin = NAN;
    // SMALL: the step belongs to the enhance march (a prefix), and to the main march only if its flag says so
    auto step = [&]<bool SMALL>(int i, T s, std::bool_constant<SMALL>) {
      const double t = (double)(T)(s - z) / D[i];
      if constexpr (SMALL) {
        smax = fmax(smax, t);
        smin = fmin(smin, t);
        if (flags[i] & 1) {
          tmax = fmax(tmax, t);
          tmin = fmin(tmin, t);
        }
      } else {
        tmax = fmax(tmax, t);
        if constexpr (MODE >= 2) tmin = fmin(tmin, t);
      }
    };
    // sky-view: the ray stops at the last on-raster cell; openness: an off-raster sample reads the cell itself
    auto hop = [&](int k) { return MODE == 1 ? min(k, kin) : (k <= kin ? k : 0); };
    const T* base = tile + (ly + H) * LW + (lx + H);
    const int off = dr * LW + dc;
    const T* gbase = a.Z + idx;
    const long long goff = (long long)dr * cols + dc;
    auto march = [&]<bool SMALL>(int i0, int i1, std::bool_constant<SMALL> sm) {
      const int im = min(max(i0, n_lds), i1);
      if constexpr (LDS)
        for (int i = i0; i < im; ++i) step(i, base[hop(steps[i]) * off], sm);
      for (int i = im; i < i1; ++i) step(i, gbase[hop(steps[i]) * goff], sm);
    };
    if constexpr (MODE == 2) march(0, n_small, std::true_type{});
    march(n_small, nsteps, std::false_type{});

    if constexpr (MODE == 0) {
      acc[d] = open_angle(tmax);
    } else if constexpr (MODE == 1) {
      const double ang = tmax != tmax ? 0.0 : fmax(0.0, atan(tmax));
      sky += sin(ang);
    } else if constexpr (MODE == 2) {
      // O = deg(openness(Z)) - deg(openness(-Z)); negating Z negates every slope exactly
      const double O = open_angle(tmax) * kRad2Deg - open_angle(-tmin) * kRad2Deg;
      npos += O > a.thr;
      nneg += O < -a.thr;
      if (a.opts & 2) {
        const double Os = open_angle(smax) * kRad2Deg - open_angle(-smin) * kRad2Deg;
        spos += Os > a.thr;
        sneg += Os < -a.thr;
      }
    } else {
      const double O = open_angle(tmax) * kRad2Deg - ((a.opts & 1) ? open_angle(-tmin) * kRad2Deg : 90.0);
      const int digit = O < -a.thr ? 0 : (O > a.thr ? 2 : 1);
      code += digit * pw;
      pw *= 3;
    }
  };
  [&]<int... D>(std::integer_sequence<int, D...>) {
    (direction(std::integral_constant<int, D>{}), ...);
  }(std::make_integer_sequence<int, 8>{});

  if constexpr (MODE == 0) {
    double s = pick(acc, a.nbr[0]);
    for (int j = 1; j < a.n_nbr; ++j) s += pick(acc, a.nbr[j]);
    static_cast<double*>(a.out0)[idx] = s / (double)a.n_nbr * kRad2Deg;
  } else if constexpr (MODE == 1) {
    static_cast<double*>(a.out0)[idx] = 1.0 - sky / 8.0;
  } else if constexpr (MODE == 2) {
    if (a.out0) static_cast<uint8_t*>(a.out0)[idx] = (uint8_t)npos;
    if (a.out1) static_cast<uint8_t*>(a.out1)[idx] = (uint8_t)nneg;
    if (a.out2) {
      const uint8_t* tab = static_cast<const uint8_t*>(a.lut);   // 9 x 9, [num_pos][num_neg]
      int g = tab[npos * 9 + nneg];
      if (a.opts & 2) {   // the correction of forms, neilpy.py:1647-1649, in that order
        const int gs = tab[spos * 9 + sneg];
        if ((g == 4 || g == 8) && gs == 1) g = 1;
        else if (g == 2 || g == 3) g = gs;
      }
      static_cast<uint8_t*>(a.out2)[idx] = (uint8_t)g;
    }
  } else {
    if (a.lut) code = static_cast<const int64_t*>(a.lut)[code];
    static_cast<int64_t*>(a.out0)[idx] = code;
  }
}

template <typename T, int MODE>
hipError_t launch_mode(const RayArgs<T>& a, bool tiled, unsigned gy, hipStream_t st) {
  const dim3 grid((a.cols + TX - 1) / TX, gy), block(TX, TY);
  if (tiled) {
    const size_t lds = (size_t)(TX + 2 * a.halo) * (TY + 2 * a.halo) * sizeof(T);
    hipLaunchKernelGGL((rays_kernel<T, MODE, true>), grid, block, lds, st, a);
  } else {
    hipLaunchKernelGGL((rays_kernel<T, MODE, false>), grid, block, 0, st, a);
  }
  return hipGetLastError();
}

template <typename T>
int terrain_rays(const T* d_Z, int rows, int cols, int mode, const int* d_steps, const uint8_t* d_flags,
                 const double* d_dist, int nsteps, int max_step, const int* d_neighbors, int n_neighbors,
                 int dir_mask, double threshold, int options, const void* d_lut, void* d_out0, void* d_out1,
                 void* d_out2, int impl, void* stream) {
  if (int rc = smrf::check_size(rows, cols, nsteps)) return rc;
  if (mode < SMRF_TERRAIN_OPENNESS || mode > SMRF_TERRAIN_TERNARY) return smrf_fail(SMRF_E_ARG, "unknown mode %d", mode);
  if (impl < SMRF_TERRAIN_IMPL_AUTO || impl > SMRF_TERRAIN_IMPL_DIRECT) return smrf_fail(SMRF_E_ARG, "unknown impl %d", impl);
  if (smrf::empty_raster(rows, cols)) return SMRF_OK;
  if (!d_Z || (nsteps > 0 && (!d_steps || !d_flags || !d_dist))) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (mode != SMRF_TERRAIN_COUNT && !d_out0) return smrf_fail(SMRF_E_ARG, "null output");
  if (mode == SMRF_TERRAIN_OPENNESS && (n_neighbors < 1 || !d_neighbors))
    return smrf_fail(SMRF_E_ARG, "openness needs a non-empty neighbors list");
  if (mode == SMRF_TERRAIN_COUNT && d_out2 && !d_lut) return smrf_fail(SMRF_E_ARG, "geomorphons need the 9 x 9 table");
  if (dir_mask < 0 || dir_mask > 255) return smrf_fail(SMRF_E_ARG, "dir_mask out of range");
  unsigned gy = 0;
  if (int rc = smrf::grid_rows(rows, TY, gy)) return rc;
  RayArgs<T> a{d_Z, rows, cols, d_steps, d_flags, d_dist, nsteps, 0, d_neighbors, n_neighbors, dir_mask,
               threshold, options, d_lut, d_out0, d_out1, d_out2};
  const int cap = sizeof(T) == 8 ? SMRF_TERRAIN_HALO_CAP_F64 : SMRF_TERRAIN_HALO_CAP_F32;
  const bool tiled = impl != SMRF_TERRAIN_IMPL_DIRECT && nsteps > 0 && max_step > 0;
  if (tiled) a.halo = std::min(max_step, cap);
  const hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  switch (mode) {
    case SMRF_TERRAIN_OPENNESS: e = launch_mode<T, 0>(a, tiled, gy, st); break;
    case SMRF_TERRAIN_SKYVIEW: e = launch_mode<T, 1>(a, tiled, gy, st); break;
    case SMRF_TERRAIN_COUNT: e = launch_mode<T, 2>(a, tiled, gy, st); break;
    default: e = launch_mode<T, 3>(a, tiled, gy, st); break;
  }
  SMRF_HIP_CHECK(e);
  return SMRF_OK;
}

}  // namespace

extern "C" {

int smrf_terrain_rays_f32(const float* d_Z, int rows, int cols, int mode, const int* d_steps, const uint8_t* d_flags,
                          const double* d_dist, int nsteps, int max_step, const int* d_neighbors, int n_neighbors,
                          int dir_mask, double threshold, int options, const void* d_lut, void* d_out0, void* d_out1,
                          void* d_out2, int impl, void* stream) {
  return terrain_rays<float>(d_Z, rows, cols, mode, d_steps, d_flags, d_dist, nsteps, max_step, d_neighbors,
                             n_neighbors, dir_mask, threshold, options, d_lut, d_out0, d_out1, d_out2, impl, stream);
}

int smrf_terrain_rays_f64(const double* d_Z, int rows, int cols, int mode, const int* d_steps, const uint8_t* d_flags,
                          const double* d_dist, int nsteps, int max_step, const int* d_neighbors, int n_neighbors,
                          int dir_mask, double threshold, int options, const void* d_lut, void* d_out0, void* d_out1,
                          void* d_out2, int impl, void* stream) {
  return terrain_rays<double>(d_Z, rows, cols, mode, d_steps, d_flags, d_dist, nsteps, max_step, d_neighbors,
                              n_neighbors, dir_mask, threshold, options, d_lut, d_out0, d_out1, d_out2, impl, stream);
}

}  // extern "C"
