// A point cloud as a boolean voxel model (voxelize; the reference's voxelize at neilpy.py:195 subtracts the minima, bins the
// cloud with np.histogramdd, thresholds the counts, fills every column below its lowest occupied voxel and pads the
// bottom).  DESIGN.md section 15 is the contract.
//
//   bounds    cloud_reduce.h over XyzLoad: minimum and maximum per axis and the number of non-finite coordinates of the
//             three coordinate arrays, one reduction; the host finishes the per-workgroup partials.  No float atomics.
//   mark      voxel_mark_kernel: d = v - min, one rounded subtraction in the cloud's dtype; the bin of d on each axis by
//             np.histogramdd's rule, settled against the float64 edges the caller uploaded (voxel_bin()); then
//               threshold == 1  a bit set, one 32-bit word per 32 z-cells, [x][y][word]: the word is loaded and the
//                               atomic OR issued only when the bit is still clear.  A stale load costs a second atomic,
//                               never a bit: nothing clears a bit while the kernel runs.
//               threshold  > 1  uint32 counts [x][y][z] with integer atomic adds: the order of arrival decides nothing.
//   lowest    voxel_lowest_kernel: the lowest occupied cell of every (x, y) column, nz for a column with none.
//   expand    voxel_expand_kernel: the bool bytes [x][y][nz + pad] as one flat stream of aligned dwords.  A lane builds
//             the four bytes of its dword in a register and stores it once; consecutive lanes hold consecutive dwords.
//             Column and level of a workgroup's first byte come from one 64-bit division per workgroup, a lane's from
//             one 32-bit division per dword, a byte's from an increment.  Below a column's lowest occupied cell the
//             workspace is not read: those cells are the fill, or empty.
//
// All flat indices are 64-bit.
#include <climits>
#include <cmath>

#include "cloud_reduce.h"

namespace smrf {

constexpr int VX_TILE_DWORDS = 1024;     // dwords of the output one workgroup of the expand kernel writes: 256 lanes x 4
static_assert(cloud_bytes(3, CLOUD_COUNT, CLOUD_PARTS) == SMRF_VOXEL_BOUNDS_BYTES, "smrf_hip.h");

struct VoxelWs {
  unsigned* marks;   // threshold == 1: [nx * ny * ceil(nz / 32)] words; else [nx * ny * nz] counts
  int* low;          // [nx * ny] lowest occupied cell of the column, nz when it has none
};

inline long long vx_words(int nz) { return ((long long)nz + 31) / 32; }

// 0 when the volume is out of range.  Limits: every extent and the number of columns fit an int, and the flat byte index,
// the entries of the workspace and the kernels' workgroup counts stay far inside 64 / 31 bits.
inline size_t voxel_layout(int nx, int ny, int nz, int threshold, char* base, VoxelWs* w) {
  if (nx < 0 || ny < 0 || nz < 0 || threshold < 1) return 0;
  const long long cols = (long long)nx * ny;
  const long long per = threshold == 1 ? vx_words(nz) : (long long)nz;
  if (cols > (long long)INT_MAX || cols > (1ll << 40) || (per > 0 && cols > (1ll << 40) / per)) return 0;
  const size_t marks = smrf_up256((size_t)(cols * per) * 4);
  if (w) *w = VoxelWs{(unsigned*)base, (int*)(base + marks)};
  return marks + smrf_up256((size_t)cols * 4) + 256;      // never 0 for a volume in range, an empty one included
}

// ---------------------------------------------------------------------------------------------------------------
// bounds
// ---------------------------------------------------------------------------------------------------------------
// float32 widens to float64 exactly, so cloud_reduce.h's one reduction in float64 serves both dtypes (CLOUD_COUNT)
template <typename T>
struct XyzLoad {
  const T *x, *y, *z;
  __device__ void operator()(long long i, double* v) const { v[0] = (double)x[i]; v[1] = (double)y[i]; v[2] = (double)z[i]; }
};

// ---------------------------------------------------------------------------------------------------------------
// mark
// ---------------------------------------------------------------------------------------------------------------
// one axis of the histogram: nb bins between the nb + 1 non-decreasing edges e[0..nb]; e0 = e[0], en = e[nb], and
// scale = nb / (en - e0) only serves the guess
struct VoxelAxis {
  const double* e;
  double e0, en, scale;
  int nb;
};

// np.histogramdd's bin of d: searchsorted(e, d, side='right') - 1, a sample equal to the last edge in the last bin, -1
// for a sample below the first edge or above the last (or a NaN).  The division only guesses; the walk along the edges
// decides, so the result is right for any non-decreasing edges - and one or two steps away from the guess for evenly
// spaced ones.
__device__ __forceinline__ int voxel_bin(const VoxelAxis& ax, double d) {
  if (!(d >= ax.e0) || !(d <= ax.en)) return -1;
  const double g = (d - ax.e0) * ax.scale;                 // NaN for a zero-width histogram: bin 0 below
  int i = !(g >= 0.0) ? 0 : (g >= (double)ax.nb ? ax.nb - 1 : (int)g);
  while (i > 0 && d < ax.e[i]) --i;                        // now e[i] <= d (e[0] <= d was tested)
  while (i < ax.nb - 1 && d >= ax.e[i + 1]) ++i;           // the last such i short of nb: d == e[nb] stays in bin nb - 1
  return i;
}

__device__ __forceinline__ VoxelAxis voxel_axis(const double* __restrict__ e, int nb) {
  const double e0 = e[0], en = e[nb];
  return VoxelAxis{e, e0, en, (double)nb / (en - e0), nb};
}

template <typename T, bool COUNTS>
__global__ __launch_bounds__(256) void voxel_mark_kernel(const T* __restrict__ x, const T* __restrict__ y,
                                                         const T* __restrict__ z, long long n, T ox, T oy, T oz,
                                                         const double* __restrict__ xe, const double* __restrict__ ye,
                                                         const double* __restrict__ ze, int nx, int ny, int nz,
                                                         unsigned* marks) {
  const VoxelAxis ax = voxel_axis(xe, nx), ay = voxel_axis(ye, ny), az = voxel_axis(ze, nz);
  const long long per = COUNTS ? (long long)nz : ((long long)nz + 31) >> 5;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int ix = voxel_bin(ax, (double)(x[i] - ox));
    const int iy = voxel_bin(ay, (double)(y[i] - oy));
    const int iz = voxel_bin(az, (double)(z[i] - oz));
    if ((ix | iy | iz) < 0) continue;                      // histogramdd drops the sample
    const long long col = (long long)ix * ny + iy;
    if (COUNTS) {
      atomicAdd(&marks[col * per + iz], 1u);
    } else {
      unsigned* w = &marks[col * per + (iz >> 5)];
      const unsigned bit = 1u << (iz & 31);
      // an agent-scope load: answered by the L2, where the atomics of every CU land, not by this CU's own L1 copy
      if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// lowest occupied cell per column
// ---------------------------------------------------------------------------------------------------------------
// bit set: one thread per column walks its words upward (a column is a few words: neighbouring lanes read neighbouring
// words).  counts: one wave per column, 64 consecutive counts per step, the first lane that meets the threshold found by
// ballot - a thread of its own per column would read 4 B out of every row of nz counts.
template <bool COUNTS>
__global__ __launch_bounds__(256) void voxel_lowest_kernel(const unsigned* __restrict__ marks, long long cols, int nz,
                                                           unsigned threshold, int* __restrict__ low) {
  if (COUNTS) {
    const long long c = blockIdx.x * 4ll + (threadIdx.x >> 6);       // wave-uniform
    const int lane = threadIdx.x & 63;
    if (c >= cols) return;
    const unsigned* p = marks + c * nz;
    int at = nz;
    for (int k0 = 0; k0 < nz; k0 += 64) {
      const int k = k0 + lane;
      const unsigned long long hit = __ballot(k < nz && p[k] >= threshold);
      if (hit) {
        at = k0 + __builtin_ctzll(hit);
        break;
      }
    }
    if (lane == 0) low[c] = at;
  } else {
    const long long c = blockIdx.x * 256ll + threadIdx.x;
    if (c >= cols) return;
    const int words = (int)(((long long)nz + 31) >> 5);
    const unsigned* p = marks + c * words;
    int at = nz;
    for (int k = 0; k < words; ++k) {
      const unsigned v = p[k];
      if (v) {
        at = k * 32 + __builtin_ctz(v);
        break;
      }
    }
    low[c] = at;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// expand
// ---------------------------------------------------------------------------------------------------------------
// out[(c * L + l)] for column c and level l of L = nz + pad: 1 for l < pad; with k = l - pad, 1 for an occupied cell k,
// and with `fill` for k below the lowest occupied cell of a column that has one.  total = cols * L bytes; a last dword
// that reaches past total is stored byte by byte.
template <bool COUNTS>
__global__ __launch_bounds__(256) void voxel_expand_kernel(const unsigned* __restrict__ marks,
                                                           const int* __restrict__ low, int nz, int pad,
                                                           unsigned threshold, int fill, long long total,
                                                           uint8_t* __restrict__ out) {
  const unsigned L = (unsigned)nz + (unsigned)pad;         // 1 <= L <= INT_MAX (checked by the host)
  const long long per = COUNTS ? (long long)nz : ((long long)nz + 31) >> 5;
  __shared__ long long s_col;
  __shared__ unsigned s_lev;
  if (threadIdx.x == 0) {
    const unsigned long long b = (unsigned long long)blockIdx.x * (VX_TILE_DWORDS * 4ull);
    s_col = (long long)(b / L);
    s_lev = (unsigned)(b % L);
  }
  __syncthreads();
  const long long col0 = s_col;
  const unsigned lev0 = s_lev;
#pragma unroll
  for (int j = 0; j < VX_TILE_DWORDS / 256; ++j) {
    const unsigned dw = (unsigned)j * 256u + threadIdx.x;
    const long long byte0 = ((long long)blockIdx.x * VX_TILE_DWORDS + dw) * 4;
    if (byte0 >= total) break;
    const unsigned off = lev0 + dw * 4u;                   // < 2^31 + 4096
    long long c = col0 + off / L;
    unsigned l = off % L;
    long long have_c = -1, have_w = -1;                    // the column whose `low`, the word whose bits are in registers
    int lo = 0;
    unsigned word = 0, v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned bit = 0;
      if (byte0 + k < total) {
        if (l < (unsigned)pad) {
          bit = 1;
        } else {
          const int cell = (int)(l - (unsigned)pad);
          if (have_c != c) {
            have_c = c;
            lo = low[c];
          }
          if (cell < lo) {
            bit = (fill && lo < nz) ? 1u : 0u;
          } else {
            const long long at = c * per + (COUNTS ? cell : (cell >> 5));
            if (have_w != at) {
              have_w = at;
              word = marks[at];
            }
            bit = COUNTS ? (word >= threshold ? 1u : 0u) : ((word >> (cell & 31)) & 1u);
          }
        }
      }
      v |= bit << (8 * k);
      if (++l == L) {
        l = 0;
        ++c;
      }
    }
    if (byte0 + 4 <= total) {
      *reinterpret_cast<unsigned*>(out + byte0) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (byte0 + k < total) out[byte0 + k] = (uint8_t)(v >> (8 * k));
    }
  }
}

template <typename T>
int voxel_bounds(const T* d_x, const T* d_y, const T* d_z, int64_t n, double* h_box, int64_t* h_nonfinite,
                 void* d_workspace, size_t workspace_bytes, hipStream_t stream) {
  if (n < 1 || n > (int64_t)INT_MAX) return smrf_fail(SMRF_E_ARG, "%lld points: 1 to 2^31 - 1 expected", (long long)n);
  if (!d_x || !d_y || !d_z || !h_box || !h_nonfinite) return smrf_fail(SMRF_E_ARG, "null pointer");
  return cloud_bounds<3, 3, CLOUD_COUNT>(XyzLoad<T>{d_x, d_y, d_z}, n, h_box, h_nonfinite, d_workspace, workspace_bytes,
                                         (size_t)SMRF_VOXEL_BOUNDS_BYTES, stream);
}

template <typename T>
int voxel_mark(const T* d_x, const T* d_y, const T* d_z, int64_t n, const double* h_offsets, const double* d_xedges,
               const double* d_yedges, const double* d_zedges, int nx, int ny, int nz, int threshold, void* d_workspace,
               size_t workspace_bytes, hipStream_t stream) {
  if (n < 1 || n > (int64_t)INT_MAX) return smrf_fail(SMRF_E_ARG, "%lld points: 1 to 2^31 - 1 expected", (long long)n);
  if (!d_x || !d_y || !d_z || !h_offsets || !d_xedges || !d_yedges || !d_zedges) return smrf_fail(SMRF_E_ARG, "null pointer");
  const size_t need = voxel_layout(nx, ny, nz, threshold, nullptr, nullptr);
  if (!need) return smrf_fail(SMRF_E_ARG, "a volume of %d x %d x %d voxels at threshold %d is out of range", nx, ny, nz, threshold);
  if (!d_workspace || workspace_bytes < need)
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  VoxelWs w;
  voxel_layout(nx, ny, nz, threshold, (char*)d_workspace, &w);
  if (nx == 0 || ny == 0 || nz == 0) return SMRF_OK;       // no bins: every sample is dropped
  const long long entries = (long long)nx * ny * (threshold == 1 ? vx_words(nz) : (long long)nz);
  SMRF_HIP_CHECK(hipMemsetAsync(w.marks, 0, (size_t)entries * 4, stream));
  const int blocks = smrf_blocks(n, 16384);
  const T ox = (T)h_offsets[0], oy = (T)h_offsets[1], oz = (T)h_offsets[2];
  if (threshold == 1)
    hipLaunchKernelGGL((voxel_mark_kernel<T, false>), dim3(blocks), dim3(256), 0, stream, d_x, d_y, d_z, (long long)n, ox,
                       oy, oz, d_xedges, d_yedges, d_zedges, nx, ny, nz, w.marks);
  else
    hipLaunchKernelGGL((voxel_mark_kernel<T, true>), dim3(blocks), dim3(256), 0, stream, d_x, d_y, d_z, (long long)n, ox,
                       oy, oz, d_xedges, d_yedges, d_zedges, nx, ny, nz, w.marks);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // namespace smrf

extern "C" {

size_t smrf_voxel_workspace_bytes(int nx, int ny, int nz, int threshold) {
  return smrf::voxel_layout(nx, ny, nz, threshold, nullptr, nullptr);
}

int smrf_voxel_bounds_f32(const float* d_x, const float* d_y, const float* d_z, int64_t npoints, double* h_box,
                          int64_t* h_nonfinite, void* d_workspace, size_t workspace_bytes, void* stream) {
  return smrf::voxel_bounds(d_x, d_y, d_z, npoints, h_box, h_nonfinite, d_workspace, workspace_bytes, (hipStream_t)stream);
}

int smrf_voxel_bounds_f64(const double* d_x, const double* d_y, const double* d_z, int64_t npoints, double* h_box,
                          int64_t* h_nonfinite, void* d_workspace, size_t workspace_bytes, void* stream) {
  return smrf::voxel_bounds(d_x, d_y, d_z, npoints, h_box, h_nonfinite, d_workspace, workspace_bytes, (hipStream_t)stream);
}

int smrf_voxel_mark_f32(const float* d_x, const float* d_y, const float* d_z, int64_t npoints, const double* h_offsets,
                        const double* d_xedges, const double* d_yedges, const double* d_zedges, int nx, int ny, int nz,
                        int threshold, void* d_workspace, size_t workspace_bytes, void* stream) {
  return smrf::voxel_mark(d_x, d_y, d_z, npoints, h_offsets, d_xedges, d_yedges, d_zedges, nx, ny, nz, threshold,
                          d_workspace, workspace_bytes, (hipStream_t)stream);
}

int smrf_voxel_mark_f64(const double* d_x, const double* d_y, const double* d_z, int64_t npoints, const double* h_offsets,
                        const double* d_xedges, const double* d_yedges, const double* d_zedges, int nx, int ny, int nz,
                        int threshold, void* d_workspace, size_t workspace_bytes, void* stream) {
  return smrf::voxel_mark(d_x, d_y, d_z, npoints, h_offsets, d_xedges, d_yedges, d_zedges, nx, ny, nz, threshold,
                          d_workspace, workspace_bytes, (hipStream_t)stream);
}

int smrf_voxel_expand(void* d_workspace, size_t workspace_bytes, int nx, int ny, int nz, int threshold, int bottom_fill,
                      int pad, uint8_t* d_out, void* stream_) {
  using namespace smrf;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t need = voxel_layout(nx, ny, nz, threshold, nullptr, nullptr);
  if (!need) return smrf_fail(SMRF_E_ARG, "a volume of %d x %d x %d voxels at threshold %d is out of range", nx, ny, nz, threshold);
  if (pad < 0 || (long long)nz + pad > INT_MAX) return smrf_fail(SMRF_E_ARG, "pad %d on %d levels", pad, nz);
  if (!d_workspace || workspace_bytes < need)
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const long long cols = (long long)nx * ny, L = (long long)nz + pad;
  if (cols == 0 || L == 0) return SMRF_OK;                 // an empty result
  if (cols > (1ll << 42) / L) return smrf_fail(SMRF_E_ARG, "%lld columns of %lld levels: more than 2^42 voxels", cols, L);
  if (!d_out || ((uintptr_t)d_out & 3)) return smrf_fail(SMRF_E_ARG, "d_out must be a 4-byte aligned device pointer");
  VoxelWs w;
  voxel_layout(nx, ny, nz, threshold, (char*)d_workspace, &w);
  const long long total = cols * L;
  const dim3 cgrid((unsigned)(threshold == 1 ? (cols + 255) / 256 : (cols + 3) / 4));
  const dim3 egrid((unsigned)((total + VX_TILE_DWORDS * 4 - 1) / (VX_TILE_DWORDS * 4)));
  if (threshold == 1) {
    hipLaunchKernelGGL(voxel_lowest_kernel<false>, cgrid, dim3(256), 0, stream, w.marks, cols, nz, 1u, w.low);
    SMRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(voxel_expand_kernel<false>, egrid, dim3(256), 0, stream, w.marks, w.low, nz, pad, 1u,
                       bottom_fill ? 1 : 0, total, d_out);
  } else {
    hipLaunchKernelGGL(voxel_lowest_kernel<true>, cgrid, dim3(256), 0, stream, w.marks, cols, nz, (unsigned)threshold, w.low);
    SMRF_LAUNCH_CHECK();
    hipLaunchKernelGGL(voxel_expand_kernel<true>, egrid, dim3(256), 0, stream, w.marks, w.low, nz, pad,
                       (unsigned)threshold, bottom_fill ? 1 : 0, total, d_out);
  }
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // extern "C"
