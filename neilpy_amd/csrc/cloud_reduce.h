// The bounds reduction of the point-cloud entry points: the box of a cloud's first BOX axes and what its bad coordinates
// do to it, in one pass.  create_dem's extent (grid.hip), the search grid of nearest_points (points.hip) and voxelize's
// histogram range (voxel.hip) bring a loader - `load(i, v)` puts the CHECK >= BOX coordinates of point i into v as
// doubles - and call cloud_bounds().
//
// Rule for a bad coordinate:
//   CLOUD_POISON  a NaN among the CHECK coordinates turns the whole box into NaN, as np.min / np.max do; +-inf is a value.
//   CLOUD_COUNT   NaN and +-inf among the CHECK coordinates are counted and the box is left alone (fmin / fmax skip a NaN,
//                 an infinity enters); the count is the last value of a partial row and goes to *h_nonfinite.
// A partial row holds (min, max) per box axis and then the count, if there is one: cloud_stride() values.
//
// The order of the reduction is part of the contract, because fmin(-0.0, +0.0) depends on it: smrf_blocks(n, CLOUD_PARTS)
// workgroups of 256 threads, a grid-stride loop, a 64-lane __shfl_down tree (offsets 32 .. 1), lane 0 of each of the four
// waves into LDS, thread 0 folding them as (w0, w1), (w2, w3), and the host folding the partial rows in workgroup order
// with std::min / std::max.  No float atomics.
#pragma once
#include <type_traits>

#include "smrf_common.h"

namespace smrf {

constexpr int CLOUD_PARTS = 1024;        // workgroups at most
constexpr int CLOUD_MAX_STRIDE = 7;      // three box axes and a count
enum CloudRule { CLOUD_POISON, CLOUD_COUNT };

constexpr int cloud_stride(int box, CloudRule rule) { return 2 * box + (rule == CLOUD_COUNT ? 1 : 0); }
constexpr size_t cloud_bytes(int box, CloudRule rule, int blocks) {
  return (size_t)blocks * cloud_stride(box, rule) * sizeof(double);
}

template <typename Load, int BOX, int CHECK, CloudRule RULE>
__global__ __launch_bounds__(256) void cloud_bounds_kernel(const Load load, long long n, double* __restrict__ part) {
  static_assert(1 <= BOX && BOX <= CHECK && cloud_stride(BOX, RULE) <= CLOUD_MAX_STRIDE);
  using Bad = std::conditional_t<RULE == CLOUD_POISON, int, unsigned long long>;   // a flag, or a count
  double lo[BOX], hi[BOX];
#pragma unroll
  for (int a = 0; a < BOX; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
  Bad bad = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    double v[CHECK];
    load(i, v);
#pragma unroll
    for (int a = 0; a < CHECK; ++a) {
      if constexpr (RULE == CLOUD_POISON) bad |= (v[a] != v[a]);
      else bad += !(fabs(v[a]) < INFINITY);
    }
#pragma unroll
    for (int a = 0; a < BOX; ++a) { lo[a] = fmin(lo[a], v[a]); hi[a] = fmax(hi[a], v[a]); }
  }
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < BOX; ++a) {
      lo[a] = fmin(lo[a], __shfl_down(lo[a], o, 64));
      hi[a] = fmax(hi[a], __shfl_down(hi[a], o, 64));
    }
    if constexpr (RULE == CLOUD_POISON) bad |= __shfl_down(bad, o, 64);
    else bad += __shfl_down(bad, o, 64);
  }
  __shared__ double s[2 * BOX][4];
  __shared__ Bad sbad[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < BOX; ++a) { s[2 * a][w] = lo[a]; s[2 * a + 1][w] = hi[a]; }
    sbad[w] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + (long long)blockIdx.x * cloud_stride(BOX, RULE);
    const bool poison = RULE == CLOUD_POISON && (sbad[0] | sbad[1] | sbad[2] | sbad[3]);
#pragma unroll
    for (int a = 0; a < BOX; ++a) {
      o[2 * a] = poison ? NAN : fmin(fmin(s[2 * a][0], s[2 * a][1]), fmin(s[2 * a][2], s[2 * a][3]));
      o[2 * a + 1] = poison ? NAN : fmax(fmax(s[2 * a + 1][0], s[2 * a + 1][1]), fmax(s[2 * a + 1][2], s[2 * a + 1][3]));
    }
    if constexpr (RULE == CLOUD_COUNT) o[2 * BOX] = (double)(sbad[0] + sbad[1] + sbad[2] + sbad[3]);   // < 2^53: exact
  }
}

// where the partial rows land on the host: one buffer per host thread, whatever the instantiation
inline double* cloud_host_rows() {
  static thread_local double rows[CLOUD_PARTS * CLOUD_MAX_STRIDE];
  return rows;
}

// h_box[2 * BOX] = (min, max) per axis of the n >= 1 points behind `load`; *h_nonfinite (CLOUD_COUNT only) = the count.
// `need` = the workspace the entry point demands, at least cloud_bytes(BOX, RULE, smrf_blocks(n, CLOUD_PARTS)); a call
// refused for it launches nothing and leaves the outputs alone.  Returns after the stream has been synchronised.
template <int BOX, int CHECK, CloudRule RULE, typename Load>
int cloud_bounds(const Load& load, long long n, double* h_box, int64_t* h_nonfinite, void* d_workspace,
                 size_t workspace_bytes, size_t need, hipStream_t stream) {
  constexpr int STRIDE = cloud_stride(BOX, RULE);
  const int blocks = smrf_blocks(n, CLOUD_PARTS);
  if (!d_workspace || workspace_bytes < need)
    return smrf_fail(SMRF_E_WORKSPACE, "bounds workspace of %zu bytes, %zu needed", workspace_bytes, need);
  double* part = (double*)d_workspace;
  hipLaunchKernelGGL((cloud_bounds_kernel<Load, BOX, CHECK, RULE>), dim3(blocks), dim3(256), 0, stream, load, n, part);
  SMRF_LAUNCH_CHECK();
  double* host = cloud_host_rows();
  SMRF_HIP_CHECK(hipMemcpyAsync(host, part, cloud_bytes(BOX, RULE, blocks), hipMemcpyDeviceToHost, stream));
  SMRF_HIP_CHECK(hipStreamSynchronize(stream));
  double r[2 * BOX], bad = 0.0;
  for (int a = 0; a < BOX; ++a) { r[2 * a] = INFINITY; r[2 * a + 1] = -INFINITY; }
  bool poison = false;
  for (int b = 0; b < blocks; ++b) {
    const double* p = host + b * STRIDE;
    for (int a = 0; a < BOX; ++a) {
      if (RULE == CLOUD_POISON) poison |= (p[2 * a] != p[2 * a]) | (p[2 * a + 1] != p[2 * a + 1]);
      r[2 * a] = std::min(r[2 * a], p[2 * a]);
      r[2 * a + 1] = std::max(r[2 * a + 1], p[2 * a + 1]);
    }
    if (RULE == CLOUD_COUNT) bad += p[2 * BOX];
  }
  for (int k = 0; k < 2 * BOX; ++k) h_box[k] = poison ? NAN : r[k];
  if (RULE == CLOUD_COUNT) *h_nonfinite = (int64_t)bad;
  return SMRF_OK;
}

}  // namespace smrf
