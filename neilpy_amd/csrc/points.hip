// Nearest point of one cloud for every point of another (nearest_points, chamfer_distance; the reference's
// chamfer_distance at neilpy.py:2679 asks a KD-tree): a counting sort of the cloud into a uniform grid of square cells and
// one search kernel.  DESIGN.md section 14 is the contract.
//
//   bounds    cloud_reduce.h over RowLoad: box of the two planar axes and the number of non-finite coordinates.
//   grid      points_grid(): a square cell sized for about two points per cell over the box of axes 0 and 1.  The grid
//             has two axes whatever the dimension, so a 2.5-D lidar cloud does not make a mostly empty lattice; the third
//             coordinate only enters the distance.
//   sort      points_count_kernel (one atomic per point), a three-launch exclusive scan, points_scatter_kernel: rows and
//             coordinates in cell order (row-major cells), so the cells ix0..ix1 of one grid row are ONE run of points.
//             The order inside a cell is whatever the atomics gave; no result depends on it (see the tie rule).
//   search    points_search_kernel: one thread per query point walks square rings of cells around the query's cell.
//   sum       points_sum_kernel x 2: float64 sum in a fixed order, no float atomics.
//
// The distance is sqrt(((q0-p0)*(q0-p0) + (q1-p1)*(q1-p1)) [+ (q2-p2)*(q2-p2)]) in float64, each operation rounded
// (__dmul_rn / __dadd_rn: no FMA whatever the flags).  The winner is the lowest (distance, row) in that order - the
// rounded distance, as numpy.argmin over the distances decides - so the result is a function of the inputs alone.
//
// The search is exact because of three rules.
//   1. A side of a ring (and with it the ring) is skipped only on a LOWER bound of the squared distance from the query to
//      any point sorted into that side's cells, taken from the cell edge x0 + i * cell that faces the query, not from
//      k * cell.  cell_of() is monotone in the coordinate, and a point with cell index >= i has coordinate
//      >= x0 + i * cell * (1 - 2u) (u = 2^-53; <= the mirrored bound on the other side), so edge_gap2() takes the rounded
//      edge distance and subtracts 2^-48 of the magnitudes that went into it: rounding can make the bound smaller, never
//      larger.  Squared values are compared.
//   2. The stop test is strict: a side is searched unless its bound is > the largest squared distance that could still
//      win or tie (`hi`, see Best::take).  A cell whose bound equals the best so far is searched, or the lowest-row rule
//      would fail across cell borders.
//   3. A cell index is floor((coord - origin) / cell) clamped to [0, n - 1] AFTER the floor, by comparisons on the double
//      (cell_of()): a point on the box's upper edge, a zero-extent axis (n = 1) and a query outside the box land in a
//      valid cell; a cloud of equal points gets cell = 1 and a 1 x 1 grid, nothing divides by zero.
// The ring count is bounded by the larger grid dimension, so the loop ends for any query.
#include <climits>
#include <cmath>

#include "cloud_reduce.h"

namespace smrf {

constexpr int PN_SCAN = 2048;        // cell counts per workgroup of the scan: 256 threads x 8
constexpr int PN_PARTS = CLOUD_PARTS;   // workgroups of the bounds and of the sum reduction at most
constexpr long long PN_MAX_POINTS = 1ll << 30;   // rows are int32 and cell indices fit int32

struct PointsGrid {
  double x0, y0, cell;   // origin = the box's minimum corner; cell > 0 (may be +inf: then nx = ny = 1)
  int nx, ny;
};

// most cells points_grid() makes for n points: (ex / cell + 1) (ey / cell + 1) <= T + 2T + 1 with T = max(1, n / 2)
inline long long points_cells_cap(long long n) { return 3 * std::max<long long>(1, n / 2) + 4; }

// box = (min0, max0, min1, max1), finite.  Host code, shared by the build and the search.
inline PointsGrid points_grid(const double* box, long long n) {
  PointsGrid g{box[0], box[2], 1.0, 1, 1};
  const double ex = box[1] - box[0], ey = box[3] - box[2];
  const double m = std::max(ex, ey);
  if (!(m > 0.0)) return g;                            // all points equal in the plane
  const long long T = std::max<long long>(1, n / 2);   // about two points per cell
  // square cells over the box; never more than T + 1 along an axis (a thin box, or a line: ex * ey = 0)
  double cell = std::max(std::sqrt(ex * ey / (double)T), m / (double)T);
  if (!(cell > 0.0)) cell = m;                         // m / T underflowed
  for (;;) {
    const double fx = std::floor(ex / cell), fy = std::floor(ey / cell);   // <= T up to rounding, or 0 for cell = inf
    const long long nx = (long long)std::min(fx, (double)T) + 1, ny = (long long)std::min(fy, (double)T) + 1;
    if (nx * ny <= points_cells_cap(n)) {
      g.cell = cell;
      g.nx = (int)nx;
      g.ny = (int)ny;
      return g;
    }
    cell *= 2.0;                                       // not reached by the bound above; keeps the workspace promise
  }
}

// rule 3
__host__ __device__ inline int cell_of(double v, double origin, double cell, int n) {
  const double t = floor((v - origin) / cell);
  if (!(t >= 0.0)) return 0;
  return t >= (double)n ? n - 1 : (int)t;
}

struct PointsWs {
  double* part;      // [PN_PARTS * 5] partials of the bounds and of the sum
  unsigned* start;   // [cells + 1] first sorted slot of a cell
  unsigned* cnt;     // [cells]     points per cell; counted down to 0 by the scatter
  unsigned* bsum;    // [ceil(cells / PN_SCAN)]
  int* rows;         // [n]         row of the point in slot s
  double* sorted;    // [n * dim]   its coordinates
};

// the same offsets for every call with the same (n, dim): the search finds what the build left
inline size_t points_layout(long long n, int dim, char* base, PointsWs* w) {
  const size_t cap = (size_t)points_cells_cap(n);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += smrf_up256(bytes);
    return p;
  };
  double* part = (double*)take(cloud_bytes(2, CLOUD_COUNT, PN_PARTS));
  unsigned* start = (unsigned*)take((cap + 1) * 4);
  unsigned* cnt = (unsigned*)take(cap * 4);
  unsigned* bsum = (unsigned*)take(((cap + PN_SCAN - 1) / PN_SCAN) * 4);
  int* rows = (int*)take((size_t)n * 4);
  double* sorted = (double*)take((size_t)n * dim * sizeof(double));
  if (w) *w = PointsWs{part, start, cnt, bsum, rows, sorted};
  return off;
}

// ---------------------------------------------------------------------------------------------------------------
// bounds: box of axes 0 and 1, count of non-finite coordinates over all axes, inf included, so the caller can refuse
// the cloud (cloud_reduce.h, CLOUD_COUNT); this is how a row of DIM doubles is read
// ---------------------------------------------------------------------------------------------------------------
template <int DIM>
struct RowLoad {
  const double* p;
  __device__ void operator()(long long i, double* v) const {
    const double* q = p + i * DIM;
#pragma unroll
    for (int a = 0; a < DIM; ++a) v[a] = q[a];
  }
};

// ---------------------------------------------------------------------------------------------------------------
// counting sort into cell order
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long point_cell(const double* q, const PointsGrid& g) {
  return (long long)cell_of(q[1], g.y0, g.cell, g.ny) * g.nx + cell_of(q[0], g.x0, g.cell, g.nx);
}

__global__ __launch_bounds__(256) void points_count_kernel(const double* __restrict__ p, long long n, int dim,
                                                           PointsGrid g, unsigned* __restrict__ cnt) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    atomicAdd(&cnt[point_cell(p + i * dim, g)], 1u);
}

// exclusive scan of one value per thread over the 256 threads of a workgroup; total = their sum
__device__ __forceinline__ unsigned pn_block_scan(unsigned v, unsigned& total) {
  __shared__ unsigned wsum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                       // the previous call's wsum has been read
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned before = 0;
  for (int j = 0; j < w; ++j) before += wsum[j];
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return before + inc - v;
}

__global__ __launch_bounds__(256) void points_scan_sums_kernel(const unsigned* __restrict__ cnt, long long cells,
                                                               unsigned* __restrict__ bsum) {
  const long long i0 = (long long)blockIdx.x * PN_SCAN + threadIdx.x * 8;
  unsigned v = 0;
  for (int j = 0; j < 8; ++j)
    if (i0 + j < cells) v += cnt[i0 + j];
  unsigned total;
  pn_block_scan(v, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum becomes its own exclusive scan
__global__ __launch_bounds__(256) void points_scan_blocks_kernel(unsigned* __restrict__ bsum, long long nb) {
  unsigned carry = 0;
  for (long long i0 = 0; i0 < nb; i0 += 256) {
    const long long i = i0 + threadIdx.x;
    const unsigned v = i < nb ? bsum[i] : 0u;
    unsigned total;
    const unsigned ex = pn_block_scan(v, total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(256) void points_scan_apply_kernel(const unsigned* __restrict__ cnt, long long cells,
                                                                const unsigned* __restrict__ bsum,
                                                                unsigned* __restrict__ start, unsigned n) {
  const long long i0 = (long long)blockIdx.x * PN_SCAN + threadIdx.x * 8;
  unsigned c[8], v = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = i0 + j < cells ? cnt[i0 + j] : 0u;
    v += c[j];
  }
  unsigned total;
  unsigned at = bsum[blockIdx.x] + pn_block_scan(v, total);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (i0 + j < cells) start[i0 + j] = at;
    at += c[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) start[cells] = n;
}

__global__ __launch_bounds__(256) void points_scatter_kernel(const double* __restrict__ p, long long n, int dim,
                                                             PointsGrid g, const unsigned* __restrict__ start,
                                                             unsigned* __restrict__ cnt, int* __restrict__ rows,
                                                             double* __restrict__ sorted) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double* q = p + i * dim;
    const long long c = point_cell(q, g);
    const long long s = (long long)start[c] + (atomicSub(&cnt[c], 1u) - 1u);   // the cell's slots, last first
    rows[s] = (int)i;
    double* o = sorted + s * dim;
    o[0] = q[0];
    o[1] = q[1];
    if (dim == 3) o[2] = q[2];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// search
// ---------------------------------------------------------------------------------------------------------------
// Rule 1.  Lower bound of the squared distance, along one planar axis, from coordinate qv to any point whose cell index
// on that axis is >= i (toward = +1: the points lie at >= origin + i * cell up to rounding) or < i (toward = -1: at
// < origin + i * cell up to rounding).  The rounded gap errs by less than 6u of the magnitudes summed below; 2^-48 = 32u
// of them is taken off, and what is left is also below the rounded |q - p| of every such point, so its rounded square
// is <= the rounded squared distance the kernel computes for the point.  0 when the query is not clear of the edge.
__device__ __forceinline__ double edge_gap2(double origin, double cell, int i, double qv, int toward) {
  const double ic = __dmul_rn((double)i, cell);
  const double e = __dadd_rn(origin, ic);
  double gap = toward > 0 ? e - qv : qv - e;
  gap -= 0x1p-48 * (fabs(origin) + ic + fabs(qv));
  return gap > 0.0 ? __dmul_rn(gap, gap) : 0.0;
}

// the lowest (rounded distance, row) so far.  hi: every squared distance whose rounded root is <= dist is <= hi
// (sqrt_rn(x) <= s needs x <= s^2 (1 + u)^2; hi = rn(s * s) (1 + 8u) + a few subnormal steps), so `d2 <= hi` loses no
// candidate that could win or tie, and `bound > hi` is the strict stop test of rule 2.
struct Best {
  double dist, hi;
  int row;
  __device__ __forceinline__ void take(double d2, int r) {
    if (!(d2 <= hi)) return;
    const double s = __dsqrt_rn(d2);
    if (s < dist || (s == dist && r < row)) {
      dist = s;
      row = r;
      hi = __dmul_rn(__dmul_rn(s, s), 1.0 + 0x1p-50) + 0x1p-1070;
    }
  }
};

template <int DIM>
__global__ __launch_bounds__(256) void points_search_kernel(const double* __restrict__ query, long long nq, PointsGrid g,
                                                            const unsigned* __restrict__ start,
                                                            const int* __restrict__ rows,
                                                            const double* __restrict__ sorted,
                                                            double* __restrict__ dist, long long* __restrict__ index) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= nq) return;
  const double q0 = query[i * DIM], q1 = query[i * DIM + 1];
  double q2 = 0.0;
  if (DIM == 3) q2 = query[i * DIM + 2];
  const int jx = cell_of(q0, g.x0, g.cell, g.nx), jy = cell_of(q1, g.y0, g.cell, g.ny);
  Best best{INFINITY, INFINITY, INT_MAX};

  // the points of the cells (ix0..ix1, iy): one run of the sorted arrays
  auto scan = [&](int iy, int ix0, int ix1) {
    const long long c = (long long)iy * g.nx;
    const unsigned s1 = start[c + ix1 + 1];
    for (unsigned s = start[c + ix0]; s < s1; ++s) {
      const double* p = sorted + (long long)s * DIM;
      const double d0 = q0 - p[0], d1 = q1 - p[1];
      double d2 = __dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1));
      if (DIM == 3) {
        const double dz = q2 - p[2];
        d2 = __dadd_rn(d2, __dmul_rn(dz, dz));
      }
      best.take(d2, rows[s]);
    }
  };

  scan(jy, jx, jx);
  const int kmax = max(max(jx, g.nx - 1 - jx), max(jy, g.ny - 1 - jy));
  for (int k = 1; k <= kmax; ++k) {
    const int xl = jx - k, xr = jx + k, yt = jy - k, yb = jy + k;
    // Every unvisited cell lies in column <= xl, column >= xr, row <= yt or row >= yb.  A side that is off the grid or
    // whose bound is beyond hi holds nothing for this ring or any later one: the bounds grow with k, hi only shrinks.
    const bool left = xl >= 0 && !(edge_gap2(g.x0, g.cell, xl + 1, q0, -1) > best.hi);
    const bool right = xr < g.nx && !(edge_gap2(g.x0, g.cell, xr, q0, +1) > best.hi);
    const bool top = yt >= 0 && !(edge_gap2(g.y0, g.cell, yt + 1, q1, -1) > best.hi);
    const bool bottom = yb < g.ny && !(edge_gap2(g.y0, g.cell, yb, q1, +1) > best.hi);
    if (!(left || right || top || bottom)) break;
    const int cx0 = max(xl, 0), cx1 = min(xr, g.nx - 1);
    const int cy0 = max(yt + 1, 0), cy1 = min(yb - 1, g.ny - 1);
    if (top) scan(yt, cx0, cx1);
    if (bottom) scan(yb, cx0, cx1);
    if (left)
      for (int iy = cy0; iy <= cy1; ++iy) scan(iy, xl, xl);
    if (right)
      for (int iy = cy0; iy <= cy1; ++iy) scan(iy, xr, xr);
  }
  if (dist) dist[i] = best.dist;
  if (index) index[i] = best.row;
}

// ---------------------------------------------------------------------------------------------------------------
// ordered sum: thread t of workgroup b adds x[(b + j * blocks) * 256 + t], j = 0, 1, ... in that order; the 256 sums go
// through a binary tree in LDS; one workgroup adds the partials the same way.  blocks depends on n only.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pn_tree_sum(double v) {
  __shared__ double t[256];
  t[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) t[threadIdx.x] = __dadd_rn(t[threadIdx.x], t[threadIdx.x + o]);
    __syncthreads();
  }
  return t[0];
}

__global__ __launch_bounds__(256) void points_sum_kernel(const double* __restrict__ x, long long n,
                                                         double* __restrict__ out) {
  double v = 0.0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) v = __dadd_rn(v, x[i]);
  v = pn_tree_sum(v);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

inline int points_args(long long n, int dim) {
  if (dim < 2 || dim > 3) return smrf_fail(SMRF_E_ARG, "points of dimension %d: 2 or 3 expected", dim);
  if (n < 1 || n > PN_MAX_POINTS) return smrf_fail(SMRF_E_ARG, "%lld points: 1 to %lld expected", n, PN_MAX_POINTS);
  return SMRF_OK;
}

}  // namespace smrf

extern "C" {

size_t smrf_points_nn_workspace_bytes(int64_t npoints, int dim) {
  if (npoints < 1 || npoints > smrf::PN_MAX_POINTS || dim < 2 || dim > 3) return 0;
  return smrf::points_layout(npoints, dim, nullptr, nullptr);
}

int smrf_points_nn_bounds_f64(const double* d_points, int64_t npoints, int dim, double* h_box, int64_t* h_nonfinite,
                              void* d_workspace, size_t workspace_bytes, void* stream_) {
  using namespace smrf;
  hipStream_t stream = (hipStream_t)stream_;
  if (dim < 2 || dim > 3 || npoints < 1) return smrf_fail(SMRF_E_ARG, "bounds of %lld points of dimension %d", (long long)npoints, dim);
  if (!d_points || !h_box || !h_nonfinite) return smrf_fail(SMRF_E_ARG, "null pointer");
  const size_t need = cloud_bytes(2, CLOUD_COUNT, PN_PARTS);
  if (dim == 2)
    return cloud_bounds<2, 2, CLOUD_COUNT>(RowLoad<2>{d_points}, npoints, h_box, h_nonfinite, d_workspace, workspace_bytes,
                                           need, stream);
  return cloud_bounds<2, 3, CLOUD_COUNT>(RowLoad<3>{d_points}, npoints, h_box, h_nonfinite, d_workspace, workspace_bytes,
                                         need, stream);
}

int smrf_points_nn_build_f64(const double* d_points, int64_t npoints, int dim, const double* h_box, void* d_workspace,
                             size_t workspace_bytes, void* stream_) {
  using namespace smrf;
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = points_args(npoints, dim)) return rc;
  if (!d_points || !h_box) return smrf_fail(SMRF_E_ARG, "null pointer");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(h_box[k])) return smrf_fail(SMRF_E_ARG, "the box of the points is not finite");
  if (!d_workspace || workspace_bytes < points_layout(npoints, dim, nullptr, nullptr))
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes,
                     points_layout(npoints, dim, nullptr, nullptr));
  PointsWs w;
  points_layout(npoints, dim, (char*)d_workspace, &w);
  const PointsGrid g = points_grid(h_box, npoints);
  const long long cells = (long long)g.nx * g.ny, nb = (cells + PN_SCAN - 1) / PN_SCAN;
  const int blocks = smrf_blocks(npoints, 8192);
  SMRF_HIP_CHECK(hipMemsetAsync(w.cnt, 0, (size_t)cells * 4, stream));
  hipLaunchKernelGGL(points_count_kernel, dim3(blocks), dim3(256), 0, stream, d_points, (long long)npoints, dim, g, w.cnt);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(points_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, stream, w.cnt, cells, w.bsum);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(points_scan_blocks_kernel, dim3(1), dim3(256), 0, stream, w.bsum, nb);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(points_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, stream, w.cnt, cells, w.bsum, w.start,
                     (unsigned)npoints);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(points_scatter_kernel, dim3(blocks), dim3(256), 0, stream, d_points, (long long)npoints, dim, g,
                     w.start, w.cnt, w.rows, w.sorted);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

int smrf_points_nn_search_f64(const double* d_query, int64_t nquery, const double* d_points, int64_t npoints, int dim,
                              const double* h_box, double* d_dist, int64_t* d_index, const void* d_workspace,
                              size_t workspace_bytes, void* stream) {
  using namespace smrf;
  if (int rc = points_args(npoints, dim)) return rc;
  if (nquery < 0 || nquery > (int64_t)INT_MAX * 256) return smrf_fail(SMRF_E_ARG, "bad query count");
  if (nquery == 0) return SMRF_OK;
  if (!d_query || !d_points || !h_box) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (!d_dist && !d_index) return smrf_fail(SMRF_E_ARG, "null output");
  if (!d_workspace || workspace_bytes < points_layout(npoints, dim, nullptr, nullptr))
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes,
                     points_layout(npoints, dim, nullptr, nullptr));
  PointsWs w;
  points_layout(npoints, dim, (char*)d_workspace, &w);
  const PointsGrid g = points_grid(h_box, npoints);
  const dim3 grid((unsigned)((nquery + 255) / 256));
  if (dim == 2)
    hipLaunchKernelGGL(points_search_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, d_query, (long long)nquery, g,
                       w.start, w.rows, w.sorted, d_dist, (long long*)d_index);
  else
    hipLaunchKernelGGL(points_search_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, d_query, (long long)nquery, g,
                       w.start, w.rows, w.sorted, d_dist, (long long*)d_index);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

int smrf_points_nn_sum_f64(const double* d_x, int64_t n, double* d_sum, void* d_workspace, size_t workspace_bytes,
                           void* stream) {
  using namespace smrf;
  if (n < 1 || !d_x || !d_sum) return smrf_fail(SMRF_E_ARG, "sum of %lld values", (long long)n);
  if (!d_workspace || workspace_bytes < (size_t)PN_PARTS * sizeof(double))
    return smrf_fail(SMRF_E_WORKSPACE, "sum workspace too small");
  const int blocks = smrf_blocks(n, PN_PARTS);
  double* part = (double*)d_workspace;
  hipLaunchKernelGGL(points_sum_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_x, (long long)n, part);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(points_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (long long)blocks, d_sum);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // extern "C"
