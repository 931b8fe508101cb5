// Connected-component labelling of a 2-D mask: scipy.ndimage.label for the 16 centrally symmetric 3 x 3 structures, with
// the sizes and bounding boxes of the objects and the keep pass of remove_small_objects.  Host side: neilpy_amd/label.py;
// C ABI: include/smrf_label.h; contract and byte model: DESIGN.md section 21.
//
// The labels plane P first holds a union-find forest over linear cell indices (-1 = background), the scratch plane W its
// flattened copy, and P then the object numbers.  Every phase is a launch of its own and the kernel boundary is the only
// synchronisation between workgroups: no cooperative launch, no grid barrier, no loop that waits for another workgroup.
//
//   1. tile      one workgroup labels a 64 x 64 tile in LDS (label_runs.h: row masks from __ballot, run starts by bit
//                operations, smrf_row_links between adjacent rows, smrf_unite_min on LDS) and writes
//                P[i] = the tile-local root of cell i as a linear index of the raster - the object's first cell of the
//                tile in C order, so P[i] <= i.
//   2. seam      one thread per cell of a tile's bottom row and right column: unite it with its linked neighbours across
//                the seam (the corner neighbours included) by smrf_unite_min on P.
//   3. flatten   W[i] = the root of i, read from P as the seam pass left it; counts the roots of every block of
//                SMRF_LABEL_SCAN_BLOCK cells.
//   4. scan      the block counts become their exclusive scan (one workgroup); the total goes to d_count.
//   5. number    P[root] = 1 + the number of roots before it in C order.
//   6. relabel   P[i] = P[W[i]] for every cell that is not a root, 0 for background.  It reads P at roots only and writes P
//                at every other cell, so no cell is read that the launch overwrites.
//
// Why the seam pass needs no fence.  The invariant is parent[i] <= i, and links are only ever lowered, by an agent-scope
// atomic min whose returned value - not an earlier read - decides what the thread does next.  A stale read of parent[i]
// (another XCD's L2, this CU's L1) gives a value parent[i] held before: an ancestor of i in the same object, from which
// the walk goes on downwards.  smrf_unite_min's comment carries the argument through; its end is that every object's
// root is its smallest linear index, its first cell in C order, whichever order the atomics land in.  Numbering the roots
// in index order is then scipy.ndimage.label's numbering, and the same on every run.
#include <climits>

#include "label_runs.h"
#include "raster_stencil.h"
#include "smrf_label.h"

namespace {

constexpr int TR = SMRF_LABEL_TILE_ROWS, TC = SMRF_LABEL_TILE_COLS, WAVES = 4, NT = 64 * WAVES;
constexpr int SCAN = SMRF_LABEL_SCAN_BLOCK, SCAN_STEPS = SCAN / NT;
static_assert(TC == 64 && TR % WAVES == 0 && SCAN % NT == 0, "a tile row is one wave64; whole waves per step");

struct LabelWs {
  int* flat;        // W: the flattened forest
  unsigned* bsum;   // roots per block of SCAN cells, then their exclusive scan
};

inline long long scan_blocks_of(long long cells) { return (cells + SCAN - 1) / SCAN; }

size_t label_layout(long long cells, char* base, LabelWs* w) {
  const size_t plane = smrf_up256((size_t)cells * 4), sums = smrf_up256((size_t)scan_blocks_of(cells) * 4);
  if (w) *w = LabelWs{(int*)base, (unsigned*)(base + plane)};
  return plane + sums;
}

// ---------------------------------------------------------------------------------------------------------------
// 1. tile
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void label_tile_kernel(const unsigned char* __restrict__ mask, int* __restrict__ P,
                                                        int rows, int cols, int tiles_x, int links) {
  __shared__ uint64_t row_mask[TR];
  __shared__ int par[TR * TC];              // of a run's first cell: the forest over runs, as tile indices r * 64 + c
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = (int)(blockIdx.x / (unsigned)tiles_x) * TR, col0 = (int)(blockIdx.x % (unsigned)tiles_x) * TC;
  const int col = col0 + lane;
  const auto load = [&](int i) { return __hip_atomic_load(&par[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  const auto lower = [&](int i, int v) {
    return __hip_atomic_fetch_min(&par[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };

  for (int r = wave; r < TR; r += WAVES) {
    const int row = row0 + r;
    const bool fg = row < rows && col < cols && mask[(long long)row * cols + col] != 0;
    const uint64_t m = __ballot(fg);
    if (lane == 0) row_mask[r] = m;
    if (smrf_run_starts(m, links) >> lane & 1) par[r * TC + lane] = r * TC + lane;
  }
  __syncthreads();
  for (int r = wave ? wave : WAVES; r < TR; r += WAVES) {       // every row but the tile's first
    const uint64_t m = row_mask[r], up = row_mask[r - 1];
    if (m >> lane & 1) {
      const int mine = r * TC + smrf_run_start_of(smrf_run_starts(m, links), lane);
      const uint64_t up_starts = smrf_run_starts(up, links);
      smrf_row_links(up, m, lane, links, [&](int cu) {
        smrf_unite_min(mine, (r - 1) * TC + smrf_run_start_of(up_starts, cu), load, lower);
      });
    }
  }
  __syncthreads();
  for (int r = wave; r < TR; r += WAVES) {
    const int row = row0 + r;
    if (row >= rows || col >= cols) continue;
    const uint64_t m = row_mask[r];
    int v = -1;
    if (m >> lane & 1) {
      const int root = smrf_find_root(r * TC + smrf_run_start_of(smrf_run_starts(m, links), lane), load);
      v = (row0 + root / TC) * cols + col0 + root % TC;
    }
    P[(long long)row * cols + col] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// 2. seam
// ---------------------------------------------------------------------------------------------------------------
// One job per cell of every tile's bottom row that has a row below (jobs 0 .. n_h - 1: its S, SE and SW neighbours) and of
// every tile's right column that has a column to its right (the rest: its E neighbour, its SE neighbour, and the SW link
// from its E neighbour down to the cell below it).  A pair that both kinds of job reach is left to the first kind.
// With the E and S links both present a pair is passed over where links inside the tiles and the neighbouring job of the
// same seam join it already; the chain of such jobs along a seam ends at the tile's edge at the latest, where none is
// passed over.
__global__ __launch_bounds__(NT) void label_seam_kernel(int* __restrict__ P, int rows, int cols, long long n_h,
                                                        long long n_jobs, int links) {
  const auto load = [&](int i) { return __hip_atomic_load(&P[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  const auto lower = [&](int i, int v) { return __hip_atomic_fetch_min(&P[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  const auto fg = [&](int r, int c) { return load(r * cols + c) >= 0; };            // -1 or not: no union changes that
  const auto unite = [&](int r, int c, int r2, int c2) {
    if (fg(r2, c2)) smrf_unite_min(r * cols + c, r2 * cols + c2, load, lower);
  };
  const bool grid4 = (links & SMRF_LINK_E) && (links & SMRF_LINK_S);
  for (long long j = blockIdx.x * (long long)NT + threadIdx.x; j < n_jobs; j += (long long)gridDim.x * NT) {
    if (j < n_h) {
      const int r = (int)(j / cols) * TR + TR - 1, c = (int)(j % cols), lc = c % TC;       // r + 1 < rows
      if (!fg(r, c)) continue;
      const bool below = fg(r + 1, c);
      if ((links & SMRF_LINK_S) && below && !(grid4 && lc != 0 && fg(r, c - 1) && fg(r + 1, c - 1)))
        smrf_unite_min(r * cols + c, (r + 1) * cols + c, load, lower);
      if ((links & SMRF_LINK_SE) && c + 1 < cols && !(grid4 && below && lc != TC - 1)) unite(r, c, r + 1, c + 1);
      if ((links & SMRF_LINK_SW) && c > 0 && !(grid4 && below && lc != 0)) unite(r, c, r + 1, c - 1);
    } else {
      const long long k = j - n_h;
      const int c = (int)(k / rows) * TC + TC - 1, r = (int)(k % rows), lr = r % TR;       // c + 1 < cols
      const bool here = fg(r, c), right = fg(r, c + 1);
      if ((links & SMRF_LINK_E) && here && right && !(grid4 && lr != 0 && fg(r - 1, c) && fg(r - 1, c + 1)))
        smrf_unite_min(r * cols + c, r * cols + c + 1, load, lower);
      if (lr == TR - 1 || r + 1 >= rows) continue;                                         // the row below: the other kind of job
      if ((links & SMRF_LINK_SE) && here && !(grid4 && right)) unite(r, c, r + 1, c + 1);
      if ((links & SMRF_LINK_SW) && right && !(grid4 && here)) unite(r, c + 1, r + 1, c);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// 3. - 6. flatten, scan, number, relabel
// ---------------------------------------------------------------------------------------------------------------
// exclusive scan of one value per thread over the 256 threads of a workgroup; total = their sum (points.hip's)
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned& total) {
  __shared__ unsigned wsum[WAVES];
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

// A block takes SCAN consecutive cells in SCAN_STEPS steps of 256, one cell per thread and step: cell index and C order
// agree, so the roots before a root within its block are those of earlier steps, of earlier waves of its step and of
// lower lanes of its wave.
__global__ __launch_bounds__(NT) void label_flatten_kernel(const int* __restrict__ P, int* __restrict__ W, int cells,
                                                           unsigned* __restrict__ bsum) {
  __shared__ unsigned count;
  if (threadIdx.x == 0) count = 0;
  __syncthreads();
  const auto load = [&](int i) { return P[i]; };
  unsigned mine = 0;
  for (int s = 0; s < SCAN_STEPS; ++s) {
    const long long i = (long long)blockIdx.x * SCAN + s * NT + threadIdx.x;
    if (i >= cells) break;
    const int p = P[i];
    const int root = p < 0 ? -1 : smrf_find_root(p, load);
    W[i] = root;
    mine += root == (int)i;
  }
  for (int o = 32; o; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&count, mine);
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = count;
}

// one workgroup: bsum becomes its own exclusive scan, *d_count their sum
__global__ __launch_bounds__(NT) void label_scan_kernel(unsigned* __restrict__ bsum, long long nb, int* __restrict__ d_count) {
  unsigned carry = 0;
  for (long long i0 = 0; i0 < nb; i0 += NT) {
    const long long i = i0 + threadIdx.x;
    const unsigned v = i < nb ? bsum[i] : 0u;
    unsigned total;
    const unsigned ex = block_scan(v, total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *d_count = (int)carry;
}

__global__ __launch_bounds__(NT) void label_number_kernel(const int* __restrict__ W, int* __restrict__ P, int cells,
                                                          const unsigned* __restrict__ bsum) {
  __shared__ unsigned before[SCAN_STEPS * WAVES + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t roots[SCAN_STEPS];
#pragma unroll
  for (int s = 0; s < SCAN_STEPS; ++s) {
    const long long i = (long long)blockIdx.x * SCAN + s * NT + threadIdx.x;
    roots[s] = __ballot(i < cells && W[i] == (int)i);
    if (lane == 0) before[s * WAVES + wave] = (unsigned)__popcll(roots[s]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned run = bsum[blockIdx.x];
    for (int k = 0; k < SCAN_STEPS * WAVES; ++k) {
      const unsigned n = before[k];
      before[k] = run;
      run += n;
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < SCAN_STEPS; ++s) {
    const long long i = (long long)blockIdx.x * SCAN + s * NT + threadIdx.x;
    if (roots[s] >> lane & 1) P[i] = (int)(before[s * WAVES + wave] + (unsigned)__popcll(roots[s] & ((1ull << lane) - 1))) + 1;
  }
}

__global__ __launch_bounds__(NT) void label_relabel_kernel(const int* __restrict__ W, int* P, int cells) {
  for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < cells; i += (long long)gridDim.x * NT) {
    const int root = W[i];
    if (root == (int)i) continue;           // a root: its number is in place, and is what the other cells of its object read
    P[i] = root < 0 ? 0 : P[root];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// regions: sizes and boxes
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void regions_clear_kernel(int n, long long* __restrict__ size, int* __restrict__ box) {
  for (long long k = blockIdx.x * (long long)NT + threadIdx.x; k <= n; k += (long long)gridDim.x * NT) {
    if (size) size[k] = 0;
    if (box && k < n) {
      box[4 * k + 0] = INT_MAX;
      box[4 * k + 1] = 0;
      box[4 * k + 2] = INT_MAX;
      box[4 * k + 3] = 0;
    }
  }
}

// A wave takes 64 consecutive cells.  A stretch of equal labels within one raster row is counted by its first lane: one
// add to the size and, a stretch being a row segment, one min / max per side of the box.  Zeros are summed per thread over
// the whole grid-stride loop and added once per wave.
__global__ __launch_bounds__(NT) void regions_kernel(const int* __restrict__ L, int cols, long long cells, int n,
                                                     unsigned long long* __restrict__ size, int* __restrict__ box) {
  const int lane = threadIdx.x & 63;
  unsigned long long zeros = 0;
  const long long span = (long long)gridDim.x * NT;
  for (long long base = blockIdx.x * (long long)NT + (threadIdx.x - lane); base < cells; base += span) {
    const long long i = base + lane;
    const bool in = i < cells;
    const int v = in ? L[i] : -1;
    const int r = in ? (int)(i / cols) : 0, c = in ? (int)(i - (long long)r * cols) : 0;
    zeros += v == 0;
    const int left = __shfl_up(v, 1, 64);
    const bool first = lane == 0 || c == 0 || left != v;
    const uint64_t firsts = __ballot(first);
    if (first && v >= 1 && v <= n) {
      const uint64_t later = lane == 63 ? 0 : firsts >> (lane + 1);
      const int len = later ? __builtin_ctzll(later) + 1 : 64 - lane;     // the next stretch starts len lanes on
      if (size) atomicAdd(&size[v], (unsigned long long)len);
      if (box) {
        int* b = box + 4 * (long long)(v - 1);
        atomicMin(&b[0], r);
        atomicMax(&b[1], r + 1);
        atomicMin(&b[2], c);
        atomicMax(&b[3], c + len);
      }
    }
  }
  if (size) {
    for (int o = 32; o; o >>= 1) zeros += __shfl_down(zeros, o, 64);
    if (lane == 0 && zeros) atomicAdd(&size[0], zeros);
  }
}

// a label nobody holds keeps the cleared box: it becomes (0, 0, 0, 0)
__global__ __launch_bounds__(NT) void regions_close_kernel(int n, int* __restrict__ box) {
  for (long long k = blockIdx.x * (long long)NT + threadIdx.x; k < n; k += (long long)gridDim.x * NT)
    if (box[4 * k + 1] == 0) box[4 * k + 0] = box[4 * k + 2] = 0;
}

__global__ __launch_bounds__(NT) void keep_kernel(const int* __restrict__ L, const long long* __restrict__ size,
                                                  long long cells, long long min_size, unsigned char* __restrict__ out) {
  for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < cells; i += (long long)gridDim.x * NT) {
    const int v = L[i];
    out[i] = v > 0 && size[v] >= min_size;
  }
}

constexpr int GRID_CAP = 1 << 16;

int check_plane(int rows, int cols, long long& cells) {
  if (int rc = smrf::check_size(rows, cols)) return rc;
  cells = (long long)rows * cols;
  if (cells >= (1ll << 31)) return smrf_fail(SMRF_E_UNSUPPORTED, "raster of %d x %d: cell indices are int32", rows, cols);
  return SMRF_OK;
}

}  // namespace

extern "C" {

int smrf_label_links(const unsigned char* s) {
  if (!s) return smrf_fail(SMRF_E_ARG, "null structure");
  const int links = smrf_links_of(s);
  return links < 0 ? smrf_fail(SMRF_E_ARG, "the structure is not centrally symmetric") : links;
}

long long smrf_label_workspace_bytes(int rows, int cols) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  return cells ? (long long)label_layout(cells, nullptr, nullptr) : 0;
}

int smrf_label_u8(const unsigned char* d_mask, int* d_labels, int rows, int cols, int links, void* d_work,
                  long long work_bytes, int* d_count, void* stream) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  if (links < 0 || links > 15) return smrf_fail(SMRF_E_ARG, "link mask %d", links);
  if (!d_count) return smrf_fail(SMRF_E_ARG, "null pointer");
  const hipStream_t st = (hipStream_t)stream;
  if (cells == 0) {
    SMRF_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(int), st));
    return SMRF_OK;
  }
  if (!d_mask || !d_labels) return smrf_fail(SMRF_E_ARG, "null pointer");
  const long long need = (long long)label_layout(cells, nullptr, nullptr);
  if (!d_work || work_bytes < need)
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %lld bytes, %lld needed", work_bytes, need);
  LabelWs w;
  label_layout(cells, (char*)d_work, &w);
  const long long tiles_x = (cols + TC - 1) / TC, tiles_y = (rows + TR - 1) / TR;
  const long long n_h = (tiles_y - 1) * cols, n_jobs = n_h + (tiles_x - 1) * rows, nb = scan_blocks_of(cells);
  hipLaunchKernelGGL(label_tile_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(NT), 0, st, d_mask, d_labels, rows, cols,
                     (int)tiles_x, links);
  SMRF_LAUNCH_CHECK();
  if (n_jobs && links) {
    hipLaunchKernelGGL(label_seam_kernel, dim3(smrf_blocks(n_jobs, GRID_CAP)), dim3(NT), 0, st, d_labels, rows, cols, n_h,
                       n_jobs, links);
    SMRF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(label_flatten_kernel, dim3((unsigned)nb), dim3(NT), 0, st, d_labels, w.flat, (int)cells, w.bsum);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(NT), 0, st, w.bsum, nb, d_count);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(label_number_kernel, dim3((unsigned)nb), dim3(NT), 0, st, w.flat, d_labels, (int)cells, w.bsum);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(label_relabel_kernel, dim3(smrf_blocks(cells, GRID_CAP)), dim3(NT), 0, st, w.flat, d_labels, (int)cells);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

int smrf_label_regions(const int* d_labels, int rows, int cols, int n, long long* d_size, int* d_box, void* stream) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  if (n < 0) return smrf_fail(SMRF_E_ARG, "%d labels", n);
  if (!d_size && !d_box) return smrf_fail(SMRF_E_ARG, "null output");
  if (cells && !d_labels) return smrf_fail(SMRF_E_ARG, "null pointer");
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(regions_clear_kernel, dim3(smrf_blocks((long long)n + 1, GRID_CAP)), dim3(NT), 0, st, n, d_size, d_box);
  SMRF_LAUNCH_CHECK();
  if (cells) {
    hipLaunchKernelGGL(regions_kernel, dim3(smrf_blocks(cells, 8192)), dim3(NT), 0, st, d_labels, cols, cells, n,
                       (unsigned long long*)d_size, d_box);
    SMRF_LAUNCH_CHECK();
  }
  if (d_box && n) {
    hipLaunchKernelGGL(regions_close_kernel, dim3(smrf_blocks(n, GRID_CAP)), dim3(NT), 0, st, n, d_box);
    SMRF_LAUNCH_CHECK();
  }
  return SMRF_OK;
}

int smrf_label_keep(const int* d_labels, const long long* d_size, long long cells, long long min_size,
                    unsigned char* d_out, void* stream) {
  if (cells < 0) return smrf_fail(SMRF_E_ARG, "negative size");
  if (cells == 0) return SMRF_OK;
  if (!d_labels || !d_size || !d_out) return smrf_fail(SMRF_E_ARG, "null pointer");
  hipLaunchKernelGGL(keep_kernel, dim3(smrf_blocks(cells, GRID_CAP)), dim3(NT), 0, (hipStream_t)stream, d_labels, d_size,
                     cells, min_size, d_out);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // extern "C"
