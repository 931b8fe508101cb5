// inpaint_nans_by_fda on the device (neilpy.py:1170-1216): matrix-free LSQR on the finite-difference
// (second-difference) equations.
//
// The reference assembles, per raster cell i, one equation row: the vertical second difference
// [1, -2, 1] when the cell is not in the first or last raster row, plus the horizontal one when it
// is not in the first or last column (COO duplicates on the centre are summed: -4 in the interior,
// -2 on the border rows/columns, no row at the four corners, :1180-1194).  It then keeps the rows
// that touch a NaN cell, ONCE PER NaN ENTRY of the row (`k = fda[:, nan].nonzero()[0]` lists a row
// index once for every stored entry, :1207-1209), and calls
// scipy.sparse.linalg.lsqr(fda[k][:, nan], (-fda[:, known] @ A[known])[k]) with default
// tolerances (:1210).  `fast=True` only pre-filters rows that could not touch a NaN anyway, so it
// does not change the result.  As with the springs, the answer is LSQR's iterate at its stop, so
// this file follows scipy's recurrence (lsqr_core.h: scalar steps, x / w / dk step and driver, shared
// with springs.hip) and its products' accumulation order:
//   - x, v, w are rasters that stay 0 on known cells; u is one raster over equation cells with the
//     multiplicity cnt[i] (0..5 = NaN cells among centre/up/down/left/right of the stencil) beside it;
//   - A v on an equation cell: sum over its NaN stencil cells in ascending flat index (up, left,
//     centre, right, down), as scipy's CSR product does;
//   - A^T u on a NaN cell: contributions of the equation rows above, left, own, right, below in
//     that order, each added cnt times (the duplicated rows of scipy's CSC product);
//   - norms count every equation cnt times.
// Single device only (the reference's callers use it on small rasters; smrf() does not call it).
#include "lsqr_core.h"

namespace {

struct Fda {
  double *x, *v, *w, *u;
  uint8_t *hole, *cnt;
  double* part;
  double* red;
  Sc* sc;
  int rows, cols;
  int nxcd;           // XCDs of the device (lsqr_tile's placement)
};

__device__ __forceinline__ bool has_v(const Fda& b, int r) { return r >= 1 && r <= b.rows - 2; }
__device__ __forceinline__ bool has_h(const Fda& b, int c) { return c >= 1 && c <= b.cols - 2; }

__global__ __launch_bounds__(256) void fda_mask_kernel(const double* __restrict__ A, const Fda b) {
  __shared__ double red[4];
  const long long n = (long long)b.rows * b.cols;
  double c = 0.0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double a = A[i];
    const bool h = a != a;
    b.hole[i] = h;
    c += h ? 1.0 : 0.0;
  }
  const double t = block_sum(c, red);
  if (threadIdx.x == 0) b.part[blockIdx.x] = t;
}

// multiplicity and right-hand side of every equation cell: rhs = (-fda[:, known]) @ A[known]
__global__ __launch_bounds__(256) void fda_rhs_kernel(const double* __restrict__ A, const Fda b) {
  __shared__ double red[4];
  const int rows = b.rows, cols = b.cols;
  double s = 0.0;
  SMRF_FOR_CELLS(rows, cols) {
    const bool pv = has_v(b, r), ph = has_h(b, c);
    int cnt = 0;
    double y = 0.0;
    if (pv | ph) {
      const double cc = -2.0 * ((pv ? 1 : 0) + (ph ? 1 : 0));
      if (pv) { if (b.hole[i - cols]) ++cnt; else y = y + (-1.0) * A[i - cols]; }
      if (ph) { if (b.hole[i - 1]) ++cnt; else y = y + (-1.0) * A[i - 1]; }
      if (b.hole[i]) ++cnt; else y = y + (-cc) * A[i];
      if (ph) { if (b.hole[i + 1]) ++cnt; else y = y + (-1.0) * A[i + 1]; }
      if (pv) { if (b.hole[i + cols]) ++cnt; else y = y + (-1.0) * A[i + cols]; }
    }
    b.cnt[i] = (uint8_t)cnt;
    const double ui = cnt > 0 ? y : 0.0;
    b.u[i] = ui;
    b.x[i] = 0.0;
    b.v[i] = 0.0;
    b.w[i] = 0.0;
    s += cnt * (ui * ui);
  }
  const double t = block_sum(s, red);
  if (threadIdx.x == 0) b.part[blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// A^T u_s on one NaN cell: the equations whose stencil holds it, each cnt times, in SciPy's CSC order
__device__ __forceinline__ double fda_col_dot(const Fda& b, long long i, int r, int c, double ib) {
  const int rows = b.rows, cols = b.cols;
  double y = 0.0;
  if (r >= 1 && has_v(b, r - 1)) {                      // the row above holds this cell as its "down" entry
    const double t = ib * b.u[i - cols];
    for (int k = b.cnt[i - cols]; k > 0; --k) y = y + t;
  }
  if (c >= 1 && has_h(b, c - 1)) {
    const double t = ib * b.u[i - 1];
    for (int k = b.cnt[i - 1]; k > 0; --k) y = y + t;
  }
  {
    const bool pv = has_v(b, r), ph = has_h(b, c);
    if (pv | ph) {
      const double cc = -2.0 * ((pv ? 1 : 0) + (ph ? 1 : 0));
      const double t = cc * (ib * b.u[i]);
      for (int k = b.cnt[i]; k > 0; --k) y = y + t;
    }
  }
  if (c + 1 < cols && has_h(b, c + 1)) {
    const double t = ib * b.u[i + 1];
    for (int k = b.cnt[i + 1]; k > 0; --k) y = y + t;
  }
  if (r + 1 < rows && has_v(b, r + 1)) {
    const double t = ib * b.u[i + cols];
    for (int k = b.cnt[i + cols]; k > 0; --k) y = y + t;
  }
  return y;
}

// v = A^T u_s - beta * v_s on the NaN cells, partial |v|^2 (the set-up's first v; smrf_fda_apply_f64)
__global__ __launch_bounds__(256) void fda_atu_kernel(const Fda b) {
  __shared__ double red[4];
  const Sc* sc = b.sc;
  if (stopped(sc) || !sc->beta_pos) return;
  const double ib = sc->inv_beta, ia = sc->inv_alfa, beta = sc->beta;
  const int rows = b.rows, cols = b.cols;
  double s = 0.0;
  const LsqrTile tl = lsqr_tile(b.nxcd);                      // XCD-aware placement of the walk (lsqr_core.h)
  SMRF_FOR_CELLS_T(tl, rows, cols, cols) {
    if (!b.hole[i]) continue;
    const double nv = fda_col_dot(b, i, r, c, ib) - beta * (ia * b.v[i]);
    b.v[i] = nv;
    s += nv * nv;
  }
  const double t = block_sum(s, red);
  if (threadIdx.x == 0) b.part[SMRF_TILE_SLOT(tl)] = t;
}

// The iteration's v pass with the x / w / dk steps riding in it (lsqr_core.h: lsqr_xw_step has the derivation).
// part[0..] <- |v|^2, part[MAXB..] <- |dk|^2.
__global__ __launch_bounds__(256) void fda_atuxw_kernel(const Fda b) {
  __shared__ double red[4];
  __shared__ double red2[4];
  const Sc* sc = b.sc;
  if (stopped(sc)) return;
  const AtuxwSc q = atuxw_scalars(sc);
  double s = 0.0, sd = 0.0;
  const LsqrTile tl = lsqr_tile(b.nxcd);
  SMRF_FOR_CELLS_T(tl, b.rows, b.cols, b.cols) {
    if (!b.hole[i]) continue;
    const LsqrXw o = lsqr_xw_step(q, b.x, b.v, b.w, i);
    sd += o.dk * o.dk;
    if (q.bpos) {
      const double nv = fda_col_dot(b, i, r, c, q.ib) - q.beta * o.vs;
      b.v[i] = nv;
      s += nv * nv;
    }
  }
  const double t = block_sum(s, red);
  const double td = block_sum(sd, red2);
  if (threadIdx.x == 0) { b.part[SMRF_TILE_SLOT(tl)] = t; b.part[MAXB + SMRF_TILE_SLOT(tl)] = td; }
}

// A v_s on one equation cell (ascending flat index of the stencil's NaN cells)
__device__ __forceinline__ double fda_row_dot(const Fda& b, long long i, int r, int c, double ia) {
  const bool pv = has_v(b, r), ph = has_h(b, c);
  const int cols = b.cols;
  double y = 0.0;
  if (pv && b.hole[i - cols]) y = y + ia * b.v[i - cols];
  if (ph && b.hole[i - 1]) y = y + ia * b.v[i - 1];
  if (b.hole[i]) y = y + (-2.0 * ((pv ? 1 : 0) + (ph ? 1 : 0))) * (ia * b.v[i]);
  if (ph && b.hole[i + 1]) y = y + ia * b.v[i + 1];
  if (pv && b.hole[i + cols]) y = y + ia * b.v[i + cols];
  return y;
}

// u = A v_s - alfa * u_s, partial |u|^2
__global__ __launch_bounds__(256) void fda_av_kernel(const Fda b) {
  __shared__ double red[4];
  const Sc* sc = b.sc;
  if (stopped(sc)) return;
  const double ib = sc->inv_beta, ia = sc->inv_alfa, alfa = sc->alfa;
  double s = 0.0;
  const LsqrTile tl = lsqr_tile(b.nxcd);                      // XCD-aware placement of the walk (lsqr_core.h)
  SMRF_FOR_CELLS_T(tl, b.rows, b.cols, b.cols) {
    const int cnt = b.cnt[i];
    if (cnt == 0) continue;
    const double nu = fda_row_dot(b, i, r, c, ia) - alfa * (ib * b.u[i]);
    b.u[i] = nu;
    s += cnt * (nu * nu);
  }
  const double t = block_sum(s, red);
  if (threadIdx.x == 0) b.part[SMRF_TILE_SLOT(tl)] = t;
}

__global__ __launch_bounds__(256) void fda_scatter_kernel(double* __restrict__ A, const Fda b) {
  const long long n = (long long)b.rows * b.cols;
  const bool pend = lsqr_x_pending(b.sc);
  const double t1 = b.sc->t1;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    if (b.hole[i]) A[i] = pend ? b.x[i] + t1 * b.w[i] : b.x[i];
}

struct FdaLayout { size_t plane, bytes, x, v, w, u, hole, cnt, part, red, sc, total; };
FdaLayout fda_layout(int rows, int cols) {
  FdaLayout L;
  const size_t n = (size_t)rows * (size_t)cols;
  L.plane = smrf_up256(n * sizeof(double));
  L.bytes = smrf_up256(n);
  size_t o = 0;
  L.x = o; o += L.plane;
  L.v = o; o += L.plane;
  L.w = o; o += L.plane;
  L.u = o; o += L.plane;
  L.hole = o; o += L.bytes;
  L.cnt = o; o += L.bytes;
  L.part = o; o += smrf_up256(2 * MAXB * sizeof(double));
  L.red = o; o += 256;
  L.sc = o; o += smrf_up256(sizeof(Sc));
  L.total = o;
  return L;
}
Fda fda_bind(void* ws, int rows, int cols) {
  const FdaLayout L = fda_layout(rows, cols);
  char* p = (char*)ws;
  Fda b;
  b.x = (double*)(p + L.x); b.v = (double*)(p + L.v); b.w = (double*)(p + L.w); b.u = (double*)(p + L.u);
  b.hole = (uint8_t*)(p + L.hole); b.cnt = (uint8_t*)(p + L.cnt);
  b.part = (double*)(p + L.part); b.red = (double*)(p + L.red); b.sc = (Sc*)(p + L.sc);
  b.rows = rows; b.cols = cols; b.nxcd = lsqr_xcd_count();
  return b;
}
// 1-D launch of the mask and scatter kernels
int fda_grid1d(int rows, int cols) {
  return smrf_blocks((long long)rows * cols, MAXB);
}

}  // namespace

extern "C" {

size_t smrf_fda_workspace_bytes(int rows, int cols) { return fda_layout(rows, cols).total; }

int smrf_fda_lsqr_f64(double* d_A, int rows, int cols, double atol, double btol, double conlim, int64_t iter_lim,
                      int* h_istop, int64_t* h_itn, int64_t* h_n_unknown, void* d_workspace, size_t workspace_bytes,
                      void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!d_A || !h_istop || !h_itn) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (rows < 1 || cols < 1) return smrf_fail(SMRF_E_ARG, "bad raster size %d x %d", rows, cols);
  if (!d_workspace || workspace_bytes < fda_layout(rows, cols).total) return smrf_fail(SMRF_E_WORKSPACE, "fda workspace too small");
  const Fda b = fda_bind(d_workspace, rows, cols);
  if (int rc = lsqr_init_scalars(b.sc, atol, btol, conlim, iter_lim, stream)) return rc;
  const int nb1 = fda_grid1d(rows, cols);
  const dim3 g2 = lsqr_grid2d(rows, cols);
  const int nb = (int)(g2.x * g2.y);
  auto reduce = [&](int count) {
    hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(256), 0, stream, (const double*)b.part, count, b.red);
  };
  hipLaunchKernelGGL(fda_mask_kernel, dim3(nb1), dim3(256), 0, stream, (const double*)d_A, b);
  reduce(nb1);
  hipLaunchKernelGGL((setup_scalar_kernel<LSQR_COUNT, Fda>), dim3(1), dim3(1), 0, stream, b);
  hipLaunchKernelGGL(fda_rhs_kernel, g2, dim3(256), 0, stream, (const double*)d_A, b);
  reduce(nb);
  hipLaunchKernelGGL((setup_scalar_kernel<LSQR_BNORM, Fda>), dim3(1), dim3(1), 0, stream, b);
  hipLaunchKernelGGL(fda_atu_kernel, g2, dim3(256), 0, stream, b);
  reduce(nb);
  hipLaunchKernelGGL((setup_scalar_kernel<LSQR_INIT_ALFA, Fda>), dim3(1), dim3(1), 0, stream, b);
  SMRF_LAUNCH_CHECK();
  Sc out{};
  if (int rc = lsqr_iterate(b, fda_atuxw_kernel, fda_av_kernel, g2, nb, 64, stream, out)) return rc;
  if (out.nunk > 0) {
    hipLaunchKernelGGL(fda_scatter_kernel, dim3(nb1), dim3(256), 0, stream, d_A, b);
    SMRF_LAUNCH_CHECK();
    SMRF_HIP_CHECK(hipStreamSynchronize(stream));
  }
  *h_istop = out.istop;
  *h_itn = (int64_t)out.itn;
  if (h_n_unknown) *h_n_unknown = (int64_t)out.nunk;
  return SMRF_OK;
}

// Diagnostic entry (tests only; not used by inpaint_nans_by_fda): the operator the solver iterates with, applied
// once.  d_rhs / d_cnt receive the right-hand side and the multiplicity of every equation cell, d_Av = A v on the
// equation cells (v read on the NaN cells of d_A), d_Atu = A^T u on the NaN cells (u read on the equation cells,
// every equation counted cnt times).  tests/test_fda.py compares them with the reference's explicit sparse
// system (neilpy.py:1180-1209) so that the LSQR iteration-count tolerance is not the only guard on the stencils.
int smrf_fda_apply_f64(const double* d_A, int rows, int cols, const double* d_v, const double* d_u, double* d_rhs,
                       uint8_t* d_cnt, double* d_Av, double* d_Atu, void* d_workspace, size_t workspace_bytes,
                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!d_A || !d_v || !d_u || !d_rhs || !d_cnt || !d_Av || !d_Atu) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (rows < 1 || cols < 1) return smrf_fail(SMRF_E_ARG, "bad raster size %d x %d", rows, cols);
  if (!d_workspace || workspace_bytes < fda_layout(rows, cols).total) return smrf_fail(SMRF_E_WORKSPACE, "fda workspace too small");
  const Fda b = fda_bind(d_workspace, rows, cols);
  if (int rc = lsqr_init_scalars(b.sc, 0.0, 0.0, 0.0, -1, stream, true)) return rc;   // alfa = beta = 0: the bare products
  const size_t n = (size_t)rows * cols;
  const int nb1 = fda_grid1d(rows, cols);
  const dim3 g2 = lsqr_grid2d(rows, cols);
  hipLaunchKernelGGL(fda_mask_kernel, dim3(nb1), dim3(256), 0, stream, d_A, b);
  hipLaunchKernelGGL(fda_rhs_kernel, g2, dim3(256), 0, stream, d_A, b);
  SMRF_LAUNCH_CHECK();
  SMRF_HIP_CHECK(hipMemcpyAsync(d_rhs, b.u, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
  SMRF_HIP_CHECK(hipMemcpyAsync(d_cnt, b.cnt, n, hipMemcpyDeviceToDevice, stream));
  SMRF_HIP_CHECK(hipMemcpyAsync(b.v, d_v, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
  hipLaunchKernelGGL(fda_av_kernel, g2, dim3(256), 0, stream, b);          // u = A v - 0 * u
  SMRF_LAUNCH_CHECK();
  SMRF_HIP_CHECK(hipMemcpyAsync(d_Av, b.u, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
  SMRF_HIP_CHECK(hipMemcpyAsync(b.u, d_u, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
  hipLaunchKernelGGL(fda_atu_kernel, g2, dim3(256), 0, stream, b);         // v = A^T u - 0 * v
  SMRF_LAUNCH_CHECK();
  SMRF_HIP_CHECK(hipMemcpyAsync(d_Atu, b.v, n * sizeof(double), hipMemcpyDeviceToDevice, stream));
  SMRF_HIP_CHECK(hipStreamSynchronize(stream));
  return SMRF_OK;
}

}  // extern "C"
