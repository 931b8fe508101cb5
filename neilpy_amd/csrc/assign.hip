// Point-set matching (hungarian_algorithm, bdr, bdr_bootstrap; the reference's neilpy.py:2724, :2642, :2735): the linear
// assignment problem on Euclidean costs and the bidimensional regression, batched.  DESIGN.md section 18 is the contract.
//
// One problem belongs to one wave64; several waves, each with its own problem, share a workgroup, and no workgroup
// barrier is reached after the kernel's first instruction (the waves run different numbers of steps).
//
//   solve     shortest augmenting paths (Jonker-Volgenant in Crouse's rectangular form, what SciPy runs) with float64
//             duals.  Column j lives on lane j % 64.  v[j], the tentative distance, the predecessor row, the owner row and
//             the reached flag of the first AS_REG columns of a lane are registers, those of the columns from AS_REG_COLS
//             on sit in the wave's slice of LDS.  u[i] and the column of row i sit in LDS.  A row is reached exactly when
//             it is the augmentation's first row or owns a reached column, so the reached rows need no flag of their own:
//             the lane of a reached column updates its owner's u.
//   minimum   each lane folds its columns, then six __shfl_xor steps on the key (distance, owner present, column): the
//             lowest distance, among equals an unassigned column, among those the lowest column.  The key is total, so the
//             winner does not depend on which lane holds which column.
//   costs     sqrt((x0-a0)*(x0-a0) + (x1-a1)*(x1-a1) [+ (x2-a2)*(x2-a2)]), every operation rounded (no FMA).  Kept as an
//             nr x nc matrix in the wave's LDS where sixteen such waves fit a CU (CACHED), else recomputed from the
//             coordinates, which are in LDS either way: the same bits.  No cost ever goes to global memory except
//             min_costs.
//   regress   lane l sums elements l, l + 64, ... in that order from +0.0; the 64 partials go through the __shfl_xor tree
//             (offsets 32 .. 1), p += p[lane ^ o], which leaves the same bits in every lane.  add, mul, div, sqrt only.
//
// Every loop of the solve is bounded: a scan step reaches a new column or ends the problem with ASSIGN_ST_INFEASIBLE (an
// overflowed cost), an augmentation walks at most nr predecessors.
#include <climits>
#include <cmath>

#include "smrf_common.h"

namespace smrf {

constexpr int AS_REG = 4;                        // columns per lane with their state in registers
constexpr int AS_REG_COLS = 64 * AS_REG;         // columns 0 .. 255: registers; from 256 on: LDS
constexpr int AS_WAVES = 4;                      // waves (problems) per workgroup at most
constexpr int AS_RESIDENT = 16;                  // waves a CU holds by the kernel's registers (4 per SIMD)
constexpr size_t AS_LDS_WG = 160 * 1024;         // one workgroup may claim the CU's whole LDS on gfx950
constexpr int AS_OWNED = 1 << 30;                // key bit of a column that has an owner row
constexpr size_t AS_WS_BYTES = 256;              // int64 bad sample entries, then the int32 status
enum { ASSIGN_ST_INFEASIBLE = 1, ASSIGN_ST_SAMPLE = 2 };

struct AssignLayout {   // byte offsets inside a wave's slice of LDS
  size_t rowc, colc, u, cost, lv, lsh, c4r, lpa, lr4, lsc, bytes;
};

__host__ __device__ inline AssignLayout assign_layout(int nr, int nc, int dim, bool cached) {
  AssignLayout L;
  size_t off = 0;
  const size_t ext = nc > AS_REG_COLS ? (size_t)(nc - AS_REG_COLS) : 0;   // columns with their state in LDS
  L.rowc = off; off += (size_t)nr * dim * 8;      // planar: axis a of row i at [a * nr + i]
  L.colc = off; off += (size_t)nc * dim * 8;      // planar
  L.u = off; off += (size_t)nr * 8;
  L.cost = off; off += cached ? (size_t)nr * nc * 8 : 0;
  L.lv = off; off += ext * 8;
  L.lsh = off; off += ext * 8;
  L.c4r = off; off += (((size_t)nr + 1) & ~(size_t)1) * 4;
  L.lpa = off; off += ext * 4;
  L.lr4 = off; off += ext * 4;
  L.lsc = off; off += ext * 4;
  L.bytes = (off + 15) & ~(size_t)15;
  return L;
}

struct AssignRoute {
  bool cached;
  int waves;           // waves per workgroup
  size_t wave_bytes;
};

// nr <= nc.  The costs are cached where the matrix does not cost residency: AS_RESIDENT waves with their matrices fit the
// LDS of a CU.  (A matrix that leaves room for 4 waves per CU ran 64 of 128 points slower than recomputing at 16.)
inline AssignRoute assign_route(int nr, int nc, int dim) {
  const size_t c = assign_layout(nr, nc, dim, true).bytes;
  AssignRoute r;
  r.cached = c * AS_RESIDENT <= AS_LDS_WG;
  r.wave_bytes = r.cached ? c : assign_layout(nr, nc, dim, false).bytes;
  r.waves = (int)std::min<size_t>(AS_WAVES, AS_LDS_WG / r.wave_bytes);
  return r;
}

// the largest n whose n x n problem of dimension 3 fits the 160 KiB of one workgroup without the cost matrix
inline int assign_limit() {
  static const int limit = [] {   // initialised once, whichever host thread asks first
    int n = 1024;
    while (assign_layout(n + 1, n + 1, 3, false).bytes <= AS_LDS_WG) ++n;
    return n;
  }();
  return limit;
}

inline int assign_cached_square(int dim) {
  int n = 1;
  while (assign_route(n + 1, n + 1, dim).cached) ++n;
  return n;
}

struct AssignArgs {
  const double* rowpts;       // (nr, dim) the solve's rows; the regression's XY
  const double* colpts;       // (m, dim) the cloud the columns are taken from
  const long long* samples;   // (k, nc) rows of colpts, or NULL: column t is row t
  long long k, m;
  int nr, nc;
  int solve;                  // 0: the identity matching, nothing staged in LDS (bdr)
  int swapped;                // hungarian with nr > nc: rowpts is AB, colpts is XY
  size_t wave_bytes;
  long long* out_rows;        // hungarian: (nr,)
  long long* out_cols;
  double* out_costs;
  double* scal;               // regression: (k, 9) beta1 beta2 alpha1 alpha2 rsquare D Dmax DI F, or NULL
  double* aprime;             // (k, n) or NULL
  double* bprime;
  double* rsq;                // (k,) or NULL
  double* di;
  int* status;
};

__device__ __forceinline__ void as_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double as_wave_sum(double p) {
  for (int o = 32; o > 0; o >>= 1) p = __dadd_rn(p, __shfl_xor(p, o, 64));
  return p;
}

// load(i, x, y, a, b): point i of XY and the point of AB matched to it.  Every lane of the wave calls this.
template <typename Load>
__device__ void as_regress(const Load& load, int n, int lane, double* scal, double* aprime, double* bprime, double* rsq,
                           double* di) {
  const double dn = (double)n;
  double sx = 0.0, sy = 0.0, sa = 0.0, sb = 0.0;
  for (int i = lane; i < n; i += 64) {
    double x, y, a, b;
    load(i, x, y, a, b);
    sx = __dadd_rn(sx, x);
    sy = __dadd_rn(sy, y);
    sa = __dadd_rn(sa, a);
    sb = __dadd_rn(sb, b);
  }
  const double mx = __ddiv_rn(as_wave_sum(sx), dn), my = __ddiv_rn(as_wave_sum(sy), dn);
  const double ma = __ddiv_rn(as_wave_sum(sa), dn), mb = __ddiv_rn(as_wave_sum(sb), dn);
  double xa = 0.0, yb = 0.0, xb = 0.0, ya = 0.0, xx = 0.0, yy = 0.0, aa = 0.0, bb = 0.0;
  for (int i = lane; i < n; i += 64) {
    double x, y, a, b;
    load(i, x, y, a, b);
    const double cx = __dsub_rn(x, mx), cy = __dsub_rn(y, my), ca = __dsub_rn(a, ma), cb = __dsub_rn(b, mb);
    xa = __dadd_rn(xa, __dmul_rn(cx, ca));
    yb = __dadd_rn(yb, __dmul_rn(cy, cb));
    xb = __dadd_rn(xb, __dmul_rn(cx, cb));
    ya = __dadd_rn(ya, __dmul_rn(cy, ca));
    xx = __dadd_rn(xx, __dmul_rn(cx, cx));
    yy = __dadd_rn(yy, __dmul_rn(cy, cy));
    aa = __dadd_rn(aa, __dmul_rn(ca, ca));
    bb = __dadd_rn(bb, __dmul_rn(cb, cb));
  }
  xa = as_wave_sum(xa); yb = as_wave_sum(yb); xb = as_wave_sum(xb); ya = as_wave_sum(ya);
  xx = as_wave_sum(xx); yy = as_wave_sum(yy); aa = as_wave_sum(aa); bb = as_wave_sum(bb);
  const double den = __dadd_rn(xx, yy);
  const double beta1 = __ddiv_rn(__dadd_rn(xa, yb), den), beta2 = __ddiv_rn(__dsub_rn(xb, ya), den);
  const double alpha1 = __dadd_rn(__dsub_rn(ma, __dmul_rn(beta1, mx)), __dmul_rn(beta2, my));
  const double alpha2 = __dsub_rn(__dsub_rn(mb, __dmul_rn(beta2, mx)), __dmul_rn(beta1, my));
  double res = 0.0;
  for (int i = lane; i < n; i += 64) {
    double x, y, a, b;
    load(i, x, y, a, b);
    const double ap = __dsub_rn(__dadd_rn(alpha1, __dmul_rn(beta1, x)), __dmul_rn(beta2, y));
    const double bp = __dadd_rn(__dadd_rn(alpha2, __dmul_rn(beta2, x)), __dmul_rn(beta1, y));
    if (aprime) aprime[i] = ap;
    if (bprime) bprime[i] = bp;
    const double ea = __dsub_rn(a, ap), eb = __dsub_rn(b, bp);
    res = __dadd_rn(res, __dadd_rn(__dmul_rn(ea, ea), __dmul_rn(eb, eb)));
  }
  res = as_wave_sum(res);
  const double tot = __dadd_rn(aa, bb);
  const double r2 = __dsub_rn(1.0, __ddiv_rn(res, tot));
  const double om = __dsub_rn(1.0, r2);
  const double DI = __dsqrt_rn(om);
  if (lane == 0) {
    if (rsq) *rsq = r2;
    if (di) *di = DI;
    if (scal) {
      scal[0] = beta1; scal[1] = beta2; scal[2] = alpha1; scal[3] = alpha2; scal[4] = r2;
      scal[5] = __dsqrt_rn(res);
      scal[6] = __dsqrt_rn(tot);
      scal[7] = DI;
      scal[8] = __dmul_rn(__ddiv_rn((double)(2ll * n - 4), 2.0), __ddiv_rn(r2, om));
    }
  }
}

template <int DIM, bool CACHED>
__global__ __launch_bounds__(64 * AS_WAVES) void assign_kernel(const AssignArgs a) {
  extern __shared__ __align__(16) unsigned char as_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long s = (long long)blockIdx.x * (blockDim.x >> 6) + w;   // this wave's problem
  if (s >= a.k) return;
  const int nr = a.nr, nc = a.nc;
  double* const scal = a.scal ? a.scal + s * 9 : nullptr;
  double* const aprime = a.aprime ? a.aprime + s * nr : nullptr;
  double* const bprime = a.bprime ? a.bprime + s * nr : nullptr;
  double* const rsq = a.rsq ? a.rsq + s : nullptr;
  double* const di = a.di ? a.di + s : nullptr;

  if (!a.solve) {   // bdr: row i of XY against row i of AB, read where they lie
    const double* xy = a.rowpts;
    const double* ab = a.colpts;
    as_regress([&](int i, double& x, double& y, double& p, double& q) {
      x = xy[2 * (long long)i]; y = xy[2 * (long long)i + 1]; p = ab[2 * (long long)i]; q = ab[2 * (long long)i + 1];
    }, nr, lane, scal, aprime, bprime, rsq, di);
    return;
  }

  const AssignLayout L = assign_layout(nr, nc, DIM, CACHED);
  unsigned char* const base = as_lds + (size_t)w * a.wave_bytes;
  double* const rowc = (double*)(base + L.rowc);
  double* const colc = (double*)(base + L.colc);
  double* const u = (double*)(base + L.u);
  double* const cost = (double*)(base + L.cost);
  double* const Lv = (double*)(base + L.lv);       // indexed by the column less AS_REG_COLS
  double* const Lsh = (double*)(base + L.lsh);
  int* const c4r = (int*)(base + L.c4r);
  int* const Lpa = (int*)(base + L.lpa);
  int* const Lr4 = (int*)(base + L.lr4);
  int* const Lsc = (int*)(base + L.lsc);

  // ---- stage: coordinates, planar; the sample's rows of colpts are checked as they are read
  bool bad = false;
  for (int i = lane; i < nr; i += 64) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) rowc[d * nr + i] = a.rowpts[(long long)i * DIM + d];
    u[i] = 0.0;
    c4r[i] = -1;
  }
  for (int t = lane; t < nc; t += 64) {
    long long r = t;
    if (a.samples) {
      r = a.samples[s * nc + t];
      if ((unsigned long long)r >= (unsigned long long)a.m) { bad = true; r = 0; }
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) colc[d * nc + t] = a.colpts[r * DIM + d];
  }
  as_wave_sync();
  if (__any(bad)) {
    if (lane == 0) {
      atomicOr(a.status, ASSIGN_ST_SAMPLE);
      if (rsq) *rsq = NAN;
      if (di) *di = NAN;
    }
    return;
  }

  auto pair_cost = [&](int i, int j) {
    const double d0 = __dsub_rn(rowc[i], colc[j]), d1 = __dsub_rn(rowc[nr + i], colc[nc + j]);
    double d2 = __dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1));
    if (DIM == 3) {
      const double dz = __dsub_rn(rowc[2 * nr + i], colc[2 * nc + j]);
      d2 = __dadd_rn(d2, __dmul_rn(dz, dz));
    }
    return __dsqrt_rn(d2);
  };
  if (CACHED) {
    for (int i = 0; i < nr; ++i)
      for (int j = lane; j < nc; j += 64) cost[i * nc + j] = pair_cost(i, j);
    as_wave_sync();
  }

  // ---- per-column state
  double v[AS_REG], sh[AS_REG];
  int pa[AS_REG], r4[AS_REG];
  bool sc[AS_REG];
#pragma unroll
  for (int q = 0; q < AS_REG; ++q) { v[q] = 0.0; sh[q] = INFINITY; pa[q] = -1; r4[q] = -1; sc[q] = true; }
  for (int e = lane; e < nc - AS_REG_COLS; e += 64) { Lv[e] = 0.0; Lsh[e] = INFINITY; Lr4[e] = -1; Lpa[e] = -1; Lsc[e] = 0; }

  // f(j, v, shortest, predecessor, owner, reached) for every column of this lane, ascending
  auto for_cols = [&](auto&& f) {
#pragma unroll
    for (int q = 0; q < AS_REG; ++q) {
      const int j = lane + 64 * q;
      if (64 * q < nc) {   // the same in every lane: a group of 64 columns the problem does not have is skipped, not masked
        if (j < nc) f(j, v[q], sh[q], pa[q], r4[q], sc[q]);
      }
    }
    for (int e = lane; e < nc - AS_REG_COLS; e += 64) {
      bool reached = Lsc[e] != 0;
      f(e + AS_REG_COLS, Lv[e], Lsh[e], Lpa[e], Lr4[e], reached);
      Lsc[e] = reached;
    }
  };
  // an int of column j's state, j the same in every lane
  auto fetch = [&](const int (&reg)[AS_REG], const int* lds, int j) {
    if (j >= AS_REG_COLS) return lds[j - AS_REG_COLS];
    int val = reg[0];
#pragma unroll
    for (int q = 1; q < AS_REG; ++q)
      if ((j >> 6) == q) val = reg[q];
    return __shfl(val, j & 63, 64);
  };

  bool failed = false;
  for (int cur = 0; cur < nr && !failed; ++cur) {
    for_cols([&](int, double&, double& shj, int&, int&, bool& scj) { shj = INFINITY; scj = false; });
    int i = cur, sink = -1;
    double minval = 0.0;
    while (sink < 0) {
      const double ui = u[i];
      double bd = INFINITY;
      int bkey = INT_MAX, br4 = -1;
      for_cols([&](int j, double& vj, double& shj, int& paj, int& r4j, bool& scj) {
        if (scj) return;
        const double c = CACHED ? cost[i * nc + j] : pair_cost(i, j);
        const double r = __dsub_rn(__dsub_rn(__dadd_rn(minval, c), ui), vj);
        if (r < shj) { shj = r; paj = i; }
        const int key = (r4j >= 0 ? AS_OWNED : 0) | j;
        if (shj < bd || (shj == bd && key < bkey)) { bd = shj; bkey = key; br4 = r4j; }
      });
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int ok = __shfl_xor(bkey, o, 64);
        if (od < bd || (od == bd && ok < bkey)) { bd = od; bkey = ok; }
      }
      // no unreached column within a finite distance (the fold lets a column at +inf through, and an overflowed cost makes
      // one): the problem has no finite augmenting path.  Decided before anything is marked reached or any dual moves.
      if (!(bd < INFINITY)) { failed = true; break; }
      const int j = bkey & (AS_OWNED - 1);
      const int owner = __shfl(br4, j & 63, 64);        // that lane's best is column j
      minval = bd;
      for_cols([&](int jj, double&, double&, int&, int&, bool& scj) { if (jj == j) scj = true; });
      if (owner < 0) sink = j; else i = owner;
    }
    if (failed) break;
    // duals: the rows reached are cur and the owners of the reached columns
    as_wave_sync();
    if (lane == 0) u[cur] = __dadd_rn(u[cur], minval);
    for_cols([&](int, double& vj, double& shj, int&, int& r4j, bool& scj) {
      if (!scj) return;
      const double dlt = __dsub_rn(minval, shj);
      vj = __dsub_rn(vj, dlt);
      if (r4j >= 0) u[r4j] = __dadd_rn(u[r4j], dlt);
    });
    as_wave_sync();
    // augment along the predecessors, from the sink back to cur
    int j = sink;
    for (int guard = 0; guard <= nr; ++guard) {
      const int ip = fetch(pa, Lpa, j);
      for_cols([&](int jj, double&, double&, int&, int& r4j, bool&) { if (jj == j) r4j = ip; });
      const int prev = c4r[ip];
      as_wave_sync();
      if (lane == 0) c4r[ip] = j;
      as_wave_sync();
      j = prev;
      if (ip == cur) break;
    }
  }
  if (failed) {
    if (lane == 0) {
      atomicOr(a.status, ASSIGN_ST_INFEASIBLE);
      if (rsq) *rsq = NAN;
      if (di) *di = NAN;
    }
    return;
  }

  // ---- results
  if (a.out_rows) {
    if (!a.swapped) {
      for (int i = lane; i < nr; i += 64) {
        a.out_rows[i] = i;
        a.out_cols[i] = c4r[i];
        a.out_costs[i] = pair_cost(i, c4r[i]);
      }
    } else {   // the columns are XY's rows: the owned ones in ascending order
      int at = 0;
      for (int j0 = 0; j0 < nc; j0 += 64) {
        const int j = j0 + lane;
        int mine = -1;
        for_cols([&](int jj, double&, double&, int&, int& r4j, bool&) { if (jj == j) mine = r4j; });
        const unsigned long long mask = __ballot(mine >= 0);
        if (mine >= 0) {
          const int p = at + __popcll(mask & ((1ull << lane) - 1ull));
          if (p < nr) {   // nr columns have an owner
            a.out_rows[p] = j;
            a.out_cols[p] = mine;
            a.out_costs[p] = pair_cost(mine, j);
          }
        }
        at += __popcll(mask);
      }
    }
  }
  if (scal || rsq || di || aprime || bprime) {
    as_regress([&](int i, double& x, double& y, double& p, double& q) {
      const int j = c4r[i];
      x = rowc[i]; y = rowc[nr + i]; p = colc[j]; q = colc[nc + j];
    }, nr, lane, scal, aprime, bprime, rsq, di);
  }
}

__global__ __launch_bounds__(256) void assign_samples_kernel(const long long* __restrict__ s, long long count,
                                                             long long m, unsigned long long* __restrict__ bad) {
  unsigned long long c = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256)
    c += (unsigned long long)s[i] >= (unsigned long long)m;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(bad, c);   // an integer count: any order gives the same value
}

inline int assign_launch(const AssignArgs& a, int dim, hipStream_t stream) {
  if (!a.solve) {
    hipLaunchKernelGGL((assign_kernel<2, false>), dim3((unsigned)a.k), dim3(64), 0, stream, a);
    SMRF_LAUNCH_CHECK();
    return SMRF_OK;
  }
  const AssignRoute r = assign_route(a.nr, a.nc, dim);
  const int waves = (int)std::min<long long>(r.waves, a.k);
  const size_t lds = (size_t)waves * r.wave_bytes;
  AssignArgs b = a;
  b.wave_bytes = r.wave_bytes;
  const dim3 grid((unsigned)((a.k + waves - 1) / waves)), block(64 * waves);
#define AS_GO(D, C)                                                                                              \
  do {                                                                                                           \
    if (lds > 48 * 1024)                                                                                         \
      SMRF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(assign_kernel<D, C>),                     \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)AS_LDS_WG));           \
    hipLaunchKernelGGL((assign_kernel<D, C>), grid, block, lds, stream, b);                                      \
  } while (0)
  if (dim == 2) { if (r.cached) AS_GO(2, true); else AS_GO(2, false); }
  else { if (r.cached) AS_GO(3, true); else AS_GO(3, false); }
#undef AS_GO
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

inline bool assign_in_range(int64_t nrows, int64_t ncols, int dim) {
  return nrows >= 1 && ncols >= 1 && nrows <= assign_limit() && ncols <= assign_limit() && (dim == 2 || dim == 3);
}

}  // namespace smrf

extern "C" {

int smrf_assign_limit(void) { return smrf::assign_limit(); }

size_t smrf_assign_workspace_bytes(int64_t nrows, int64_t ncols, int dim) {
  return smrf::assign_in_range(nrows, ncols, dim) ? smrf::AS_WS_BYTES : 0;
}

int smrf_assign_route(int64_t nrows, int64_t ncols, int dim, int* h_route) {
  using namespace smrf;
  if (!h_route) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (!assign_in_range(nrows, ncols, dim))
    return smrf_fail(SMRF_E_ARG, "a %lld x %lld assignment of dimension %d: 1 to %d points of dimension 2 or 3 expected",
                     (long long)nrows, (long long)ncols, dim, assign_limit());
  const int nr = (int)std::min(nrows, ncols), nc = (int)std::max(nrows, ncols);
  const AssignRoute r = assign_route(nr, nc, dim);
  h_route[0] = AS_REG_COLS;
  h_route[1] = r.cached;
  h_route[2] = r.waves;
  h_route[3] = (int)r.wave_bytes;
  h_route[4] = assign_cached_square(dim);
  return SMRF_OK;
}

int smrf_assign_solve_f64(const double* d_xy, int64_t nrows, const double* d_ab, int64_t ncols, int dim,
                          int64_t* d_row_ind, int64_t* d_col_ind, double* d_costs, void* d_workspace,
                          size_t workspace_bytes, void* stream_) {
  using namespace smrf;
  hipStream_t stream = (hipStream_t)stream_;
  if (!assign_in_range(nrows, ncols, dim))
    return smrf_fail(SMRF_E_ARG, "a %lld x %lld assignment of dimension %d: 1 to %d points of dimension 2 or 3 expected",
                     (long long)nrows, (long long)ncols, dim, assign_limit());
  if (!d_xy || !d_ab || !d_row_ind || !d_col_ind || !d_costs) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (!d_workspace || workspace_bytes < AS_WS_BYTES)
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, AS_WS_BYTES);
  AssignArgs a{};
  a.swapped = nrows > ncols;
  a.rowpts = a.swapped ? d_ab : d_xy;
  a.colpts = a.swapped ? d_xy : d_ab;
  a.nr = (int)std::min(nrows, ncols);
  a.nc = (int)std::max(nrows, ncols);
  a.m = a.nc;
  a.k = 1;
  a.solve = 1;
  a.out_rows = (long long*)d_row_ind;
  a.out_cols = (long long*)d_col_ind;
  a.out_costs = d_costs;
  a.status = (int*)((char*)d_workspace + 8);
  SMRF_HIP_CHECK(hipMemsetAsync(d_workspace, 0, 16, stream));
  return assign_launch(a, dim, stream);
}

int smrf_assign_samples_check(const int64_t* d_samples, int64_t k, int64_t n, int64_t m, int64_t* h_bad,
                              void* d_workspace, size_t workspace_bytes, void* stream_) {
  using namespace smrf;
  hipStream_t stream = (hipStream_t)stream_;
  if (k < 1 || n < 1 || m < 1 || k > INT_MAX || n > assign_limit())
    return smrf_fail(SMRF_E_ARG, "a (%lld, %lld) sample table over %lld points", (long long)k, (long long)n, (long long)m);
  if (!d_samples || !h_bad) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (!d_workspace || workspace_bytes < AS_WS_BYTES)
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, AS_WS_BYTES);
  SMRF_HIP_CHECK(hipMemsetAsync(d_workspace, 0, 16, stream));
  hipLaunchKernelGGL(assign_samples_kernel, dim3(smrf_blocks(k * n, 1024)), dim3(256), 0, stream,
                     (const long long*)d_samples, (long long)(k * n), (long long)m, (unsigned long long*)d_workspace);
  SMRF_LAUNCH_CHECK();
  SMRF_HIP_CHECK(hipMemcpyAsync(h_bad, d_workspace, 8, hipMemcpyDeviceToHost, stream));
  SMRF_HIP_CHECK(hipStreamSynchronize(stream));
  return SMRF_OK;
}

int smrf_assign_bdr_f64(const double* d_xy, int64_t n, const double* d_ab, int64_t m, const int64_t* d_samples,
                        int64_t k, int solve, double* d_scalars, double* d_aprime, double* d_bprime, double* d_rsquare,
                        double* d_di, void* d_workspace, size_t workspace_bytes, void* stream_) {
  using namespace smrf;
  hipStream_t stream = (hipStream_t)stream_;
  if (n < 3 || n > INT_MAX / 2) return smrf_fail(SMRF_E_ARG, "a regression over %lld points: at least 3 expected", (long long)n);
  if (k < 1 || k > INT_MAX) return smrf_fail(SMRF_E_ARG, "%lld samples", (long long)k);
  if (solve && n > assign_limit())
    return smrf_fail(SMRF_E_ARG, "%lld points to match: at most %d", (long long)n, assign_limit());
  if (m < 1 || (!d_samples && m != n))
    return smrf_fail(SMRF_E_ARG, "%lld points against %lld", (long long)n, (long long)m);
  if (!solve && (k != 1 || d_samples)) return smrf_fail(SMRF_E_ARG, "samples need the solve");
  if (!d_xy || !d_ab) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (!d_scalars && !d_rsquare && !d_di) return smrf_fail(SMRF_E_ARG, "null output");
  if (!d_workspace || workspace_bytes < AS_WS_BYTES)
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, AS_WS_BYTES);
  AssignArgs a{};
  a.rowpts = d_xy;
  a.colpts = d_ab;
  a.samples = (const long long*)d_samples;
  a.nr = a.nc = (int)n;
  a.m = m;
  a.k = k;
  a.solve = solve != 0;
  a.scal = d_scalars;
  a.aprime = d_aprime;
  a.bprime = d_bprime;
  a.rsq = d_rsquare;
  a.di = d_di;
  a.status = (int*)((char*)d_workspace + 8);
  SMRF_HIP_CHECK(hipMemsetAsync(d_workspace, 0, 16, stream));
  return assign_launch(a, 2, stream);
}

}  // extern "C"
