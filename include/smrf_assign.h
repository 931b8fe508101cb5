/* The point-set matching block of the C ABI of libsmrf_hip.so (gfx950).  Included by smrf_hip.h, inside its extern "C"
 * region and after its SMRF_API and status codes; include that header, not this one. */
#ifndef SMRF_ASSIGN_H
#define SMRF_ASSIGN_H
#ifndef SMRF_HIP_H
#error "include smrf_hip.h: smrf_assign.h is a part of it"
#endif

/* ------------------------------------------------------------------------------------------
 * point-set matching: assignment and bidimensional regression (neilpy_amd/matching.py)
 * ------------------------------------------------------------------------------------------ */
/* Clouds are contiguous float64 (n, dim) arrays, dim 2 or 3, finite.  One problem is solved by one wave64 out of its
 * slice of LDS: the coordinates, the row duals and, from column 256 on, the per-column state.  Without the cost matrix
 * a problem of nr <= nc points takes 8 (dim + 1) nr + 4 nr + 8 dim nc + 28 max(0, nc - 256) bytes, and one workgroup may
 * claim the 160 KiB of a gfx950 CU; smrf_assign_limit() is the largest n whose n x n problem of dimension 3 fits, 1943.
 * Either side of a problem may be that long, no longer.
 * smrf_assign_workspace_bytes(nrows, ncols, dim) bytes of device scratch (0 for arguments out of range) serve every call
 * below: an int64 count of sample entries out of range, then an int32 status that the solve ORs into (1: a problem had
 * no finite augmenting path, which takes an overflowed cost; 2: a sample entry out of range met in the launch).  The
 * calls clear it first. */
SMRF_API int smrf_assign_limit(void);
SMRF_API size_t smrf_assign_workspace_bytes(int64_t nrows, int64_t ncols, int dim);
/* How the library would run an nrows x ncols problem: h_route[0] = the number of columns whose state lives in registers
 * (the columns from there on keep it in LDS), [1] = 1 when the cost matrix is kept in LDS, 0 when costs are recomputed
 * from the coordinates, [2] = waves (problems) per workgroup of a large batch, [3] = LDS bytes per wave, [4] = the
 * largest n whose n x n problem of this dimension keeps its costs in LDS. */
SMRF_API int smrf_assign_route(int64_t nrows, int64_t ncols, int dim, int* h_route);
/* hungarian_algorithm(): the minimum-cost assignment of d_xy (nrows, dim) to d_ab (ncols, dim) under the cost
 * sqrt((x0-a0)*(x0-a0) + (x1-a1)*(x1-a1) [+ (x2-a2)*(x2-a2)]), every operation rounded.  min(nrows, ncols) entries each:
 * d_row_ind ascending, d_col_ind, d_costs = the cost of each pair.  Shortest augmenting paths with float64 duals; among
 * columns at the lowest tentative distance an unassigned one, among those the lowest index.  One launch of one wave. */
SMRF_API int smrf_assign_solve_f64(const double* d_xy, int64_t nrows, const double* d_ab, int64_t ncols, int dim,
                     int64_t* d_row_ind, int64_t* d_col_ind, double* d_costs, void* d_workspace,
                     size_t workspace_bytes, void* stream);
/* h_bad = the number of the k * n entries of d_samples outside 0 .. m - 1, in one reduction (an integer count).
 * Synchronises the stream. */
SMRF_API int smrf_assign_samples_check(const int64_t* d_samples, int64_t k, int64_t n, int64_t m, int64_t* h_bad,
                     void* d_workspace, size_t workspace_bytes, void* stream);
/* bdr() / bdr_bootstrap(): k bidimensional regressions of d_ab's points on d_xy (n, 2), n >= 3, in one launch.
 * solve == 0: k = 1, m = n, no samples: row i of d_ab belongs to row i of d_xy (any n).  solve != 0: sample s is the rows
 * d_samples[s][0 .. n) of d_ab (m, 2) (NULL: m = n, the rows in order); its wave solves the n x n assignment against
 * d_xy as the call above does, n <= smrf_assign_limit(), and regresses the matched points.  Per sample: d_scalars[s][9] =
 * beta1 beta2 alpha1 alpha2 rsquare D Dmax DI F, d_aprime[s][n], d_bprime[s][n], d_rsquare[s], d_di[s]; any may be NULL,
 * not all of scalars, rsquare and DI.  float64 add, multiply, divide and square root, each rounded; a sum takes element
 * l, l + 64, ... on lane l from +0.0, then p += p[lane ^ o] for o = 32 .. 1.  No float atomics. */
SMRF_API int smrf_assign_bdr_f64(const double* d_xy, int64_t n, const double* d_ab, int64_t m, const int64_t* d_samples,
                     int64_t k, int solve, double* d_scalars, double* d_aprime, double* d_bprime, double* d_rsquare,
                     double* d_di, void* d_workspace, size_t workspace_bytes, void* stream);

#endif /* SMRF_ASSIGN_H */
