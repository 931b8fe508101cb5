/* The rank-filter block of the C ABI of libsmrf_hip.so (gfx950): scipy.ndimage.rank_filter / median_filter /
 * percentile_filter / minimum_filter / maximum_filter of a 2-D raster by a flat footprint (neilpy_amd/rank.py,
 * csrc/rank.hip).  A header of its own beside smrf_hip.h: it takes SMRF_API and the SMRF_E_* status
 * codes from there, and its prototypes are bound by neilpy_amd/rank.py on the library neilpy_amd._lib.load() returns. */
#ifndef SMRF_RANK_H
#define SMRF_RANK_H

#include "smrf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMRF_RANK_REFLECT 0 /* border mode 'reflect': the period-2n fold (d c b a | a b c d | d c b a) */
#define SMRF_RANK_NEAREST 1 /* border mode 'nearest': indices clamped to the raster */

/* impl = a selection method, plus at most one of the two sample-source flags */
#define SMRF_RANK_IMPL_AUTO 0    /* COUNT up to smrf_rank_count_max_taps(elem_size) members, BISECT above */
#define SMRF_RANK_IMPL_COUNT 1   /* position of every member by counting: n^2 compares */
#define SMRF_RANK_IMPL_BISECT 2  /* radix select on the key, one bit per pass: at most (key bits + 1) n compares */
#define SMRF_RANK_IMPL_GLOBAL 8  /* every sample from global memory, through the border rule */
#define SMRF_RANK_IMPL_TILE 16   /* tile + halo as keys in LDS, (8 + bh - 1) x (64 + bw - 1) keys and ntaps int32 offsets
                                    behind them; SMRF_E_UNSUPPORTED when that passes SMRF_RANK_TILE_BYTES.
                                    Neither flag: TILE while it fits, GLOBAL otherwise */

/* what smrf_rank_path returns: a method bit or'ed with a source bit */
#define SMRF_RANK_PATH_COUNT 0
#define SMRF_RANK_PATH_BISECT 1
#define SMRF_RANK_PATH_TILE 0
#define SMRF_RANK_PATH_GLOBAL 2

#define SMRF_RANK_TILE_BYTES 53248 /* LDS of one workgroup's tile: the footprint family's cap, three workgroups per CU */
#define SMRF_RANK_COUNT_BLOCK 8    /* candidates the COUNT method holds in registers per sweep of the members */
/* The largest member count the automatic choice gives to COUNT (profiles/rank_bench.md: the largest all-ones square at
 * which COUNT was not slower than BISECT on the terrain raster).  Speed only: both methods give the same bits. */
#define SMRF_RANK_COUNT_MAX_TAPS_F32 25
#define SMRF_RANK_COUNT_MAX_TAPS_F64 81

/* The LDS a workgroup of the TILE source may take, SMRF_RANK_TILE_BYTES. */
SMRF_API int smrf_rank_tile_bytes(void);
/* SMRF_RANK_COUNT_MAX_TAPS_* for elem_size 4 or 8; SMRF_E_ARG otherwise. */
SMRF_API int smrf_rank_count_max_taps(int elem_size);
/* The path a launch with this plan head takes under impl, SMRF_RANK_PATH_{COUNT,BISECT} | SMRF_RANK_PATH_{TILE,GLOBAL},
 * or a negative SMRF_E_* code where the launch would be refused (a malformed head, an unknown impl, TILE forced on a
 * tile that does not fit).  Host logic only. */
SMRF_API int smrf_rank_path(const int* h_head, int elem_size, int impl);
/* One launch over a contiguous rows x cols raster: d_out[r, c] = the element at position `rank` (0 <= rank < ntaps,
 * checked here) of the cell's ntaps samples sorted ascending, the samples X[idx(r + drow), idx(c + dcol)] with idx the
 * border mode's index rule.  h_head (host, 24 int32) and d_plan (device) are neilpy_amd.morphology.plan's of the
 * erosion, as smrf_footprint_filter_* takes them; of the head ntaps, r_lo, c_lo, bh, bw are read, of the plan its first
 * ntaps (drow, dcol) records.  -0.0 sorts before +0.0.  nan_aware 1: NaN sorts after +inf whatever its sign, so a cell
 * is NaN iff fewer than rank + 1 of its samples are not NaN; nan_aware 0 promises a raster without NaN.  Every global
 * index goes through idx and every LDS index is clamped to the tile, whatever the plan holds. */
SMRF_API int smrf_rank_filter_f32(const float* d_in, float* d_out, int rows, int cols, const void* d_plan,
                   const int* h_head, int rank, int mode, int nan_aware, int impl, void* stream);
SMRF_API int smrf_rank_filter_f64(const double* d_in, double* d_out, int rows, int cols, const void* d_plan,
                   const int* h_head, int rank, int mode, int nan_aware, int impl, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SMRF_RANK_H */
