/*
 * smrf_hip.h -- C ABI of libsmrf_hip.so: the MI355X (gfx950) implementation of neilpy's
 * SMRF bare-earth path.
 *
 * The reference (thomaspingel/neilpy) is a pure-Python function library with no FFI of its
 * own; the interfaces this library replaces are therefore the Python callables of the path
 * and the third-party primitives they dispatch to.  Each entry point cites what it replaces
 * (paths relative to the reference checkout):
 *
 *   smrf_disk_filter_*        skimage.morphology.erosion/dilation with disk(r) as reached by
 *                             opening(last_surface, disk(window)), neilpy/neilpy.py:1670
 *                             (-> scipy.ndimage.grey_erosion/grey_dilation, mode='reflect')
 *   smrf_progressive_filter_* progressive_filter(), neilpy/neilpy.py:1659-1680
 *   smrf_points_extent_f64,
 *   smrf_grid_*               create_dem(), neilpy/neilpy.py:1110-1166 (pandas groupby min/max
 *                             at :1151-1156, affine index arithmetic at :1141-1143)
 *   smrf_points_band_count_f64, smrf_points_band_pack_f64
 *                             the same index arithmetic (:1141-1143) used to route points to the rank that owns
 *                             their raster row when the cloud is sharded over GPUs (no counterpart in the reference)
 *   smrf_springs_lsqr_f64     inpaint_nans_by_springs(), neilpy/neilpy.py:1227-1271, whose
 *                             solve is scipy.sparse.linalg.lsqr (:1264)
 *   smrf_fda_lsqr_f64         inpaint_nans_by_fda(), neilpy/neilpy.py:1170-1216
 *   smrf_fda_apply_f64        (diagnostic) the same operator applied once, for the structural parity test
 *   smrf_gradient_slope_f64   np.gradient + sqrt, neilpy/neilpy.py:1785-1786
 *   smrf_pssm_f64             pssm(), neilpy/neilpy.py:846-867
 *   smrf_las_decode_xyz_f64   the coordinate decode of read_las(), neilpy/neilpy.py:903-1087 (host
 *                             side: neilpy_amd/las.py)
 *   smrf_spline_solve_f64, smrf_spline_solve_ws_f64, smrf_spline_eval_f64, smrf_classify_points_f64
 *                             RectBivariateSpline(...).ev and the point test, neilpy/neilpy.py:1768-1795
 *   smrf_negate_f64, smrf_mask_apply_f64
 *                             the elementwise glue of smrf(), neilpy/neilpy.py:1744, :1748, :1762-1763
 *   smrf_terrain_rays_*       openness(), skyview_factor(), count_openness(), geomorphons() and
 *                             ternary_pattern_from_openness(), neilpy/neilpy.py:1290-1653 (host side:
 *                             neilpy_amd/terrain.py)
 *   smrf_surface_*            slope(), aspect(), hillshade(), multiple_illumination(), esri_slope(), curvature(),
 *                             esri_curvature(), zevenbergen_and_thorne_curvature(), evans_curvature() and
 *                             wilson_gallant_curvature(), neilpy/neilpy.py:434-842 (host side: neilpy_amd/surface.py)
 *   smrf_focal_*              std(), topographic_position_index() and reduce_peaks(), neilpy/neilpy.py:2039-2124,
 *                             each scipy.ndimage.convolve(mode='nearest') plus cell-wise arithmetic (host side:
 *                             neilpy_amd/focal.py)
 *   smrf_morphometry_*, smrf_vip_*, smrf_ashift_*
 *                             scaled_morphometry(), vip_score() and ashift(), neilpy/neilpy.py:2472, :1832, :1290
 *                             (host side: neilpy_amd/morphometry.py)
 *   smrf_footprint_*          scipy.ndimage.grey_erosion / grey_dilation with any flat footprint, modes 'reflect' and
 *                             'nearest', and the openings, closings, top-hats and gradient composed of them (host
 *                             side: neilpy_amd/morphology.py)
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory (hipMalloc or a torch CUDA tensor's data_ptr);
 *     h_* is host memory.  The library never allocates or frees caller-visible memory; scratch
 *     comes from the caller through (workspace, workspace_bytes).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Unless stated, calls
 *     only enqueue work on `stream` and return without synchronising.
 *   - return value: 0 on success, a negative SMRF_E_* code on failure; smrf_last_error() gives
 *     a human-readable message for the calling thread.  No exceptions cross the boundary.
 *   - rasters are row-major, row 0 = north, `ld` = elements between consecutive rows.
 *   - a caller's data pointer (rasters, clouds, tables, outputs) needs the alignment of its element and nothing
 *     wider: any row or element slice of an array is valid input, and every plane is dense (contiguous but for `ld`).
 *     The one exception says so and refuses: smrf_voxel_expand writes d_out in dwords and returns SMRF_E_ARG for a
 *     d_out that is not 4-byte aligned.  A workspace is different: the library lays its parts out at multiples of
 *     256 bytes from the workspace's base and relies on the base being 256-byte aligned, as hipMalloc's and torch's
 *     allocations are, for the alignment of every part's element (8 bytes at the most).  Allocate
 *     *_workspace_bytes(...) bytes with either and pass the allocation's own base.
 *   - there is no CPU fallback: without a HIP device every compute entry returns SMRF_E_HIP.
 */
#ifndef SMRF_HIP_H
#define SMRF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMRF_ABI_VERSION 1

#if defined(__GNUC__)
#define SMRF_API __attribute__((visibility("default")))
#else
#define SMRF_API
#endif

#define SMRF_OK 0
#define SMRF_E_ARG (-1)       /* invalid argument (null pointer, bad size, band does not cover halo) */
#define SMRF_E_HIP (-2)       /* a HIP runtime call failed, or no device */
#define SMRF_E_WORKSPACE (-3) /* workspace too small */
#define SMRF_E_RANGE (-4)     /* a point falls outside the grid (create_dem with edges=) */
#define SMRF_E_UNSUPPORTED (-5)

/* implementation selector for the disk filter (tests exercise both; 0 is the product default) */
#define SMRF_IMPL_AUTO 0
#define SMRF_IMPL_RING 1   /* register-ring kernels, radius 1..SMRF_RING_MAX_RADIUS */
#define SMRF_IMPL_DIRECT 2 /* footprint-gather kernel, any radius */
#define SMRF_RING_MAX_RADIUS 64

SMRF_API int smrf_abi_version(void);
SMRF_API const char* smrf_last_error(void);
/* number of visible HIP devices (0 when there is none); never fails */
SMRF_API int smrf_device_count(void);
/* (diagnostic) The SMRF_* environment switches (SMRF_FUSED, SMRF_CHAIN, SMRF_NT, SMRF_RING_DUAL, SMRF_RING_SEG, ... - developer
 * A/B runs and the parity tests that force every launch variant on small rasters) are read ONCE, when the library first needs
 * them; no launch path calls getenv.  A process that changes them afterwards calls this to have them read again.  Not
 * thread-safe against concurrent launches. */
SMRF_API void smrf_switches_reload(void);

/* ------------------------------------------------------------------------------------------
 * Grey erosion / dilation by skimage's disk(radius) with scipy's mode='reflect' borders.
 *
 * The raster has `img_rows` x `cols` cells.  `d_in` holds global rows
 * [in_row0, in_row0+in_rows), `d_out` receives global rows [out_row0, out_row0+out_rows);
 * both pointers address the first row they hold.  Single GPU: in_row0 = out_row0 = 0 and
 * in_rows = out_rows = img_rows.  Row-band sharding: every row reflect(y) for
 * y in [out_row0-radius, out_row0+out_rows+radius) must lie inside the input band
 * (otherwise SMRF_E_ARG).
 *
 * nan_aware != 0 reproduces scipy's NaN rule (the result is NaN iff the first visited
 * footprint element, offset (-radius, 0), is NaN; other NaNs are ignored); 0 assumes the input
 * has no NaN and skips the extra read.
 * ------------------------------------------------------------------------------------------ */
SMRF_API int smrf_disk_filter_f32(const float* d_in, float* d_out, int img_rows, int cols, int64_t ld,
                         int in_row0, int in_rows, int out_row0, int out_rows, int radius,
                         int is_dilate, int nan_aware, int impl, void* stream);
SMRF_API int smrf_disk_filter_f64(const double* d_in, double* d_out, int img_rows, int cols, int64_t ld,
                         int in_row0, int in_rows, int out_row0, int out_rows, int radius,
                         int is_dilate, int nan_aware, int impl, void* stream);

/* One progressive_filter step after the erosion: opened = dilate(eroded, disk(radius)), then
 *   new_obj = (double)(last - opened) > threshold   (subtraction in the raster dtype,
 *   comparison in float64: NumPy-2 promotion of neilpy.py:1671)
 *   mask |= new_obj;  when_dropped[new_obj] = window_index   (d_when_dropped may be NULL)
 * d_last, d_opened, d_mask, d_when_dropped address global row out_row0. */
SMRF_API int smrf_pf_dilate_flag_f32(const float* d_eroded, const float* d_last, float* d_opened,
                            uint8_t* d_mask, uint8_t* d_when_dropped, double threshold,
                            int window_index, int img_rows, int cols, int64_t ld, int in_row0,
                            int in_rows, int out_row0, int out_rows, int radius, int nan_aware,
                            int impl, void* stream);
SMRF_API int smrf_pf_dilate_flag_f64(const double* d_eroded, const double* d_last, double* d_opened,
                            uint8_t* d_mask, uint8_t* d_when_dropped, double threshold,
                            int window_index, int img_rows, int cols, int64_t ld, int in_row0,
                            int in_rows, int out_row0, int out_rows, int radius, int nan_aware,
                            int impl, void* stream);

/* One progressive_filter window in ONE launch for the small disks (csrc/morph_fused.h): opened =
 * dilate(erode(last, disk(radius)), disk(radius)) and the flag step of smrf_pf_dilate_flag_*, the eroded
 * surface never leaving the CU.  Row-band form as above, with the band of `last` reaching 2*radius rows
 * (reflected at the raster's true borders) beyond the output rows: d_last holds global rows in_row0 ..
 * in_row0 + in_rows - 1; d_opened, d_mask, d_when_dropped address global row out_row0; the same `last` values
 * are used for the flag comparison.  d_mask may be NULL (opening only).  No NaN rule: the caller must not hand
 * it rasters with NaNs.  Returns SMRF_E_UNSUPPORTED for radii without a fused kernel
 * (smrf_fused_open_supported tells which: fp32 1..8 and 10..14, fp64 1..6; csrc/pf_route.h). */
SMRF_API int smrf_fused_open_supported(int elem_size, int radius);
SMRF_API int smrf_pf_open_flag_f32(const float* d_last, float* d_opened, uint8_t* d_mask, uint8_t* d_when_dropped,
                          double threshold, int window_index, int img_rows, int cols, int64_t ld, int in_row0,
                          int in_rows, int out_row0, int out_rows, int radius, void* stream);
SMRF_API int smrf_pf_open_flag_f64(const double* d_last, double* d_opened, uint8_t* d_mask, uint8_t* d_when_dropped,
                          double threshold, int window_index, int img_rows, int cols, int64_t ld, int in_row0,
                          int in_rows, int out_row0, int out_rows, int radius, void* stream);

/* Several CONSECUTIVE progressive_filter windows with small disks in ONE launch (csrc/morph_chain.h): opens `last` with
 * disk(h_radii[0]), flags, opens the result with disk(h_radii[1]), flags, ...; only the LAST opened surface is written
 * (d_opened), every window's flags go to d_mask / d_when_dropped (window i writes h_window_index[i]) exactly as a sequence of
 * smrf_pf_open_flag_* calls would.  Replaces n iterations of the loop of neilpy/neilpy.py:1667-1676.  Row-band form: the band
 * of `last` must reach sum(2 * radius) rows (reflected at the raster's true borders) beyond the output rows; flags are
 * written for the output rows only.  No NaN rule.  smrf_pf_chain_length: how many of the windows at the head of h_radii one
 * launch takes on a raster of raster_cells cells (0: none; e.g. 3 for 1, 2, 3, ...; 1 = a table-free single launch; the pattern table of csrc/pf_route.h);
 * smrf_pf_chain_flag_* returns SMRF_E_UNSUPPORTED unless n_windows is a length this function reports for those radii
 * at some raster size. */
SMRF_API int smrf_pf_chain_length(int elem_size, const int32_t* h_radii, int n, int64_t raster_cells);
SMRF_API int smrf_pf_chain_flag_f32(const float* d_last, float* d_opened, uint8_t* d_mask, uint8_t* d_when_dropped,
                           const int32_t* h_radii, const double* h_thresholds, const int32_t* h_window_index,
                           int n_windows, int img_rows, int cols, int64_t ld, int in_row0, int in_rows, int out_row0,
                           int out_rows, void* stream);
SMRF_API int smrf_pf_chain_flag_f64(const double* d_last, double* d_opened, uint8_t* d_mask, uint8_t* d_when_dropped,
                           const int32_t* h_radii, const double* h_thresholds, const int32_t* h_window_index,
                           int n_windows, int img_rows, int cols, int64_t ld, int in_row0, int in_rows, int out_row0,
                           int out_rows, void* stream);

/* Whole progressive_filter on one device.  d_Z is read only.  h_windows / h_thresholds are HOST
 * arrays of n_windows entries; thresholds are slope_threshold*(windows*cellsize) evaluated by
 * the caller in float64 (neilpy.py:1661).  d_mask (rows*cols bytes, 0/1) and d_when_dropped
 * (may be NULL) are overwritten.  Workspace: smrf_progressive_filter_workspace_bytes().
 * nan_aware < 0: the library counts NaNs itself (one small synchronising readback). */
SMRF_API size_t smrf_progressive_filter_workspace_bytes(int rows, int cols, int elem_size);
SMRF_API int smrf_progressive_filter_f32(const float* d_Z, int rows, int cols, const int32_t* h_windows,
                                const double* h_thresholds, int n_windows, uint8_t* d_mask,
                                uint8_t* d_when_dropped, void* d_workspace,
                                size_t workspace_bytes, int nan_aware, int impl, void* stream);
SMRF_API int smrf_progressive_filter_f64(const double* d_Z, int rows, int cols, const int32_t* h_windows,
                                const double* h_thresholds, int n_windows, uint8_t* d_mask,
                                uint8_t* d_when_dropped, void* d_workspace,
                                size_t workspace_bytes, int nan_aware, int impl, void* stream);

/* Measurement form of the same call (bench.py's per-class roofline, tools/): an event is recorded on `stream` at
 * every window boundary and, after the last window has finished (the call synchronises), h_window_ms[i] holds the
 * device time of window i and h_window_route[i] (may be NULL) how it ran: SMRF_ROUTE_*.  Same result, same routing
 * as smrf_progressive_filter_*; no reference counterpart (the reference has no timers). */
#define SMRF_ROUTE_TWO_PASS 0   /* ring erosion, then ring dilation + flag: 5s + 2 B/cell (s = sizeof element) */
#define SMRF_ROUTE_FUSED 1      /* one fused opening + flag launch: 2s + 2 B/cell */
#define SMRF_ROUTE_DIRECT 2     /* footprint-gather kernels, two passes (radius > SMRF_RING_MAX_RADIUS or impl = direct) */
#define SMRF_ROUTE_COPY 3       /* radius 0 */
#define SMRF_ROUTE_CHAIN 4      /* table-free launch of morph_chain.h: route = 4 + position in a chain of windows opened in one launch (its
                                 * time is reported on position 0, the others read ~0); a single window is a chain of one */
SMRF_API int smrf_progressive_filter_timed_f32(const float* d_Z, int rows, int cols, const int32_t* h_windows,
                                const double* h_thresholds, int n_windows, uint8_t* d_mask,
                                uint8_t* d_when_dropped, void* d_workspace, size_t workspace_bytes, int nan_aware,
                                int impl, void* stream, float* h_window_ms, int32_t* h_window_route);
SMRF_API int smrf_progressive_filter_timed_f64(const double* d_Z, int rows, int cols, const int32_t* h_windows,
                                const double* h_thresholds, int n_windows, uint8_t* d_mask,
                                uint8_t* d_when_dropped, void* d_workspace, size_t workspace_bytes, int nan_aware,
                                int impl, void* stream, float* h_window_ms, int32_t* h_window_route);

/* Which windows of the calling host thread's latest smrf_progressive_filter_* call took their erosion from the window
 * before (e_R = min(erode(e_{R-1}, cross), leftover cells of the opened surface): bit-identical to the ring erosion; taken
 * for a two-pass window whose radius is the previous two-pass window's + 1 on a raster without NaN, switch SMRF_ERO_INC =
 * 0 never / 1 per measured table / 2 always).  Writes n bytes (0 / 1; 0 beyond the call's windows) and returns the
 * call's window count.  Such a window still reports SMRF_ROUTE_TWO_PASS: it is two launches, 3s + (3s + 2) B/cell. */
SMRF_API int smrf_pf_ero_inc_windows(uint8_t* h_taken, int n);

/* The launch plan of progressive_filter, without running anything (host logic, no device needed; csrc/pf_route.h is the single
 * statement of the rule): h_route[i] = the SMRF_ROUTE_* that smrf_progressive_filter_timed_* reports for window i of the n
 * h_windows on a `rows`-row raster of `cells` cells, h_ero_inc[i] = what smrf_pf_ero_inc_windows reports, under the library's
 * SMRF_FUSED / SMRF_CHAIN / SMRF_ERO_INC switches.  nan_aware: 0 = a raster without NaN, anything else = one that may hold
 * some (a call with nan_aware < 0 finds out which and then follows that plan).  band = 0: the whole-raster call.  band = 1: the
 * row-band driver (neilpy_amd/sharded.py) - rows = the image's rows, cells = what one launch marches (the longest band with its
 * two-sided margin); the launch at the head of the list is h_route[0], smrf_pf_chain_flag_* when it reads SMRF_ROUTE_CHAIN
 * (with the windows that read SMRF_ROUTE_CHAIN + 1, + 2 after it), smrf_pf_open_flag_* for SMRF_ROUTE_FUSED, else the two
 * passes; a band takes fused openings up to radius 8 only and no incremental erosion.  band = 2: a row band whose launches
 * cannot be chained either (one split edge-first, or a single band). */
SMRF_API int smrf_pf_plan(int elem_size, const int32_t* h_windows, int n, int rows, int64_t cells, int nan_aware, int impl,
                 int band, int32_t* h_route, uint8_t* h_ero_inc);

/* number of NaN cells of a contiguous array, written to *h_count (synchronises `stream`) */
SMRF_API int smrf_count_nan_f32(const float* d_a, int64_t n, int64_t* h_count, void* stream);
SMRF_API int smrf_count_nan_f64(const double* d_a, int64_t n, int64_t* h_count, void* stream);

/* ------------------------------------------------------------------------------------------
 * create_dem
 * ------------------------------------------------------------------------------------------ */
/* h_out[4] = min x, max x, min y, max y over n points (synchronises `stream`).
 * workspace: 4 * 1024 doubles. */
SMRF_API int smrf_points_extent_f64(const double* d_x, const double* d_y, int64_t n, double* h_out,
                           void* d_workspace, size_t workspace_bytes, void* stream);
/* LAS point records (packed, record_length bytes each, x/y/z int32 first) -> float64 coordinates
 * x = X * scale + offset (neilpy.py:1055-1057 in read_las); h_scale_offset = {sx, sy, sz, ox, oy, oz} */
SMRF_API int smrf_las_decode_xyz_f64(const uint8_t* d_records, int64_t npts, int record_length,
                            const double* h_scale_offset, double* d_x, double* d_y, double* d_z,
                            void* stream);
/* fractional pixel coordinates (col, row) = ~t * (x, y) with h_inv = (a,b,c,d,e,f) of the inverse
 * transform, products and sums rounded separately like the affine package (neilpy.py:1772) */
SMRF_API int smrf_affine_apply_f64(const double* d_x, const double* d_y, int64_t npts, const double* h_inv,
                          double* d_col, double* d_row, void* stream);
/* keys: one uint64 per cell; all-ones = empty */
SMRF_API int smrf_grid_clear_u64(uint64_t* d_keys, int64_t ncells, void* stream);
/* col = floor(x*inv[0] + y*inv[1] + inv[2]), row = floor(x*inv[3] + y*inv[4] + inv[5]) with
 * separately rounded multiplies and adds (no FMA), inv = coefficients (a,b,c,d,e,f) of the
 * inverse affine transform.  Points with NaN z are skipped (pandas min/max skip NaN).
 * h_filter (may be NULL) = {xedges[0], xedges[-1], yedges[-1], yedges[0]}: points outside are
 * dropped first (neilpy.py:1128).  Rows [row0, row0+rows_local) of the rows_total x cols grid
 * are held in d_keys (row-band sharding; single GPU: row0 = 0, rows_local = rows_total);
 * points of other bands are ignored, points outside the whole grid are counted in
 * *d_n_outside (device int64, caller zeroes it). */
SMRF_API int smrf_grid_bin_f64(const double* d_x, const double* d_y, const double* d_z, int64_t npts,
                      const double* h_inv, const double* h_filter, uint64_t* d_keys,
                      int rows_total, int cols, int row0, int rows_local, int is_max,
                      int64_t* d_n_outside, void* stream);
/* keys -> float64 grid, empty -> NaN; d_empty (may be NULL) gets 1 where empty */
SMRF_API int smrf_grid_finalize_f64(const uint64_t* d_keys, double* d_grid, uint8_t* d_empty,
                           int64_t ncells, int is_max, void* stream);

/* Sharded create_dem without replicated points (the all-to-all form; create_dem semantics of
 * neilpy/neilpy.py:1141-1156 are unchanged).  Every rank holds 1/N of the points; each point belongs to the
 * rank whose row band holds floor(row) of `~t * (x, y)` (h_inv = the six inverse-affine coefficients, the same
 * rounding as smrf_grid_bin_f64); bands are sharded.band_rows(): the first rows_total % nbands bands hold one
 * row more.  nbands <= 64.
 *   smrf_points_band_count_f64: d_counts[nbands] <- points of this rank per destination band.
 *   smrf_points_band_pack_f64:  points copied into d_out_{x,y,z} grouped by destination band; d_cursors[nbands]
 *     holds each band's first output index on entry (exclusive prefix sum of the counts) and its end on return.
 *     Order inside a band's run is arbitrary (the binning is order independent).
 * The host exchanges the runs (counts first) with all_to_all over RCCL and bins what it receives with
 * smrf_grid_bin_f64(row0, rows_local). */
SMRF_API int smrf_points_band_count_f64(const double* d_x, const double* d_y, int64_t npts, const double* h_inv,
                               int rows_total, int nbands, uint64_t* d_counts, void* stream);
SMRF_API int smrf_points_band_pack_f64(const double* d_x, const double* d_y, const double* d_z, int64_t npts,
                              const double* h_inv, int rows_total, int nbands, uint64_t* d_cursors,
                              double* d_out_x, double* d_out_y, double* d_out_z, void* stream);

/* ------------------------------------------------------------------------------------------
 * inpaint_nans_by_springs: matrix-free LSQR on the raster's edge planes, scipy's recurrence
 * and stopping rule (damp = 0).  d_A (rows x cols, contiguous, float64) is updated in place:
 * NaN cells receive the solution, known cells are untouched.  iter_lim < 0 -> 2*n_unknown.
 * Synchronous: returns after the solve; *h_istop, *h_itn as scipy reports them.
 * ------------------------------------------------------------------------------------------ */
SMRF_API size_t smrf_springs_workspace_bytes(int rows, int cols);
SMRF_API int smrf_springs_lsqr_f64(double* d_A, int rows, int cols, double atol, double btol,
                          double conlim, int64_t iter_lim, int* h_istop, int64_t* h_itn,
                          int64_t* h_n_unknown, void* d_workspace, size_t workspace_bytes,
                          void* stream);

/* Row-band form of the same solver for rasters sharded over several GPUs.  The band
 * holds rows_local x cols cells of d_A_band.  The workspace keeps every plane with one halo row
 * above and one below; smrf_springs_band_layout() gives the byte offsets the host needs to
 * exchange halo rows and to all-reduce the phase sums:
 *   h_out[0] v plane, h_out[1] uv plane (rows_local + 2 rows, h_out[6] doubles apart, the first cols used; row 0 = halo above),
 *   h_out[2] hole plane (rows_local + 2 rows, h_out[6] bytes apart), h_out[6] the planes' row pitch in cells (>= cols),
 *   h_out[3] cols doubles = raster row
 *   below the band, h_out[4] two doubles = the phase's local sums (phase 7 fills both: |v|^2 and |dk|^2,
 *   to be all-reduced as ONE 2-element buffer; every other phase uses the first), h_out[5] total bytes.
 * Phases (in order; "<- X" = what the host must have delivered before the phase):
 *   0 mask+count | 1 rhs <- hole halo below, A row below, all-reduced count | 2 |b| <- all-reduce
 *   3 first v = S^T u <- uv halo above | 4 first alfa <- all-reduce
 *   loop (the split rotation of lsqr.py:424-555, csrc/lsqr_core.h; the single-device solver's kernels):
 *         5 u = S v - alfa u <- v halo below | 6 beta, rho, t1 <- all-reduce
 *         7 w, dk, (x every second iteration), v = S^T u - beta v <- uv halo above
 *         8 alfa, rest of the rotation, stopping tests <- all-reduce (2 values)
 *   10 scatter the solution into d_A_band (adds the pending x step when the solve stopped at an odd iteration).
 * Two halo rows and two all-reduces per iteration, 12 plane touches (round 4's phases 5, 6, 3, 7, 8, 9: 15).
 * neilpy_amd/sharded.py drives it over torch.distributed (RCCL). */
SMRF_API size_t smrf_springs_band_workspace_bytes(int rows_local, int cols);
SMRF_API int smrf_springs_band_layout(int rows_local, int cols, int64_t* h_out);
SMRF_API int smrf_springs_band_begin(int rows_local, int cols, double atol, double btol, double conlim,
                            int64_t iter_lim, void* d_workspace, size_t workspace_bytes,
                            void* stream);
SMRF_API int smrf_springs_band_phase(int phase, double* d_A_band, int rows_local, int cols, int has_above,
                            int has_below, void* d_workspace, size_t workspace_bytes, void* stream);
SMRF_API int smrf_springs_band_status(const void* d_workspace, int rows_local, int cols, int* h_istop,
                             int64_t* h_itn, int64_t* h_n_unknown, int* h_done, void* stream);

/* inpaint_nans_by_fda(A), neilpy/neilpy.py:1170-1216: the NaN cells of d_A (rows x cols, float64,
 * C order) are replaced in place by scipy.sparse.linalg.lsqr's iterate on the second-difference
 * equations that touch a NaN cell, every equation weighted by its number of NaN stencil cells
 * as the reference's row selection does (:1207-1210).  Arguments as smrf_springs_lsqr_f64.
 * Single device. */
SMRF_API size_t smrf_fda_workspace_bytes(int rows, int cols);
SMRF_API int smrf_fda_lsqr_f64(double* d_A, int rows, int cols, double atol, double btol, double conlim,
                      int64_t iter_lim, int* h_istop, int64_t* h_itn, int64_t* h_n_unknown,
                      void* d_workspace, size_t workspace_bytes, void* stream);
/* Diagnostic (tests): one application of the operator smrf_fda_lsqr_f64 iterates with, against the
 * reference's explicit sparse system (neilpy/neilpy.py:1180-1209).  All buffers are rows x cols rasters on
 * the device: d_rhs / d_cnt <- right-hand side and multiplicity (NaN entries, :1207-1209) of every
 * equation cell; d_Av <- A v on the equation cells (v read on the NaN cells of d_A); d_Atu <- A^T u on the
 * NaN cells (u read on the equation cells, each counted d_cnt times).  Workspace as smrf_fda_workspace_bytes. */
SMRF_API int smrf_fda_apply_f64(const double* d_A, int rows, int cols, const double* d_v, const double* d_u,
                      double* d_rhs, uint8_t* d_cnt, double* d_Av, double* d_Atu, void* d_workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * smrf tail
 * ------------------------------------------------------------------------------------------ */
/* S = sqrt(gy^2 + gx^2), (gy, gx) = np.gradient(Z, cellsize) (second-order interior,
 * first-order one-sided edges).  rows, cols >= 2. */
SMRF_API int smrf_gradient_slope_f64(const double* d_Z, double* d_S, int rows, int cols, double cellsize,
                            void* stream);

/* pssm(), neilpy/neilpy.py:846-867 (the bonemaps of examples/smrf/ *.ipynb): slope as above, then
 * P = uint8(round(255 * (rad2deg(arctan(ve * S)) / 90))) into d_P (rows x cols, nullable) and, when
 * d_rgba is given, the colormap lookup d_rgba[i][0..3] = d_lut[P[i]][0..3] (d_lut: 256 x 4 doubles,
 * what plt.cm.bone_r / plt.cm.bone hold; d_rgba: rows x cols x 4 doubles). */
SMRF_API int smrf_pssm_f64(const double* d_Z, uint8_t* d_P, double* d_rgba, const double* d_lut, int rows, int cols,
                  double cellsize, double ve, void* stream);

/* Interpolating bicubic spline of scipy.interpolate.RectBivariateSpline(rows, cols, Z) with its
 * defaults kx = ky = 3, s = 0 (neilpy.py:1773, :1788): d_C holds the raster on entry and the
 * B-spline coefficients on return.  d_lu_rows / d_lu_cols: banded LU factors (5 x rows, 5 x cols
 * doubles: l2, l1, d, u1, u2) of the per-axis collocation systems; neilpy_amd/spline.py builds them. */
SMRF_API int smrf_spline_solve_f64(double* d_C, int rows, int cols, const double* d_lu_rows,
                          const double* d_lu_cols, void* stream);
/* The same solve with a scratch plane of rows x cols doubles, which lets every line be cut into chunks that run side by
 * side (each chunk re-derives its start state from 64 entries of warm-up; the substitutions contract by 0.268 per entry,
 * so nothing of the cut is left in float64).  d_C: raster in, coefficients out; d_scratch: clobbered.  This is the entry
 * neilpy_amd.smrf uses; the one above is the line-by-line sequential form the tests compare it with. */
SMRF_API int smrf_spline_solve_ws_f64(double* d_C, double* d_scratch, int rows, int cols, const double* d_lu_rows,
                             const double* d_lu_cols, void* stream);
/* .ev(px, py) of that spline (FITPACK bispeu): px runs along the rows axis, py along the columns
 * axis; d_tx (rows + 4) and d_ty (cols + 4) are the knots; arguments are clamped to the knot range. */
SMRF_API int smrf_spline_eval_f64(const double* d_C, int rows, int cols, const double* d_tx, const double* d_ty,
                         const double* d_px, const double* d_py, int64_t npts, double* d_out,
                         void* stream);
/* is_object_point = abs(elev - z) > elevation_threshold + elevation_scaler * slope (neilpy.py:1794-1795) */
SMRF_API int smrf_classify_points_f64(const double* d_elev, const double* d_slope, const double* d_z,
                             int64_t npts, double elevation_threshold, double elevation_scaler,
                             uint8_t* d_is_object, void* stream);

/* out = -in (smrf runs the low-outlier filter on -Zmin, neilpy.py:1744) */
SMRF_API int smrf_negate_f64(const double* d_in, double* d_out, int64_t n, void* stream);
/* u = a | b | c (b, c, d_union may be NULL); Z[u] = NaN  (neilpy.py:1748 and :1762-1763) */
SMRF_API int smrf_mask_apply_f64(double* d_Z, const uint8_t* d_a, const uint8_t* d_b, const uint8_t* d_c,
                        uint8_t* d_union, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * terrain ray marches (neilpy_amd/terrain.py)
 * ------------------------------------------------------------------------------------------ */
#define SMRF_TERRAIN_OPENNESS 0   /* openness(), neilpy.py:1325-1357 -> d_out0 float64 degrees */
#define SMRF_TERRAIN_SKYVIEW 1    /* skyview_factor(), neilpy.py:1360-1384 -> d_out0 float64 */
#define SMRF_TERRAIN_COUNT 2      /* count_openness() / geomorphons(), neilpy.py:1600-1653 -> d_out0 num_pos,
                                     d_out1 num_neg, d_out2 geomorphon class (uint8 each, any of them NULL) */
#define SMRF_TERRAIN_TERNARY 3    /* ternary_pattern_from_openness(), neilpy.py:1404-1428 -> d_out0 int64 code */
#define SMRF_TERRAIN_IMPL_AUTO 0    /* = TILED */
#define SMRF_TERRAIN_IMPL_TILED 1   /* workgroup tile + halo of min(max_step, cap) cells in LDS, longer steps from global */
#define SMRF_TERRAIN_IMPL_DIRECT 2  /* every sample from global memory; same bits as TILED */
#define SMRF_TERRAIN_HALO_CAP_F32 40
#define SMRF_TERRAIN_HALO_CAP_F64 24
#define SMRF_TERRAIN_OPT_NEGATIVE 1 /* TERNARY: use_negative_openness */
#define SMRF_TERRAIN_OPT_ENHANCE 2  /* COUNT: geomorphons(enhance=True)'s second count and correction (:1640-1649) */

/* One launch of the ray-march family over a rows x cols raster d_Z (contiguous).  For each direction d in dir_mask
 * (bit d; d = 0..7 clockwise from the upper left, ashift at neilpy.py:1290-1307) and each step i < nsteps the slope
 * t = fp64(Z[sample] - Z[cell]) / d_dist[(d & 1) * nsteps + i] is taken at distance d_steps[i] (ascending, >= 1;
 * max_step >= the largest; d_dist holds (cellsize * k) * sqrt(2) for even d, then cellsize * k for odd d, as the
 * host computes it).  Off-raster samples read the cell itself (openness family) or the last on-raster cell of the
 * ray (SKYVIEW).  d_flags[i]: bit 0 = the step belongs to the main march, bit 1 = to the enhance march (COUNT; other
 * modes use every step).  OPENNESS: mean over d_neighbors[0..n_neighbors) of the per-direction angle, in degrees.
 * COUNT / TERNARY compare each direction's positive minus negative openness with +-threshold (degrees); d_lut is the
 * 9 x 9 uint8 table [num_pos][num_neg] (COUNT with d_out2) or NULL / 6561 int64 lowest-equivalent codes (TERNARY). */
SMRF_API int smrf_terrain_rays_f32(const float* d_Z, int rows, int cols, int mode, const int* d_steps,
                          const uint8_t* d_flags, const double* d_dist, int nsteps, int max_step,
                          const int* d_neighbors, int n_neighbors, int dir_mask, double threshold, int options,
                          const void* d_lut, void* d_out0, void* d_out1, void* d_out2, int impl, void* stream);
SMRF_API int smrf_terrain_rays_f64(const double* d_Z, int rows, int cols, int mode, const int* d_steps,
                          const uint8_t* d_flags, const double* d_dist, int nsteps, int max_step,
                          const int* d_neighbors, int n_neighbors, int dir_mask, double threshold, int options,
                          const void* d_lut, void* d_out0, void* d_out1, void* d_out2, int impl, void* stream);

/* ------------------------------------------------------------------------------------------
 * local surface derivatives: 3 x 3 stencils (neilpy_amd/surface.py)
 * ------------------------------------------------------------------------------------------ */
#define SMRF_SURFACE_SLOPE 0      /* slope(), neilpy.py:456 -> d_out0 T; p0 = cellsize / z_factor */
#define SMRF_SURFACE_ASPECT 1     /* aspect(), :471 -> d_out0 T; p0 = the value of flat cells (flat_as, NaN allowed) */
#define SMRF_SURFACE_HILLSHADE 2  /* hillshade() / multiple_illumination(), :814 / :830; p0 = cellsize / z_factor ->
                                     d_out0 uint8 max over the angle table, d_out1 float64 H (one angle only) */
#define SMRF_SURFACE_HORN 3       /* esri_slope(), :434 -> d_out0 T; p0 = cellsize, p1 = z_factor */
#define SMRF_SURFACE_LAPLACE 4    /* curvature(), :487 -> d_out0 T; p0 = cellsize */
#define SMRF_SURFACE_ESRI 5       /* esri_curvature(), :520 -> K, K_plan, K_profile; p0 = L**2, p1 = 4*(L**2), p2 = 2*L */
#define SMRF_SURFACE_ZT 6         /* zevenbergen_and_thorne_curvature(), :596 -> K, K_profile, K_plan, K_tan, K_long,
                                     K_cross; parameters as ESRI */
#define SMRF_SURFACE_EVANS 7      /* evans_curvature(), :671 -> the same six; p0 = 6*L**2, p1 = 3*L**2, p2 = 4*L**2,
                                     p3 = 6*L */
#define SMRF_SURFACE_WG 8         /* wilson_gallant_curvature(), :753 -> K, Kp, Kc, Kt; p0 = 2*H, p1 = H**2 */
#define SMRF_SURFACE_OPT_RADIANS 1  /* SLOPE: arctan of the gradient norm */
#define SMRF_SURFACE_OPT_DEGREES 2  /* SLOPE, ASPECT, HORN: in degrees (np.rad2deg) */

/* One launch over a rows x cols raster d_Z (contiguous).  p0..p3 are the mode's parameters, formed by the host with the
 * reference's expressions and rounded to T in the kernel.  Edge rules: np.gradient's (SLOPE, ASPECT, HILLSHADE; rows,
 * cols >= 2), ndimage 'reflect' (HORN, LAPLACE) and ashift's, an off-raster neighbour read as the cell (the other
 * curvatures).  Multi-output modes write every non-NULL d_out* (up to six, in the reference's return order) from one
 * read of d_Z; outputs beyond the mode's count must be NULL.  HILLSHADE: d_angles is a device table of n_angles rows
 * (cos zenith, sin zenith, azimuth in radians; float64, computed as the reference computes them); d_out0 gets the
 * largest uint8 shade over the rows, d_out1 (n_angles = 1) the float64 shade. */
SMRF_API int smrf_surface_f32(const float* d_Z, int rows, int cols, int mode, int options, double p0, double p1,
                     double p2, double p3, const double* d_angles, int n_angles, void* d_out0, void* d_out1,
                     void* d_out2, void* d_out3, void* d_out4, void* d_out5, void* stream);
SMRF_API int smrf_surface_f64(const double* d_Z, int rows, int cols, int mode, int options, double p0, double p1,
                     double p2, double p3, const double* d_angles, int n_angles, void* d_out0, void* d_out1,
                     void* d_out2, void* d_out3, void* d_out4, void* d_out5, void* stream);

/* ------------------------------------------------------------------------------------------
 * nearest-source infill: exact Euclidean feature transform (neilpy_amd/nearest.py)
 * ------------------------------------------------------------------------------------------ */
/* inpaint_nearest(), neilpy.py:1277.  A hole is a cell that is not finite (NaN, +-inf), a source any other cell.  Every
 * hole of the contiguous rows x cols raster d_in takes the bits of its nearest source in squared Euclidean index
 * distance; among sources at the minimal distance the lowest row, then the lowest column wins.  Sources are copied.
 * d_out (may equal d_in, may be NULL), d_src_index (flat index rows * cols of the chosen source, the cell's own for a
 * source; may be NULL) and d_dist2 (the exact squared distance, unsigned 32-bit; may be NULL) are written for every
 * cell.  A raster without a source comes back unchanged with index -1 and distance 0xFFFFFFFF.  rows, cols <= 46341
 * (the largest squared distance fits 32 bits).  Workspace: smrf_nearest_workspace_bytes() (integer planes only,
 * elem_size is 4 or 8 and does not change it). */
SMRF_API size_t smrf_nearest_workspace_bytes(int rows, int cols, int elem_size);
SMRF_API int smrf_nearest_f32(const float* d_in, float* d_out, int64_t* d_src_index, uint32_t* d_dist2, int rows,
                     int cols, void* d_workspace, size_t workspace_bytes, void* stream);
SMRF_API int smrf_nearest_f64(const double* d_in, double* d_out, int64_t* d_src_index, uint32_t* d_dist2, int rows,
                     int cols, void* d_workspace, size_t workspace_bytes, void* stream);
/* The planes nearest_source() returns, from the two above over n cells: d_dist = sqrt(d_dist2) in float64 (inf where
 * there is no source), d_row / d_col = the source's row and column (-1 where there is none).  d_dist alone, or d_row
 * and d_col together, may be NULL. */
SMRF_API int smrf_nearest_planes(const int64_t* d_src_index, const uint32_t* d_dist2, int64_t n, int cols,
                     double* d_dist, int64_t* d_row, int64_t* d_col, void* stream);

/* ------------------------------------------------------------------------------------------
 * weighted focal sums: scipy.ndimage.convolve(mode='nearest') and what rests on it (neilpy_amd/focal.py; DESIGN.md
 * section 12)
 * ------------------------------------------------------------------------------------------ */
#define SMRF_FOCAL_SUM 0      /* d_out0 T = conv(X) */
#define SMRF_FOCAL_SUM_SQ 1   /* d_out0 T = conv(X), d_out1 T = conv(X*X), the square formed and rounded in T */
#define SMRF_FOCAL_STD 2      /* std(), neilpy.py:2039 -> d_out0 float64, from the two sums and S = np.sum(strel) */
#define SMRF_FOCAL_TPI 3      /* topographic_position_index(), :2098 -> d_out0 T = X - conv(X); the workspace's first
                                 three doubles get sum(conv(X*X)), sum(X - conv(X)) and sd = sqrt(mean - mean**2),
                                 the means and sd in T */
#define SMRF_FOCAL_IMPL_AUTO 0    /* TILED when the whole halo fits SMRF_FOCAL_TILE_BYTES and the raster holds a tile */
#define SMRF_FOCAL_IMPL_TILED 1   /* workgroup tile + halo of (kh / 2, kw / 2) cells in LDS; a larger kernel keeps the
                                     largest common halo that fits and reads its other taps from global memory */
#define SMRF_FOCAL_IMPL_DIRECT 2  /* every sample from global memory; same bits as TILED */
#define SMRF_FOCAL_TILE_BYTES 53248 /* LDS of one tile: three workgroups per CU (160 KB) */

/* 1 when the 64 x 8 tile plus the whole halo of a kh x kw kernel fits SMRF_FOCAL_TILE_BYTES (elem_size 4 or 8). */
SMRF_API int smrf_focal_fits_tile(int kh, int kw, int elem_size);
/* Workspace of a TPI launch and of smrf_focal_minmax_f64 over rows x cols cells. */
SMRF_API size_t smrf_focal_workspace_bytes(int rows, int cols);
/* One launch over a rows x cols raster (contiguous): d_X, or d_X - d_sub formed in T when d_sub is not NULL.  d_taps
 * holds ntaps records (int32 drow, int32 dcol, float64 weight), the non-zero weights of a kh x kw kernel w in the order
 * s = kh-1 .. 0, t = kw-1 .. 0 with drow = kh/2 - s, dcol = kw/2 - t.  conv = T(sum over the taps, in that order, of
 * fp64(X[clamp(r + drow), clamp(c + dcol)]) * weight), each tap one fp64 multiply and one fp64 add.  The TPI sums are
 * taken in a fixed order (no atomics): the same bits on every run. */
SMRF_API int smrf_focal_f32(const float* d_X, const float* d_sub, int rows, int cols, int mode, const void* d_taps,
                   int ntaps, int kh, int kw, double S, void* d_out0, void* d_out1, void* d_workspace,
                   size_t workspace_bytes, int impl, void* stream);
SMRF_API int smrf_focal_f64(const double* d_X, const double* d_sub, int rows, int cols, int mode, const void* d_taps,
                   int ntaps, int kh, int kw, double S, void* d_out0, void* d_out1, void* d_workspace,
                   size_t workspace_bytes, int impl, void* stream);
/* d_io[i] /= T(d_sd[0]) over n cells: TPI's standardisation by the sd a TPI launch left at workspace + 2 doubles. */
SMRF_API int smrf_focal_divide_f32(float* d_io, int64_t n, const double* d_sd, void* stream);
SMRF_API int smrf_focal_divide_f64(double* d_io, int64_t n, const double* d_sd, void* stream);
/* np.nanmin / np.nanmax of n float64 cells into the workspace's first two doubles (NaN when every cell is NaN). */
SMRF_API int smrf_focal_minmax_f64(const double* d_x, int64_t n, void* d_workspace, size_t workspace_bytes,
                   void* stream);
/* reduce_peaks()'s tail, neilpy.py:2082-2085: V = (1 - interp(STD, (lo, hi), (0, 1)))**blend_rate,
 * d_out = (1 - V)*M + V*Z in float64; d_lohi = (lo, hi) as smrf_focal_minmax_f64 leaves them. */
SMRF_API int smrf_focal_mix_f32(const float* d_Z, const float* d_M, const double* d_STD, const double* d_lohi,
                   double blend_rate, double* d_out, int64_t n, void* stream);
SMRF_API int smrf_focal_mix_f64(const double* d_Z, const double* d_M, const double* d_STD, const double* d_lohi,
                   double blend_rate, double* d_out, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * grey morphology with arbitrary flat footprints: scipy.ndimage.grey_erosion / grey_dilation and what rests on them
 * (neilpy_amd/morphology.py)
 * ------------------------------------------------------------------------------------------ */
#define SMRF_FOOTPRINT_REFLECT 0  /* border mode 'reflect': the period-2n fold (d c b a | a b c d | d c b a) */
#define SMRF_FOOTPRINT_NEAREST 1  /* border mode 'nearest': indices clamped to the raster */
#define SMRF_FOOTPRINT_IMPL_AUTO 0 /* RUNS when its LDS planes fit SMRF_FOOTPRINT_TILE_BYTES and the footprint has at
                                      least SMRF_FOOTPRINT_RUNS_MIN_TAPS members, TAPS otherwise */
#define SMRF_FOOTPRINT_IMPL_RUNS 1 /* tile + halo in LDS, power-of-two min / max planes, two LDS reads per run of
                                      consecutive members; SMRF_E_UNSUPPORTED when the planes do not fit */
#define SMRF_FOOTPRINT_IMPL_TAPS 2 /* one compare per member, every sample from global memory; any footprint, any
                                      raster; same values as RUNS */
#define SMRF_FOOTPRINT_TILE_BYTES 53248 /* LDS of one workgroup's planes: SMRF_FOCAL_TILE_BYTES, three workgroups per CU */
#define SMRF_FOOTPRINT_RUNS_MIN_TAPS 9
#define SMRF_FOOTPRINT_STORE 0      /* d_out = the filter's result */
#define SMRF_FOOTPRINT_SUB_MINUS 1  /* d_out = d_sub - result (white top-hat's second launch) */
#define SMRF_FOOTPRINT_MINUS_SUB 2  /* d_out = result - d_sub (black top-hat's second launch) */
#define SMRF_FOOTPRINT_GRADIENT 3   /* d_out = max - min over the same samples (is_dilate is not looked at): the
                                       morphological gradient of a footprint that is its own mirror image */

/* The LDS a workgroup of the RUNS path may take, SMRF_FOOTPRINT_TILE_BYTES. */
SMRF_API int smrf_footprint_tile_bytes(void);
/* The path a launch with this plan head takes: 0 = TAPS, 1 = RUNS, or a negative SMRF_E_* code where the launch would be
 * refused (a malformed head, RUNS forced on planes that do not fit).  Host logic only. */
SMRF_API int smrf_footprint_path(const int* h_head, int elem_size, int epilogue, int impl);
/* One launch over a contiguous rows x cols raster.  The plan comes from the host (neilpy_amd.morphology.plan):
 *   h_head (host, 24 int32): ntaps, nruns, r_lo, c_lo, bh, bw, maxlevel, nplanes, slot[16] - the members' count, the
 *     count of their runs, the least (drow, dcol) of a member and the rows and columns of the members' bounding box, the
 *     largest floor(log2(run length)), and for every level up to it the LDS plane (0 .. nplanes - 1) that holds it;
 *   d_plan (device, int32): ntaps records (drow, dcol), the first visited member first, then nruns records (trow, tcol,
 *     tcol2, slot): a run of L members from (drow, dcol0) at level k = floor(log2 L) reads the plane in `slot` at tile
 *     row drow - r_lo and tile columns dcol0 - c_lo and dcol0 - c_lo + L - 2^k.
 * Offsets are the samples' own: the cell (r, c) reads X[idx(r + drow), idx(c + dcol)], idx the border mode's index rule,
 * so a dilation's plan holds the footprint mirrored about its centre.  The result is the minimum (is_dilate 0) or
 * maximum (1) of the samples, NaN iff the first visited sample is NaN (scipy.ndimage's rule); nan_aware 0 promises a
 * raster without NaN and spares the RUNS path one read per cell.  d_sub is read by epilogues 1 and 2 only.  Every
 * global index goes through idx, whatever the plan holds. */
SMRF_API int smrf_footprint_filter_f32(const float* d_in, const float* d_sub, float* d_out, int rows, int cols,
                   const void* d_plan, const int* h_head, int is_dilate, int mode, int nan_aware, int impl,
                   int epilogue, void* stream);
SMRF_API int smrf_footprint_filter_f64(const double* d_in, const double* d_sub, double* d_out, int rows, int cols,
                   const void* d_plan, const int* h_head, int is_dilate, int mode, int nan_aware, int impl,
                   int epilogue, void* stream);

/* ------------------------------------------------------------------------------------------
 * strided stencils: scaled_morphometry, vip_score, ashift (neilpy_amd/morphometry.py)
 * ------------------------------------------------------------------------------------------ */
/* One sampling rule, ashift's (neilpy.py:1290): the sample at offset (dr, dc), each in {-n, 0, +n}, of cell (r, c) of
 * the contiguous rows x cols raster d_Z is Z[r + dr, c + dc] where that row and that column are on the raster, and
 * Z[r, c] otherwise.  n >= 1; n >= rows or n >= cols makes every sample along that axis the cell. */
/* scaled_morphometry(), neilpy.py:2472: Wood's quadratic through nine samples n cells apart.  d0..d3 = 6*L**2, 3*L**2,
 * 4*L**2, 6*L with L = cellsize * lookup_pixels, formed by the host in Python floats and rounded to T in the kernel.
 * Every non-NULL output is written from one read of d_Z in one launch; a NULL one is neither computed nor stored.  No
 * NaN repair: 0 / 0 on flats is NaN in the five ratio outputs. */
SMRF_API int smrf_morphometry_f32(const float* d_Z, int rows, int cols, int n, double d0, double d1, double d2,
                     double d3, float* d_A, float* d_S, float* d_K, float* d_K_profile, float* d_K_cross,
                     float* d_K_long, float* d_K_tan, float* d_K_plan, void* stream);
SMRF_API int smrf_morphometry_f64(const double* d_Z, int rows, int cols, int n, double d0, double d1, double d2,
                     double d3, double* d_A, double* d_S, double* d_K, double* d_K_profile, double* d_K_cross,
                     double* d_K_long, double* d_K_tan, double* d_K_plan, void* stream);
/* vip_score(), neilpy.py:1832: the mean over the four lines through a cell (n = 1) of triangle_height(), :1818.
 * x_diag = sqrt(2) * cellsize, x_axis = 1 * cellsize, b2_* = (2 * x_*)**2 as the host's scalar power gives them.  The
 * neighbour differences are formed in T; everything after them, and d_out, is float64. */
SMRF_API int smrf_vip_f32(const float* d_Z, int rows, int cols, double x_diag, double x_axis, double b2_diag,
                     double b2_axis, double* d_out, void* stream);
SMRF_API int smrf_vip_f64(const double* d_Z, int rows, int cols, double x_diag, double x_axis, double b2_diag,
                     double b2_axis, double* d_out, void* stream);
/* ashift(): d_out (not d_Z) gets the sample of direction 0..7 = (r-n, c-n), (r-n, c), (r-n, c+n), (r, c+n),
 * (r+n, c+n), (r+n, c), (r+n, c-n), (r, c-n); any other direction copies the raster. */
SMRF_API int smrf_ashift_f32(const float* d_Z, int rows, int cols, int direction, int n, float* d_out, void* stream);
SMRF_API int smrf_ashift_f64(const double* d_Z, int rows, int cols, int direction, int n, double* d_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * nearest point of a cloud: uniform cell grid + ring search (neilpy_amd/points.py)
 * ------------------------------------------------------------------------------------------ */
/* Clouds are contiguous float64 (n, dim) arrays, dim 2 or 3, 1 <= npoints <= 2^30.  One workspace of
 * smrf_points_nn_workspace_bytes(npoints, dim) bytes (0 for arguments out of range) serves all four calls below; the
 * build leaves the grid in it and the search reads it, bounds and sum use its first 40 KB as scratch. */
SMRF_API size_t smrf_points_nn_workspace_bytes(int64_t npoints, int dim);
/* One reduction over a cloud: h_box = (min0, max0, min1, max1), the box of axes 0 and 1 (a NaN is skipped, an
 * infinity is not), h_nonfinite = the number of coordinates, over all axes, that are NaN or infinite.  Synchronises the stream. */
SMRF_API int smrf_points_nn_bounds_f64(const double* d_points, int64_t npoints, int dim, double* h_box,
                     int64_t* h_nonfinite, void* d_workspace, size_t workspace_bytes, void* stream);
/* The grid build: square cells over h_box (as the call above gave it for these points, all finite) on axes 0 and 1,
 * sized for about two points per cell, at most 3 * max(1, npoints / 2) + 4 cells; the points are counted per cell with
 * atomics, the counts scanned, and rows and coordinates scattered into cell order. */
SMRF_API int smrf_points_nn_build_f64(const double* d_points, int64_t npoints, int dim, const double* h_box,
                     void* d_workspace, size_t workspace_bytes, void* stream);
/* The search, one thread per query point, over the grid the build left in the workspace for (d_points, npoints, dim,
 * h_box): d_dist[i] = sqrt(((q0-p0)*(q0-p0) + (q1-p1)*(q1-p1)) [+ (q2-p2)*(q2-p2)]) in float64, every operation
 * rounded, to the nearest point; d_index[i] = its row, the lowest among the points at that distance.  Either output may
 * be NULL.  Queries may lie anywhere; they must be finite.  d_points names the cloud the workspace was built from; the
 * kernel reads the cell-ordered copy of its coordinates in the workspace. */
SMRF_API int smrf_points_nn_search_f64(const double* d_query, int64_t nquery, const double* d_points, int64_t npoints,
                     int dim, const double* h_box, double* d_dist, int64_t* d_index, const void* d_workspace,
                     size_t workspace_bytes, void* stream);
/* d_sum[0] = the sum of n float64 values in a fixed order that depends on n only (per-workgroup partials in a fixed
 * tree, then one workgroup; no float atomics): the same bits on every run. */
SMRF_API int smrf_points_nn_sum_f64(const double* d_x, int64_t n, double* d_sum, void* d_workspace,
                     size_t workspace_bytes, void* stream);

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

/* ------------------------------------------------------------------------------------------
 * point cloud -> boolean voxel model (neilpy_amd/voxel.py)
 * ------------------------------------------------------------------------------------------ */
/* The cloud is three contiguous coordinate arrays of one dtype, 1 <= npoints <= 2^31 - 1.  The volume has nx x ny x nz
 * cells (any of them may be 0), C order, z fastest. */
/* Bytes of device scratch the bounds reduction needs. */
#define SMRF_VOXEL_BOUNDS_BYTES 57344
/* One reduction over the three arrays: h_box = (min_x, max_x, min_y, max_y, min_z, max_z) as float64 (a NaN is skipped,
 * an infinity is not), h_nonfinite = the number of coordinates that are NaN or infinite.  Per-workgroup partials, finished
 * on the host: no float atomics.  Synchronises the stream. */
SMRF_API int smrf_voxel_bounds_f32(const float* d_x, const float* d_y, const float* d_z, int64_t npoints, double* h_box,
                     int64_t* h_nonfinite, void* d_workspace, size_t workspace_bytes, void* stream);
SMRF_API int smrf_voxel_bounds_f64(const double* d_x, const double* d_y, const double* d_z, int64_t npoints,
                     double* h_box, int64_t* h_nonfinite, void* d_workspace, size_t workspace_bytes, void* stream);
/* Workspace of mark and expand, 0 for a volume out of range (a negative extent, threshold < 1, more than 2^31 - 1 columns
 * or 2^40 entries).
 * It begins with the marks: for threshold == 1 a bit set, uint32 words [nx][ny][ceil(nz / 32)], bit (z & 31) of word
 * z >> 5 for cell z, 1/8 B per voxel; for threshold > 1 uint32 counts [nx][ny][nz], 4 B per voxel.  The lowest occupied
 * cell of every column (int32 [nx][ny]) follows at the next multiple of 256 bytes. */
SMRF_API size_t smrf_voxel_workspace_bytes(int nx, int ny, int nz, int threshold);
/* Clears the marks, then bins every point: d = v - h_offsets[axis], one subtraction rounded in the cloud's dtype
 * (h_offsets holds three values of that dtype, widened); its bin on an axis with edges e[0..nb] (float64, device,
 * non-decreasing, nb + 1 of them, used as handed in) is numpy.histogramdd's: searchsorted(e, d, side='right') - 1 compared
 * in float64, d == e[nb] in bin nb - 1, and the point is dropped when d < e[0] or d > e[nb] on any axis.  threshold == 1
 * sets the cell's bit (the word is read first and the atomic OR issued only for a clear bit); threshold > 1 adds 1 to the
 * cell's count with an integer atomic.  Either way the marks are a function of the input alone. */
SMRF_API int smrf_voxel_mark_f32(const float* d_x, const float* d_y, const float* d_z, int64_t npoints,
                     const double* h_offsets, const double* d_xedges, const double* d_yedges, const double* d_zedges,
                     int nx, int ny, int nz, int threshold, void* d_workspace, size_t workspace_bytes, void* stream);
SMRF_API int smrf_voxel_mark_f64(const double* d_x, const double* d_y, const double* d_z, int64_t npoints,
                     const double* h_offsets, const double* d_xedges, const double* d_yedges, const double* d_zedges,
                     int nx, int ny, int nz, int threshold, void* d_workspace, size_t workspace_bytes, void* stream);
/* From the marks of a workspace (same nx, ny, nz, threshold) to d_out, uint8 0 / 1, [nx][ny][nz + pad], 4-byte aligned:
 * out[x][y][pad + z] = (bit set, or count >= threshold), or with bottom_fill != 0 also z below the lowest such cell of a
 * column that has one; out[x][y][0..pad) = 1 for every column.  nx * ny * (nz + pad) <= 2^42.  Writes the column minima
 * into the workspace on the way. */
SMRF_API int smrf_voxel_expand(void* d_workspace, size_t workspace_bytes, int nx, int ny, int nz, int threshold,
                     int bottom_fill, int pad, uint8_t* d_out, void* stream);

/* ---- relief colouring and raster statistics (csrc/relief.hip) ---------------------------
 * raster_stats: NaN-ignoring statistics of n cells (+-inf are values).  `what` = SMRF_STATS_MOMENTS | SMRF_STATS_MEDIAN;
 * h_out = a host row of SMRF_STATS_ROW doubles, filled after the stream has been synchronised (one device-to-host copy
 * per call): the number of non-NaN cells, the number of NaN cells, min, max, mean, the sum of the squares (squared in
 * the raster's dtype, summed in float64) and the median.  Entries not asked for, and every statistic of an empty or
 * all-NaN raster, are NaN (the two counts are always set with MOMENTS).  Mean and sum of squares are float64 sums in a
 * fixed order: per thread a grid-stride chain (thread g of min(ceil(n / 256), 1024) x 256 takes cells g, g + G, ...),
 * a 64-lane shuffle tree (offsets 32 .. 1), the four waves as (w0 + w1) + (w2 + w3), the workgroups in index order.
 * The median is np.nanmedian's value, exact: a radix select on an order-preserving integer key, 11 bits per pass
 * (csrc/select_plan.h).  The u8 instance (MOMENTS only) serves brassel's `any(H > 1)`. */
#define SMRF_STATS_MOMENTS 1
#define SMRF_STATS_MEDIAN 2
#define SMRF_STATS_ROW 8
#define SMRF_STATS_COUNT 0
#define SMRF_STATS_NAN 1
#define SMRF_STATS_MIN 2
#define SMRF_STATS_MAX 3
#define SMRF_STATS_MEAN 4
#define SMRF_STATS_SUM_SQ 5
#define SMRF_STATS_MEDIAN_AT 6
SMRF_API size_t smrf_raster_stats_workspace_bytes(int elem_size, int what);
SMRF_API int smrf_raster_stats_f32(const float* d_X, int64_t n, int what, double* h_out, void* d_workspace,
                                   size_t workspace_bytes, void* stream);
SMRF_API int smrf_raster_stats_f64(const double* d_X, int64_t n, int what, double* h_out, void* d_workspace,
                                   size_t workspace_bytes, void* stream);
SMRF_API int smrf_raster_stats_u8(const uint8_t* d_X, int64_t n, int what, double* h_out, void* d_workspace,
                                  size_t workspace_bytes, void* stream);
/* normalize(): d_out[i] = np.interp(d_X[i], xp, fp) in float64 without FMA; d_knots = xp[n_knots] then fp[n_knots],
 * float64 on the device, n_knots >= 2, xp non-decreasing. */
SMRF_API int smrf_normalize_f32(const float* d_X, int64_t n, const double* d_knots, int n_knots, double* d_out,
                                void* stream);
SMRF_API int smrf_normalize_f64(const double* d_X, int64_t n, const double* d_knots, int n_knots, double* d_out,
                                void* stream);
/* colortable_shade() / swiss_shading(): d_rgb[r][c][0..2] = table[zi][H], with H the uint8 hillshade of
 * smrf_surface_* (HILLSHADE, spacing = p0, h_angle = one host row cos zenith, sin zenith, azimuth) and
 * zi = uint8(round(255 * (Z - zmin) / (zmax - zmin))) in the raster's dtype (half-even, NaN -> 0).  zmin / zmax come
 * from the caller (np.min / np.max: NaN if the raster holds one).  d_lut = 256 x 256 words R | G << 8 | B << 16.
 * One launch, the raster read once.  rows, cols >= 2 (SMRF_E_ARG below). */
SMRF_API int smrf_colortable_f32(const float* d_Z, int rows, int cols, double zmin, double zmax, double spacing,
                                 const double* h_angle, const uint32_t* d_lut, uint8_t* d_rgb, void* stream);
SMRF_API int smrf_colortable_f64(const double* d_Z, int rows, int cols, double zmin, double zmax, double spacing,
                                 const double* h_angle, const uint32_t* d_lut, uint8_t* d_rgb, void* stream);
/* brassel_atmospheric_perspective(): one element-wise launch.  d_H = the shade (h_type: uint8, float32 or float64),
 * d_Z = the elevations (the entry's dtype); zmin / zmax = np.nanmin / np.nanmax of Z, flat already in 0..1,
 * logk = log(k).  WAS_INT: H / 255 in float64 and d_out = uint8 round(255 * H_new), cast as NumPy casts on x86 (NaN -> 0,
 * otherwise the low byte of the signed 32-bit truncation); without it d_out = float64.  ZMID: Zstar is np.interp over
 * (zmin, zmid, zmax) -> (-1, 0, 1) in float64 instead of the raster-dtype formula. */
#define SMRF_SHADE_U8 0
#define SMRF_SHADE_F32 1
#define SMRF_SHADE_F64 2
#define SMRF_BRASSEL_WAS_INT 1
#define SMRF_BRASSEL_ZMID 2
#define SMRF_BRASSEL_REVERSE 4
SMRF_API int smrf_brassel_f32(const void* d_H, int h_type, const float* d_Z, int64_t n, int options, double flat,
                              double zmin, double zmax, double zmid, double logk, double c2, void* d_out, void* stream);
SMRF_API int smrf_brassel_f64(const void* d_H, int h_type, const double* d_Z, int64_t n, int options, double flat,
                              double zmin, double zmax, double zmid, double logk, double c2, void* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMRF_HIP_H */
