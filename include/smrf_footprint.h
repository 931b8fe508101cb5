/* The grey-morphology block of the C ABI of libsmrf_hip.so (gfx950).  Included by smrf_hip.h, inside its extern "C"
 * region and after its SMRF_API and status codes; include that header, not this one. */
#ifndef SMRF_FOOTPRINT_H
#define SMRF_FOOTPRINT_H
#ifndef SMRF_HIP_H
#error "include smrf_hip.h: smrf_footprint.h is a part of it"
#endif

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

#endif /* SMRF_FOOTPRINT_H */
