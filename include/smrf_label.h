/* The connected-component block of the C ABI of libsmrf_hip.so (gfx950): scipy.ndimage.label and find_objects of a 2-D
 * raster, object sizes and bounding boxes, and the removal of small objects (neilpy_amd/label.py, csrc/label.hip,
 * csrc/label_runs.h).  A header of its own beside smrf_hip.h: it takes SMRF_API and the SMRF_E_*
 * status codes from there, and its prototypes are bound by neilpy_amd/label.py on the library neilpy_amd._lib.load()
 * returns.  Every launching entry launches on `stream` and returns without waiting for it. */
#ifndef SMRF_LABEL_H
#define SMRF_LABEL_H

#include "smrf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the four independent links of a centrally symmetric 3 x 3 structure, from a cell (r, c) */
#define SMRF_LABEL_E 1  /* to (r, c + 1) */
#define SMRF_LABEL_S 2  /* to (r + 1, c) */
#define SMRF_LABEL_SE 4 /* to (r + 1, c + 1) */
#define SMRF_LABEL_SW 8 /* to (r + 1, c - 1) */

#define SMRF_LABEL_TILE_ROWS 64    /* the tile one workgroup labels in LDS */
#define SMRF_LABEL_TILE_COLS 64
#define SMRF_LABEL_SCAN_BLOCK 2048 /* cells whose roots one workgroup counts and numbers */

/* Host only.  s: a 3 x 3 structure in C order, a non-zero byte is a member, the centre is ignored.  Returns the link mask
 * (SMRF_LABEL_E | ...), 0 to 15, or SMRF_E_ARG where the structure is not centrally symmetric - the structures
 * scipy.ndimage.label refuses. */
SMRF_API int smrf_label_links(const unsigned char* s);
/* Host only.  The workspace smrf_label_u8 needs: one int32 plane and one uint32 per SMRF_LABEL_SCAN_BLOCK cells, each
 * part rounded up to 256 bytes: up256(4 rows cols) + up256(4 ceil(rows cols / SMRF_LABEL_SCAN_BLOCK)).  0 for an empty
 * raster, SMRF_E_ARG for a negative size, SMRF_E_UNSUPPORTED where rows * cols >= 2^31. */
SMRF_API long long smrf_label_workspace_bytes(int rows, int cols);
/* d_labels[r, c] = 0 where d_mask[r, c] == 0, otherwise the number of the cell's object under the links: objects are
 * numbered from 1 in the C order of their first cells.  *d_count (device, int32) = the number of objects.  Contiguous
 * rows x cols planes, rows * cols < 2^31; d_mask is read only.  Six launches on `stream` (tile, seam, flatten, scan of
 * the block counts, number, relabel), no grid barrier and no wait on another workgroup in any of them; the result does
 * not depend on the order in which atomics land. */
SMRF_API int smrf_label_u8(const unsigned char* d_mask, int* d_labels, int rows, int cols, int links, void* d_work,
                           long long work_bytes, int* d_count, void* stream);
/* Sizes and bounding boxes of the labels 1..n of a contiguous rows x cols int32 plane.  d_size (n + 1 int64, may be
 * NULL): d_size[k] = cells equal to k, k = 0 included.  d_box (n x 4 int32, may be NULL): r0, r1, c0, c1 of label k + 1,
 * half-open, (0, 0, 0, 0) for a label that does not occur.  Cells below 0 or above n are ignored.  Integer atomics only,
 * one per stretch of equal labels within a wave, so the result is exact and the same on every run. */
SMRF_API int smrf_label_regions(const int* d_labels, int rows, int cols, int n, long long* d_size, int* d_box,
                                void* stream);
/* d_out[i] = 1 where d_labels[i] > 0 and d_size[d_labels[i]] >= min_size, else 0, for i < cells.  d_labels holds values
 * in 0 .. (length of d_size) - 1, as smrf_label_u8 wrote them. */
SMRF_API int smrf_label_keep(const int* d_labels, const long long* d_size, long long cells, long long min_size,
                             unsigned char* d_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SMRF_LABEL_H */
