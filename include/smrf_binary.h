/* The binary-morphology block of the C ABI of libsmrf_hip.so (gfx950): scipy.ndimage's binary_erosion, binary_dilation,
 * binary_opening, binary_closing, binary_hit_or_miss, binary_propagation and binary_fill_holes of a 2-D raster on bit
 * planes (neilpy_amd/binary.py, csrc/binary.hip, csrc/binary_bits.h).  A header of its own beside
 * smrf_hip.h: it takes SMRF_API and the SMRF_E_* status codes from there, and its prototypes are bound by
 * neilpy_amd/binary.py on the library neilpy_amd._lib.load() returns.  Every launching entry launches on `stream` and
 * returns without waiting for it.  Null pointers, negative sizes (SMRF_E_ARG) and rasters of rows * cols >= 2^31 cells
 * (SMRF_E_UNSUPPORTED) are refused before any launch; an empty raster is SMRF_OK with nothing launched.
 *
 * A bit plane of a rows x cols raster is rows x ceil(cols / 64) words of 64 bits in C order; bit b of word w of a row is
 * the cell in column 64 w + b.  Every entry writes the bits past `cols` of a row's last word as zeros, and none trusts
 * them in a plane it reads. */
#ifndef SMRF_BINARY_H
#define SMRF_BINARY_H

#include "smrf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMRF_BINARY_ERODE 0  /* op of smrf_binary_step: AND over the members */
#define SMRF_BINARY_DILATE 1 /* OR over the members */

/* Host only.  s: a structure of srows x scols bytes in C order, a non-zero byte is a member.  Writes the member table the
 * launching entries read: n pairs (dr, dc) = member - centre, the centre at size / 2 + origin per axis, sorted by dr, then
 * dc.  reflect != 0: the pairs negated and sorted again, the table of a dilation (out[p] = OR of in[p - d]).  out holds
 * 2 * srows * scols ints, or is NULL to count the members only.  Returns n, or SMRF_E_ARG where an origin lies outside
 * -(size / 2) <= origin <= (size - 1) / 2 for its axis. */
SMRF_API int smrf_binary_offsets(const unsigned char* s, int srows, int scols, int origin_r, int origin_c, int reflect,
                                 int* out);
/* Host only.  The bytes of a bit plane: 8 rows ceil(cols / 64). */
SMRF_API long long smrf_binary_plane_bytes(int rows, int cols);
/* d_bits = the bit plane of the contiguous rows x cols byte plane d_bytes: a cell is set iff its byte is non-zero, or with
 * complement != 0 iff it is zero.  d_bytes may start at any address. */
SMRF_API int smrf_binary_pack(const unsigned char* d_bytes, unsigned long long* d_bits, int rows, int cols, int complement,
                              void* stream);
/* d_bytes = the cells of the bit plane d_bits as bytes 1 and 0, or with complement != 0 as 0 and 1.  d_bytes is written in
 * 8-byte stores and must be aligned to 8 bytes (otherwise SMRF_E_ARG). */
SMRF_API int smrf_binary_unpack(const unsigned long long* d_bits, unsigned char* d_bytes, int rows, int cols,
                                int complement, void* stream);
/* One step: d_out[p] = AND (op SMRF_BINARY_ERODE) or OR (SMRF_BINARY_DILATE) over the n members (dr, dc) of d_table
 * (device, int pairs, as smrf_binary_offsets writes them) of d_in[p + (dr, dc)]; a cell outside the raster reads as
 * border != 0.  No member: all ones for AND, all zeros for OR.  d_mask (a bit plane, may be NULL): where it is clear the
 * cell keeps d_in's value.  d_changed (device int, may be NULL): ORed with 1 if any cell of d_out differs from d_in, by
 * one atomic per wave that holds such a cell; the caller clears it.  d_in and d_out are different planes. */
SMRF_API int smrf_binary_step(const unsigned long long* d_in, unsigned long long* d_out, int rows, int cols,
                              const unsigned long long* d_mask, const int* d_table, int n, int op, int border,
                              int* d_changed, void* stream);
/* d_out[p] = AND over the n_hit members of d_hit of d_in[p + d], AND over the n_miss members of d_miss of not d_in[p + d],
 * both halves in one launch of the step kernel; the outside of the raster is background for both. */
SMRF_API int smrf_binary_hit_or_miss(const unsigned long long* d_in, unsigned long long* d_out, int rows, int cols,
                                     const int* d_hit, int n_hit, const int* d_miss, int n_miss, void* stream);
/* Host only.  The workspace of smrf_binary_propagate, each part rounded up to 256 bytes: the labels plane (4 rows cols),
 * smrf_label_workspace_bytes(rows, cols), the flag plane (rows cols + 1), three bit planes (the input, the mask, one step
 * of the input) and 256 bytes for the object count and the structure's member table.  0 for an empty raster. */
SMRF_API long long smrf_binary_propagate_workspace_bytes(int rows, int cols);
/* The converged masked dilation of d_input under d_mask - binary_propagation - for the centrally symmetric 3 x 3 structure
 * with its centre set that the link mask `links` names (SMRF_LABEL_E | ..., include/smrf_label.h), without iterating:
 * d_out[p] = d_input[p] outside the mask, and inside it 1 iff the cell's component of the mask under the links holds a
 * cell that one masked dilation step of d_input sets (that step brings in border != 0 and the set cells outside the
 * mask).  complement != 0 writes the complement, binary_fill_holes' last step.  d_input, d_mask: contiguous rows x cols
 * byte planes, non-zero is set; d_input may be NULL for all zeros.  d_out: bytes 0 and 1, written in dword stores,
 * aligned to 4 bytes.  d_work: aligned to 256 bytes.  Launches on `stream`: the member table, two packs, the step,
 * smrf_label_u8's six, a memset of the flag plane, mark and select; the object count is not read back. */
SMRF_API int smrf_binary_propagate(const unsigned char* d_input, const unsigned char* d_mask, unsigned char* d_out, int rows,
                                   int cols, int links, int border, int complement, void* d_work, long long work_bytes,
                                   void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SMRF_BINARY_H */
