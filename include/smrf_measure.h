/* The measurement block of the C ABI of libsmrf_hip.so (gfx950): scipy.ndimage's per-label sums, moments, extrema and
 * positions of a 2-D raster (neilpy_amd/measure.py, csrc/measure.hip, csrc/measure_fixed.h).  A
 * header of its own beside smrf_hip.h: it takes SMRF_API and the SMRF_E_* status codes from there, and its prototypes are
 * bound by neilpy_amd/measure.py on the library neilpy_amd._lib.load() returns.  Every launching entry launches on `stream`
 * and returns without waiting for it. */
#ifndef SMRF_MEASURE_H
#define SMRF_MEASURE_H

#include "smrf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what to compute: a mask of these */
#define SMRF_MEASURE_COUNT 1
#define SMRF_MEASURE_SUM 2
#define SMRF_MEASURE_MEAN 4
#define SMRF_MEASURE_VARIANCE 8
#define SMRF_MEASURE_MIN 16
#define SMRF_MEASURE_MAX 32
#define SMRF_MEASURE_MIN_INDEX 64
#define SMRF_MEASURE_MAX_INDEX 128
#define SMRF_MEASURE_FLAGS 256
#define SMRF_MEASURE_ALL 511

/* the bits of a label's flag word */
#define SMRF_MEASURE_HAS_NAN 1
#define SMRF_MEASURE_HAS_POS_INF 2
#define SMRF_MEASURE_HAS_NEG_INF 4

/* how the labels plane is read */
#define SMRF_MEASURE_LABELS_AS_GIVEN 0
#define SMRF_MEASURE_LABELS_POSITIVE 1 /* a cell > 0 is label 1, any other cell label 0 */

/* The results of one call: n + 1 entries each, entry k for label k, k = 0 (the background) included.  A pointer may be
 * NULL unless `what` names it.  min and max have the raster's dtype (float for _f32, double for _f64). */
typedef struct smrf_measure_out {
  long long* count;     /* cells of the label */
  double* sum;          /* the fixed-point sum of DESIGN.md section 22 */
  double* mean;         /* sum / count */
  double* variance;     /* the fixed-point sum of (x - mean)^2, over count */
  void* min;            /* first of the label's values in np.sort's order; 0 for a label that does not occur */
  void* max;            /* last of them: NaN when a NaN is present */
  long long* min_index; /* lowest linear C index of a cell that holds the minimum, -1 for a label that does not occur */
  long long* max_index; /* lowest linear C index of a cell that holds the maximum */
  int* flags;           /* SMRF_MEASURE_HAS_* */
} smrf_measure_out;

/* Host only.  The workspace smrf_measure_* needs for labels 0..n, with L = n + 1 and every part rounded up to 256 bytes:
 * 4 up256(8 L) + up256(4 L) always (count, the two extreme keys, the largest finite magnitude, the flags),
 * + up256(24 L) + up256(8 L) where `what` has SUM, MEAN or VARIANCE (three accumulators, the mean),
 * + up256(16 L) where it has MIN_INDEX or MAX_INDEX, + up256(24 L) where it has VARIANCE.
 * SMRF_E_ARG for n < 0 or a `what` that is 0 or has other bits, SMRF_E_UNSUPPORTED for n >= 2^31 - 1. */
SMRF_API long long smrf_measure_workspace_bytes(long long n, int what);
/* The measurements `what` of the cells of each label 0..n of a contiguous rows x cols raster d_x, rows * cols < 2^31.
 * d_labels: an int32 plane of the same shape, read as `mode` says, or NULL: every cell is label 1.  Cells whose label is
 * below 0 or above n are ignored.  d_x and d_labels are read only.  One to three passes over the raster and the kernels
 * over the table between them, the fewest `what` needs; integer atomics only, so every value is the same on every run.
 * An empty raster is measured like any other: every label is one that does not occur. */
SMRF_API int smrf_measure_f32(const float* d_x, const int* d_labels, int rows, int cols, int n, int mode, int what,
                              const smrf_measure_out* out, void* d_work, long long work_bytes, void* stream);
SMRF_API int smrf_measure_f64(const double* d_x, const int* d_labels, int rows, int cols, int n, int mode, int what,
                              const smrf_measure_out* out, void* d_work, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SMRF_MEASURE_H */
