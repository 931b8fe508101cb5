// Instantiates the incremental erosion kernels (morph_incero.h), fp32, R = 16..64, and dispatches on the radius.
#include "morph_incero.h"

namespace {
template <int R>
int launch_r(const smrf::IncEroArgs<float>& a, hipStream_t s) { return smrf::inc_erode_launch<float, R>(a, s); }
}  // namespace

int smrf_inc_erode_f32(const float* e_prev, const float* last, float* out, int rows, int cols, long long ld, int radius, int nt,
                       hipStream_t s) {
  smrf::IncEroArgs<float> a{};
  a.e_prev = e_prev; a.last = last; a.out = out; a.rows = rows; a.cols = cols; a.ld = ld; a.nt = nt;
  a.seg = smrf_sw().ring_seg;   // 0: the launcher sizes segments from its occupancy
#define SMRF_INCERO_CASE(R) case R: return launch_r<R>(a, s);
#define SMRF_INCERO_CASE4(R) SMRF_INCERO_CASE(R) SMRF_INCERO_CASE(R + 1) SMRF_INCERO_CASE(R + 2) SMRF_INCERO_CASE(R + 3)
#define SMRF_INCERO_CASE16(R) SMRF_INCERO_CASE4(R) SMRF_INCERO_CASE4(R + 4) SMRF_INCERO_CASE4(R + 8) SMRF_INCERO_CASE4(R + 12)
  switch (radius) {
    SMRF_INCERO_CASE16(16) SMRF_INCERO_CASE16(32) SMRF_INCERO_CASE16(48) SMRF_INCERO_CASE(64)
    default: return smrf_fail(SMRF_E_UNSUPPORTED, "no incremental erosion kernel for radius %d", radius);
  }
}
