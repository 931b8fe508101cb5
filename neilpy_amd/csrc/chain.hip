// Instantiates the chained small-window kernels of morph_chain.h, one per pattern of pf_route.h's kPatterns (which matches
// window lists against them).
#include <cmath>

#include "morph_chain.h"

namespace {

#ifndef SMRF_CHAIN_OCC
#define SMRF_CHAIN_OCC 4       // waves per SIMD the chain kernels are built for (tuning builds override)
#endif
// per pattern (fp32 singles; tuning builds override): waves per SIMD a kernel is built for
// (round 4: the single R = 7, pattern 7, fits 5 waves per SIMD - 0.641 -> 0.583 ms on 16384^2; at 5 the singles from R = 8 up and the chain 4, 5
// spill, at 3 R = 9, 10 gained on one box and lost on the next: profiles/r04_logs/chain_np_occ_ab.log)
#ifndef SMRF_CHAIN_OCC_OF
#define SMRF_CHAIN_OCC_OF(PAT) ((PAT) == 7 ? 5 : SMRF_CHAIN_OCC)
#endif
// the grouped fp64 singles hold 112-160 registers: built for 3 waves per SIMD
template <typename T>
int launch(int pat, const ChainArgs<T>& a_in, hipStream_t s) {
  ChainArgs<T> a = a_in;
  for (int i = 0; i < 4; ++i) {                            // largest float <= thr (morph_chain.h, flag step)
    a.thr_lo[i] = smrf_float_below(a.thr[i]);
  }
  constexpr bool F32 = sizeof(T) == 4;
  // a single window of radius R: fp32 as round 3 built them; F64OK: the grouped fp64 form exists (NP = 1, 3 waves per SIMD)
#define SMRF_SINGLE(PAT, R, F64OK)                                                                                        \
    case PAT:                                                                                                            \
      if constexpr (F32) return smrf::chain_launch<T, SMRF_CHAIN_NP(T, PAT), SMRF_CHAIN_OCC_OF(PAT), R, 0, 0, 0>(a, s);   \
      else if constexpr (F64OK) return smrf::chain_launch<T, 1, 3, R, 0, 0, 0>(a, s);                                    \
      else break;
  switch (pat) {
    case 0:   // fp64: one row pair per batch, built for 3 waves per SIMD (134 registers; at 4 it spills)
      if constexpr (F32) return smrf::chain_launch<T, SMRF_CHAIN_NP(T, 0), SMRF_CHAIN_OCC, 1, 2, 3, 0>(a, s);
      else return smrf::chain_launch<T, 1, 3, 1, 2, 3, 0>(a, s);
    case 1: return smrf::chain_launch<T, SMRF_CHAIN_NP(T, 1), SMRF_CHAIN_OCC, 1, 2, 0, 0>(a, s);
    case 2: return smrf::chain_launch<T, SMRF_CHAIN_NP(T, 2), SMRF_CHAIN_OCC, 2, 3, 0, 0>(a, s);
    case 3: if constexpr (F32) return smrf::chain_launch<T, SMRF_CHAIN_NP(T, 3), SMRF_CHAIN_OCC, 4, 5, 0, 0>(a, s); else break;   // fp32 only: the fp64 form spills
    SMRF_SINGLE(4, 4, true) SMRF_SINGLE(5, 5, true) SMRF_SINGLE(6, 6, false) SMRF_SINGLE(7, 7, true) SMRF_SINGLE(8, 8, true)
    SMRF_SINGLE(9, 9, false) SMRF_SINGLE(10, 10, false)
    default: break;
  }
#undef SMRF_SINGLE
  return smrf_fail(SMRF_E_ARG, "no chain kernel for pattern %d at this dtype", pat);
}

}  // namespace

int smrf_chain_f32(int pat, const ChainArgs<float>& a, hipStream_t s) { return launch<float>(pat, a, s); }
int smrf_chain_f64(int pat, const ChainArgs<double>& a, hipStream_t s) { return launch<double>(pat, a, s); }
