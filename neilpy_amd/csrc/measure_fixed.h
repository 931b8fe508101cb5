// The fixed-point arithmetic of the per-label sums (csrc/measure.hip).  Plain __host__ __device__
// functions on integers: the CPU tests compile this header with g++ under the address and undefined-behaviour sanitizers
// (tests/test_measure_host.py).
//
// A label's terms t_i are fp64 values below 2^E in magnitude.  A term becomes the integer q = trunc(t * 2^(93 - E)),
// |q| < 2^93, cut into three pieces of 31 bits that carry q's sign: q = p[2] 2^62 + p[1] 2^31 + p[0].  The pieces of up to
// 2^31 terms are added in three int64 accumulators (each sum stays below 2^62), the accumulators are put together in a
// 128-bit integer, and that total times 2^(E - 93) is rounded once to the nearest fp64, ties to even.  No step depends on
// the order of the terms.
//
// The split works on the term's bits, not on fp64 arithmetic: mantissa and exponent are taken apart and the mantissa is
// shifted, so no scaling can overflow, no subnormal loses a bit, and what is cut off is cut off towards zero exactly.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMRF_FIXED_FN __host__ __device__ inline
#else
#define SMRF_FIXED_FN inline
#endif

constexpr int SMRF_FIXED_BITS = 93;    // q = trunc(t * 2^(SMRF_FIXED_BITS - E))
constexpr int SMRF_FIXED_PIECE = 31;   // bits per piece
constexpr uint64_t SMRF_F64_SIGN = 0x8000000000000000ull, SMRF_F64_EXP = 0x7FF0000000000000ull,
                   SMRF_F64_FRAC = 0x000FFFFFFFFFFFFFull;

SMRF_FIXED_FN uint64_t smrf_f64_bits(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, 8);
  return b;
}
SMRF_FIXED_FN double smrf_f64_of(uint64_t b) {
  double v;
  __builtin_memcpy(&v, &b, 8);
  return v;
}

// E with 2^(E - 1) <= M < 2^E for the finite M > 0 whose bits (sign cleared) are `abs_bits`: math.frexp's exponent
SMRF_FIXED_FN int smrf_fixed_exponent(uint64_t abs_bits) {
  const int biased = (int)(abs_bits >> 52);
  if (biased) return biased - 1022;
  return (64 - __builtin_clzll(abs_bits)) - 1074;            // subnormal: the mantissa's bit length, abs_bits != 0
}

// m shifted left by s (right by -s, towards zero); bits pushed past bit 63 are dropped, which the callers mask anyway
SMRF_FIXED_FN uint64_t smrf_shift(uint64_t m, int s) {
  if (s >= 64 || s <= -64) return 0;
  return s >= 0 ? m << s : m >> -s;
}

// The three pieces of q = trunc(t * 2^(93 - E)) for a finite t with |t| < 2^E.  t = m 2^e with an integer m < 2^53, so
// q = m shifted by e + 93 - E, and piece k is that shifted a further 31 k down and masked.
SMRF_FIXED_FN void smrf_fixed_split(double t, int E, int64_t p[3]) {
  const uint64_t b = smrf_f64_bits(t);
  const int biased = (int)((b & SMRF_F64_EXP) >> 52);
  const uint64_t m = biased ? (b & SMRF_F64_FRAC) | (1ull << 52) : (b & SMRF_F64_FRAC);
  const int e = (biased ? biased : 1) - 1075;
  // e + 93 - E is at most 40 for |t| < 2^E; the clamp keeps the sum in int range for any E a caller derives (2 E + 3)
  const long long wide = (long long)e + SMRF_FIXED_BITS - (long long)E;
  const int s = wide < -200 ? -200 : (int)wide;
  const uint64_t mask = (1ull << SMRF_FIXED_PIECE) - 1;
  const int64_t q0 = (int64_t)(smrf_shift(m, s) & mask), q1 = (int64_t)(smrf_shift(m, s - SMRF_FIXED_PIECE) & mask),
                q2 = (int64_t)(smrf_shift(m, s - 2 * SMRF_FIXED_PIECE) & mask);
  const bool neg = (b & SMRF_F64_SIGN) != 0;
  p[0] = neg ? -q0 : q0;
  p[1] = neg ? -q1 : q1;
  p[2] = neg ? -q2 : q2;
}

// the accumulators put together: a[2] 2^62 + a[1] 2^31 + a[0]; each |a[k]| < 2^62, so the total is below 2^125
SMRF_FIXED_FN __int128 smrf_fixed_total(const int64_t a[3]) {
  return (__int128)a[2] * ((__int128)1 << 62) + (__int128)a[1] * ((__int128)1 << 31) + (__int128)a[0];
}

// total * 2^e2 rounded to the nearest fp64, ties to even: subnormal results are rounded at 2^-1074, results of 2^1024 or
// more (after rounding) are the infinity of their sign, a zero total is +0.0
SMRF_FIXED_FN double smrf_fixed_round(__int128 total, int e2) {
  if (total == 0) return 0.0;
  const bool neg = total < 0;
  const unsigned __int128 mag = neg ? (unsigned __int128)0 - (unsigned __int128)total : (unsigned __int128)total;
  const uint64_t hi = (uint64_t)(mag >> 64), lo = (uint64_t)mag;
  const int nbits = hi ? 128 - __builtin_clzll(hi) : 64 - __builtin_clzll(lo);
  const uint64_t sign = neg ? SMRF_F64_SIGN : 0;
  long long lsb = (long long)nbits - 53 + e2;                // the exponent of the result's last bit
  if (lsb < -1074) lsb = -1074;
  const long long drop = lsb - e2;                           // low bits of mag that do not fit
  uint64_t kept;
  if (drop <= 0) {
    kept = (uint64_t)(mag << (int)-drop);                    // exact: at most 53 bits
  } else if (drop > nbits) {
    return smrf_f64_of(sign);                                // below half of the smallest subnormal
  } else {
    const int d = (int)drop;                                 // 1 .. nbits <= 125
    const unsigned __int128 one = 1, rem = mag & ((one << d) - 1), half = one << (d - 1);
    kept = (uint64_t)(mag >> d);
    if (rem > half || (rem == half && (kept & 1))) ++kept;
  }
  if (kept == 0) return smrf_f64_of(sign);
  if (kept == (1ull << 53)) {
    kept >>= 1;
    ++lsb;
  }
  if (kept < (1ull << 52)) return smrf_f64_of(sign | kept);  // subnormal: lsb is -1074
  const long long biased = lsb + 52 + 1023;
  if (biased >= 2047) return smrf_f64_of(sign | SMRF_F64_EXP);
  return smrf_f64_of(sign | ((uint64_t)biased << 52) | (kept & SMRF_F64_FRAC));
}
