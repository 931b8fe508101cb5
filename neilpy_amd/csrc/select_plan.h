// The bucket walk of the radix select behind raster_stats' median (relief.hip): plain C++, so that a host test compiles
// it with g++ and fuzzes it against a sort (tests/test_relief_host.py), and the device runs the very same lines.
//
// A float is turned into an order-preserving unsigned key (float32: 32 bits, float64: 64 bits).  The two middle order
// statistics, ranks (n - 1) / 2 and n / 2 of the n non-NaN keys, are found digit by digit from the top: pass p looks at
// the key bits [select_lo(p), select_hi(p)), SELECT_BITS of them (the last pass takes what is left).  Each pass counts,
// for each of the two ranks, the keys that agree with the rank's prefix in every bit above the digit, by digit value -
// a histogram row of SELECT_BUCKETS counts - and select_step() then walks the row: the digit is the first bucket whose
// running total exceeds the rank, the prefix gets the digit, and the rank becomes its residue inside that bucket.  The
// two ranks share row 0 while their prefixes are equal; they can part ways in any pass, and row 1 belongs to the second
// from then on.  Only integers are counted, so the result does not depend on the order of the atomics.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SMRF_SELECT_HD __host__ __device__
#else
#define SMRF_SELECT_HD
#endif

namespace smrf {

constexpr int SELECT_BITS = 11;                      // 3 passes for float32, 6 for float64
constexpr int SELECT_BUCKETS = 1 << SELECT_BITS;     // one row: 8 KB of 32-bit counts in LDS

SMRF_SELECT_HD constexpr int select_passes(int key_bits) { return (key_bits + SELECT_BITS - 1) / SELECT_BITS; }
// the digit of pass p (0 = the top one) is the key bits [lo, hi)
SMRF_SELECT_HD constexpr int select_hi(int key_bits, int pass) { return key_bits - pass * SELECT_BITS; }
SMRF_SELECT_HD constexpr int select_lo(int key_bits, int pass) {
  return select_hi(key_bits, pass) > SELECT_BITS ? select_hi(key_bits, pass) - SELECT_BITS : 0;
}

struct SelectState {
  uint64_t prefix[2];   // the key bits decided so far, in place (the undecided low bits are 0)
  uint64_t rank[2];     // residual rank among the keys that carry the prefix
  uint64_t count;       // n: the number of keys (non-NaN cells)
};

// the sum of a row: pass 0 counts every key, so this is n
template <typename H>
SMRF_SELECT_HD inline uint64_t select_total(const H* row) {
  uint64_t t = 0;
  for (int b = 0; b < SELECT_BUCKETS; ++b) t += (uint64_t)row[b];
  return t;
}

// ranks of the two middle order statistics of n >= 1 keys (equal for odd n); n = 0 leaves rank 0 twice, and the
// caller reports NaN
SMRF_SELECT_HD inline void select_begin(SelectState& s, uint64_t n) {
  s.prefix[0] = s.prefix[1] = 0;
  s.count = n;
  s.rank[0] = n ? (n - 1) / 2 : 0;
  s.rank[1] = n / 2;
}

// one rank through one row: every bucket is visited, without a branch on the data, so that the loads can be in flight
// together.  Returns the digit; `rank` becomes the residue.
template <typename H>
SMRF_SELECT_HD inline int select_walk(const H* row, uint64_t& rank) {
  uint64_t cum = 0, below = 0;
  int digit = 0;
  for (int b = 0; b < SELECT_BUCKETS; ++b) {
    const uint64_t next = cum + (uint64_t)row[b];
    const bool passed = next <= rank;          // the rank lies beyond bucket b
    digit += passed ? 1 : 0;
    below = passed ? next : below;
    cum = next;
  }
  if (digit >= SELECT_BUCKETS) digit = SELECT_BUCKETS - 1;   // rank >= the row's total: not reached for a consistent row
  rank -= below;
  return digit;
}

// `rows` = [2][SELECT_BUCKETS] histogram of the digit [lo, ...): row k counts the keys that agree with prefix[k] above
// the digit.  Row 1 is read only if the prefixes differ on entry.
template <typename H>
SMRF_SELECT_HD inline void select_step(const H* rows, int lo, SelectState& s) {
  const bool together = s.prefix[0] == s.prefix[1];
  const int d0 = select_walk(rows, s.rank[0]);
  const int d1 = select_walk(together ? rows : rows + SELECT_BUCKETS, s.rank[1]);
  s.prefix[0] |= (uint64_t)d0 << lo;
  s.prefix[1] |= (uint64_t)d1 << lo;
}

}  // namespace smrf
