// Order-preserving unsigned keys of float32 / float64 values, and the two rank selections of csrc/rank.hip written over
// any indexable list of keys.  Plain __host__ __device__ functions: the CPU tests compile this
// header with g++ (tests/test_rank_host.py).
//
// key(v): a set sign bit flips all bits, a clear one sets it, so keys compare (unsigned) as the values do (as floats):
// -inf < ... < -0.0 < +0.0 < ... < +inf, and a NaN of positive sign after +inf.  With `nan_last` every NaN becomes the
// all-ones key, so NaNs of negative sign sort last as well: np.sort's order.  unkey() is the inverse; the all-ones key
// comes back as the quiet NaN.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMRF_KEY_FN __host__ __device__ inline
#else
#define SMRF_KEY_FN inline
#endif

template <typename T>
struct SmrfKey;
template <>
struct SmrfKey<float> {
  using type = uint32_t;
  static constexpr int bits = 32;
  static constexpr type quiet_nan = 0x7FC00000u;
  static constexpr type exponent = 0x7F800000u;
};
template <>
struct SmrfKey<double> {
  using type = uint64_t;
  static constexpr int bits = 64;
  static constexpr type quiet_nan = 0x7FF8000000000000ull;
  static constexpr type exponent = 0x7FF0000000000000ull;
};

template <typename T>
SMRF_KEY_FN typename SmrfKey<T>::type smrf_key(T v, bool nan_last) {
  using K = typename SmrfKey<T>::type;
  K b;
  __builtin_memcpy(&b, &v, sizeof(K));
  const K sign = (K)1 << (SmrfKey<T>::bits - 1);
  if (nan_last && (b & ~sign) > SmrfKey<T>::exponent) return ~(K)0;
  return (b & sign) ? ~b : (b | sign);
}

template <typename T>
SMRF_KEY_FN T smrf_unkey(typename SmrfKey<T>::type k) {
  using K = typename SmrfKey<T>::type;
  const K sign = (K)1 << (SmrfKey<T>::bits - 1);
  K b = (k & sign) ? (k & ~sign) : ~k;
  if (k == ~(K)0) b = SmrfKey<T>::quiet_nan;
  T v;
  __builtin_memcpy(&v, &b, sizeof(K));
  return v;
}

SMRF_KEY_FN int smrf_top_bit(uint32_t x) { return 31 - __builtin_clz(x); }          // x != 0
SMRF_KEY_FN int smrf_top_bit(uint64_t x) { return 63 - __builtin_clzll(x); }

// BISECT: the key at position `rank` (0 <= rank < n) of at(0) .. at(n - 1) sorted ascending, as a radix select on the
// key, one bit per pass from the top.  The first pass finds the least and the largest key: they are the answers at rank
// 0 and n - 1, and the bits above their first difference are common to every member, so the passes start below them;
// all members equal means no pass at all.  A pass counts the members below the candidate prefix `c`: at most `rank` of
// them means the answer is not below `c`.
template <typename K, typename At>
SMRF_KEY_FN K smrf_select_bisect(int n, int rank, At&& at) {
  K lo = at(0), hi = lo;
#pragma unroll 4
  for (int j = 1; j < n; ++j) {
    const K a = at(j);
    lo = a < lo ? a : lo;
    hi = a > hi ? a : hi;
  }
  if (rank == 0 || lo == hi) return lo;
  if (rank == n - 1) return hi;
  const int top = smrf_top_bit((K)(lo ^ hi));
  K p = lo & ~((((K)1 << top) << 1) - 1);           // the common prefix, zeros below it
  for (int bit = top; bit >= 0; --bit) {
    const K c = p | ((K)1 << bit);
    int below = 0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) below += at(j) < c ? 1 : 0;
    if (below <= rank) p = c;
  }
  return p;
}

// COUNT: member i stands at position #{a_j < a_i} + #{j < i : a_j == a_i} of the stable sort, and the member whose
// position is `rank` is the answer.  BLOCK candidates are held at a time and the members are swept once per block; a
// candidate past the end of the list answers nothing.  `done(found)` may end the search early (the kernel: once every
// lane of the wave has its answer).
template <typename K, int BLOCK, typename At, typename Done>
SMRF_KEY_FN K smrf_select_count(int n, int rank, At&& at, Done&& done) {
  K res = 0;
  bool found = false;
  for (int i0 = 0; i0 < n; i0 += BLOCK) {
    K cand[BLOCK];
    int pos[BLOCK];
#pragma unroll
    for (int k = 0; k < BLOCK; ++k) {
      cand[k] = at(i0 + k < n ? i0 + k : n - 1);
      pos[k] = 0;
    }
#pragma unroll 2
    for (int j = 0; j < i0; ++j) {                  // members ahead of the block: an equal one stands first
      const K a = at(j);
#pragma unroll
      for (int k = 0; k < BLOCK; ++k) pos[k] += a <= cand[k] ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < BLOCK; ++k)                 // the block against itself
#pragma unroll
      for (int m = 0; m < BLOCK; ++m)
        if (m != k) pos[k] += (m < k ? cand[m] <= cand[k] : cand[m] < cand[k]) && i0 + m < n ? 1 : 0;
#pragma unroll 2
    for (int j = i0 + BLOCK; j < n; ++j) {          // members behind it
      const K a = at(j);
#pragma unroll
      for (int k = 0; k < BLOCK; ++k) pos[k] += a < cand[k] ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < BLOCK; ++k)
      if (i0 + k < n && pos[k] == rank) {
        res = cand[k];
        found = true;
      }
    if (done(found)) break;
  }
  return res;
}
