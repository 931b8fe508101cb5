// The bit logic and the union-find of connected-component labelling (csrc/label.hip).  Plain
// __host__ __device__ functions over callables: the CPU tests compile this header with g++ and label tiles with the same
// text (tests/test_label_host.py).
//
// Links.  scipy.ndimage.label accepts exactly the centrally symmetric 3 x 3 structures and ignores the centre, so a
// structure is four independent links of a cell (r, c): E to (r, c + 1), S to (r + 1, c), SE to (r + 1, c + 1) and SW to
// (r + 1, c - 1); their mirror images W, N, NW and NE are the same links seen from the other cell.
//
// Rows.  A row segment of up to 64 cells is one mask, bit c = cell c is foreground.  With the E link a maximal run of set
// bits is one object already, named by its first cell: run starts are m & ~(m << 1), and the start of the run a cell lies
// in is the highest start bit at or below it.  Without the E link every foreground cell is a run of its own.
//
// Union-find to the minimum index.  parent[i] <= i always, a root has parent[i] == i, and two roots are united by
// parent[hi] = min(parent[hi], lo) done atomically, the value it held decides what follows (smrf_unite_min).  So the
// root of a set ends as its smallest index, whatever order the unions land in.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMRF_RUNS_FN __host__ __device__ inline
#else
#define SMRF_RUNS_FN inline
#endif

enum { SMRF_LINK_E = 1, SMRF_LINK_S = 2, SMRF_LINK_SE = 4, SMRF_LINK_SW = 8 };

// the link mask of a 3 x 3 structure in C order (any non-zero byte is a member; the centre is ignored), or -1 where the
// structure is not centrally symmetric
SMRF_RUNS_FN int smrf_links_of(const unsigned char s[9]) {
  for (int k = 0; k < 4; ++k)
    if ((s[k] != 0) != (s[8 - k] != 0)) return -1;
  return (s[5] ? SMRF_LINK_E : 0) | (s[7] ? SMRF_LINK_S : 0) | (s[8] ? SMRF_LINK_SE : 0) | (s[6] ? SMRF_LINK_SW : 0);
}

// bit c = cell c starts a run
SMRF_RUNS_FN uint64_t smrf_run_starts(uint64_t m, int links) { return (links & SMRF_LINK_E) ? m & ~(m << 1) : m; }

// the first cell of the run that holds cell c (bit c of `starts`' mask is set, so a start at or below c exists)
SMRF_RUNS_FN int smrf_run_start_of(uint64_t starts, int c) {
  const uint64_t upto = starts & (~0ull >> (63 - c));
  return 63 - __builtin_clzll(upto);
}

// of the set bits of j - cells linked to the row above in one direction - those that name a pair of runs not named by
// the bit below already: with the E link a stretch of consecutive bits joins the same two runs throughout
SMRF_RUNS_FN uint64_t smrf_first_of_each(uint64_t j, int links) { return (links & SMRF_LINK_E) ? j & ~(j << 1) : j; }

// Cell c of a row with mask m under a row with mask up: join(cu) for every column cu of the upper row whose run has to be
// united with the cell's run.  Called for every foreground cell of the row, the runs of the two rows end up united
// wherever a link joins them.
template <typename Join>
SMRF_RUNS_FN void smrf_row_links(uint64_t up, uint64_t m, int c, int links, Join&& join) {
  const uint64_t bit = 1ull << c;
  if ((links & SMRF_LINK_S) && (smrf_first_of_each(m & up, links) & bit)) join(c);
  if ((links & SMRF_LINK_SE) && (smrf_first_of_each(m & (up << 1), links) & bit)) join(c - 1);   // (r - 1, c - 1): its SE is (r, c)
  if ((links & SMRF_LINK_SW) && (smrf_first_of_each(m & (up >> 1), links) & bit)) join(c + 1);   // (r - 1, c + 1): its SW is (r, c)
}

// the root of x: load(i) returns parent[i], or any value parent[i] has held since x's set was last a set of its own - an
// ancestor of i either way, and the chain falls strictly, so the walk ends
template <typename Load>
SMRF_RUNS_FN int smrf_find_root(int x, Load&& load) {
  for (int p = load(x); p != x; p = load(x)) x = p;
  return x;
}

// Unite the sets of a and b.  atomic_min(i, v) does parent[i] = min(parent[i], v) as one atomic operation and returns
// what parent[i] held.  Find both roots (stale reads give ancestors, which serve as well); with hi the larger and lo the
// smaller, old = atomic_min(hi, lo).  old == hi: hi was a root and now hangs below lo, done.  Otherwise another union had
// linked hi to old < hi meanwhile; parent[hi] is now min(old, lo), so whichever of old and lo lost that place is still to
// be united with the other: carry on with (old, lo), both below hi, so this ends.  Every link ever written joins two cells
// of one object and points to a smaller index, a link that is replaced is made again by the carry-on, and nothing is
// decided from two roots being different - so once every call has returned the sets are the objects and each root is its
// object's smallest index, in any order of arrival and without a fence.
template <typename Load, typename AtomicMin>
SMRF_RUNS_FN void smrf_unite_min(int a, int b, Load&& load, AtomicMin&& atomic_min) {
  for (;;) {
    a = smrf_find_root(a, load);
    b = smrf_find_root(b, load);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomic_min(hi, lo);
    if (old == hi) return;
    a = old;
    b = lo;
  }
}
