// The bit logic of binary morphology on bit planes (csrc/binary.hip).  Plain __host__ __device__
// functions over callables, as label_runs.h: the CPU tests compile this header with g++ and run the step "lane by lane"
// with the kernel's own text (tests/test_binary_host.py).
//
// Bit planes.  A raster of rows x cols cells is rows x ceil(cols / 64) words of 64 bits; bit b of word w of a row is the
// cell in column 64 w + b.  The bits of a row's last word past `cols` are never trusted: whoever reads a word replaces
// them, and every column and row outside the raster, with the border value (smrf_bits_word).
//
// Members.  A structure travels as a table of (dr, dc) pairs sorted by dr, then dc: member k reads the cell (r + dr,
// c + dc).  For the 64 cells of output word w that is the bit string starting at column 64 w + dc of row r + dr: with
// q = floor(dc / 64) and s = dc - 64 q it is the funnel shift by s of the words w + q and w + q + 1 (smrf_bits_funnel).  dc
// may exceed 64 in magnitude, and consecutive members of a structure row mostly share their two words, which
// SmrfBitsWindow keeps.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMRF_BITS_FN __host__ __device__ inline
#else
#define SMRF_BITS_FN inline
#endif

enum { SMRF_BITS_AND = 0, SMRF_BITS_OR = 1 };   // the op of a step: erosion, dilation

// words per row
SMRF_BITS_FN int smrf_bits_words(int cols) { return (int)(((long long)cols + 63) >> 6); }

// the bits of word w of a row that are cells of the raster
SMRF_BITS_FN uint64_t smrf_bits_valid(int cols, int w) {
  const long long left = (long long)cols - 64ll * w;
  return left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1;
}

// 64 copies of the border value
SMRF_BITS_FN uint64_t smrf_bits_border(int border) { return border ? ~0ull : 0ull; }

// floor(dc / 64) and the shift dc - 64 floor(dc / 64), 0 .. 63
SMRF_BITS_FN int smrf_bits_word_shift(int dc) { return dc >> 6; }
SMRF_BITS_FN int smrf_bits_bit_shift(int dc) { return dc & 63; }

// the first and the last word index that the 64 cells of output word w read through a member at column offset dc
SMRF_BITS_FN void smrf_bits_span(int w, int dc, int* first, int* last) {
  *first = w + smrf_bits_word_shift(dc);
  *last = *first + (smrf_bits_bit_shift(dc) != 0);
}

// bits s .. s + 63 of the 128-bit string hi:lo, s in 0 .. 63
SMRF_BITS_FN uint64_t smrf_bits_funnel(uint64_t lo, uint64_t hi, int s) { return s ? (lo >> s) | (hi << (64 - s)) : lo; }

// Word j of row `row` as every reader sees it: the border word outside the raster, and inside it the stored word with the
// bits past `cols` replaced by the border value.  load(row, j) is called for words inside the raster only.
template <typename Load>
SMRF_BITS_FN uint64_t smrf_bits_word(Load&& load, int rows, int cols, int row, int j, int border) {
  const uint64_t b = smrf_bits_border(border);
  if (row < 0 || row >= rows || j < 0 || j >= smrf_bits_words(cols)) return b;
  const uint64_t valid = smrf_bits_valid(cols, j);
  return (load(row, j) & valid) | (b & ~valid);
}

// the two adjacent words a member was last taken from: a member of the same row whose span is the same, or one word on,
// loads one word or none
struct SmrfBitsWindow {
  int row, j;          // lo is word j of `row`, hi word j + 1
  bool has_hi;
  uint64_t lo, hi;
};

SMRF_BITS_FN SmrfBitsWindow smrf_bits_window() { return SmrfBitsWindow{0, 0, false, 0, 0}; }

// the 64 cells (row, 64 w + dc ..) as a word; `fresh` says that the window holds nothing yet
template <typename Load>
SMRF_BITS_FN uint64_t smrf_bits_member(Load&& load, int rows, int cols, int row, int w, int dc, int border,
                                       SmrfBitsWindow& win, bool fresh) {
  const int j = w + smrf_bits_word_shift(dc), s = smrf_bits_bit_shift(dc);
  if (fresh || win.row != row || (win.j != j && win.j + 1 != j)) {
    win.row = row;
    win.j = j;
    win.lo = smrf_bits_word(load, rows, cols, row, j, border);
    win.has_hi = false;
  } else if (win.j + 1 == j) {
    win.lo = win.has_hi ? win.hi : smrf_bits_word(load, rows, cols, row, j, border);
    win.j = j;
    win.has_hi = false;
  }
  if (s && !win.has_hi) {
    win.hi = smrf_bits_word(load, rows, cols, row, j + 1, border);
    win.has_hi = true;
  }
  return smrf_bits_funnel(win.lo, win.hi, s);
}

// AND (erosion) or OR (dilation) over the n members of `table` ((dr, dc) pairs) of the cells they read for output word w
// of row r.  No member: all ones for AND, all zeros for OR.
template <typename Load>
SMRF_BITS_FN uint64_t smrf_bits_combine(Load&& load, int rows, int cols, int r, int w, const int* table, int n, int op,
                                        int border) {
  uint64_t acc = op == SMRF_BITS_AND ? ~0ull : 0ull;
  SmrfBitsWindow win = smrf_bits_window();
  for (int k = 0; k < n; ++k) {
    const uint64_t v = smrf_bits_member(load, rows, cols, r + table[2 * k], w, table[2 * k + 1], border, win, k == 0);
    acc = op == SMRF_BITS_AND ? acc & v : acc | v;
  }
  return acc;
}

// One output word of a step, the body of the step kernel.
//   plain step      new = op over `table`, cells outside the raster read as `border`
//   hit or miss     n2 >= 0: new = (AND over `table`) & ~(OR over `table2`), the outside background for both (op and
//                   border are passed as SMRF_BITS_AND and 0)
//   mask            has_mask: new = (mask & new) | (~mask & old), old = the input's own word, mask_word = the mask's
// The bits past `cols` of the result are zero.  *changed = the result differs from the input's own word in a cell of the
// raster.
template <typename Load>
SMRF_BITS_FN uint64_t smrf_bits_step_word(Load&& load, int rows, int cols, int r, int w, const int* table, int n, int op,
                                          int border, const int* table2, int n2, bool has_mask, uint64_t mask_word,
                                          bool* changed) {
  const uint64_t valid = smrf_bits_valid(cols, w);
  const uint64_t old = load(r, w) & valid;
  uint64_t v = smrf_bits_combine(load, rows, cols, r, w, table, n, op, border);
  if (n2 >= 0) v &= ~smrf_bits_combine(load, rows, cols, r, w, table2, n2, SMRF_BITS_OR, 0);
  v &= valid;
  if (has_mask) v = (mask_word & v) | (~mask_word & old);
  *changed = v != old;
  return v;
}

// Host side of the table: the members of a structure (srows x scols bytes in C order, any non-zero byte is a member)
// about the centre c = size / 2 + origin per axis, as (dr, dc) = member - centre in C order of the members, which is
// sorted by dr, then dc.  reflect: the pairs negated and in reverse order, sorted again - dilation's out[p] = OR of
// in[p - d] as a table that reads in[p + d'].  Returns the number of members (out may be null to count them), or -1 where
// an origin lies outside -(n / 2) <= origin <= (n - 1) / 2 for its axis of length n.
SMRF_BITS_FN int smrf_bits_offsets(const unsigned char* s, int srows, int scols, int origin_r, int origin_c, int reflect,
                                   int* out) {
  if ((srows > 0 && (origin_r < -(srows / 2) || origin_r > (srows - 1) / 2)) ||
      (scols > 0 && (origin_c < -(scols / 2) || origin_c > (scols - 1) / 2)))
    return -1;
  const int cr = srows / 2 + origin_r, cc = scols / 2 + origin_c;
  const long long size = (long long)srows * scols;
  int n = 0;
  for (long long k = 0; k < size; ++k) {
    const long long m = reflect ? size - 1 - k : k;
    if (!s[m]) continue;
    if (out) {
      const int dr = (int)(m / scols) - cr, dc = (int)(m % scols) - cc;
      out[2 * n] = reflect ? -dr : dr;
      out[2 * n + 1] = reflect ? -dc : dc;
    }
    ++n;
  }
  return n;
}
