// Binary morphology on bit planes: scipy.ndimage's binary_erosion, binary_dilation, binary_opening, binary_closing,
// binary_hit_or_miss, binary_propagation and binary_fill_holes of a 2-D raster.  Host side: neilpy_amd/binary.py; C ABI:
// include/smrf_binary.h; bit logic: csrc/binary_bits.h; contract, the propagation identity and the byte model: DESIGN.md
// section 23.
//
//   pack      a byte plane (a cell is foreground iff its byte is non-zero) becomes a bit plane.  A lane takes the 8 bytes
//             of 8 consecutive cells of a row from the aligned dwords that hold them, turns them into 8 bits, and the 8
//             lanes of a word join theirs by shuffles; the bits past `cols` are written as zeros.
//   unpack    a bit plane becomes 0 / 1 bytes, 8 cells of the flat plane per lane in one 8-byte store.
//   step      one lane makes one output word: smrf_bits_step_word over the member table, which every lane of a wave
//             walks in step, so the table is read with scalar loads.  The mask= select, hit-or-miss' second table and
//             the "changed" flag ride in the same launch; the flag is one atomic OR per wave that changed a cell.
//   propagate the converged masked dilation for the symmetric 3 x 3 structures without iterating: one step, the
//             components of the mask from smrf_label_u8, a mark pass and a select pass.
//
// Every kernel is a grid-stride loop over long long indices; no kernel waits for another workgroup.
#include "binary_bits.h"
#include "raster_stencil.h"
#include "smrf_binary.h"
#include "smrf_label.h"

namespace {

constexpr int NT = 256, GRID_CAP = 1 << 16;

// ---------------------------------------------------------------------------------------------------------------
// pack and unpack
// ---------------------------------------------------------------------------------------------------------------
// bit i of the result = byte i of v is non-zero
__device__ __forceinline__ unsigned bits_of_bytes(uint64_t v) {
  const uint64_t low7 = 0x7f7f7f7f7f7f7f7full;
  const uint64_t top = (((v & low7) + low7) | v) & ~low7;           // bit 7 of a byte: the byte is non-zero
  return (unsigned)(((top >> 7) * 0x0102040810204080ull) >> 56);    // the terms 2^(8 i + 7 j + 7) are distinct: no carry
}

// Lane i takes byte k = i % 8 of word i / 8: the cells 64 w + 8 k .. + 7 of row r, those below `cols`.  Its bytes start at
// any address; it loads the up to three aligned dwords that hold one of them - a dword that holds a byte of the plane lies
// in the plane's pages - and shifts the 8 bytes out of them.
__global__ __launch_bounds__(NT) void binary_pack_kernel(const unsigned char* __restrict__ bytes, uint64_t* __restrict__ bits,
                                                         int cols, int W, long long words, int complement) {
  const long long stride = (long long)gridDim.x * NT;
  for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < 8 * words; i += stride) {
    const long long word = i >> 3;
    const int k = (int)(i & 7), w = (int)(word % W);
    const long long r = word / W;
    const int c0 = 64 * w + 8 * k, have = min(8, cols - c0);        // cells of this lane that exist (may be <= 0)
    unsigned mine = 0;
    if (have > 0) {
      const uintptr_t a = (uintptr_t)bytes + (uintptr_t)(r * cols + c0), a0 = a & ~(uintptr_t)3, end = a + have;
      const unsigned d0 = *(const unsigned*)a0;
      const unsigned d1 = a0 + 4 < end ? *(const unsigned*)(a0 + 4) : 0u;
      const unsigned d2 = a0 + 8 < end ? *(const unsigned*)(a0 + 8) : 0u;
      const int sh = 8 * (int)(a & 3);
      uint64_t v = (uint64_t)d0 | (uint64_t)d1 << 32;
      if (sh) v = (v >> sh) | ((uint64_t)d2 << (64 - sh));
      if (have < 8) v &= (1ull << (8 * have)) - 1;
      mine = bits_of_bytes(v);
    }
    uint64_t x = (uint64_t)mine << (8 * k);
    x |= __shfl_xor(x, 1, 64);
    x |= __shfl_xor(x, 2, 64);
    x |= __shfl_xor(x, 4, 64);
    if (k == 0) bits[word] = (complement ? ~x : x) & smrf_bits_valid(cols, w);
  }
}

// Lane i makes the bytes of the cells 8 i .. 8 i + 7 of the flat plane, which may run over a row's end
__global__ __launch_bounds__(NT) void binary_unpack_kernel(const uint64_t* __restrict__ bits, unsigned char* __restrict__ bytes,
                                                           int cols, int W, long long cells, int complement) {
  const long long stride = (long long)gridDim.x * NT, groups = (cells + 7) >> 3;
  for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < groups; i += stride) {
    const long long f0 = 8 * i;
    long long r = f0 / cols;
    int c = (int)(f0 - r * cols);
    const int have = (int)min(8ll, cells - f0);
    uint64_t word = bits[r * W + (c >> 6)], v = 0;
    for (int j = 0; j < have; ++j) {
      v |= (word >> (c & 63) & 1) << (8 * j);
      if (++c == cols) {
        c = 0;
        ++r;
        if (j + 1 < have) word = bits[r * W];
      } else if ((c & 63) == 0 && j + 1 < have) {
        word = bits[r * W + (c >> 6)];
      }
    }
    if (complement) v ^= 0x0101010101010101ull;
    if (have == 8) {
      *(uint64_t*)(bytes + f0) = v;
    } else {
      for (int j = 0; j < have; ++j) bytes[f0 + j] = (unsigned char)(v >> (8 * j));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// the step
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void binary_step_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                         int rows, int cols, int W, const uint64_t* __restrict__ mask,
                                                         const int* __restrict__ table, int n, int op, int border,
                                                         const int* __restrict__ table2, int n2, int* __restrict__ changed) {
  const long long words = (long long)rows * W, stride = (long long)gridDim.x * NT;
  const auto load = [&](int row, int j) { return in[(long long)row * W + j]; };
  for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < words; i += stride) {
    const int r = (int)(i / W), w = (int)(i - (long long)r * W);
    bool diff;
    const uint64_t v = smrf_bits_step_word(load, rows, cols, r, w, table, n, op, border, table2, n2, mask != nullptr,
                                           mask ? mask[i] : 0ull, &diff);
    out[i] = v;
    if (changed) {
      const uint64_t who = __ballot(diff);
      if (diff && (int)(threadIdx.x & 63) == __builtin_ctzll(who)) atomicOr(changed, 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// propagation through the components of the mask
// ---------------------------------------------------------------------------------------------------------------
// Whether (dr, dc), each in -1 .. 1, is a member of the centrally symmetric 3 x 3 structure with its centre set that the
// link mask names: the centre, and both ends of every link.
__host__ __device__ inline bool link_member(int links, int dr, int dc) {
  if (dr < 0 || (dr == 0 && dc < 0)) dr = -dr, dc = -dc;            // the link's eastern or southern end
  return (dr == 0 && dc == 0) || (dr == 0 && dc == 1 && (links & SMRF_LABEL_E)) || (dr == 1 && dc == 0 && (links & SMRF_LABEL_S)) ||
         (dr == 1 && dc == 1 && (links & SMRF_LABEL_SE)) || (dr == 1 && dc == -1 && (links & SMRF_LABEL_SW));
}

// members of that structure: the centre and two per link
inline int link_members(int links) { return 1 + 2 * __builtin_popcount((unsigned)links & 15u); }

// One wave writes the structure's member table, (dr, dc) pairs sorted by dr, then dc: lane k < 9 stands for the cell
// (k / 3 - 1, k % 3 - 1) and a member's place is the number of members before it.  A symmetric structure is its own
// reflection, so the table serves dilation as it stands.
__global__ __launch_bounds__(64) void binary_link_table_kernel(int links, int* __restrict__ table) {
  const int k = threadIdx.x, dr = k / 3 - 1, dc = k % 3 - 1;
  const bool member = k < 9 && link_member(links, dr, dc);
  const uint64_t members = __ballot(member);
  if (member) {
    const int at = __popcll(members & ((1ull << k) - 1));
    table[2 * at] = dr;
    table[2 * at + 1] = dc;
  }
}

// flag[labels[i]] = 1 for every cell i of `seed & mask`: every writer stores the same value
__global__ __launch_bounds__(NT) void binary_mark_kernel(const uint64_t* __restrict__ seed, const uint64_t* __restrict__ mask,
                                                         const int* __restrict__ labels, unsigned char* __restrict__ flag,
                                                         int cols, int W, long long cells) {
  const long long stride = (long long)gridDim.x * NT;
  for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < cells; i += stride) {
    const long long r = i / cols;
    const int c = (int)(i - r * cols);
    const long long at = r * W + (c >> 6);
    if ((seed[at] & mask[at]) >> (c & 63) & 1) flag[labels[i]] = 1;
  }
}

// out[i] = mask[i] ? flag[labels[i]] : input[i], complemented for fill_holes; 4 cells of the flat plane per lane
__global__ __launch_bounds__(NT) void binary_select_kernel(const uint64_t* __restrict__ input, const uint64_t* __restrict__ mask,
                                                           const int* __restrict__ labels, const unsigned char* __restrict__ flag,
                                                           unsigned char* __restrict__ out, int cols, int W, long long cells,
                                                           int complement) {
  const long long stride = (long long)gridDim.x * NT, groups = (cells + 3) >> 2;
  for (long long i = blockIdx.x * (long long)NT + threadIdx.x; i < groups; i += stride) {
    const long long f0 = 4 * i;
    const int have = (int)min(4ll, cells - f0);
    long long r = f0 / cols;
    int c = (int)(f0 - r * cols);
    unsigned v = 0;
    for (int j = 0; j < have; ++j) {
      const long long at = r * W + (c >> 6);
      const unsigned bit = (mask[at] >> (c & 63) & 1) ? flag[labels[f0 + j]] : (unsigned)(input[at] >> (c & 63) & 1);
      v |= (bit ^ (unsigned)complement) << (8 * j);
      if (++c == cols) c = 0, ++r;
    }
    if (have == 4) {
      *(unsigned*)(out + f0) = v;
    } else {
      for (int j = 0; j < have; ++j) out[f0 + j] = (unsigned char)(v >> (8 * j));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
int check_plane(int rows, int cols, long long& cells) {
  if (int rc = smrf::check_size(rows, cols)) return rc;
  cells = (long long)rows * cols;
  if (cells >= (1ll << 31)) return smrf_fail(SMRF_E_UNSUPPORTED, "raster of %d x %d: cell indices are int32", rows, cols);
  return SMRF_OK;
}

inline size_t plane_bytes(int rows, int cols) { return smrf_up256((size_t)rows * smrf_bits_words(cols) * 8); }

struct PropWs {
  int* labels;
  char* label_ws;
  long long label_bytes;
  unsigned char* flag;
  uint64_t *input, *mask, *seed;
  int* count;      // the object count smrf_label_u8 writes; the member table of the structure lies 64 bytes on
  int* table;
};

// the labels plane, label's own workspace, the flag plane of cells + 1 bytes, three bit planes (input, mask, one step of
// the input) and 256 bytes for the object count smrf_label_u8 writes and the structure's member table, each part rounded
// up to 256 bytes
size_t prop_layout(int rows, int cols, long long cells, char* base, PropWs* w) {
  const long long lb = smrf_label_workspace_bytes(rows, cols);
  const size_t labels = smrf_up256((size_t)cells * 4), flag = smrf_up256((size_t)cells + 1), plane = plane_bytes(rows, cols);
  if (w) {
    char* p = base;
    w->labels = (int*)p, p += labels;
    w->label_ws = p, w->label_bytes = lb, p += lb;
    w->flag = (unsigned char*)p, p += flag;
    w->input = (uint64_t*)p, p += plane;
    w->mask = (uint64_t*)p, p += plane;
    w->seed = (uint64_t*)p, p += plane;
    w->count = (int*)p;
    w->table = (int*)(p + 64);
  }
  return labels + (size_t)lb + flag + 3 * plane + 256;
}

int launch_step(const uint64_t* in, uint64_t* out, int rows, int cols, const uint64_t* mask, const int* table, int n, int op,
                int border, const int* table2, int n2, int* changed, hipStream_t st) {
  const int W = smrf_bits_words(cols);
  hipLaunchKernelGGL(binary_step_kernel, dim3(smrf_blocks((long long)rows * W, GRID_CAP)), dim3(NT), 0, st, in, out, rows,
                     cols, W, mask, table, n, op, border, table2, n2, changed);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

int launch_pack(const unsigned char* bytes, uint64_t* bits, int rows, int cols, int complement, hipStream_t st) {
  const int W = smrf_bits_words(cols);
  const long long words = (long long)rows * W;
  hipLaunchKernelGGL(binary_pack_kernel, dim3(smrf_blocks(8 * words, GRID_CAP)), dim3(NT), 0, st, bytes, bits, cols, W, words,
                     complement);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // namespace

extern "C" {

int smrf_binary_offsets(const unsigned char* s, int srows, int scols, int origin_r, int origin_c, int reflect, int* out) {
  if (srows < 0 || scols < 0) return smrf_fail(SMRF_E_ARG, "negative size");
  if ((long long)srows * scols >= (1ll << 30)) return smrf_fail(SMRF_E_UNSUPPORTED, "structure of %d x %d", srows, scols);
  if (!s && (long long)srows * scols) return smrf_fail(SMRF_E_ARG, "null structure");
  const int n = smrf_bits_offsets(s, srows, scols, origin_r, origin_c, reflect, out);
  return n < 0 ? smrf_fail(SMRF_E_ARG, "origin (%d, %d) outside a structure of %d x %d", origin_r, origin_c, srows, scols) : n;
}

long long smrf_binary_plane_bytes(int rows, int cols) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  return 8ll * rows * smrf_bits_words(cols);
}

int smrf_binary_pack(const unsigned char* d_bytes, unsigned long long* d_bits, int rows, int cols, int complement,
                     void* stream) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  if (cells == 0) return SMRF_OK;
  if (!d_bytes || !d_bits) return smrf_fail(SMRF_E_ARG, "null pointer");
  return launch_pack(d_bytes, (uint64_t*)d_bits, rows, cols, complement != 0, (hipStream_t)stream);
}

int smrf_binary_unpack(const unsigned long long* d_bits, unsigned char* d_bytes, int rows, int cols, int complement,
                       void* stream) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  if (cells == 0) return SMRF_OK;
  if (!d_bytes || !d_bits) return smrf_fail(SMRF_E_ARG, "null pointer");
  if ((uintptr_t)d_bytes & 7) return smrf_fail(SMRF_E_ARG, "d_bytes is written in 8-byte stores and must be aligned to 8 bytes");
  hipLaunchKernelGGL(binary_unpack_kernel, dim3(smrf_blocks((cells + 7) >> 3, GRID_CAP)), dim3(NT), 0, (hipStream_t)stream,
                     (const uint64_t*)d_bits, d_bytes, cols, smrf_bits_words(cols), cells, complement != 0);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

int smrf_binary_step(const unsigned long long* d_in, unsigned long long* d_out, int rows, int cols,
                     const unsigned long long* d_mask, const int* d_table, int n, int op, int border, int* d_changed,
                     void* stream) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  if (n < 0) return smrf_fail(SMRF_E_ARG, "%d members", n);
  if (op != SMRF_BITS_AND && op != SMRF_BITS_OR) return smrf_fail(SMRF_E_ARG, "op %d", op);
  if (cells == 0) return SMRF_OK;
  if (!d_in || !d_out || (n && !d_table)) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (d_in == d_out) return smrf_fail(SMRF_E_ARG, "a step cannot run in place");
  return launch_step((const uint64_t*)d_in, (uint64_t*)d_out, rows, cols, (const uint64_t*)d_mask, d_table, n, op, border != 0,
                     nullptr, -1, d_changed, (hipStream_t)stream);
}

int smrf_binary_hit_or_miss(const unsigned long long* d_in, unsigned long long* d_out, int rows, int cols, const int* d_hit,
                            int n_hit, const int* d_miss, int n_miss, void* stream) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  if (n_hit < 0 || n_miss < 0) return smrf_fail(SMRF_E_ARG, "%d and %d members", n_hit, n_miss);
  if (cells == 0) return SMRF_OK;
  if (!d_in || !d_out || (n_hit && !d_hit) || (n_miss && !d_miss)) return smrf_fail(SMRF_E_ARG, "null pointer");
  if (d_in == d_out) return smrf_fail(SMRF_E_ARG, "a step cannot run in place");
  return launch_step((const uint64_t*)d_in, (uint64_t*)d_out, rows, cols, nullptr, d_hit, n_hit, SMRF_BITS_AND, 0, d_miss,
                     n_miss, nullptr, (hipStream_t)stream);
}

long long smrf_binary_propagate_workspace_bytes(int rows, int cols) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  return cells ? (long long)prop_layout(rows, cols, cells, nullptr, nullptr) : 0;
}

int smrf_binary_propagate(const unsigned char* d_input, const unsigned char* d_mask, unsigned char* d_out, int rows, int cols,
                          int links, int border, int complement, void* d_work, long long work_bytes, void* stream) {
  long long cells;
  if (int rc = check_plane(rows, cols, cells)) return rc;
  if (links < 0 || links > 15) return smrf_fail(SMRF_E_ARG, "link mask %d", links);
  if (cells == 0) return SMRF_OK;
  if (!d_mask || !d_out) return smrf_fail(SMRF_E_ARG, "null pointer");
  if ((uintptr_t)d_out & 3) return smrf_fail(SMRF_E_ARG, "d_out is written in dword stores and must be aligned to 4 bytes");
  const long long need = (long long)prop_layout(rows, cols, cells, nullptr, nullptr);
  if (!d_work || work_bytes < need)
    return smrf_fail(SMRF_E_WORKSPACE, "workspace of %lld bytes, %lld needed", work_bytes, need);
  if ((uintptr_t)d_work & 255) return smrf_fail(SMRF_E_ARG, "the workspace must be aligned to 256 bytes");
  const hipStream_t st = (hipStream_t)stream;
  PropWs w;
  prop_layout(rows, cols, cells, (char*)d_work, &w);
  const int W = smrf_bits_words(cols);
  hipLaunchKernelGGL(binary_link_table_kernel, dim3(1), dim3(64), 0, st, links, w.table);
  SMRF_LAUNCH_CHECK();
  if (d_input) {
    if (int rc = launch_pack(d_input, w.input, rows, cols, 0, st)) return rc;
  } else {
    SMRF_HIP_CHECK(hipMemsetAsync(w.input, 0, (size_t)rows * W * 8, st));
  }
  if (int rc = launch_pack(d_mask, w.mask, rows, cols, 0, st)) return rc;
  if (int rc = launch_step(w.input, w.seed, rows, cols, w.mask, w.table, link_members(links), SMRF_BITS_OR,
                           border != 0, nullptr, -1, nullptr, st))
    return rc;
  if (int rc = smrf_label_u8(d_mask, w.labels, rows, cols, links, w.label_ws, w.label_bytes, w.count, stream)) return rc;
  SMRF_HIP_CHECK(hipMemsetAsync(w.flag, 0, (size_t)cells + 1, st));
  hipLaunchKernelGGL(binary_mark_kernel, dim3(smrf_blocks(cells, GRID_CAP)), dim3(NT), 0, st, w.seed, w.mask, w.labels, w.flag,
                     cols, W, cells);
  SMRF_LAUNCH_CHECK();
  hipLaunchKernelGGL(binary_select_kernel, dim3(smrf_blocks((cells + 3) >> 2, GRID_CAP)), dim3(NT), 0, st, w.input, w.mask,
                     w.labels, w.flag, d_out, cols, W, cells, complement != 0);
  SMRF_LAUNCH_CHECK();
  return SMRF_OK;
}

}  // extern "C"
