// Per-label measurements of a 2-D raster: scipy.ndimage's sum_labels, mean, variance, minimum, maximum and the two
// positions, for every label of an int32 plane at once.  Host side: neilpy_amd/measure.py; C ABI: include/smrf_measure.h;
// contract, error bound and byte model: DESIGN.md section 22.
//
// The table of a call lies in the workspace, one entry per label 0..n.  Launches, each on the caller's stream, the kernel
// boundary the only synchronisation:
//
//   clear      the table's start values.
//   pass 1     per label: the cell count, the least and the largest order-preserving key (float_key.h, NaN last), the
//              largest finite magnitude M as an unsigned maximum on the bits, the flags NaN / +inf / -inf.
//   pass 2     reads M, hence E, and the extreme keys: adds the three fixed-point pieces (measure_fixed.h) of every finite
//              value to the label's accumulators, and lowers the label's two positions to the index of every cell that
//              holds an extreme key.  Runs only for sums, moments and positions.
//   finalize   over labels: rounds the accumulators' total once (the sum), divides (the mean), turns keys back into values
//              and writes the results asked for.
//   pass 3     only for the variance: the same accumulation for d * d, d = x - mean, under the exponent 2 E + 3.
//   variance   over labels: rounds that total and divides by the count.
//
// Integer atomics only.  A wave takes 64 consecutive cells, and what goes to memory is one set of atomics per stretch of
// equal labels within the wave: the stretch's values are combined by a segmented shuffle reduction first (a raster that is
// one object sends one set per 64 cells, not per cell).  A minimum or maximum is sent only where a plain load of the entry
// shows that it would still change it; entries move one way only, so a stale load lets a needless atomic through and never
// holds a needed one back.  Sums of integers and extrema of integers do not depend on the order in which they land.
#include <climits>

#include "float_key.h"
#include "measure_fixed.h"
#include "raster_stencil.h"
#include "smrf_measure.h"

namespace {

constexpr int NT = 256;
constexpr int FLAG_INF_TERM = 8;          // pass 3: a squared difference overflowed (kept out of the flags handed out)
using u64 = unsigned long long;
using i64 = long long;

struct Table {
  u64* count;
  u64* min_key;
  u64* max_key;
  u64* abs_max;
  unsigned* flags;
  i64* acc;        // 3 per label
  double* mean;
  u64* index;      // 2 per label: min, max
  i64* acc2;       // 3 per label
};

constexpr int WANT_SUMS = SMRF_MEASURE_SUM | SMRF_MEASURE_MEAN | SMRF_MEASURE_VARIANCE;
constexpr int WANT_INDEX = SMRF_MEASURE_MIN_INDEX | SMRF_MEASURE_MAX_INDEX;

size_t table_layout(long long n, int what, char* base, Table* t) {
  const size_t L = (size_t)n + 1;
  size_t at = 0;
  const auto take = [&](size_t bytes) {
    char* p = base ? base + at : nullptr;
    at += smrf_up256(bytes);
    return p;
  };
  Table w{};
  w.count = (u64*)take(8 * L);
  w.min_key = (u64*)take(8 * L);
  w.max_key = (u64*)take(8 * L);
  w.abs_max = (u64*)take(8 * L);
  w.flags = (unsigned*)take(4 * L);
  if (what & WANT_SUMS) {
    w.acc = (i64*)take(24 * L);
    w.mean = (double*)take(8 * L);
  }
  if (what & WANT_INDEX) w.index = (u64*)take(16 * L);
  if (what & SMRF_MEASURE_VARIANCE) w.acc2 = (i64*)take(24 * L);
  if (t) *t = w;
  return at;
}

__global__ __launch_bounds__(NT) void measure_clear_kernel(Table t, long long n) {
  for (long long k = blockIdx.x * (long long)NT + threadIdx.x; k <= n; k += (long long)gridDim.x * NT) {
    t.count[k] = 0;
    t.min_key[k] = ~0ull;
    t.max_key[k] = 0;
    t.abs_max[k] = 0;
    t.flags[k] = 0;
    if (t.acc) t.acc[3 * k] = t.acc[3 * k + 1] = t.acc[3 * k + 2] = 0;
    if (t.index) t.index[2 * k] = t.index[2 * k + 1] = ~0ull;
    if (t.acc2) t.acc2[3 * k] = t.acc2[3 * k + 1] = t.acc2[3 * k + 2] = 0;
  }
}

// the label of cell i, -1 for a cell that is ignored
__device__ __forceinline__ int label_of(const int* __restrict__ L, long long i, int mode, int n) {
  if (!L) return 1 <= n ? 1 : -1;
  int v = L[i];
  if (mode == SMRF_MEASURE_LABELS_POSITIVE) v = v > 0;
  return v < 0 || v > n ? -1 : v;
}

// The stretches of equal labels among the 64 lanes: `end` = the last lane of this lane's stretch, `head` = this lane is
// its first.
__device__ __forceinline__ void stretch_of(int v, int lane, int& end, bool& head) {
  const int left = __shfl_up(v, 1, 64);
  head = lane == 0 || left != v;
  const uint64_t firsts = __ballot(head);
  const uint64_t later = lane == 63 ? 0 : firsts >> (lane + 1);
  end = later ? lane + __builtin_ctzll(later) : 63;
}

// op over the lanes lane .. end of a stretch: after the step of offset o a lane holds op over min(2 o, what is left of its
// stretch) lanes, so a head ends with its whole stretch.  lane + o <= end <= 63 keeps every source inside the wave.
template <typename V, typename Op>
__device__ __forceinline__ V stretch_reduce(V v, int lane, int end, Op op) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V other = __shfl_down(v, o, 64);
    if (lane + o <= end) v = op(v, other);
  }
  return v;
}

__device__ __forceinline__ u64 peek(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lower(u64* p, u64 v) {
  if (v < peek(p)) atomicMin(p, v);
}
__device__ __forceinline__ void raise(u64* p, u64 v) {
  if (v > peek(p)) atomicMax(p, v);
}

template <typename T>
__global__ __launch_bounds__(NT) void measure_pass1_kernel(const T* __restrict__ X, const int* __restrict__ L, long long cells,
                                                           int n, int mode, Table t) {
  const int lane = threadIdx.x & 63;
  const long long span = (long long)gridDim.x * NT;
  for (long long base = blockIdx.x * (long long)NT + (threadIdx.x - lane); base < cells; base += span) {
    const long long i = base + lane;
    const bool in = i < cells;
    const int v = in ? label_of(L, i, mode, n) : -1;
    const double x = in ? (double)X[i] : 0.0;
    int end;
    bool head;
    stretch_of(v, lane, end, head);
    const u64 abs_bits = smrf_f64_bits(x) & ~SMRF_F64_SIGN;
    const bool nan = abs_bits > SMRF_F64_EXP, inf = abs_bits == SMRF_F64_EXP;
    const u64 key = smrf_key(x, true);
    const u64 lo = stretch_reduce(key, lane, end, [](u64 a, u64 b) { return a < b ? a : b; });
    const u64 hi = stretch_reduce(key, lane, end, [](u64 a, u64 b) { return a > b ? a : b; });
    const u64 mag = stretch_reduce((u64)(nan || inf ? 0 : abs_bits), lane, end, [](u64 a, u64 b) { return a > b ? a : b; });
    const unsigned own = nan ? SMRF_MEASURE_HAS_NAN : !inf ? 0 : x > 0 ? SMRF_MEASURE_HAS_POS_INF : SMRF_MEASURE_HAS_NEG_INF;
    const unsigned fl = stretch_reduce(own, lane, end, [](unsigned a, unsigned b) { return a | b; });
    if (head && v >= 0) {
      atomicAdd(&t.count[v], (u64)(end - lane + 1));
      lower(&t.min_key[v], lo);
      raise(&t.max_key[v], hi);
      if (mag) raise(&t.abs_max[v], mag);
      if (fl & ~__hip_atomic_load(&t.flags[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&t.flags[v], fl);
    }
  }
}

// Adds the pieces of the stretches' terms to acc.  `term(x, v, ok)` gives the lane's term, ok = false for none; the terms
// lie below 2^(e_scale E + e_shift) for the E of the label's largest finite magnitude.
template <typename Term>
__device__ __forceinline__ void add_pieces(i64* __restrict__ acc, const u64* __restrict__ abs_max, int v, int lane, int end,
                                           bool head, int e_scale, int e_shift, double x, bool finite, Term term) {
  int64_t p[3] = {0, 0, 0};
  if (v >= 0 && finite) {
    const u64 m = abs_max[v];
    if (m) {
      const int E = e_scale * smrf_fixed_exponent(m) + e_shift;
      bool ok = true;
      const double tv = term(x, v, ok);
      if (ok) smrf_fixed_split(tv, E, p);
    }
  }
  const auto add = [](i64 a, i64 b) { return a + b; };
  const i64 s0 = stretch_reduce((i64)p[0], lane, end, add), s1 = stretch_reduce((i64)p[1], lane, end, add),
            s2 = stretch_reduce((i64)p[2], lane, end, add);
  if (head && v >= 0) {
    u64* a = (u64*)acc + 3 * (long long)v;                  // two's complement: an unsigned add is the signed one
    if (s0) atomicAdd(&a[0], (u64)s0);
    if (s1) atomicAdd(&a[1], (u64)s1);
    if (s2) atomicAdd(&a[2], (u64)s2);
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void measure_pass2_kernel(const T* __restrict__ X, const int* __restrict__ L, long long cells,
                                                           int n, int mode, Table t) {
  const int lane = threadIdx.x & 63;
  const long long span = (long long)gridDim.x * NT;
  for (long long base = blockIdx.x * (long long)NT + (threadIdx.x - lane); base < cells; base += span) {
    const long long i = base + lane;
    const bool in = i < cells;
    const int v = in ? label_of(L, i, mode, n) : -1;
    const double x = in ? (double)X[i] : 0.0;
    int end;
    bool head;
    stretch_of(v, lane, end, head);
    if (t.acc) {
      const bool finite = (smrf_f64_bits(x) & ~SMRF_F64_SIGN) < SMRF_F64_EXP;
      add_pieces(t.acc, t.abs_max, v, lane, end, head, 1, 0, x, finite, [](double xv, int, bool&) { return xv; });
    }
    if (t.index) {
      const u64 key = smrf_key(x, true);
      const auto least = [](int a, int b) { return a < b ? a : b; };
      const int at_min = stretch_reduce(v >= 0 && key == t.min_key[v] ? lane : 64, lane, end, least);
      const int at_max = stretch_reduce(v >= 0 && key == t.max_key[v] ? lane : 64, lane, end, least);
      if (head && v >= 0) {
        if (at_min < 64) lower(&t.index[2 * (long long)v], (u64)(base + at_min));
        if (at_max < 64) lower(&t.index[2 * (long long)v + 1], (u64)(base + at_max));
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void measure_pass3_kernel(const T* __restrict__ X, const int* __restrict__ L, long long cells,
                                                           int n, int mode, Table t) {
  const int lane = threadIdx.x & 63;
  const long long span = (long long)gridDim.x * NT;
  for (long long base = blockIdx.x * (long long)NT + (threadIdx.x - lane); base < cells; base += span) {
    const long long i = base + lane;
    const bool in = i < cells;
    const int v = in ? label_of(L, i, mode, n) : -1;
    const double x = in ? (double)X[i] : 0.0;
    int end;
    bool head;
    stretch_of(v, lane, end, head);
    // a label with a NaN or an infinity has the variance NaN whatever is added here: its cells add nothing
    const bool finite = v >= 0 && (t.flags[v] & 7) == 0;
    add_pieces(t.acc2, t.abs_max, v, lane, end, head, 2, 3, x, finite, [&](double xv, int lv, bool& ok) {
      const double d = xv - t.mean[lv];
      const double sq = d * d;
      if ((smrf_f64_bits(sq) & ~SMRF_F64_SIGN) >= SMRF_F64_EXP) {       // overflow, or the mean is an infinity: +inf
        ok = false;
        if (!(__hip_atomic_load(&t.flags[lv], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & FLAG_INF_TERM))
          atomicOr(&t.flags[lv], (unsigned)FLAG_INF_TERM);
      }
      return sq;
    });
  }
}

template <typename T>
struct Results {
  long long* count;
  double* sum;
  double* mean;
  double* variance;
  T* min;
  T* max;
  long long* min_index;
  long long* max_index;
  int* flags;
};

__device__ __forceinline__ double quiet_nan() { return smrf_f64_of(SmrfKey<double>::quiet_nan); }

// the sum of a label's values from its flags and accumulators
__device__ __forceinline__ double sum_of(unsigned fl, u64 abs_max, const i64* acc) {
  if ((fl & SMRF_MEASURE_HAS_NAN) || (fl & 6) == 6) return quiet_nan();
  if (fl & SMRF_MEASURE_HAS_POS_INF) return smrf_f64_of(SMRF_F64_EXP);
  if (fl & SMRF_MEASURE_HAS_NEG_INF) return smrf_f64_of(SMRF_F64_EXP | SMRF_F64_SIGN);
  if (!abs_max) return 0.0;
  const int64_t a[3] = {acc[0], acc[1], acc[2]};
  return smrf_fixed_round(smrf_fixed_total(a), smrf_fixed_exponent(abs_max) - SMRF_FIXED_BITS);
}

template <typename T>
__global__ __launch_bounds__(NT) void measure_finalize_kernel(Table t, long long n, int what, Results<T> r) {
  for (long long k = blockIdx.x * (long long)NT + threadIdx.x; k <= n; k += (long long)gridDim.x * NT) {
    const u64 count = t.count[k];
    const unsigned fl = t.flags[k];
    if (what & SMRF_MEASURE_COUNT) r.count[k] = (long long)count;
    if (what & SMRF_MEASURE_FLAGS) r.flags[k] = (int)(fl & 7);
    if (what & SMRF_MEASURE_MIN) r.min[k] = count ? (T)smrf_unkey<double>(t.min_key[k]) : (T)0;
    if (what & SMRF_MEASURE_MAX) r.max[k] = count ? (T)smrf_unkey<double>(t.max_key[k]) : (T)0;
    if (what & SMRF_MEASURE_MIN_INDEX) r.min_index[k] = (long long)t.index[2 * k];           // all ones: -1
    if (what & SMRF_MEASURE_MAX_INDEX) r.max_index[k] = (long long)t.index[2 * k + 1];
    if (what & WANT_SUMS) {
      const double sum = sum_of(fl, t.abs_max[k], t.acc + 3 * k);
      const double mean = sum / (double)count;                       // 0 / 0: NaN for a label that does not occur
      t.mean[k] = mean;
      if (what & SMRF_MEASURE_SUM) r.sum[k] = sum;
      if (what & SMRF_MEASURE_MEAN) r.mean[k] = mean;
    }
  }
}

__global__ __launch_bounds__(NT) void measure_variance_kernel(Table t, long long n, double* __restrict__ variance) {
  for (long long k = blockIdx.x * (long long)NT + threadIdx.x; k <= n; k += (long long)gridDim.x * NT) {
    const u64 count = t.count[k], m = t.abs_max[k];
    const unsigned fl = t.flags[k];
    double total;
    if (fl & 7) {
      total = quiet_nan();
    } else if (fl & FLAG_INF_TERM) {
      total = smrf_f64_of(SMRF_F64_EXP);
    } else if (!m) {
      total = 0.0;
    } else {
      const int64_t a[3] = {t.acc2[3 * k], t.acc2[3 * k + 1], t.acc2[3 * k + 2]};
      total = smrf_fixed_round(smrf_fixed_total(a), 2 * smrf_fixed_exponent(m) + 3 - SMRF_FIXED_BITS);
    }
    variance[k] = total / (double)count;
  }
}

int check_what(int what) {
  return (what <= 0 || (what & ~SMRF_MEASURE_ALL)) ? smrf_fail(SMRF_E_ARG, "measurement mask %d", what) : SMRF_OK;
}

template <typename T>
int measure(const T* d_x, const int* d_labels, int rows, int cols, int n, int mode, int what, const smrf_measure_out* out,
            void* d_work, long long work_bytes, void* stream) {
  if (int rc = smrf::check_size(rows, cols)) return rc;
  const long long cells = (long long)rows * cols;
  if (cells >= (1ll << 31)) return smrf_fail(SMRF_E_UNSUPPORTED, "raster of %d x %d: cell indices are int32", rows, cols);
  if (n < 0 || n == INT_MAX) return smrf_fail(n < 0 ? SMRF_E_ARG : SMRF_E_UNSUPPORTED, "%d labels", n);
  if (mode != SMRF_MEASURE_LABELS_AS_GIVEN && mode != SMRF_MEASURE_LABELS_POSITIVE) return smrf_fail(SMRF_E_ARG, "label mode %d", mode);
  if (int rc = check_what(what)) return rc;
  if (!out) return smrf_fail(SMRF_E_ARG, "null output");
  const void* const wanted[9] = {out->count, out->sum, out->mean, out->variance, out->min, out->max, out->min_index,
                                 out->max_index, out->flags};
  for (int b = 0; b < 9; ++b)
    if ((what >> b & 1) && !wanted[b]) return smrf_fail(SMRF_E_ARG, "null output for measurement %d", 1 << b);
  if (cells && !d_x) return smrf_fail(SMRF_E_ARG, "null raster");
  const long long need = (long long)table_layout(n, what, nullptr, nullptr);
  if (!d_work || work_bytes < need) return smrf_fail(SMRF_E_WORKSPACE, "workspace of %lld bytes, %lld needed", work_bytes, need);
  Table t;
  table_layout(n, what, (char*)d_work, &t);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 over_labels(smrf_blocks((long long)n + 1, 1 << 16)), over_cells(smrf_blocks(cells, 8192)), nt(NT);
  hipLaunchKernelGGL(measure_clear_kernel, over_labels, nt, 0, st, t, (long long)n);
  SMRF_LAUNCH_CHECK();
  if (cells) {
    hipLaunchKernelGGL(measure_pass1_kernel<T>, over_cells, nt, 0, st, d_x, d_labels, cells, n, mode, t);
    SMRF_LAUNCH_CHECK();
    if (what & (WANT_SUMS | WANT_INDEX)) {
      hipLaunchKernelGGL(measure_pass2_kernel<T>, over_cells, nt, 0, st, d_x, d_labels, cells, n, mode, t);
      SMRF_LAUNCH_CHECK();
    }
  }
  const Results<T> r{out->count, out->sum, out->mean, out->variance, (T*)out->min, (T*)out->max, out->min_index,
                     out->max_index, out->flags};
  hipLaunchKernelGGL(measure_finalize_kernel<T>, over_labels, nt, 0, st, t, (long long)n, what, r);
  SMRF_LAUNCH_CHECK();
  if (what & SMRF_MEASURE_VARIANCE) {
    if (cells) {
      hipLaunchKernelGGL(measure_pass3_kernel<T>, over_cells, nt, 0, st, d_x, d_labels, cells, n, mode, t);
      SMRF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(measure_variance_kernel, over_labels, nt, 0, st, t, (long long)n, out->variance);
    SMRF_LAUNCH_CHECK();
  }
  return SMRF_OK;
}

}  // namespace

extern "C" {

long long smrf_measure_workspace_bytes(long long n, int what) {
  if (n < 0) return smrf_fail(SMRF_E_ARG, "%lld labels", n);
  if (int rc = check_what(what)) return rc;
  if (n >= INT_MAX) return smrf_fail(SMRF_E_UNSUPPORTED, "%lld labels", n);
  return (long long)table_layout(n, what, nullptr, nullptr);
}

int smrf_measure_f32(const float* d_x, const int* d_labels, int rows, int cols, int n, int mode, int what,
                     const smrf_measure_out* out, void* d_work, long long work_bytes, void* stream) {
  return measure<float>(d_x, d_labels, rows, cols, n, mode, what, out, d_work, work_bytes, stream);
}

int smrf_measure_f64(const double* d_x, const int* d_labels, int rows, int cols, int n, int mode, int what,
                     const smrf_measure_out* out, void* d_work, long long work_bytes, void* stream) {
  return measure<double>(d_x, d_labels, rows, cols, n, mode, what, out, d_work, work_bytes, stream);
}

}  // extern "C"
