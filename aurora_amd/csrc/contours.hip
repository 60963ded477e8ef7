// The closed-contour test of local extrema on the device (aurora_amd.closed_contours).  include/aurora_hip.h has the rule; the
// window and word arithmetic is contour_fill.h; this file has the one launch.  Everything is an integer.
//
// A 256-thread workgroup owns one (plane, candidate slot); a slot at or past min(count, max_points) writes its zero rows and
// exits.  The workgroup reads the candidate's row of the extrema table, the source rows of its disc and their half widths (the
// table of aurora_hip_smooth) and lays out the WINDOW of contour_fill.h: the disc's rows and columns and one ring of each
// around them, as rows of 64-bit words in LDS.  Per delta it
//   builds   three bitmaps -- A, passable member; X, passable non-member; R, reached = the candidate's own bit -- a wavefront
//            per word: a lane reads its point once (4-byte loads: no alignment rule), and two ballots are the words;
//   fills    R |= A & dilate(R), a thread per word of the member rows, in place, with the horizontal shortcut of
//            contour_run_fill, until a sweep changes no word;
//   counts   points = popcount(R), exits = popcount(R & (dilate(X) | the edge of a regional grid)), lanes, then waves through
//            LDS, and thread 0 stores the row.
// Plain stores, no atomics on global memory, no workspace; no workgroup waits for another.  LDS: 24 bytes per word of the
// largest window the caller announces, (max_rows + 2) x max_words words, at most kContourLdsBudget.
//
// Every trip count comes from the tables, and every table value is clamped into its row or plane before use; a window that
// does not fit what the caller announced is not filled (its rows are zero).
#include "planes.h"
#include "contour_fill.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxRows = 255;                                  // source rows of a target row
constexpr int kMaxLon = 4096;
constexpr int kMaxWords = kMaxLon / 64 + 1;                    // a regional window has the ring beside all columns
constexpr int kMaxPoints = 65536;
constexpr int kMaxDeltas = 8;
constexpr int kMinLdsBytes = 64;

struct ContourArgs {
  const float* const* planes;
  const int64_t* table;                                        // n_planes x max_points x 2: the table of aurora_hip_extrema
  const int32_t* count;                                        // n_planes
  const float* delta;                                          // n_planes x n_deltas, NaN: none
  int32_t* out;                                                // n_planes x n_deltas x max_points x 2
  const int32_t* row_lo;
  const int32_t* row_count;
  const int32_t* half;
  int n_lat, n_lon, n_deltas, max_points, max_rows, max_words, wrap, is_max, eight;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A word of the bitmap that other threads are writing during a sweep: relaxed, so every read sees a value that was stored.
__device__ __forceinline__ uint64_t peek(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void poke(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(kThreads) void closed_contours_kernel(const ContourArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds[];      // A, X, R: rows x words each
  __shared__ int s_half[kMaxRows + 2];                                // the half width of every local row, -1 for none
  __shared__ int s_part[kWaves][2];
  const int tid = (int)threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const int slot = (int)(blockIdx.x % (unsigned)a.max_points);
  const int64_t plane = (int64_t)(blockIdx.x / (unsigned)a.max_points);
  const int H = a.n_lat, W = a.n_lon, T = a.n_deltas;
  const bool wrap = a.wrap != 0, is_max = a.is_max != 0, eight = a.eight != 0;
  const gptr<int32_t> out = (gptr<int32_t>)a.out + (plane * T * a.max_points + slot) * 2;   // + t max_points 2
  const int64_t t_stride = 2 * (int64_t)a.max_points;

  // (workgroup-uniform from here to the loop over the deltas: the candidate, its rows, its window)
  const int live = clampi(((gptr<const int32_t>)a.count)[plane], 0, a.max_points);
  bool fill = slot < live;
  int p0 = 0, i0 = 0, j0 = 0, k_lo = 0, cnt = 0;
  if (fill) {
    const int64_t raw = ((gptr<const int64_t>)a.table)[(plane * a.max_points + slot) * 2];
    const int64_t most = (int64_t)H * W - 1;
    p0 = (int)(raw < 0 ? 0 : (raw > most ? most : raw));
    i0 = p0 / W, j0 = p0 - i0 * W;
    k_lo = clampi(a.row_lo[i0], 0, H - 1);
    cnt = clampi(a.row_count[i0], 0, min(a.max_rows, H - k_lo));
    fill = i0 >= k_lo && i0 < k_lo + cnt;                       // (a table of `disc_table` always holds the row itself)
  }
  if (!fill) {
    if (tid < T) out[tid * t_stride] = 0, out[tid * t_stride + 1] = 0;
    return;
  }
  const int rows = cnt + 2;
  int n_max = -1;
  for (int r = tid; r < rows; r += kThreads) {
    int n = -1;
    if (r >= 1 && r <= cnt) {
      n = clampi(a.half[(int64_t)i0 * a.max_rows + r - 1], -1, W);
      if (k_lo + r - 1 == i0) n = max(n, 0);                    // a point is a member of its own disc
    }
    s_half[r] = n;
    n_max = max(n_max, n);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_max = max(n_max, __shfl_xor(n_max, o, kWave));
  if (lane == 0) s_part[wave][0] = n_max;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kWaves; ++k) n_max = max(n_max, s_part[k][0]);
  ContourWindow q = contour_window(j0, n_max, W, wrap);           // (n_max >= 0: the candidate's own row)
  q.rows = rows;
  if (q.words > a.max_words) {                                    // more than the caller announced: not filled
    if (tid < T) out[tid * t_stride] = 0, out[tid * t_stride + 1] = 0;
    return;
  }
  const int words = q.words, n_items = rows * words;
  uint64_t* const A = lds;
  uint64_t* const X = lds + n_items;
  uint64_t* const R = lds + 2 * n_items;
  const int seed_row = i0 - k_lo + 1, seed_col = q.cyclic ? j0 : j0 - q.first;
  const gptr<const float> x = (gptr<const float>)a.planes[plane];
  const double v0 = (double)x[p0];
  const auto reached = [R, words](int r, int w) { return peek(R + r * words + w); };
  const auto outside = [X, words](int r, int w) { return X[r * words + w]; };

  for (int t = 0; t < T; ++t) {
    const float delta = ((gptr<const float>)a.delta)[plane * T + t];
    if (!(delta > 0.0f)) {                                        // a padded delta: a zero row
      if (tid == 0) out[t * t_stride] = 0, out[t * t_stride + 1] = 0;
      continue;
    }
    const double dd = (double)delta;
    __syncthreads();                                              // the bitmaps and s_part of the delta before are read

    // build: a wavefront per word, a lane per point
    for (int item = wave; item < n_items; item += kWaves) {       // wave-uniform
      const int r = item / words, w = item - r * words;
      const int l = 64 * w + lane, k = k_lo - 1 + r;
      const int c = contour_column(q, l, W, wrap);
      bool pass = false, member = false;
      if (k >= 0 && k < H && c >= 0) {
        const float v = x[(int64_t)k * W + c];
        const double rise = is_max ? v0 - (double)v : (double)v - v0;
        pass = !__builtin_isfinite(v) || rise < dd;
        member = contour_is_member(q, l, j0, s_half[r], W);
      }
      const uint64_t am = __ballot(pass && member), xm = __ballot(pass && !member);
      if (lane == 0) {
        A[item] = am, X[item] = xm;
        R[item] = (r == seed_row && w == (seed_col >> 6)) ? am & (1ull << (seed_col & 63)) : 0;
      }
    }
    __syncthreads();

    // fill.  TERMINATION: a sweep either adds at least one bit to R or is the last; R only grows and stays inside A, so there
    // are at most |members| + 1 sweeps.  A word is written by its own thread alone; a neighbour's word is read as it was before
    // or after that thread's store of this sweep, and either is a subset of the fill, so the fixed point -- the smallest set
    // that holds the candidate and every passable member next to it -- does not depend on the order.  The barrier is the
    // workgroup's own: no workgroup waits for another.
    for (;;) {
      int changed = 0;
      for (int item = words + tid; item < n_items - words; item += kThreads) {
        const uint64_t am = A[item], old = peek(R + item);
        if (am == old) continue;                                  // nothing left to reach in this word
        const int r = item / words, w = item - r * words;
        const uint64_t now = contour_reach(reached, am, r, w, q, eight);
        if (now != old) {
          poke(R + item, now);
          changed = 1;
        }
      }
      if (!__syncthreads_or(changed)) break;
    }

    // count
    int points = 0, exits = 0;
    for (int item = words + tid; item < n_items - words; item += kThreads) {
      const uint64_t f = R[item];
      if (f == 0) continue;
      const int r = item / words, w = item - r * words;
      uint64_t open = contour_dilate(outside, r, w, q, eight);
      if (!wrap) {
        const int k = k_lo - 1 + r;
        open |= contour_edge(q, w, k == 0 || k == H - 1, W);
      }
      points += __popcll(f);
      exits += __popcll(f & open);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) points += __shfl_xor(points, o, kWave), exits += __shfl_xor(exits, o, kWave);
    if (lane == 0) s_part[wave][0] = points, s_part[wave][1] = exits;
    __syncthreads();
    if (tid == 0) {
      points = 0, exits = 0;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) points += s_part[k][0], exits += s_part[k][1];
      out[t * t_stride] = points, out[t * t_stride + 1] = exits;
    }
  }
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_closed_contours(const float* const* planes, const int64_t* table, const int32_t* count,
                                          const float* delta, int32_t* out, int n_planes, int n_lat, int n_lon, int n_deltas,
                                          int max_points, const int32_t* row_lo, const int32_t* row_count, const int32_t* half,
                                          int max_rows, int max_words, int wrap, int is_max, int connectivity, void* stream) {
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1 && n_lon >= 1, "closed_contours: bad sizes (planes %d, grid %d x %d)", n_planes, n_lat,
                   n_lon);
  AURORA_CHECK_ARG(n_lon <= kMaxLon, "closed_contours: the grid has %d longitudes; 1 to %d are supported", n_lon, kMaxLon);
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= 0x7fffffffll, "closed_contours: a plane of %d x %d points is too large", n_lat, n_lon);
  AURORA_CHECK_ARG(n_deltas >= 1 && n_deltas <= kMaxDeltas, "closed_contours: 1 to %d deltas, got %d", kMaxDeltas, n_deltas);
  AURORA_CHECK_ARG(max_points >= 1 && max_points <= kMaxPoints, "closed_contours: max_points must be in 1..%d, got %d", kMaxPoints,
                   max_points);
  AURORA_CHECK_ARG(max_rows >= 1 && max_rows <= kMaxRows, "closed_contours: 1 to %d source rows per target row, got %d", kMaxRows,
                   max_rows);
  AURORA_CHECK_ARG(max_words >= 1 && max_words <= kMaxWords, "closed_contours: 1 to %d words per window row, got %d", kMaxWords,
                   max_words);
  AURORA_CHECK_ARG((wrap == 0 || wrap == 1) && (is_max == 0 || is_max == 1),
                   "closed_contours: the flags wrap and is_max must be 0 or 1, got %d and %d", wrap, is_max);
  AURORA_CHECK_ARG(connectivity == 4 || connectivity == 8, "closed_contours: connectivity must be 4 or 8, got %d", connectivity);
  const int64_t lds_need = contour_lds_bytes(max_rows, max_words);
  AURORA_CHECK_ARG(lds_need <= kContourLdsBudget,
                   "closed_contours: windows of %d rows x %d words of 64 columns need %lld bytes of LDS in three bitmaps; the "
                   "budget is %d bytes", max_rows + 2, max_words, (long long)lds_need, kContourLdsBudget);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(planes && table && count && delta && out && row_lo && row_count && half,
                   "closed_contours: null plane array, table, count, delta, output or disc table pointer");
  AURORA_CHECK_ARG(((uintptr_t)table & 7) == 0 && (((uintptr_t)count | (uintptr_t)delta | (uintptr_t)out | (uintptr_t)row_lo |
                                                    (uintptr_t)row_count | (uintptr_t)half) & 3) == 0,
                   "closed_contours: table must be 8-byte aligned, count, delta, out, row_lo, row_count and half 4-byte aligned");
  AURORA_CHECK_ARG((int64_t)n_planes * max_points <= 0x7fffffffll,
                   "closed_contours: too many planes for one launch (%d planes of %d table rows)", n_planes, max_points);
  {
    // the dynamic LDS limit, raised once per device; a failure is reported, not left to a later launch error
    static bool raised[64] = {false};
    bool& done = raised[current_device() & 63];
    if (!done) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&closed_contours_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, kContourLdsBudget);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("closed_contours: the device refused %d bytes of dynamic LDS per workgroup: %s", kContourLdsBudget,
                  hipGetErrorString(e));
        return AURORA_E_LAUNCH;
      }
      done = true;
    }
  }
  ContourArgs c;
  c.planes = planes, c.table = table, c.count = count, c.delta = delta, c.out = out, c.row_lo = row_lo, c.row_count = row_count;
  c.half = half, c.n_lat = n_lat, c.n_lon = n_lon, c.n_deltas = n_deltas, c.max_points = max_points, c.max_rows = max_rows;
  c.max_words = max_words, c.wrap = wrap, c.is_max = is_max, c.eight = connectivity == 8 ? 1 : 0;
  const size_t lds_bytes = (size_t)lds_need > (size_t)kMinLdsBytes ? (size_t)lds_need : (size_t)kMinLdsBytes;
  hipLaunchKernelGGL(closed_contours_kernel, dim3((unsigned)((int64_t)n_planes * max_points)), dim3(kThreads), lds_bytes,
                     as_stream(stream), c);
  return check_launch("closed_contours");
}
