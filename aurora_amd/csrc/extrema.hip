// Local extrema over a great-circle disc on the device (aurora_amd.extrema).  include/aurora_hip.h has the rule; the window
// arithmetic is extrema_window.h; this file has the four launches.  Everything is an integer or a copied fp32: a point's
// COMPOSITE is (key << 32) | flat index as a uint64, all ones where the point is not finite, and every stage takes minima.
//
// Row extremes.  A WAVEFRONT owns one row of one plane and folds its composites by an xor butterfly into the workspace: what a
// window that is the whole row reads (the discs near a pole).
//
// Filter.  A 256-thread workgroup owns kFilterRows adjacent target rows and ALL columns of the plane; a thread owns the columns
// tid, tid + 256, ... (CPT of them, a template argument, so that the running minima are registers).  It takes every source row k
// of the union of the target rows' tables in ascending order: a target row whose window is the whole row folds the row's
// extreme; if any other target row reaches k, the row's composites are staged in LDS (4-byte loads: no alignment rule) and the
// DOUBLING levels m[l + 1][c] = min(m[l][c], m[l][c + 2^l]) are built between two LDS buffers, level l in buffer l & 1; the
// target row with floor(log2(2 n + 1)) = l is answered at step l with two LDS reads per column.  The work per (point, source
// row) is therefore O(log n / kFilterRows), not O(n).  LDS: 16 bytes per column, 64 KiB at n_lon = 4096.  It stores index and
// filtered, and the number of extrema of each of its target rows.  Plain stores, no atomics.
//
// Scan.  A workgroup per plane: its first wave turns the row counts into exclusive row bases and the plane's count (a fixed
// shuffle tree per 64 rows, the running sum carried), then all waves zero the table rows past min(count, max_points).
//
// Number.  A wavefront per row finds its extrema in the index map by ballot, 64 columns at a time, and writes table row
// base + rank for the ranks below max_points.
//
// Every trip count comes from the tables, and every table value is clamped into its row or plane before use.
#include "planes.h"
#include "extrema_window.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kFilterRows = 4;                                 // target rows of a filter workgroup
constexpr int kMaxRows = 255;                                  // source rows of a target row
constexpr int kMaxLon = 4096;
constexpr int kMaxPoints = 65536;
constexpr int kMinLdsBytes = 256;                              // the counts of the waves go through LDS at the end
constexpr uint64_t kNone = ~(uint64_t)0;

// K(v) of the rule (`is_max`: ~K): ascending with v, -0 below +0.
__device__ __forceinline__ uint32_t value_key(float v, bool is_max) {
  const uint32_t u = __float_as_uint(v);
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return is_max ? ~k : k;
}
__device__ __forceinline__ float key_value(uint32_t key, bool is_max) {
  const uint32_t k = is_max ? ~key : key;
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ uint64_t composite(float v, uint32_t flat, bool is_max) {
  return __builtin_isfinite(v) ? ((uint64_t)value_key(v, is_max) << 32) | flat : kNone;
}
__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return b < a ? b : a; }

struct RowArgs {
  const float* const* planes;
  uint64_t* row_ext;
  int64_t n_rows;                                              // n_planes x n_lat
  int n_lat, n_lon, is_max;
};
struct FilterArgs {
  const float* const* planes;
  int32_t* index;                                              // n_planes x n_lat x n_lon
  float* filtered;
  const uint64_t* row_ext;
  int32_t* row_cnt;
  const int32_t* row_lo;
  const int32_t* row_count;
  const int32_t* half;
  int n_lat, n_lon, max_rows, n_row_blocks, wrap, is_max;
};
struct ScanArgs {
  const int32_t* row_cnt;
  int32_t* row_base;
  int32_t* count;
  int64_t* table;
  int n_lat, max_points;
};
struct NumberArgs {
  const int32_t* index;
  const float* filtered;
  const int32_t* row_base;
  int64_t* table;
  int64_t n_rows;
  int n_lat, n_lon, max_points;
};

__global__ __launch_bounds__(kThreads) void extrema_rows_kernel(const RowArgs a) {
  const int wave = (int)threadIdx.x / kWave, lane = (int)threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kWaves + wave;    // wave-uniform
  if (row >= a.n_rows) return;
  const int64_t plane = row / a.n_lat;
  const int i = (int)(row - plane * a.n_lat);
  const int W = a.n_lon;
  const gptr<const float> src = (gptr<const float>)a.planes[plane] + (int64_t)i * W;
  uint64_t m = kNone;
  for (int c = lane; c < W; c += kWave) m = min_u64(m, composite(src[c], (uint32_t)(i * W + c), a.is_max != 0));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = min_u64(m, (uint64_t)__shfl_xor((unsigned long long)m, o, kWave));
  if (lane == 0) ((gptr<uint64_t>)a.row_ext)[row] = m;
}

template <int CPT>
__global__ __launch_bounds__(kThreads) void extrema_filter_kernel(const FilterArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds[];      // two buffers of n_lon composites
  const int tid = (int)threadIdx.x;
  const int row_block = (int)(blockIdx.x % (unsigned)a.n_row_blocks);
  const int64_t plane = (int64_t)(blockIdx.x / (unsigned)a.n_row_blocks);
  const int H = a.n_lat, W = a.n_lon;
  const bool wrap = a.wrap != 0, is_max = a.is_max != 0;
  const gptr<const float> in = (gptr<const float>)a.planes[plane];
  const gptr<const uint64_t> row_ext = (gptr<const uint64_t>)(a.row_ext + plane * H);
  const int i0 = row_block * kFilterRows;

  // (workgroup-uniform: the source rows of every target row, clamped into the plane, and their union)
  int k0[kFilterRows], cnt[kFilterRows];
  int k_first = H, k_end = 0;
#pragma unroll
  for (int t = 0; t < kFilterRows; ++t) {
    const int i = i0 + t;
    k0[t] = 0, cnt[t] = 0;
    if (i < H) {
      k0[t] = extrema_clamp(a.row_lo[i], 0, H - 1);
      cnt[t] = extrema_clamp(a.row_count[i], 0, min(a.max_rows, H - k0[t]));
      if (cnt[t] > 0) k_first = min(k_first, k0[t]), k_end = max(k_end, k0[t] + cnt[t]);
    }
  }

  uint64_t best[kFilterRows][CPT];
#pragma unroll
  for (int t = 0; t < kFilterRows; ++t)
#pragma unroll
    for (int s = 0; s < CPT; ++s) best[t][s] = kNone;

  for (int k = k_first; k < k_end; ++k) {                       // ascending source rows
    int n[kFilterRows], level[kFilterRows];
    int top = -1;
#pragma unroll
    for (int t = 0; t < kFilterRows; ++t) {
      const int r = k - k0[t];
      n[t] = -1, level[t] = -1;
      if (r >= 0 && r < cnt[t]) {
        n[t] = min(a.half[(int64_t)(i0 + t) * a.max_rows + r], W);
        if (k == i0 + t) n[t] = max(n[t], 0);                  // a point is a member of its own disc
      }
      if (n[t] < 0) continue;                                  // no column of this row is inside the disc
      if (extrema_whole_row(n[t], W, wrap)) {
        const uint64_t q = row_ext[k];
#pragma unroll
        for (int s = 0; s < CPT; ++s) best[t][s] = min_u64(best[t][s], q);
      } else {
        level[t] = extrema_level(n[t]);
        top = max(top, level[t]);
      }
    }
    if (top < 0) continue;                                     // (uniform: no target row needs the tables of this row)

#pragma unroll
    for (int s = 0; s < CPT; ++s) {
      const int c = tid + s * kThreads;
      if (c < W) lds[c] = composite(in[(int64_t)k * W + c], (uint32_t)(k * W + c), is_max);
    }
    __syncthreads();
    for (int l = 0; l <= top; ++l) {
      uint64_t* const cur = lds + (l & 1) * W;
      uint64_t* const other = lds + ((l & 1) ^ 1) * W;          // level l - 1 until this step overwrites it with level l + 1
      bool answered = false;
#pragma unroll
      for (int t = 0; t < kFilterRows; ++t) {
        if (level[t] != l) continue;
        answered = true;
#pragma unroll
        for (int s = 0; s < CPT; ++s) {
          const int c = tid + s * kThreads;
          if (c < W) {
            const ExtremaWindow q = extrema_window(c, n[t], W, wrap);
            const uint64_t* const m = q.back ? other : cur;
            best[t][s] = min_u64(best[t][s], min_u64(m[q.a], m[q.b]));
          }
        }
      }
      if (l < top) {
        if (!wrap && answered) __syncthreads();                  // a clipped window may have read level l - 1
#pragma unroll
        for (int s = 0; s < CPT; ++s) {
          const int c = tid + s * kThreads;
          if (c < W) {
            const int p = extrema_partner(c, l, W, wrap);
            uint64_t v = cur[c];
            if (p >= 0) v = min_u64(v, cur[p]);
            other[c] = v;
          }
        }
      }
      __syncthreads();
    }
  }

  const gptr<int32_t> index = (gptr<int32_t>)(a.index + plane * H * W);
  const gptr<float> filtered = (gptr<float>)(a.filtered + plane * H * W);
  int found[kFilterRows];
#pragma unroll
  for (int t = 0; t < kFilterRows; ++t) {
    found[t] = 0;
    const int i = i0 + t;
    if (i >= H) continue;
#pragma unroll
    for (int s = 0; s < CPT; ++s) {
      const int c = tid + s * kThreads;
      if (c < W) {
        const int at = i * W + c;
        const uint64_t q = best[t][s];
        const int idx = q == kNone ? -1 : (int)(uint32_t)q;
        index[at] = idx;
        filtered[at] = q == kNone ? __builtin_nanf("") : key_value((uint32_t)(q >> 32), is_max);
        found[t] += idx == at ? 1 : 0;
      }
    }
  }
  // the extrema of each target row: lanes, then the waves through LDS (every read of the tables is behind a barrier)
  int* const s_found = (int*)lds;
#pragma unroll
  for (int t = 0; t < kFilterRows; ++t) {
    int v = found[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    if (tid % kWave == 0) s_found[(tid / kWave) * kFilterRows + t] = v;
  }
  __syncthreads();
  if (tid < kFilterRows && i0 + tid < H) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += s_found[w * kFilterRows + tid];
    ((gptr<int32_t>)a.row_cnt)[plane * H + i0 + tid] = v;
  }
}

__global__ __launch_bounds__(kThreads) void extrema_scan_kernel(const ScanArgs a) {
  __shared__ int s_count;
  const int tid = (int)threadIdx.x, lane = tid % kWave;
  const int64_t plane = blockIdx.x;
  const int H = a.n_lat;
  if (tid < kWave) {
    const gptr<const int32_t> cnt = (gptr<const int32_t>)(a.row_cnt + plane * H);
    const gptr<int32_t> base = (gptr<int32_t>)(a.row_base + plane * H);
    int carry = 0;
    for (int r0 = 0; r0 < H; r0 += kWave) {                     // wave-uniform trip count: the shuffles see whole waves
      const int i = r0 + lane;
      const int v = i < H ? cnt[i] : 0;
      int incl = v;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const int up = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += up;
      }
      if (i < H) base[i] = carry + incl - v;
      carry += __shfl(incl, kWave - 1, kWave);
    }
    if (lane == 0) {
      ((gptr<int32_t>)a.count)[plane] = carry;
      s_count = carry;
    }
  }
  __syncthreads();
  const int64_t first = 2 * (int64_t)extrema_clamp(s_count, 0, a.max_points), end = 2 * (int64_t)a.max_points;
  const gptr<int64_t> table = (gptr<int64_t>)(a.table + plane * end);
  for (int64_t e = first + tid; e < end; e += kThreads) table[e] = 0;
}

__global__ __launch_bounds__(kThreads) void extrema_number_kernel(const NumberArgs a) {
  const int wave = (int)threadIdx.x / kWave, lane = (int)threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kWaves + wave;    // wave-uniform
  if (row >= a.n_rows) return;
  const int64_t plane = row / a.n_lat;
  const int i = (int)(row - plane * a.n_lat);
  const int W = a.n_lon;
  int rank = ((gptr<const int32_t>)a.row_base)[row];
  if (rank < 0 || rank >= a.max_points) return;               // the rows of the table are full
  const int64_t at0 = plane * a.n_lat * W + (int64_t)i * W;
  const gptr<const int32_t> index = (gptr<const int32_t>)(a.index + at0);
  const gptr<const float> filtered = (gptr<const float>)(a.filtered + at0);
  const gptr<int64_t> table = (gptr<int64_t>)(a.table + plane * 2 * (int64_t)a.max_points);
  for (int c0 = 0; c0 < W && rank < a.max_points; c0 += kWave) {   // wave-uniform
    const int c = c0 + lane;
    const int at = i * W + min(c, W - 1);
    const bool is = c < W && index[c] == at;
    const unsigned long long mask = __ballot(is);
    const int mine = rank + __popcll(mask & ((1ull << lane) - 1ull));
    if (is && mine < a.max_points) {
      table[2 * (int64_t)mine] = at;
      table[2 * (int64_t)mine + 1] = (int64_t)value_key(filtered[c], false);
    }
    rank += __popcll(mask);
  }
}

size_t workspace_bytes(int64_t n_planes, int n_lat) { return (size_t)(n_planes * n_lat * 16); }

bool sizes_ok(int n_planes, int n_lat, int n_lon) {
  return n_planes >= 1 && n_lat >= 1 && n_lon >= 1 && n_lon <= kMaxLon && (int64_t)n_lat * n_lon <= 0x7fffffffll;
}

template <int CPT> void launch_filter(const FilterArgs& f, unsigned groups, size_t lds_bytes, hipStream_t s) {
  hipLaunchKernelGGL(extrema_filter_kernel<CPT>, dim3(groups), dim3(kThreads), lds_bytes, s, f);
}

}  // namespace
}  // namespace aurora

using namespace aurora;

// 16 bytes per row of every plane: the row's extreme composite (uint64), its number of extrema and its base (int32 each).
extern "C" size_t aurora_hip_extrema_workspace_bytes(int n_planes, int n_lat, int n_lon) {
  if (!sizes_ok(n_planes, n_lat, n_lon)) return 0;
  return workspace_bytes(n_planes, n_lat);
}

extern "C" int aurora_hip_extrema(const float* const* planes, int32_t* index, float* filtered, int64_t* table, int32_t* count,
                                  int n_planes, int n_lat, int n_lon, const int32_t* row_lo, const int32_t* row_count,
                                  const int32_t* half, int max_rows, int wrap, int is_max, int max_points, void* workspace,
                                  size_t workspace_size, void* stream) {
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1 && n_lon >= 1, "extrema: bad sizes (planes %d, grid %d x %d)", n_planes, n_lat, n_lon);
  AURORA_CHECK_ARG(n_lon <= kMaxLon, "extrema: the grid has %d longitudes; 1 to %d are supported", n_lon, kMaxLon);
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= 0x7fffffffll, "extrema: a plane of %d x %d points is too large", n_lat, n_lon);
  AURORA_CHECK_ARG(max_rows >= 1 && max_rows <= kMaxRows, "extrema: 1 to %d source rows per target row, got %d", kMaxRows, max_rows);
  AURORA_CHECK_ARG((wrap == 0 || wrap == 1) && (is_max == 0 || is_max == 1),
                   "extrema: the flags wrap and is_max must be 0 or 1, got %d and %d", wrap, is_max);
  AURORA_CHECK_ARG(max_points >= 1 && max_points <= kMaxPoints, "extrema: max_points must be in 1..%d, got %d", kMaxPoints, max_points);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(planes && index && filtered && table && count && row_lo && row_count && half && workspace,
                   "extrema: null plane array, output, table or workspace pointer");
  AURORA_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)table) & 7) == 0 &&
                       (((uintptr_t)row_lo | (uintptr_t)row_count | (uintptr_t)half | (uintptr_t)index | (uintptr_t)filtered |
                         (uintptr_t)count) & 3) == 0,
                   "extrema: table and the workspace must be 8-byte aligned, index, filtered, count, row_lo, row_count and half "
                   "4-byte aligned");
  const size_t need = workspace_bytes(n_planes, n_lat);
  AURORA_CHECK_ARG(workspace_size >= need, "extrema: the workspace has %zu bytes, %zu are needed", workspace_size, need);
  const int64_t n_rows = (int64_t)n_planes * n_lat;
  const int64_t row_groups = (n_rows + kWaves - 1) / kWaves;
  const int64_t n_row_blocks = ((int64_t)n_lat + kFilterRows - 1) / kFilterRows;
  AURORA_CHECK_ARG(row_groups <= 0x7fffffff && n_row_blocks * n_planes <= 0x7fffffff,
                   "extrema: too many planes for one launch (%d planes of %d x %d)", n_planes, n_lat, n_lon);
  const hipStream_t s = as_stream(stream);
  uint64_t* const row_ext = (uint64_t*)workspace;
  int32_t* const row_cnt = (int32_t*)(row_ext + n_rows);
  int32_t* const row_base = row_cnt + n_rows;

  RowArgs r;
  r.planes = planes, r.row_ext = row_ext, r.n_rows = n_rows, r.n_lat = n_lat, r.n_lon = n_lon, r.is_max = is_max;
  hipLaunchKernelGGL(extrema_rows_kernel, dim3((unsigned)row_groups), dim3(kThreads), 0, s, r);
  int code = check_launch("extrema (row extremes)");
  if (code != AURORA_OK) return code;

  FilterArgs f;
  f.planes = planes, f.index = index, f.filtered = filtered, f.row_ext = row_ext, f.row_cnt = row_cnt, f.row_lo = row_lo;
  f.row_count = row_count, f.half = half, f.n_lat = n_lat, f.n_lon = n_lon, f.max_rows = max_rows;
  f.n_row_blocks = (int)n_row_blocks, f.wrap = wrap, f.is_max = is_max;
  const unsigned groups = (unsigned)(n_row_blocks * n_planes);
  const size_t lds_bytes = (size_t)n_lon * 16 > (size_t)kMinLdsBytes ? (size_t)n_lon * 16 : (size_t)kMinLdsBytes;   // <= 64 KiB
  const int per_thread = (n_lon + kThreads - 1) / kThreads;    // 1 .. 16 columns of a thread
  if (per_thread <= 1) launch_filter<1>(f, groups, lds_bytes, s);
  else if (per_thread <= 2) launch_filter<2>(f, groups, lds_bytes, s);
  else if (per_thread <= 4) launch_filter<4>(f, groups, lds_bytes, s);
  else if (per_thread <= 6) launch_filter<6>(f, groups, lds_bytes, s);
  else if (per_thread <= 8) launch_filter<8>(f, groups, lds_bytes, s);
  else if (per_thread <= 12) launch_filter<12>(f, groups, lds_bytes, s);
  else launch_filter<16>(f, groups, lds_bytes, s);
  code = check_launch("extrema (filter)");
  if (code != AURORA_OK) return code;

  ScanArgs c;
  c.row_cnt = row_cnt, c.row_base = row_base, c.count = count, c.table = table, c.n_lat = n_lat, c.max_points = max_points;
  hipLaunchKernelGGL(extrema_scan_kernel, dim3((unsigned)n_planes), dim3(kThreads), 0, s, c);
  code = check_launch("extrema (scan)");
  if (code != AURORA_OK) return code;

  NumberArgs m;
  m.index = index, m.filtered = filtered, m.row_base = row_base, m.table = table, m.n_rows = n_rows, m.n_lat = n_lat;
  m.n_lon = n_lon, m.max_points = max_points;
  hipLaunchKernelGGL(extrema_number_kernel, dim3((unsigned)row_groups), dim3(kThreads), 0, s, m);
  return check_launch("extrema (number)");
}
