// Connected components of threshold events on the device (aurora_amd.objects: label maps, object counts and the integer
// table of sizes, positions and peaks; the rule is stated in aurora_amd/objects.py and include/aurora_hip.h).
//
// For every plane (n_lat x n_lon fp32, row-major) and every threshold t the EVENTS are the finite points with v >= t (v <= t
// with `below`); objects are their maximal 4- or 8-connected sets, periodic in longitude with `wrap`, never across a pole.
// Union-find over planes (objects_uf.h) in a fixed sequence of launches on the caller's stream; a wavefront owns one row:
//
//   zero      the table.
//   rows      (plane, row), every threshold: the event mask of each 64-column chunk by ballot, each point's run start by bit
//             operations with the open run carried across chunks; parent[x] = flat index of the run start, -1 for background.
//   unite     (plane, threshold, row): every contact with the row above that the point's left neighbour does not already carry,
//             and the seam (column n_lon - 1 with column 0 of the same row), by lock-free uf_unite.
//   flatten   every event point replaces its parent by its root (the object's first point); the wave counts its row's roots.
//   scan      one wave per (plane, threshold): row counts -> row bases (exclusive) and count.
//   number    a root's number is its row base + the roots before it in the row + 1; it writes its label and, if numbered at
//             most max_objects, `first` and `row_min` of its table row.  Background gets label 0.
//   tabulate  every other event point copies its root's label; every event point of a tabulated object enters the table
//             with INTEGER global atomics (64-bit add / min / max), the lanes of a wave that share an object combined first.
//
// Order between the phases is the order of the launches: no kernel spins or waits on a value that another workgroup writes in
// the same launch, and every loop is bounded by the data (see objects_uf.h for the two union-find loops).  Integer sums,
// minima and maxima do not depend on the order of the atomics, and the root of an object is its first point whatever the
// order of the unions: labels, count and table are repeatable bit for bit and depend on the plane's own values alone.
// The planes are read four bytes at a time (a lane per column), so nothing depends on the alignment of a plane pointer.
#include "objects_uf.h"
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxThresholds = 8;
constexpr int kMaxLon = 4096;
constexpr int kColumns = 10;                       // of a table row (include/aurora_hip.h)
enum { kPoints, kArea, kFirst, kRowMin, kRowMax, kRowSum, kOffMin, kOffMax, kOffSum, kPeak };

// parent[] of one (plane, threshold) for objects_uf.h: relaxed, agent-scope atomics on global memory.
struct Parents {
  gptr<int32_t> p;
  __device__ __forceinline__ bool event(int32_t i) const { return p[i] >= 0; }
  __device__ __forceinline__ int32_t load(int32_t i) const {
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void store(int32_t i, int32_t v) const {
    __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ int32_t fetch_min(int32_t i, int32_t v) const {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// The row this wave owns: wave w of the launch is row w % n_lat of item w / n_lat; false past the last one (wave-uniform).
__device__ __forceinline__ bool my_row(int64_t n_items, int n_lat, int64_t& item, int& row, int& lane) {
  lane = (int)threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (w >= n_items * n_lat) return false;
  item = w / n_lat;
  row = (int)(w % n_lat);
  return true;
}

__device__ __forceinline__ uint64_t lanes_upto(int lane) { return ~0ull >> (63 - lane); }   // bits 0 .. lane

// The 32-bit key that ascends with the value: -0 below +0 (events are finite, so NaN does not arise).
__device__ __forceinline__ uint32_t value_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kThreads) void zero_kernel(int64_t* __restrict__ table, int64_t n_words) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_words; i += stride) table[i] = 0;   // bounded by n_words
}

// ---- rows ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void rows_kernel(const float* const* __restrict__ planes, int64_t n_planes, int n_lat,
                                                        int n_lon, const float* __restrict__ thresholds, int T, int below,
                                                        int32_t* __restrict__ parent) {
  int64_t plane;
  int row, lane;
  if (!my_row(n_planes, n_lat, plane, row, lane)) return;
  const gptr<const float> P = (gptr<const float>)planes[plane];
  const int64_t n_points = (int64_t)n_lat * n_lon;
  const int32_t row0 = row * n_lon;                 // < n_points <= 2^31 - 2
  float thr[kMaxThresholds];
  int open_start[kMaxThresholds];                   // the column at which the run open at the end of the last chunk began
  bool open[kMaxThresholds];
#pragma unroll
  for (int t = 0; t < kMaxThresholds; ++t) {
    thr[t] = t < T ? thresholds[plane * T + t] : __builtin_nanf("");
    open[t] = false, open_start[t] = 0;
  }
  for (int j0 = 0; j0 < n_lon; j0 += 64) {          // bounded by n_lon
    const int j = j0 + lane;
    const bool in = j < n_lon;
    const float v = P[row0 + (in ? j : n_lon - 1)]; // clamped into the row: loaded, never used
    const bool finite = in && __builtin_isfinite(v);
#pragma unroll
    for (int t = 0; t < kMaxThresholds; ++t) {
      if (t >= T) break;                            // wave-uniform
      const bool ev = finite && (below ? v <= thr[t] : v >= thr[t]);   // a NaN threshold: never
      const uint64_t m = __ballot(ev);
      const uint64_t starts = m & ~((m << 1) | (open[t] ? 1ull : 0ull));
      const uint64_t mine = starts & lanes_upto(lane);
      const int start = mine ? j0 + 63 - __builtin_clzll(mine) : open_start[t];
      if (in) parent[(plane * T + t) * n_points + row0 + j] = ev ? row0 + start : -1;
      if (m >> 63) {
        if (starts) open_start[t] = j0 + 63 - __builtin_clzll(starts);
        open[t] = true;
      } else {
        open[t] = false;
      }
    }
  }
}

// ---- unite -----------------------------------------------------------------------------------------------------------------
// Event-ness (parent >= 0) never changes after rows_kernel, so plain loads tell it; the parents themselves go through Parents.
__global__ __launch_bounds__(kThreads) void unite_kernel(int32_t* __restrict__ parent, int64_t n_items, int n_lat, int n_lon,
                                                         int eight, int wrap) {
  int64_t item;
  int row, lane;
  if (!my_row(n_items, n_lat, item, row, lane)) return;
  const Parents mem{(gptr<int32_t>)(parent + item * ((int64_t)n_lat * n_lon))};
  for (int j = lane; j < n_lon; j += 64)            // bounded by n_lon
    if (mem.event(row * n_lon + j)) uf_unite_point(mem, row, j, n_lon, eight != 0, wrap != 0);
}

// ---- flatten ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void flatten_kernel(int32_t* __restrict__ parent, int64_t n_items, int n_lat, int n_lon,
                                                           int32_t* __restrict__ row_count) {
  int64_t item;
  int row, lane;
  if (!my_row(n_items, n_lat, item, row, lane)) return;
  const Parents mem{(gptr<int32_t>)(parent + item * ((int64_t)n_lat * n_lon))};
  const int32_t row0 = row * n_lon;
  int roots = 0;
  for (int j0 = 0; j0 < n_lon; j0 += 64) {          // bounded by n_lon
    const int j = j0 + lane;
    const int32_t x = row0 + j;
    const int32_t p = j < n_lon ? mem.load(x) : -1;
    // Other waves store roots over parents meanwhile: a root is a point of the same object that is <= the value it replaces,
    // so the invariant of objects_uf.h holds throughout and uf_find is bounded as it says.
    const int32_t r = p >= 0 ? uf_find(mem, x) : -1;
    if (p >= 0 && r != p) mem.store(x, r);
    roots += __builtin_popcountll(__ballot(p >= 0 && r == x));
  }
  if (lane == 0) row_count[item * n_lat + row] = roots;
}

// ---- scan ------------------------------------------------------------------------------------------------------------------
// One wave per (plane, threshold): row_count -> the number of roots in the rows before (in place), count = their total.
__global__ __launch_bounds__(64) void scan_kernel(int32_t* __restrict__ row_count, int n_lat, int32_t* __restrict__ count) {
  const int lane = (int)threadIdx.x;
  int32_t* const rc = row_count + (int64_t)blockIdx.x * n_lat;
  int32_t before = 0;
  for (int i0 = 0; i0 < n_lat; i0 += 64) {          // bounded by n_lat
    const int i = i0 + lane;
    const int32_t c = i < n_lat ? rc[i] : 0;
    int32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (i < n_lat) rc[i] = before + incl - c;
    before += __shfl(incl, 63, 64);
  }
  if (lane == 0) count[blockIdx.x] = before;
}

// ---- number ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void number_kernel(const int32_t* __restrict__ parent, int64_t n_items, int n_lat,
                                                          int n_lon, const int32_t* __restrict__ row_base, int max_objects,
                                                          int32_t* __restrict__ labels, int64_t* __restrict__ table) {
  int64_t item;
  int row, lane;
  if (!my_row(n_items, n_lat, item, row, lane)) return;
  const int64_t base = item * ((int64_t)n_lat * n_lon);
  const int32_t row0 = row * n_lon;
  int32_t before = row_base[item * n_lat + row];
  for (int j0 = 0; j0 < n_lon; j0 += 64) {          // bounded by n_lon
    const int j = j0 + lane;
    const int32_t x = row0 + j;
    const int32_t p = j < n_lon ? parent[base + x] : 0;
    const bool root = j < n_lon && p == x;
    const uint64_t m = __ballot(root);
    const int32_t k = before + __builtin_popcountll(m & (lanes_upto(lane) >> 1)) + 1;
    if (root) {
      labels[base + x] = k;
      if (k <= max_objects) {
        int64_t* const out = table + (item * max_objects + (k - 1)) * kColumns;
        out[kFirst] = x;
        out[kRowMin] = row;                         // the first point is in the object's first row
      }
    } else if (j < n_lon && p < 0) {
      labels[base + x] = 0;
    }
    before += __builtin_popcountll(m);
  }
}

// ---- tabulate --------------------------------------------------------------------------------------------------------------
template <typename V> __device__ __forceinline__ void add64(int64_t* p, V v) {
  __hip_atomic_fetch_add(p, (int64_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void tabulate_kernel(const float* const* __restrict__ planes,
                                                            const int32_t* __restrict__ parent, int64_t n_items, int T,
                                                            int n_lat, int n_lon, const int64_t* __restrict__ unit, int below,
                                                            int wrap, int max_objects, int32_t* __restrict__ labels,
                                                            int64_t* __restrict__ table) {
  int64_t item;
  int row, lane;
  if (!my_row(n_items, n_lat, item, row, lane)) return;
  const gptr<const float> P = (gptr<const float>)planes[item / T];
  const int64_t base = item * ((int64_t)n_lat * n_lon);
  const int32_t row0 = row * n_lon;
  const int64_t area_unit = unit[row];
  const int half = n_lon / 2;
  for (int j0 = 0; j0 < n_lon; j0 += 64) {          // bounded by n_lon
    const int j = j0 + lane;
    const int32_t x = row0 + j;
    const int32_t p = j < n_lon ? parent[base + x] : -1;   // the root, since flatten_kernel
    const bool ev = p >= 0;
    // the root's label is from number_kernel, the launch before; this launch writes the labels of other points only
    const int32_t k = ev ? labels[base + p] : 0;
    if (ev && p != x) labels[base + x] = k;
    const uint32_t vk = ev ? value_key(P[x]) : 0u;
    const uint64_t key = ((uint64_t)(below ? ~vk : vk) << 32) | (uint64_t)(0xffffffffu - (uint32_t)x);
    uint64_t todo = __ballot(ev && k <= max_objects);
    while (todo) {                                  // bounded: every iteration clears the lowest set bit of todo at least
      const int leader = __builtin_ctzll(todo);
      const int32_t k0 = __shfl(k, leader, 64);
      const uint64_t sel = __ballot(ev && k == k0);
      todo &= ~sel;
      const bool mine = (sel >> lane) & 1;
      int d = j - __shfl(p, leader, 64) % n_lon;    // the column offset from the object's first point
      if (wrap) d = d < -half ? d + n_lon : (d >= n_lon - half ? d - n_lon : d);
      int dmin = mine ? d : 0x7fffffff, dmax = mine ? d : -0x7fffffff - 1, dsum = mine ? d : 0;   // |dsum| <= 64 n_lon
      uint64_t peak = mine ? key : 0ull;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        dmin = min(dmin, __shfl_xor(dmin, o, 64));
        dmax = max(dmax, __shfl_xor(dmax, o, 64));
        dsum += __shfl_xor(dsum, o, 64);
        const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)peak, o, 64);
        peak = other > peak ? other : peak;
      }
      if (lane == leader) {
        const int64_t n = __builtin_popcountll(sel);
        int64_t* const out = table + (item * max_objects + (k0 - 1)) * kColumns;   // 1 <= k0 <= max_objects
        add64(out + kPoints, n);
        add64(out + kArea, n * area_unit);
        __hip_atomic_fetch_max(out + kRowMax, (int64_t)row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        add64(out + kRowSum, n * row);
        __hip_atomic_fetch_min(out + kOffMin, (int64_t)dmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(out + kOffMax, (int64_t)dmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        add64(out + kOffSum, dsum);
        __hip_atomic_fetch_max((uint64_t*)(out + kPeak), peak, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

size_t workspace_bytes(int64_t n_planes, int64_t n_lat, int64_t n_lon, int64_t T) {
  const int64_t words = n_planes * T * (n_lat * n_lon + n_lat);   // parent, then the row counters
  return (size_t)((words * 4 + 7) & ~(int64_t)7);
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_objects_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_thresholds) {
  if (n_planes < 1 || n_lat < 1 || n_lon < 1 || n_lon > kMaxLon || n_thresholds < 1 || n_thresholds > kMaxThresholds ||
      (int64_t)n_lat * n_lon > 0x7ffffffell)
    return 0;
  return workspace_bytes(n_planes, n_lat, n_lon, n_thresholds);
}

extern "C" int aurora_hip_objects(const float* const* planes, int n_planes, int n_lat, int n_lon, const float* thresholds,
                                  int n_thresholds, const int64_t* unit, int below, int connectivity, int wrap, int max_objects,
                                  int32_t* labels, int32_t* count, int64_t* table, void* workspace, size_t workspace_size,
                                  void* stream) {
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1 && n_lon >= 1, "objects: bad sizes (planes %d, grid %d x %d)", n_planes, n_lat,
                   n_lon);
  AURORA_CHECK_ARG(n_lon <= kMaxLon, "objects: at most %d longitudes, got %d", kMaxLon, n_lon);
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= 0x7ffffffell, "objects: a grid of %d x %d points is beyond the 2^31 - 2 of an int32 label map",
                   n_lat, n_lon);
  AURORA_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= kMaxThresholds, "objects: 1 to %d thresholds, got %d", kMaxThresholds,
                   n_thresholds);
  AURORA_CHECK_ARG(connectivity == 4 || connectivity == 8, "objects: connectivity must be 4 or 8, got %d", connectivity);
  AURORA_CHECK_ARG((below == 0 || below == 1) && (wrap == 0 || wrap == 1), "objects: the flags below and wrap must be 0 or 1, got %d and %d",
                   below, wrap);
  AURORA_CHECK_ARG(max_objects >= 1, "objects: max_objects must be at least 1, got %d", max_objects);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(planes && thresholds && unit && labels && count && table && workspace,
                   "objects: null plane array, threshold, unit, output or workspace pointer");
  AURORA_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)table & 7) == 0 && ((uintptr_t)unit & 7) == 0 &&
                       ((uintptr_t)labels & 3) == 0 && ((uintptr_t)count & 3) == 0 && ((uintptr_t)thresholds & 3) == 0,
                   "objects: unit, table and workspace must be 8-byte aligned, thresholds, labels and count 4-byte aligned");
  const size_t need = workspace_bytes(n_planes, n_lat, n_lon, n_thresholds);
  AURORA_CHECK_ARG(workspace_size >= need, "objects: the workspace has %zu bytes, %zu are needed", workspace_size, need);
  const int64_t n_items = (int64_t)n_planes * n_thresholds;
  const int64_t groups = (n_items * n_lat + kWaves - 1) / kWaves;
  AURORA_CHECK_ARG(groups <= 0x7fffffff && n_items <= 0x7fffffff, "objects: too many planes for one launch (%d planes x %d thresholds x %d rows)",
                   n_planes, n_thresholds, n_lat);
  int32_t* const parent = (int32_t*)workspace;
  int32_t* const row_count = parent + n_items * ((int64_t)n_lat * n_lon);
  const hipStream_t s = as_stream(stream);
  const int64_t n_words = n_items * max_objects * kColumns;
  const unsigned zero_groups = (unsigned)(n_words / kThreads + 1 < 4096 ? n_words / kThreads + 1 : 4096);
  const unsigned row_groups = (unsigned)(((int64_t)n_planes * n_lat + kWaves - 1) / kWaves);
  int code;
  hipLaunchKernelGGL(zero_kernel, dim3(zero_groups), dim3(kThreads), 0, s, table, n_words);
  if ((code = check_launch("objects (zero)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(rows_kernel, dim3(row_groups), dim3(kThreads), 0, s, planes, (int64_t)n_planes, n_lat, n_lon, thresholds,
                     n_thresholds, below, parent);
  if ((code = check_launch("objects (rows)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(unite_kernel, dim3((unsigned)groups), dim3(kThreads), 0, s, parent, n_items, n_lat, n_lon,
                     connectivity == 8 ? 1 : 0, wrap);
  if ((code = check_launch("objects (unite)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(flatten_kernel, dim3((unsigned)groups), dim3(kThreads), 0, s, parent, n_items, n_lat, n_lon, row_count);
  if ((code = check_launch("objects (flatten)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(scan_kernel, dim3((unsigned)n_items), dim3(64), 0, s, row_count, n_lat, count);
  if ((code = check_launch("objects (scan)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(number_kernel, dim3((unsigned)groups), dim3(kThreads), 0, s, (const int32_t*)parent, n_items, n_lat, n_lon,
                     (const int32_t*)row_count, max_objects, labels, table);
  if ((code = check_launch("objects (number)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(tabulate_kernel, dim3((unsigned)groups), dim3(kThreads), 0, s, planes, (const int32_t*)parent, n_items,
                     n_thresholds, n_lat, n_lon, unit, below, wrap, max_objects, labels, table);
  return check_launch("objects (tabulate)");
}
