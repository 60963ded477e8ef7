// The nearest event of every grid point on the sphere, and the separations of objects that follow from it
// (aurora_amd.nearest_event, aurora_amd.object_separations; the rule is stated in aurora_amd/distances.py and
// include/aurora_hip.h, what decides a result is in nearest_event_search.h).
//
// An item is a plane and a threshold: an n_lat x n_lon int32 label map, row-major; an EVENT is a point with label > 0.  For two
// fixed rows the distance grows with the column gap, so the nearest event of a source row is its ROW CANDIDATE, the event with
// the smallest gap, and the search over points is a search over rows.  aurora_hip_nearest_event, three launches on the caller's
// stream:
//
//   rows     a wavefront owns a row of an item: the event bits by ballot, 64 columns at a time, one mask per lane; the last
//            event before a chunk and the first after it by a prefix maximum and a suffix minimum over the lanes (once more
//            round the circle on a wrapping grid); then every column's candidate as int16 into the workspace (2 bytes per point)
//            and the row's "has an event" flag.
//   extent   a wavefront per item: the first and the last row that has an event (n_lat and -1 in an item without one, whose
//            points then walk no row at all).
//   search   a wavefront owns 64 adjacent columns of a row, so the candidates of a source row are read side by side and the
//            sine and cosine of a source row are wave-uniform.  It walks the rows outward from its own, up and down in turn,
//            inside the extent; every lane keeps its best (key, flat index) and stops a direction by the test of
//            nearest_event_search.h; the wave goes on while one lane does.
//
// No launch waits on a value written within it.  Every loop is bounded by n_lat, n_lon / 64 or 64 and moves strictly onward.
// Nothing is accumulated: index and key of a point depend on its own item alone, not on the order in which workgroups run.
//
// aurora_hip_object_separations, four launches: init, least (a 64-bit atomic minimum of the key bits per object, the lanes of a
// wave that share a label combined first as in the tabulate step of objects.hip, and an atomic maximum for the Hausdorff cell),
// point (an atomic minimum of (a_point << 32) | b_point among the points that attain the object's key), finish (unpack; zero
// the rows past count).  Minima and maxima of integers: the order of the atomics does not matter.  Vector atomics only.
#include "nearest_event_search.h"
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int64_t kInfBits = 0x7ff0000000000000ll;
constexpr int64_t kNoPoint = 0x7fffffffffffffffll;

// wave w of the launch is row w % n_lat of item w / n_lat (wave-uniform)
__device__ __forceinline__ bool my_row(int64_t n_items, int n_lat, int64_t& item, int& row, int& lane) {
  lane = (int)threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (w >= n_items * n_lat) return false;
  item = w / n_lat;
  row = (int)(w % n_lat);
  return true;
}

// ---- rows ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void nearest_rows_kernel(const int32_t* __restrict__ labels, int64_t n_items, int n_lat, int n_lon,
                                                        int wrap, int16_t* __restrict__ cand, int32_t* __restrict__ flag) {
  int64_t item;
  int row, lane;
  if (!my_row(n_items, n_lat, item, row, lane)) return;
  const int64_t row0 = (item * n_lat + row) * (int64_t)n_lon;
  const gptr<const int32_t> L = (gptr<const int32_t>)(labels + row0);
  const int n_chunks = (n_lon + 63) / 64;            // <= 64: one mask per lane
  uint64_t mine = 0;
  for (int c = 0; c < n_chunks; ++c) {               // bounded by n_lon / 64
    const int j = 64 * c + lane;
    const uint64_t mask = __ballot(j < n_lon && L[j < n_lon ? j : n_lon - 1] > 0);
    if (lane == c) mine = mask;
  }
  // lane c: the last event column before chunk c and the first after it
  int last = mine ? ne::chunk_last(mine, lane) : -ne::kNone, first = mine ? ne::chunk_first(mine, lane) : ne::kNone;
  int west = last, east = first;                     // inclusive scans first
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(west, o, 64), down = __shfl_down(east, o, 64);
    if (lane >= o) west = max(west, up);
    if (lane + o < 64) east = min(east, down);
  }
  const int row_last = __shfl(west, 63, 64), row_first = __shfl(east, 0, 64);
  west = __shfl_up(west, 1, 64);
  east = __shfl_down(east, 1, 64);
  if (lane == 0) west = -ne::kNone;
  if (lane == 63) east = ne::kNone;
  const bool any = row_first < ne::kNone;
  if (wrap && any) {
    if (west == -ne::kNone) west = row_last - n_lon;
    if (east == ne::kNone) east = row_first + n_lon;
  }
  const gptr<int16_t> C = (gptr<int16_t>)(cand + row0);
  for (int c = 0; c < n_chunks; ++c) {               // bounded by n_lon / 64
    const uint64_t mask = (uint64_t)__shfl((unsigned long long)mine, c, 64);
    const int wb = __shfl(west, c, 64), ea = __shfl(east, c, 64);
    const int j = 64 * c + lane;
    if (j < n_lon) C[j] = (int16_t)ne::candidate(j, ne::west_of(mask, c, lane, wb), ne::east_of(mask, c, lane, ea), n_lon);
  }
  if (lane == 0) flag[item * n_lat + row] = any ? 1 : 0;
}

// ---- extent ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void nearest_extent_kernel(const int32_t* __restrict__ flag, int n_lat, int32_t* __restrict__ extent) {
  const int lane = (int)threadIdx.x;
  const int32_t* const f = flag + (int64_t)blockIdx.x * n_lat;
  int lo = n_lat, hi = -1;
  for (int i = lane; i < n_lat; i += 64)             // bounded by n_lat
    if (f[i]) lo = min(lo, i), hi = max(hi, i);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  if (lane == 0) extent[2 * (int64_t)blockIdx.x] = lo, extent[2 * (int64_t)blockIdx.x + 1] = hi;
}

// ---- search ----------------------------------------------------------------------------------------------------------------
// tables: sin(lat) (n_lat), max(cos(lat), 0) (n_lat), cos(d dlon) (n_lon).
__global__ __launch_bounds__(kThreads) void nearest_search_kernel(const int16_t* __restrict__ cand, const int32_t* __restrict__ flag,
                                                          const int32_t* __restrict__ extent, int64_t n_items, int n_lat,
                                                          int n_lon, const double* __restrict__ tables, int wrap, double key_max,
                                                          int32_t* __restrict__ index, double* __restrict__ key) {
  // wave w of the launch is chunk w % n_chunks of row (w / n_chunks) % n_lat of item w / (n_chunks n_lat) (wave-uniform)
  const int lane = (int)threadIdx.x & 63;
  const int n_chunks = (n_lon + 63) / 64;
  const int64_t w = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (w >= n_items * n_lat * n_chunks) return;
  const int64_t item = w / ((int64_t)n_lat * n_chunks);
  const int i = (int)((w / n_chunks) % n_lat);
  const int j = 64 * (int)(w % n_chunks) + lane;
  const bool in = j < n_lon;
  const int jc = in ? j : n_lon - 1;                 // clamped into the row: loaded, never stored
  const double* const S = tables;
  const double* const Cs = tables + n_lat;
  const double* const cd = tables + 2 * (int64_t)n_lat;
  const int64_t rows0 = item * n_lat;
  const int lo = extent[2 * item], hi = extent[2 * item + 1];
  const double si = S[i], ci = Cs[i];
  ne::Best best{__builtin_inf(), -1};
  // The rows with events are lo .. hi.  Upwards the walk takes min(i, hi), then the rows above it down to lo; downwards
  // max(i + 1, lo) and the rows below it up to hi: the rows it leaps over at the start have no event.  A lane is done with a
  // direction once ne::stops says so; the wave is done with it when every lane is, or when the extent ends.
  int ku = i < hi ? i : hi, kd = i + 1 > lo ? i + 1 : lo;
  bool up = true, down = true;                       // this lane still walks
  bool wave_up = ku >= lo, wave_down = kd <= hi;     // (wave-uniform) the wave still walks
  while (wave_up || wave_down) {                     // bounded by n_lat: every turn moves ku or kd strictly outward
    if (wave_up) {
      const double sk = S[ku], ck = Cs[ku];
      const double key0 = ne::key_of(si, ci, sk, ck, 1.0);
      const double bound = best.key < key_max ? best.key : key_max;
      up = up && !ne::stops(key0, bound);
      // the row itself is skipped without a margin where its zero-gap key is already beyond the bound
      if (flag[rows0 + ku] && __ballot(up && !(key0 > bound))) {
        const int col = cand[(rows0 + ku) * (int64_t)n_lon + jc];
        if (up && !(key0 > bound)) ne::visit(best, i, jc, ku, col, si, ci, sk, ck, cd, n_lon, wrap != 0, key_max);
      }
      --ku;
      wave_up = ku >= lo && __ballot(up) != 0;
    }
    if (wave_down) {
      const double sk = S[kd], ck = Cs[kd];
      const double key0 = ne::key_of(si, ci, sk, ck, 1.0);
      const double bound = best.key < key_max ? best.key : key_max;
      down = down && !ne::stops(key0, bound);
      if (flag[rows0 + kd] && __ballot(down && !(key0 > bound))) {
        const int col = cand[(rows0 + kd) * (int64_t)n_lon + jc];
        if (down && !(key0 > bound)) ne::visit(best, i, jc, kd, col, si, ci, sk, ck, cd, n_lon, wrap != 0, key_max);
      }
      ++kd;
      wave_down = kd <= hi && __ballot(down) != 0;
    }
  }
  if (in) {
    const int64_t at = (rows0 + i) * (int64_t)n_lon + j;
    index[at] = best.index;
    key[at] = best.key;
  }
}

// ---- separations -----------------------------------------------------------------------------------------------------------
// table rows are [key_bits, packed point pair, unused] until separations_finish_kernel.
__global__ __launch_bounds__(kThreads) void separations_init_kernel(int64_t* __restrict__ table, int64_t n_rows, int64_t* __restrict__ hausdorff,
                                                        int64_t n_items) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n_rows; r += stride) {   // bounded by n_rows
    table[3 * r] = kInfBits;
    table[3 * r + 1] = kNoPoint;
    table[3 * r + 2] = 0;
    if (r < n_items) hausdorff[r] = 0;
  }
}

__device__ __forceinline__ int64_t shfl_xor64(int64_t v, int o) { return (int64_t)__shfl_xor((long long)v, o, 64); }

// POINT = false: the least key of every object and the greatest of the item; POINT = true: the least packed point pair among the
// points that attain the object's key (read from the table: the launch before has finished it).
template <bool POINT>
__global__ __launch_bounds__(kThreads) void separations_least_kernel(const int32_t* __restrict__ labels_a, const double* __restrict__ key,
                                                         const int32_t* __restrict__ index, int64_t n_items, int n_lat, int n_lon,
                                                         int max_objects, int64_t* __restrict__ table,
                                                         int64_t* __restrict__ hausdorff) {
  int64_t item;
  int row, lane;
  if (!my_row(n_items, n_lat, item, row, lane)) return;
  const int64_t row0 = (item * n_lat + row) * (int64_t)n_lon;
  const gptr<const int32_t> A = (gptr<const int32_t>)(labels_a + row0);
  const gptr<const int64_t> K = (gptr<const int64_t>)((const int64_t*)key + row0);   // a key >= 0 orders like its bits
  const gptr<const int32_t> X = (gptr<const int32_t>)(index + row0);
  int64_t* const rows = table + item * (int64_t)max_objects * 3;
  int64_t far = 0;                                   // the greatest key of the wave's events
  for (int j0 = 0; j0 < n_lon; j0 += 64) {           // bounded by n_lon
    const int j = j0 + lane;
    const bool in = j < n_lon;
    const int jc = in ? j : n_lon - 1;
    const int32_t k = in ? A[jc] : 0;
    const bool ev = k > 0;
    const int64_t bits = K[jc];
    if (!POINT && ev) far = bits > far ? bits : far;
    const bool has_row = ev && k <= max_objects;
    int64_t v = bits;
    bool live = has_row;
    if (POINT) {
      live = has_row && bits != kInfBits && bits == rows[3 * (int64_t)(has_row ? k - 1 : 0)];
      v = (int64_t)(((uint64_t)(uint32_t)((int32_t)row * n_lon + j) << 32) | (uint64_t)(uint32_t)X[jc]);
    }
    uint64_t todo = __ballot(live);
    while (todo) {                                   // bounded: every iteration clears the lowest set bit of todo at least
      const int leader = __builtin_ctzll(todo);
      const int32_t k0 = __shfl(k, leader, 64);
      const uint64_t sel = __ballot(live && k == k0);
      todo &= ~sel;
      int64_t least = (sel >> lane) & 1 ? v : kNoPoint;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int64_t other = shfl_xor64(least, o);
        least = other < least ? other : least;
      }
      if (lane == leader)                            // 1 <= k0 <= max_objects
        __hip_atomic_fetch_min(rows + 3 * (int64_t)(k0 - 1) + (POINT ? 1 : 0), least, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (!POINT) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int64_t other = shfl_xor64(far, o);
      far = other > far ? other : far;
    }
    if (lane == 0 && far > 0) __hip_atomic_fetch_max(hausdorff + item, far, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kThreads) void separations_finish_kernel(const int32_t* __restrict__ count_a, int64_t n_items, int max_objects,
                                                          int64_t* __restrict__ table) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n_items * max_objects) return;
  const int32_t n = count_a[r / max_objects];
  int64_t* const out = table + 3 * r;
  if (r % max_objects >= n) {
    out[0] = 0, out[1] = 0, out[2] = 0;
    return;
  }
  const int64_t packed = out[1];
  const bool none = out[0] == kInfBits || packed == kNoPoint;
  out[1] = none ? -1 : packed >> 32;
  out[2] = none ? -1 : (int64_t)(int32_t)(packed & 0xffffffffll);
}

struct Layout {
  size_t cand, flag, extent, bytes;                  // offsets into the workspace, and its size
};
Layout layout_of(int64_t n_items, int64_t n_lat, int64_t n_lon) {
  const auto up8 = [](int64_t b) { return (size_t)((b + 7) & ~(int64_t)7); };
  Layout l;
  l.cand = 0;
  l.flag = up8(n_items * n_lat * n_lon * 2);
  l.extent = l.flag + up8(n_items * n_lat * 4);
  l.bytes = l.extent + up8(n_items * 2 * 4);
  return l;
}

bool sizes_ok(int64_t n_items, int n_lat, int n_lon) {
  return n_items >= 0 && n_items <= 0x7fffffff && n_lat >= 1 && n_lon >= 1 && n_lon <= ne::kMaxLon &&
         (int64_t)n_lat * n_lon <= 0x7ffffffell;
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_nearest_event_workspace_bytes(int64_t n_items, int n_lat, int n_lon) {
  if (!sizes_ok(n_items, n_lat, n_lon)) return 0;
  return layout_of(n_items, n_lat, n_lon).bytes;
}

extern "C" int aurora_hip_nearest_event(const int32_t* labels, int64_t n_items, int n_lat, int n_lon, const double* tables,
                                        int wrap, double key_max, int32_t* index, double* key, void* workspace,
                                        size_t workspace_size, void* stream) {
  AURORA_CHECK_ARG(n_items >= 0 && n_lat >= 1 && n_lon >= 1, "nearest_event: bad sizes (%lld items, grid %d x %d)",
                   (long long)n_items, n_lat, n_lon);
  AURORA_CHECK_ARG(n_lon <= ne::kMaxLon, "nearest_event: at most %d longitudes, got %d", ne::kMaxLon, n_lon);
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= 0x7ffffffell, "nearest_event: a grid of %d x %d points is beyond the 2^31 - 2 of an int32 label map",
                   n_lat, n_lon);
  AURORA_CHECK_ARG(wrap == 0 || wrap == 1, "nearest_event: the flag wrap must be 0 or 1, got %d", wrap);
  AURORA_CHECK_ARG(key_max >= 0.0, "nearest_event: key_max must be at least 0 (+inf: no bound), got %g", key_max);
  if (n_items == 0) return AURORA_OK;
  AURORA_CHECK_ARG(labels && tables && index && key && workspace, "nearest_event: null label map, table, output or workspace pointer");
  AURORA_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)key & 7) == 0 && ((uintptr_t)tables & 7) == 0 &&
                       ((uintptr_t)labels & 3) == 0 && ((uintptr_t)index & 3) == 0,
                   "nearest_event: tables, key and workspace must be 8-byte aligned, the label maps and index 4-byte aligned");
  const int n_chunks = (n_lon + 63) / 64;
  const int64_t row_groups = (n_items * n_lat + kWaves - 1) / kWaves;
  const int64_t search_groups = (n_items * n_lat * n_chunks + kWaves - 1) / kWaves;
  AURORA_CHECK_ARG(search_groups <= 0x7fffffff && n_items <= 0x7fffffff, "nearest_event: too many items for one launch (%lld items x %d rows)",
                   (long long)n_items, n_lat);
  const Layout l = layout_of(n_items, n_lat, n_lon);
  AURORA_CHECK_ARG(workspace_size >= l.bytes, "nearest_event: the workspace has %zu bytes, %zu are needed", workspace_size, l.bytes);
  int16_t* const cand = (int16_t*)((char*)workspace + l.cand);
  int32_t* const flag = (int32_t*)((char*)workspace + l.flag);
  int32_t* const extent = (int32_t*)((char*)workspace + l.extent);
  const hipStream_t s = as_stream(stream);
  int code;
  hipLaunchKernelGGL(nearest_rows_kernel, dim3((unsigned)row_groups), dim3(kThreads), 0, s, labels, n_items, n_lat, n_lon, wrap, cand, flag);
  if ((code = check_launch("nearest_event (rows)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(nearest_extent_kernel, dim3((unsigned)n_items), dim3(64), 0, s, (const int32_t*)flag, n_lat, extent);
  if ((code = check_launch("nearest_event (extent)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(nearest_search_kernel, dim3((unsigned)search_groups), dim3(kThreads), 0, s, (const int16_t*)cand, (const int32_t*)flag,
                     (const int32_t*)extent, n_items, n_lat, n_lon, tables, wrap, key_max, index, key);
  return check_launch("nearest_event (search)");
}

extern "C" int aurora_hip_object_separations(const int32_t* labels_a, const double* key, const int32_t* index,
                                             const int32_t* count_a, int64_t n_items, int n_lat, int n_lon, int max_objects,
                                             int64_t* table, int64_t* hausdorff, void* stream) {
  AURORA_CHECK_ARG(n_items >= 0 && n_lat >= 1 && n_lon >= 1, "object_separations: bad sizes (%lld items, grid %d x %d)",
                   (long long)n_items, n_lat, n_lon);
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= 0x7ffffffell, "object_separations: a grid of %d x %d points is beyond the 2^31 - 2 of an int32 label map",
                   n_lat, n_lon);
  AURORA_CHECK_ARG(max_objects >= 1, "object_separations: max_objects must be at least 1, got %d", max_objects);
  if (n_items == 0) return AURORA_OK;
  AURORA_CHECK_ARG(labels_a && key && index && count_a && table && hausdorff,
                   "object_separations: null label map, key, index, count or output pointer");
  AURORA_CHECK_ARG(((uintptr_t)key & 7) == 0 && ((uintptr_t)table & 7) == 0 && ((uintptr_t)hausdorff & 7) == 0 &&
                       ((uintptr_t)labels_a & 3) == 0 && ((uintptr_t)index & 3) == 0 && ((uintptr_t)count_a & 3) == 0,
                   "object_separations: key, table and hausdorff must be 8-byte aligned, the label maps, index and count 4-byte aligned");
  const int64_t groups = (n_items * n_lat + kWaves - 1) / kWaves;
  const int64_t n_rows = n_items * max_objects;
  AURORA_CHECK_ARG(groups <= 0x7fffffff && n_items <= 0x7fffffff && (n_rows + kThreads - 1) / kThreads <= 0x7fffffff,
                   "object_separations: too many items for one launch (%lld items x %d rows, %d objects)", (long long)n_items, n_lat,
                   max_objects);
  const hipStream_t s = as_stream(stream);
  const unsigned init_groups = (unsigned)(n_rows / kThreads + 1 < 4096 ? n_rows / kThreads + 1 : 4096);
  int code;
  hipLaunchKernelGGL(separations_init_kernel, dim3(init_groups), dim3(kThreads), 0, s, table, n_rows, hausdorff, n_items);
  if ((code = check_launch("object_separations (init)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(separations_least_kernel<false>, dim3((unsigned)groups), dim3(kThreads), 0, s, labels_a, key, index, n_items, n_lat, n_lon,
                     max_objects, table, hausdorff);
  if ((code = check_launch("object_separations (least)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(separations_least_kernel<true>, dim3((unsigned)groups), dim3(kThreads), 0, s, labels_a, key, index, n_items, n_lat, n_lon,
                     max_objects, table, hausdorff);
  if ((code = check_launch("object_separations (point)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(separations_finish_kernel, dim3((unsigned)((n_rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, count_a, n_items,
                     max_objects, table);
  return check_launch("object_separations (finish)");
}
