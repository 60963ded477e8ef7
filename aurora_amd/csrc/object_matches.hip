// The overlap pair table of two label maps on the device (aurora_amd.object_matches: which object of `a` is which object of
// `b`, and by how much they overlap; the rule is stated in aurora_amd/object_matches.py and include/aurora_hip.h).
//
// For every item (a plane and a threshold: two n_lat x n_lon int32 label maps, row-major) a point contributes where
// 1 <= la <= max_objects_a and 1 <= lb <= max_objects_b, to the pair (la, lb): one point and unit[row] area units.  The set of
// pairs is sparse and its keys are not known in advance, so they are aggregated in a bounded open-addressed hash table per item
// (pairs_hash.h: 64-bit key, 64-bit points, 64-bit units, C = max(64, pow2ceil(2 max_pairs)) slots) in three launches on the
// caller's stream:
//
//   zero        the tables.
//   accumulate  a wavefront owns a row of an item and reads both maps once, 64 columns at a time.  The lanes that hold the same
//               key are combined by ballot; the key of the chunk's last contributing lane is CARRIED in (wave-uniform)
//               registers into the next chunk and leaves the wave only when it is displaced or the row ends, so a long run
//               costs one insert per row, not per chunk; every other distinct key of a chunk is inserted by its leader lane,
//               the leaders of a chunk side by side.  An insert is one probe sequence and two 64-bit integer adds.  All points
//               of a wave's span share a row, so the units are points x unit[row].
//   finish      a workgroup per item: the occupied keys are gathered into LDS; if a contribution was dropped or there are more
//               than max_pairs, count = -1 and the rows are zero; else the keys are sorted (bitonic, in LDS), every row finds
//               its slot again by the probe sequence and writes [ka, kb, points, units], the rest is zeroed.
//
// No launch waits on a value written within it: the insert loop is bounded by C (pairs_hash.h says why), the combining loop
// clears a bit per iteration, the sort is a fixed network.  Everything accumulated is an integer, so pairs and count do not depend
// on the order of the atomics; which SLOT a key lands in does, and nothing that is written out depends on the slot.  An item
// that overflows is "-1, all zero" whatever order its keys arrived in.  The maps are read four bytes at a time (a lane per
// column, clamped into the row), so nothing depends on the alignment of a map.
#include "pairs_hash.h"
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kFinishThreads = 1024;

// The words of one item's table for pairs_hash.h: relaxed, agent-scope atomics on global memory.  The sums are zeroed by the
// launch before and only ever added to, and are read by the launch after: claiming a key needs no ordering with the adds.
struct Table {
  gptr<uint64_t> w;
  __device__ __forceinline__ uint64_t load(int64_t i) const {
    return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ uint64_t cas(int64_t i, uint64_t expected, uint64_t desired) const {
    __hip_atomic_compare_exchange_strong(w + i, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expected;                                // the value found
  }
  __device__ __forceinline__ void fetch_add(int64_t i, uint64_t v) const {
    __hip_atomic_fetch_add(w + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// The finished table, read by the launch after the inserts: plain loads.
struct Settled {
  gptr<const uint64_t> w;
  __device__ __forceinline__ uint64_t load(int64_t i) const { return w[i]; }
};

__global__ __launch_bounds__(kThreads) void zero_kernel(uint64_t* __restrict__ words, int64_t n_words) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_words; i += stride) words[i] = 0;   // bounded by n_words
}

// ---- accumulate ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void accumulate_kernel(const int32_t* __restrict__ labels_a,
                                                              const int32_t* __restrict__ labels_b, int64_t n_items, int n_lat,
                                                              int n_lon, const int64_t* __restrict__ unit, int max_a, int max_b,
                                                              int log2c, uint64_t* __restrict__ tables) {
  // wave w of the launch is row w % n_lat of item w / n_lat (wave-uniform)
  const int lane = (int)threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (w >= n_items * n_lat) return;
  const int64_t item = w / n_lat;
  const int row = (int)(w % n_lat);
  const Table mem{(gptr<uint64_t>)(tables + item * pairs_table_words(log2c))};
  // An item that has dropped a contribution is "overflow" whatever else its table holds: the rest of it costs only this load.
  if (pairs_overflowed(mem, log2c)) return;
  const int64_t row0 = item * ((int64_t)n_lat * n_lon) + (int64_t)row * n_lon;
  const gptr<const int32_t> A = (gptr<const int32_t>)(labels_a + row0), B = (gptr<const int32_t>)(labels_b + row0);
  const int64_t area_unit = unit[row];
  uint64_t carried = 0;                              // the key that continues from the chunks before (0: none), wave-uniform
  int64_t carried_n = 0;                             // and its points so far
  int jc = lane < n_lon ? lane : n_lon - 1;          // clamped into the row: loaded, never used
  int32_t la = A[jc], lb = B[jc];
  for (int j0 = 0; j0 < n_lon; j0 += 64) {           // bounded by n_lon
    const bool in = j0 + lane < n_lon;
    const bool valid = in && la >= 1 && la <= max_a && lb >= 1 && lb <= max_b;
    const uint64_t key = valid ? pairs_key(la, lb) : 0ull;
    jc = j0 + 64 + lane < n_lon ? j0 + 64 + lane : n_lon - 1;   // the next chunk's loads, under this chunk's work
    la = A[jc], lb = B[jc];
    uint64_t todo = __ballot(valid);
    if (todo == 0) continue;                         // (wave-uniform) a chunk with no contributing point costs only its read
    const uint64_t last = (uint64_t)__shfl((unsigned long long)key, 63 - __builtin_clzll(todo), 64);
    uint64_t out_key = 0;                            // what this lane, as a leader, has to insert
    int64_t out_n = 0;
    while (todo) {                                   // bounded: every iteration clears the lowest set bit of todo at least
      const int leader = __builtin_ctzll(todo);
      const uint64_t k0 = (uint64_t)__shfl((unsigned long long)key, leader, 64);
      const uint64_t sel = __ballot(key == k0);      // k0 != 0, so only contributing lanes
      todo &= ~sel;
      const int64_t n = __builtin_popcountll(sel);
      if (k0 == carried) {
        carried_n += n;
      } else if (k0 == last) {                       // the new carry; the displaced one leaves through this leader
        if (lane == leader) out_key = carried, out_n = carried_n;
        carried = k0, carried_n = n;
      } else if (lane == leader) {
        out_key = k0, out_n = n;
      }
    }
    if (out_key) pairs_insert(mem, log2c, out_key, out_n, out_n * area_unit);
  }
  if (carried && lane == 0) pairs_insert(mem, log2c, carried, carried_n, carried_n * area_unit);
}

// ---- finish ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pow2ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;                             // bounded: n <= 8192
  return p;
}

// LDS: max(2, pow2ceil(max_pairs)) 64-bit words, given at the launch.
__global__ __launch_bounds__(kFinishThreads) void finish_kernel(const uint64_t* __restrict__ tables, int log2c, int max_pairs,
                                                                int32_t* __restrict__ count, int64_t* __restrict__ pairs) {
  extern __shared__ uint64_t sorted[];
  __shared__ int occupied;
  const int tid = (int)threadIdx.x;
  const int64_t item = blockIdx.x, C = (int64_t)1 << log2c;
  const Settled mem{(gptr<const uint64_t>)(tables + item * pairs_table_words(log2c))};
  const int cap = max(2, pow2ceil(max_pairs));
  if (tid == 0) occupied = 0;
  __syncthreads();
  for (int64_t s = tid; s < C; s += kFinishThreads) {   // bounded by C
    const uint64_t k = mem.load(s);
    if (k) {
      const int at = atomicAdd(&occupied, 1);       // the order is arbitrary; the sort below undoes it
      if (at < cap) sorted[at] = k;
    }
  }
  __syncthreads();
  const int n = occupied;
  gptr<int64_t> const rows = (gptr<int64_t>)(pairs + item * (int64_t)max_pairs * 4);
  if (mem.load(3 * C) != 0 || n > max_pairs) {      // (block-uniform) the item overflows: no partial table
    for (int i = tid; i < max_pairs * 4; i += kFinishThreads) rows[i] = 0;
    if (tid == 0) count[item] = -1;
    return;
  }
  const int n2 = max(2, pow2ceil(n));               // <= cap
  for (int i = n + tid; i < n2; i += kFinishThreads) sorted[i] = ~0ull;   // above every key
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)                 // a bitonic network over n2 words: fixed, bounded by log2(n2)^2 stages
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += kFinishThreads) {
        const int o = i ^ j;
        if (o > i) {
          const uint64_t x = sorted[i], y = sorted[o];
          if ((x > y) == ((i & k) == 0)) sorted[i] = y, sorted[o] = x;
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < max_pairs; i += kFinishThreads) {
    int64_t ka = 0, kb = 0, points = 0, units = 0;
    if (i < n) {
      const uint64_t key = sorted[i];
      const int64_t s = pairs_find(mem, log2c, key);   // bounded by C; the key is in the table
      if (s >= 0) ka = (int64_t)(key >> 32), kb = (int64_t)(key & 0xffffffffull), points = (int64_t)mem.load(C + s), units = (int64_t)mem.load(2 * C + s);
    }
    rows[4 * i] = ka, rows[4 * i + 1] = kb, rows[4 * i + 2] = points, rows[4 * i + 3] = units;
  }
  if (tid == 0) count[item] = n;
}

bool sizes_ok(int64_t n_items, int max_pairs) { return n_items >= 0 && max_pairs >= 1 && max_pairs <= kPairsMaxPairs; }

size_t workspace_bytes(int64_t n_items, int max_pairs) {
  return (size_t)(n_items * pairs_table_words(pairs_log2c(max_pairs)) * 8);
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_object_matches_workspace_bytes(int64_t n_items, int max_pairs) {
  if (!sizes_ok(n_items, max_pairs) || n_items > 0x7fffffff) return 0;
  return workspace_bytes(n_items, max_pairs);
}

extern "C" int aurora_hip_object_matches(const int32_t* labels_a, const int32_t* labels_b, int64_t n_items, int n_lat, int n_lon,
                                         const int64_t* unit, int max_objects_a, int max_objects_b, int max_pairs, int32_t* count,
                                         int64_t* pairs, void* workspace, size_t workspace_size, void* stream) {
  AURORA_CHECK_ARG(n_items >= 0 && n_lat >= 1 && n_lon >= 1, "object_matches: bad sizes (%lld items, grid %d x %d)",
                   (long long)n_items, n_lat, n_lon);
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= 0x7ffffffell, "object_matches: a grid of %d x %d points is beyond the 2^31 - 2 of an int32 label map",
                   n_lat, n_lon);
  AURORA_CHECK_ARG(max_objects_a >= 1 && max_objects_b >= 1, "object_matches: max_objects must be at least 1, got %d and %d",
                   max_objects_a, max_objects_b);
  AURORA_CHECK_ARG(max_pairs >= 1 && max_pairs <= kPairsMaxPairs, "object_matches: max_pairs must be 1 to %d, got %d",
                   kPairsMaxPairs, max_pairs);
  if (n_items == 0) return AURORA_OK;
  AURORA_CHECK_ARG(labels_a && labels_b && unit && count && pairs && workspace,
                   "object_matches: null label map, unit, output or workspace pointer");
  AURORA_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)pairs & 7) == 0 && ((uintptr_t)unit & 7) == 0 &&
                       ((uintptr_t)labels_a & 3) == 0 && ((uintptr_t)labels_b & 3) == 0 && ((uintptr_t)count & 3) == 0,
                   "object_matches: unit, pairs and workspace must be 8-byte aligned, the label maps and count 4-byte aligned");
  const int64_t groups = (n_items * n_lat + kWaves - 1) / kWaves;
  AURORA_CHECK_ARG(groups <= 0x7fffffff && n_items <= 0x7fffffff, "object_matches: too many items for one launch (%lld items x %d rows)",
                   (long long)n_items, n_lat);
  const size_t need = workspace_bytes(n_items, max_pairs);
  AURORA_CHECK_ARG(workspace_size >= need, "object_matches: the workspace has %zu bytes, %zu are needed", workspace_size, need);
  const int log2c = pairs_log2c(max_pairs);
  int cap = 2;
  while (cap < max_pairs) cap <<= 1;
  const size_t lds = (size_t)cap * 8;                // at most 64 KiB, beside the kernel's own counter
  once_per_device([] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              kPairsMaxPairs * 8);
  });
  uint64_t* const tables = (uint64_t*)workspace;
  const hipStream_t s = as_stream(stream);
  const int64_t n_words = n_items * pairs_table_words(log2c);
  const unsigned zero_groups = (unsigned)(n_words / kThreads + 1 < 4096 ? n_words / kThreads + 1 : 4096);
  int code;
  hipLaunchKernelGGL(zero_kernel, dim3(zero_groups), dim3(kThreads), 0, s, tables, n_words);
  if ((code = check_launch("object_matches (zero)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)groups), dim3(kThreads), 0, s, labels_a, labels_b, n_items, n_lat, n_lon,
                     unit, max_objects_a, max_objects_b, log2c, tables);
  if ((code = check_launch("object_matches (accumulate)")) != AURORA_OK) return code;
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)n_items), dim3(kFinishThreads), lds, s, (const uint64_t*)tables, log2c,
                     max_pairs, count, pairs);
  return check_launch("object_matches (finish)");
}
