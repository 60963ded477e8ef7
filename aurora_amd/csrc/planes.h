// Plane access and fixed-order reduction shared by the verification kernels (scores, region_scores, conditional_scores,
// ensemble_scores, ensemble_quantiles, probability_scores, event_scores, field_stats, spectra, diagnostics, objects,
// field_quantiles) and the
// two regrids.  Three contracts live here and nowhere else: the quad rule, the reduction tree (its one kernel and its launch
// are in planes.hip) and the wind-speed expression.  A plane is n_lat x n_lon fp32, row-major, in global memory.
#pragma once

#include "common.h"

namespace aurora {

// A pointer known to be global memory: said so, the loads and stores are global_*, not flat_*.
template <typename T> using gptr = __attribute__((address_space(1))) T*;

// ---- the quad rule ------------------------------------------------------------------------------------------------------
// A lane takes four consecutive elements: the columns 4 q .. 4 q + 3 of a row (a quad), or the points i0 .. i0 + 3 of a flat
// plane.  Where the row length (n_lon, or the number of points) is a multiple of 4 and EVERY pointer of the plane that is
// read or written this way is 16-byte aligned, that is one 16-byte access per pointer; otherwise it is four 4-byte ones,
// with loads past the end clamped to the last element (loaded, never used) and stores past the end skipped.  Either way
// the same elements arrive in the same order, so no result depends on the alignment of the plane pointers.  The choice
// is wave-uniform: it is made from the plane's pointers and its size alone.

// May the quads of a plane's rows be accessed as 16 bytes?  planes: every pointer of the plane.  (A kernel whose plane has
// a table of member pointers folds them in a loop of its own -- bits = first | (n_lon & 3); bits |= member ...; (bits & 15)
// == 0 -- which is this test: a loop inlined from here would be laid out differently from the loops those kernels have.)
template <typename... P> __device__ __forceinline__ bool quads_aligned(int n_lon, const P&... planes) {
  return (n_lon & 3) == 0 && (((uintptr_t)0 | ... | (uintptr_t)planes) & 15) == 0;
}

// The quad `item` of a row: columns 4 item .. 4 item + 3 (VEC), or the columns col[0 .. 3], which the caller has clamped into
// the row (it also owns the guard that says which of the four are in the row).
template <bool VEC, typename C>
__device__ __forceinline__ f32x4 load_quad(gptr<const float> row, int item, const C (&col)[4]) {
  if (VEC) return ((gptr<const f32x4>)row)[item];
  return f32x4{row[col[0]], row[col[1]], row[col[2]], row[col[3]]};
}

// 16 bytes of V: four 4-byte or two 8-byte elements.
template <typename V> struct Vec16 { typedef V type __attribute__((ext_vector_type(16 / sizeof(V)))); };

// Four consecutive elements of a flat plane from element i0 of `base`; elements past `last` are clamped loads, and only
// the first `cnt` of the four are stored.  vec: quads_aligned, or the same test on the pointers at hand.
template <typename V>
__device__ __forceinline__ void load4(const V* base, int64_t i0, int64_t last, bool vec, V (&out)[4]) {
  const gptr<const V> g = (gptr<const V>)base;
  typedef typename Vec16<V>::type vec_t;
  constexpr int kPer = 16 / (int)sizeof(V);
  if (vec) {
#pragma unroll
    for (int j = 0; j < 4 / kPer; ++j) {
      const vec_t q = ((gptr<const vec_t>)(g + i0))[j];
#pragma unroll
      for (int k = 0; k < kPer; ++k) out[j * kPer + k] = q[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = g[i0 + k < last ? i0 + k : last];
  }
}
template <typename V>
__device__ __forceinline__ void store4(V* base, int64_t i0, int cnt, bool vec, const V (&in)[4]) {
  const gptr<V> g = (gptr<V>)base;
  typedef typename Vec16<V>::type vec_t;
  constexpr int kPer = 16 / (int)sizeof(V);
  if (vec) {
#pragma unroll
    for (int j = 0; j < 4 / kPer; ++j) {
      vec_t q;
#pragma unroll
      for (int k = 0; k < kPer; ++k) q[k] = in[j * kPer + k];
      ((gptr<vec_t>)(g + i0))[j] = q;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) g[i0 + k] = in[k];
  }
}

// ---- the reduction tree -------------------------------------------------------------------------------------------------
// A plane's fp64 sums are repeatable bit for bit and depend on nothing but its own values, n_lat, n_lon and the chunk size
// -- not on the other planes of the call and (by the quad rule) not on pointer alignment -- because the tree is fixed:
//   lane      items (quads or columns) lane, lane + 64, ... of a row, over the rows wave, wave + W, ... of the workgroup's
//             row chunk (W waves; a chunk is chunk_rows consecutive rows);
//   wave      xor butterfly over the 64 lanes (wave_sum_f64);
//   workgroup the W waves' sums through LDS, added in wave order (sum_waves): one partial per (plane, row chunk);
//   plane     a second launch (finish_partials below; ensemble_scores.hip folds its histogram in a finish kernel of its own,
//             by the same rule) adds the partials of a plane in chunk order: v = partial 0, then v += partial 1, 2, ...
// No floating-point atomics, no tickets: the second launch is the hand-off.
constexpr int kSumSlots = 8;                    // fp64 sums per plane, per partial and per wave
// Target size of a row chunk (elements of one input) of scores and region_scores, whose sums must agree; conditional_scores
// and ensemble_scores have their own.
#ifndef AURORA_SCORES_CHUNK_ELEMS               // (a probe build may set it: AURORA_BUILD_FLAGS=-DAURORA_SCORES_CHUNK_ELEMS=...)
#define AURORA_SCORES_CHUNK_ELEMS 40960
#endif
constexpr int kScoresChunkElems = AURORA_SCORES_CHUNK_ELEMS;

// Rows per chunk: a function of n_lon and the target chunk size (elements of one input) alone, never of n_planes; at least
// a row per wave.  Chunks per plane: of n_lat besides.
__host__ __device__ constexpr int chunk_rows(int n_lon, int chunk_elems, int waves) {
  const int r = (chunk_elems + n_lon - 1) / n_lon;
  return r < waves ? waves : r;
}
inline int64_t chunks_per_plane(int n_lat, int n_lon, int chunk_elems, int waves) {
  const int r = chunk_rows(n_lon, chunk_elems, waves);
  return ((int64_t)n_lat + r - 1) / r;
}

// The launch of a kernel that reduces by row chunks: one workgroup per (plane, row chunk), `groups` of them, and as many
// partials in the workspace.  Nothing to do (groups 0) where a size is below 1.
struct ChunkPlan {
  int64_t n_chunks, groups;                     // chunks per plane; n_planes x n_chunks
};
inline ChunkPlan chunk_plan(int n_planes, int n_lat, int n_lon, int chunk_elems, int waves) {
  if (n_planes < 1 || n_lat < 1 || n_lon < 1) return {0, 0};
  const int64_t n_chunks = chunks_per_plane(n_lat, n_lon, chunk_elems, waves);
  return {n_chunks, n_chunks * n_planes};
}
// The plan of the entry `name`, or AURORA_E_ARG and its message: sizes that are no grid, more workgroups than one launch takes.
int plan_chunks(const char* name, int n_planes, int n_lat, int n_lon, int chunk_elems, int waves, ChunkPlan* plan);

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// Slot s of the workgroup: lane 0 of wave k has stored its wave's sum in s_wave[k][s], and a barrier has passed.  (S slots
// per wave: kSumSlots, or bins x slots where a kernel keeps its sums per bin.)
template <int W, int S>
__device__ __forceinline__ double sum_waves(const double (&s_wave)[W][S], int s) {
  double v = s_wave[0][s];
#pragma unroll
  for (int k = 1; k < W; ++k) v += s_wave[k][s];
  return v;
}

// The plane stage: sums[plane][j] = partial[plane][0][j] + partial[plane][1][j] + ... for the n_out sums j of every plane, as
// the second launch of the entry `name` on `stream`: the launch's code, with "<name> (finish)" in the message of a failure.
int finish_partials(const char* name, const double* partial, int n_planes, int n_chunks, int n_out, double* sums,
                    hipStream_t stream);

// ---- the wind-speed expression --------------------------------------------------------------------------------------------
// |(u, v)| in fp64 from fp32 components: both squares are exact, so the sum rounds once and the root once.  FieldStats over
// a derived wind speed and aurora_amd.diagnostics agree bit for bit because both call this and round to fp32 once.
__device__ __forceinline__ double wind_speed_f64(float u, float v) {
  const double a = (double)u, b = (double)v;
  return __builtin_sqrt(__builtin_fma(a, a, b * b));
}

}  // namespace aurora
