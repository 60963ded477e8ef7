// Per-point statistics over a SEQUENCE of planes on the device (aurora_amd.FieldStats: mean, spread, RMS, minimum and
// maximum with the sample that reached them, exceedance counts and run lengths as maps).
//
// Every scorer next to this file reduces a plane over SPACE to a few numbers.  This one reduces over samples (the steps
// of a roll-out, the members of an ensemble, forecast - truth pairs) and keeps the map: a point's state (36 + 12 T bytes,
// include/aurora_hip.h has the table) is read once, updated by the call's n_samples values of that point in sample order
// in registers, and written once.  Nothing is reduced across threads, so there is no tree to fix: a point's state
// depends on its own samples alone -- not on n_planes, on the other planes, on how the samples are grouped into calls
// (the one `update` below runs once per sample whether a call brings 1 or 64), or on pointer alignment (planes.h).
//
// The sums are SHIFTED: d = v - origin with origin the point's first valid value, so a pressure of 1e5 Pa that varies by
// a few hundred keeps its digits (sum d^2 - (sum d)^2 / n cancels at the size of the variation, not of the raw value).
//
// One workgroup = one chunk of 1024 consecutive points of one plane, a lane = four consecutive points (load4 / store4 of
// planes.h).  The samples are loaded four at a time, then applied one after the other.  The kernel is a template on a
// threshold-count bucket (0, 1, 2, 4, 8) with a wave-uniform `t < T` guard, so the per-threshold state has compile-time
// register indices.  The global index of the call's first sample is read from device memory; a second one-thread launch
// advances it, so a captured call replays with the right indices.
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 4;
constexpr int kChunk = kThreads * kPerLane;     // points of a workgroup
constexpr int kGroup = 4;                       // samples in flight
constexpr int kMaxSamples = 64;
constexpr int kMaxThresholds = 8;


struct State {
  int32_t* n;
  float* origin;
  double *s1, *s2;
  float *vmin, *vmax;
  int32_t *argmin, *argmax, *exceed, *run, *longest;
};
struct Args {
  const float* const* planes;
  const float* const* ref;
  const float* const* second;
  const float* thresholds;
  const int64_t* sample_index;
  int64_t n_points;
  int n_samples, n_planes, n_chunks, T, below;
  State st;
};

template <int TB> struct Point {
  int n;
  float origin;
  double s1, s2;
  float vmin, vmax;
  int amin, amax;
  int ex[TB ? TB : 1], run[TB ? TB : 1], lg[TB ? TB : 1];
};

// One sample of one point.  x: the value (the first operand a with a second operand b), r: the reference.  A sample with
// a non-finite x, b or r leaves the state as it is.
template <int TB>
__device__ __forceinline__ void update(Point<TB>& p, float x, float b, float r, bool has_b, bool has_r,
                                       const float (&thr)[TB ? TB : 1], int T, bool below, int index) {
  bool ok = __builtin_isfinite(x);
  if (has_b) {
    ok = ok && __builtin_isfinite(b);
    x = (float)wind_speed_f64(x, b);
    ok = ok && __builtin_isfinite(x);
  }
  if (has_r) ok = ok && __builtin_isfinite(r);
  if (!ok) return;
  const double v = has_r ? (double)x - (double)r : (double)x;
  const float w = (float)v;
  const bool first = p.n == 0;
  if (first) p.origin = w;
  const double d = v - (double)p.origin;
  p.s1 += d;
  p.s2 = __builtin_fma(d, d, p.s2);
  if (first || w < p.vmin) p.vmin = w, p.amin = index;
  if (first || w > p.vmax) p.vmax = w, p.amax = index;
#pragma unroll
  for (int t = 0; t < TB; ++t)
    if (t < T) {
      const bool ev = below ? w <= thr[t] : w >= thr[t];        // (a NaN threshold compares false: no event)
      p.ex[t] += ev ? 1 : 0;
      p.run[t] = ev ? p.run[t] + 1 : 0;
      p.lg[t] = max(p.lg[t], p.run[t]);
    }
  p.n += 1;
}

#define AURORA_FS_LOAD(V, array, field)                                 \
  {                                                                     \
    V tmp[kPerLane];                                                    \
    load4<V>(array, s0, s_last, vec_state, tmp);                        \
    _Pragma("unroll") for (int k = 0; k < kPerLane; ++k) pt[k].field = tmp[k]; \
  }
#define AURORA_FS_STORE(V, array, field)                                \
  {                                                                     \
    V tmp[kPerLane];                                                    \
    _Pragma("unroll") for (int k = 0; k < kPerLane; ++k) tmp[k] = pt[k].field; \
    store4<V>(array, s0, cnt, vec_state, tmp);                          \
  }

template <int TB> __global__ __launch_bounds__(kThreads) void field_stats_kernel(const Args a) {
  const int plane = (int)(blockIdx.x / (unsigned)a.n_chunks), chunk = (int)(blockIdx.x % (unsigned)a.n_chunks);
  const int S = a.n_samples, T = a.T;
  const int64_t i0 = (int64_t)chunk * kChunk + (int64_t)threadIdx.x * kPerLane;   // first point of the lane, in the plane
  if (i0 >= a.n_points) return;
  const int64_t left = a.n_points - i0;
  const int cnt = left < kPerLane ? (int)left : kPerLane;
  const int64_t last = a.n_points - 1;
  const bool below = a.below != 0;
  const int index0 = (int)*a.sample_index;

  // (wave-uniform: the plane's pointers)
  const float* const R = a.ref ? a.ref[plane] : nullptr;
  const bool has_r = R != nullptr;
  const bool has_b = a.second != nullptr && a.second[plane] != nullptr;
  uintptr_t bits = (uintptr_t)R | (uintptr_t)((a.n_points & 3) * 4);   // the quad rule over every input pointer of the plane
  for (int s = 0; s < S; ++s) {
    bits |= (uintptr_t)a.planes[(int64_t)s * a.n_planes + plane];
    if (has_b) bits |= (uintptr_t)a.second[(int64_t)s * a.n_planes + plane];
  }
  const bool vec_in = (bits & 15) == 0;
  const State& st = a.st;
  const bool vec_state =
      (a.n_points & 3) == 0 && ((((uintptr_t)st.n | (uintptr_t)st.origin | (uintptr_t)st.s1 | (uintptr_t)st.s2 | (uintptr_t)st.vmin |
                                  (uintptr_t)st.vmax | (uintptr_t)st.argmin | (uintptr_t)st.argmax | (uintptr_t)st.exceed |
                                  (uintptr_t)st.run | (uintptr_t)st.longest) & 15) == 0);

  float thr[TB ? TB : 1] = {};
#pragma unroll
  for (int t = 0; t < TB; ++t)
    if (t < T) thr[t] = a.thresholds[(int64_t)plane * T + t];

  // ---- the state of the lane's four points ---------------------------------------------------------------------------
  const int64_t s0 = (int64_t)plane * a.n_points + i0;           // in the [plane][point] arrays
  const int64_t s_last = (int64_t)plane * a.n_points + last;
  Point<TB> pt[kPerLane];
  AURORA_FS_LOAD(int32_t, st.n, n)
  AURORA_FS_LOAD(float, st.origin, origin)
  AURORA_FS_LOAD(double, st.s1, s1)
  AURORA_FS_LOAD(double, st.s2, s2)
  AURORA_FS_LOAD(float, st.vmin, vmin)
  AURORA_FS_LOAD(float, st.vmax, vmax)
  AURORA_FS_LOAD(int32_t, st.argmin, amin)
  AURORA_FS_LOAD(int32_t, st.argmax, amax)
#pragma unroll
  for (int t = 0; t < TB; ++t) {
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) pt[k].ex[t] = pt[k].run[t] = pt[k].lg[t] = 0;
    if (t < T) {
      const int64_t off = ((int64_t)plane * T + t) * a.n_points - (int64_t)plane * a.n_points;   // [plane][t][point]
      AURORA_FS_LOAD(int32_t, st.exceed + off, ex[t])
      AURORA_FS_LOAD(int32_t, st.run + off, run[t])
      AURORA_FS_LOAD(int32_t, st.longest + off, lg[t])
    }
  }
  float r[kPerLane] = {};
  if (has_r) load4<float>(R, i0, last, vec_in, r);

  // ---- the samples, in order -----------------------------------------------------------------------------------------
  for (int g0 = 0; g0 < S; g0 += kGroup) {
    float x[kGroup][kPerLane], b[kGroup][kPerLane];
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) x[g][k] = b[g][k] = 0.f;
      if (g0 + g < S) {
        load4<float>(a.planes[(int64_t)(g0 + g) * a.n_planes + plane], i0, last, vec_in, x[g]);
        if (has_b) load4<float>(a.second[(int64_t)(g0 + g) * a.n_planes + plane], i0, last, vec_in, b[g]);
      }
    }
#pragma unroll
    for (int g = 0; g < kGroup; ++g)
      if (g0 + g < S) {
#pragma unroll
        for (int k = 0; k < kPerLane; ++k)
          update<TB>(pt[k], x[g][k], b[g][k], r[k], has_b, has_r, thr, T, below, index0 + g0 + g);
      }
  }

  AURORA_FS_STORE(int32_t, st.n, n)
  AURORA_FS_STORE(float, st.origin, origin)
  AURORA_FS_STORE(double, st.s1, s1)
  AURORA_FS_STORE(double, st.s2, s2)
  AURORA_FS_STORE(float, st.vmin, vmin)
  AURORA_FS_STORE(float, st.vmax, vmax)
  AURORA_FS_STORE(int32_t, st.argmin, amin)
  AURORA_FS_STORE(int32_t, st.argmax, amax)
#pragma unroll
  for (int t = 0; t < TB; ++t)
    if (t < T) {
      const int64_t off = ((int64_t)plane * T + t) * a.n_points - (int64_t)plane * a.n_points;
      AURORA_FS_STORE(int32_t, st.exceed + off, ex[t])
      AURORA_FS_STORE(int32_t, st.run + off, run[t])
      AURORA_FS_STORE(int32_t, st.longest + off, lg[t])
    }
}
#undef AURORA_FS_LOAD
#undef AURORA_FS_STORE

// After the main launch, in stream order: the next call's first sample index.
__global__ void field_stats_advance_kernel(int64_t* sample_index, int n_samples) { *sample_index += n_samples; }

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_field_stats_update(const float* const* sample_planes, const float* const* ref_planes,
                                             const float* const* second_planes, int n_samples, int n_planes, int64_t n_points,
                                             const float* thresholds, int n_thresholds, int below, int64_t* sample_index,
                                             int32_t* n, float* origin, double* s1, double* s2, float* vmin, float* vmax,
                                             int32_t* argmin, int32_t* argmax, int32_t* exceed, int32_t* run, int32_t* longest,
                                             void* stream) {
  AURORA_CHECK_ARG(n_samples >= 1 && n_samples <= kMaxSamples, "field_stats_update: n_samples must be in 1..%d, got %d",
                   kMaxSamples, n_samples);
  AURORA_CHECK_ARG(n_thresholds >= 0 && n_thresholds <= kMaxThresholds,
                   "field_stats_update: n_thresholds must be in 0..%d, got %d", kMaxThresholds, n_thresholds);
  AURORA_CHECK_ARG(n_planes >= 0 && n_points >= 1, "field_stats_update: bad sizes (planes %d, points %lld)", n_planes,
                   (long long)n_points);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(sample_planes && sample_index, "field_stats_update: null plane array or sample index pointer");
  AURORA_CHECK_ARG(n && origin && s1 && s2 && vmin && vmax && argmin && argmax, "field_stats_update: null state pointer");
  AURORA_CHECK_ARG(n_thresholds == 0 || (thresholds && exceed && run && longest),
                   "field_stats_update: %d thresholds but a null threshold or threshold state pointer", n_thresholds);
  AURORA_CHECK_ARG((((uintptr_t)s1 | (uintptr_t)s2 | (uintptr_t)sample_index) & 7) == 0,
                   "field_stats_update: s1, s2 and the sample index must be 8-byte aligned");
  AURORA_CHECK_ARG((((uintptr_t)n | (uintptr_t)origin | (uintptr_t)vmin | (uintptr_t)vmax | (uintptr_t)argmin | (uintptr_t)argmax |
                     (uintptr_t)exceed | (uintptr_t)run | (uintptr_t)longest | (uintptr_t)thresholds) & 3) == 0,
                   "field_stats_update: the state arrays and thresholds must be 4-byte aligned");
  const int64_t n_chunks = (n_points + kChunk - 1) / kChunk;
  AURORA_CHECK_ARG(n_chunks <= 0x7fffffff && n_chunks * n_planes <= 0x7fffffff,
                   "field_stats_update: too many points for one launch (%d planes x %lld chunks)", n_planes, (long long)n_chunks);
  Args a;
  a.planes = sample_planes, a.ref = ref_planes, a.second = second_planes, a.thresholds = thresholds;
  a.sample_index = sample_index, a.n_points = n_points, a.n_samples = n_samples, a.n_planes = n_planes;
  a.n_chunks = (int)n_chunks, a.T = n_thresholds, a.below = below;
  a.st = State{n, origin, s1, s2, vmin, vmax, argmin, argmax, exceed, run, longest};
  const dim3 grid((unsigned)(n_chunks * n_planes)), block(kThreads);
  const hipStream_t q = as_stream(stream);
  if (n_thresholds == 0) hipLaunchKernelGGL(field_stats_kernel<0>, grid, block, 0, q, a);
  else if (n_thresholds == 1) hipLaunchKernelGGL(field_stats_kernel<1>, grid, block, 0, q, a);
  else if (n_thresholds == 2) hipLaunchKernelGGL(field_stats_kernel<2>, grid, block, 0, q, a);
  else if (n_thresholds <= 4) hipLaunchKernelGGL(field_stats_kernel<4>, grid, block, 0, q, a);
  else hipLaunchKernelGGL(field_stats_kernel<8>, grid, block, 0, q, a);
  const int code = check_launch("field_stats_update");
  if (code != AURORA_OK) return code;
  hipLaunchKernelGGL(field_stats_advance_kernel, dim3(1), dim3(1), 0, q, sample_index, n_samples);
  return check_launch("field_stats_update (advance)");
}
