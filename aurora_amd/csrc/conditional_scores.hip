// Conditional verification sums on the device (aurora_amd.conditional_scores: error by truth bin, tail RMSE / bias / MAE).
//
// For every plane (one variable, level and batch element; n_lat x n_lon fp32, row-major) the prediction p, the truth t and,
// if given, a centre map c and a scale map s are read ONCE.  Every valid point falls into one of n_edges + 1 bins by the
// rule of include/aurora_hip.h -- a = (double)v - (double)c with v the binned field, bin = #{j : a >= (double)e_j * (double)s}
// -- and the five fp64 sums of aurora_hip_scores' first five slots (count, w, w d, w d^2, w |d| with d = p - t) are kept
// per bin.
//
// A lane takes quads of columns (the quad rule of planes.h) and keeps the sums of EVERY bin in registers, indexed by
// unrolled constants only; a point is applied to every bin by select: its term w d enters the bin it falls into and +0
// enters the others.  x + (+0) = x, so a bin's sums are the sums over the points of that bin alone, in the order of the
// reduction tree of planes.h: they do not depend on how many other edges the call has or on which instantiation ran.
// That only holds while every instantiation rounds alike, so contraction is off in this file's arithmetic and the one
// fused multiply-add that is wanted is written out.  finish_partials ((n_edges + 1) x 5 sums to a chunk) is the second launch
// of the tree.
#include <type_traits>

#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlots = 5;                       // count, w, w d, w d^2, w |d|
constexpr int kMaxEdges = 8;
#ifndef AURORA_CONDITIONAL_CHUNK_ELEMS          // (a probe build may set it: AURORA_BUILD_FLAGS=-DAURORA_CONDITIONAL_CHUNK_ELEMS=...)
#define AURORA_CONDITIONAL_CHUNK_ELEMS 40960
#endif
constexpr int kChunkElems = AURORA_CONDITIONAL_CHUNK_ELEMS;   // target size of a row chunk (elements of one input)

template <int kE> struct Acc {
  double s2[kE + 1], s3[kE + 1], s4[kE + 1];
  int n[kE + 1];                                // valid points of the current row, per bin
};

// One point into every bin.  thr[j] = (double)e_j, NaN for an edge the plane does not have (never passed).  An invalid
// point has bin -1: it is in no bin, and its p and t are replaced by 0 so that d is finite.
template <int kE, bool kCentre, bool kScale>
__device__ __forceinline__ void point(Acc<kE>& acc, const double (&thr)[kE], double w, bool by_pred, float pf, float tf,
                                      float cf, float sf, bool in_row) {
#pragma clang fp contract(off)
  bool ok = in_row && __builtin_isfinite(pf) && __builtin_isfinite(tf);
  if (kCentre) ok = ok && __builtin_isfinite(cf);
  if (kScale) ok = ok && __builtin_isfinite(sf) && sf >= 0.f;
  const double p = (double)(ok ? pf : 0.f), t = (double)(ok ? tf : 0.f);
  const double v = by_pred ? p : t;
  const double a = kCentre ? v - (double)cf : v;
  const double sg = (double)sf;
  int bin = 0;
#pragma unroll
  for (int j = 0; j < kE; ++j) {
    const double edge = kScale ? thr[j] * sg : thr[j];         // ONE product, alone on its side of the comparison
    bin += a >= edge ? 1 : 0;
  }
  bin = ok ? bin : -1;
  const double d = p - t;
  const double wd = w * d;
#pragma unroll
  for (int k = 0; k <= kE; ++k) {
    const bool in = bin == k;
    const double wdk = in ? wd : 0.0;                          // +0 for every bin but the point's own
    acc.n[k] += in ? 1 : 0;
    acc.s2[k] = acc.s2[k] + wdk;
    acc.s3[k] = __builtin_fma(wdk, d, acc.s3[k]);              // (+0) d = +-0: leaves s3 as it is
    acc.s4[k] = acc.s4[k] + __builtin_fabs(wdk);
  }
  __builtin_amdgcn_sched_barrier(0);   // a point at a time: interleaving the four points of a quad costs a wave of occupancy
}

// One workgroup = one row chunk of one plane; partial[((plane * n_chunks + chunk) * (n_edges + 1) + bin) * 5 + slot].
template <int kE, bool kCentre, bool kScale>
__global__ __launch_bounds__(kThreads) void conditional_kernel(const float* const* __restrict__ pred_planes,
                                                               const float* const* __restrict__ truth_planes,
                                                               const float* const* __restrict__ centre_planes,
                                                               const float* const* __restrict__ scale_planes, int n_lat,
                                                               int n_lon, int n_chunks, const float* __restrict__ edges,
                                                               int n_edges, int by_pred, const double* __restrict__ row_w,
                                                               double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double s_wave[kWaves][(kE + 1) * kSlots];
  const int plane = (int)(blockIdx.x / (unsigned)n_chunks), chunk = (int)(blockIdx.x % (unsigned)n_chunks);
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const gptr<const float> P = (gptr<const float>)pred_planes[plane];
  const gptr<const float> T = (gptr<const float>)truth_planes[plane];
  const gptr<const float> C = kCentre ? (gptr<const float>)centre_planes[plane] : P;   // an absent array is never read
  const gptr<const float> S = kScale ? (gptr<const float>)scale_planes[plane] : P;
  const bool vec = quads_aligned(n_lon, P, T, C, S);
  const bool pred_binned = by_pred != 0;
  const int n_quads = (n_lon + 3) >> 2;
  const int rows = chunk_rows(n_lon, kChunkElems, kWaves);
  const int r_begin = chunk * rows, r_end = min(r_begin + rows, n_lat);

  double thr[kE];
#pragma unroll
  for (int j = 0; j < kE; ++j)
    thr[j] = j < n_edges ? (double)edges[(int64_t)plane * n_edges + j] : (double)__builtin_nanf("");

  Acc<kE> acc;
  double s1[kE + 1];
  int count[kE + 1];
#pragma unroll
  for (int k = 0; k <= kE; ++k) acc.s2[k] = acc.s3[k] = acc.s4[k] = s1[k] = 0.0, acc.n[k] = count[k] = 0;

  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r = r_begin + wave; r < r_end; r += kWaves) {       // wave-uniform: w is one scalar load per row
    const double w = row_w[r];
    const int64_t row0 = (int64_t)r * n_lon;
#pragma unroll
    for (int k = 0; k <= kE; ++k) acc.n[k] = 0;
    if (vec) {                                                 // the quad rule, column by column
      const gptr<const f32x4> p4 = (gptr<const f32x4>)(P + row0), t4 = (gptr<const f32x4>)(T + row0),
                              c4 = (gptr<const f32x4>)(C + row0), s4 = (gptr<const f32x4>)(S + row0);
      for (int q = lane; q < n_quads; q += 64) {
        const f32x4 p = p4[q], t = t4[q], c = kCentre ? c4[q] : zero4, s = kScale ? s4[q] : zero4;
        point<kE, kCentre, kScale>(acc, thr, w, pred_binned, p.x, t.x, c.x, s.x, true);
        point<kE, kCentre, kScale>(acc, thr, w, pred_binned, p.y, t.y, c.y, s.y, true);
        point<kE, kCentre, kScale>(acc, thr, w, pred_binned, p.z, t.z, c.z, s.z, true);
        point<kE, kCentre, kScale>(acc, thr, w, pred_binned, p.w, t.w, c.w, s.w, true);
      }
    } else {
      for (int q = lane; q < n_quads; q += 64) {                // the same points in the same order, a column at a time
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
          const int col = min(4 * q + k, n_lon - 1);           // clamped: the load is in the row, the guard is in_row
          point<kE, kCentre, kScale>(acc, thr, w, pred_binned, P[row0 + col], T[row0 + col], kCentre ? C[row0 + col] : 0.f,
                                     kScale ? S[row0 + col] : 0.f, 4 * q + k < n_lon);
        }
      }
    }
#pragma unroll
    for (int k = 0; k <= kE; ++k) {
      count[k] += acc.n[k];
      s1[k] = __builtin_fma(w, (double)acc.n[k], s1[k]);
    }
  }

#pragma unroll
  for (int k = 0; k <= kE; ++k) {
    if (k <= n_edges) {                                        // wave-uniform: the plane has n_edges + 1 bins
      const double sums[kSlots] = {(double)count[k], s1[k], acc.s2[k], acc.s3[k], acc.s4[k]};
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        const double v = wave_sum_f64(sums[s]);
        if (lane == 0) s_wave[wave][k * kSlots + s] = v;
      }
    }
  }
  __syncthreads();
  const int n_out = (n_edges + 1) * kSlots;                    // <= 45 < kThreads
  if ((int)threadIdx.x < n_out)
    partial[(int64_t)blockIdx.x * n_out + threadIdx.x] = sum_waves(s_wave, (int)threadIdx.x);
}

template <int kE, bool kCentre, bool kScale>
void launch(unsigned groups, hipStream_t stream, const float* const* pred_planes, const float* const* truth_planes,
            const float* const* centre_planes, const float* const* scale_planes, int n_lat, int n_lon, int n_chunks,
            const float* edges, int n_edges, int by_pred, const double* row_w, double* partial) {
  hipLaunchKernelGGL((conditional_kernel<kE, kCentre, kScale>), dim3(groups), dim3(kThreads), 0, stream, pred_planes,
                     truth_planes, centre_planes, scale_planes, n_lat, n_lon, n_chunks, edges, n_edges, by_pred, row_w, partial);
}

template <int kE, typename... A> void launch_maps(bool centre, bool scale, A... args) {
  if (centre && scale) launch<kE, true, true>(args...);
  else if (centre) launch<kE, true, false>(args...);
  else if (scale) launch<kE, false, true>(args...);
  else launch<kE, false, false>(args...);
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_conditional_scores_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_edges) {
  if (n_edges < 1 || n_edges > kMaxEdges) return 0;
  return (size_t)chunk_plan(n_planes, n_lat, n_lon, kChunkElems, kWaves).groups * (size_t)(n_edges + 1) * kSlots * sizeof(double);
}

extern "C" int aurora_hip_conditional_scores(const float* const* pred_planes, const float* const* truth_planes,
                                             const float* const* centre_planes, const float* const* scale_planes,
                                             int n_planes, int n_lat, int n_lon, const float* edges, int n_edges, int by_pred,
                                             const double* row_w, double* sums, void* workspace, void* stream) {
  ChunkPlan plan;
  if (const int code = plan_chunks("conditional_scores", n_planes, n_lat, n_lon, kChunkElems, kWaves, &plan)) return code;
  AURORA_CHECK_ARG(n_edges >= 1 && n_edges <= kMaxEdges, "conditional_scores: 1 to %d edges, got %d", kMaxEdges, n_edges);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(pred_planes && truth_planes && edges && row_w && sums && workspace,
                   "conditional_scores: null plane array, edge table, weight, output or workspace pointer");
  AURORA_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)row_w & 7) == 0 &&
                       ((uintptr_t)edges & 3) == 0,
                   "conditional_scores: weights, output and workspace must be 8-byte aligned, the edge table 4-byte aligned");
  double* const partial = (double*)workspace;
  const hipStream_t s = as_stream(stream);
  const auto run = [&](auto max_edges) {        // max_edges: the instantiation, an integral_constant
    launch_maps<decltype(max_edges)::value>(centre_planes != nullptr, scale_planes != nullptr, (unsigned)plan.groups, s,
                                            pred_planes, truth_planes, centre_planes, scale_planes, n_lat, n_lon,
                                            (int)plan.n_chunks, edges, n_edges, by_pred, row_w, partial);
  };
  if (n_edges <= 2) run(std::integral_constant<int, 2>{});
  else if (n_edges <= 4) run(std::integral_constant<int, 4>{});
  else run(std::integral_constant<int, 8>{});
  const int code = check_launch("conditional_scores");
  if (code != AURORA_OK) return code;
  return finish_partials("conditional_scores", partial, n_planes, (int)plan.n_chunks, (n_edges + 1) * kSlots, sums, s);
}
