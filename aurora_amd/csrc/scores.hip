// Verification sums of a forecast against truth on the device (aurora_amd.scores: weighted RMSE / bias / MAE / ACC).
//
// For every plane (one variable, level and batch element; n_lat x n_lon fp32, row-major) the prediction p, the truth t
// and, if given, the climatology c are read ONCE and reduced to eight fp64 sums over the points where every input
// that is present is finite, with the row weight w[i] (include/aurora_hip.h has the table).  All differences and
// products are formed in fp64 from the fp32 inputs; nothing is accumulated in fp32.
//
// A lane takes quads of columns (the quad rule of planes.h) and the sums go through the reduction tree of planes.h, four
// waves to a workgroup; finish_partials (eight sums to a chunk) is its second launch.
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlots = kSumSlots;
constexpr int kChunkElems = kScoresChunkElems;  // target size of a row chunk (elements of one input)

struct Acc {
  double s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
  int n = 0;                                    // valid points of the current row
};

// One point.  An invalid point is replaced by p = t = c = 0: every term is then exactly +0 and leaves the sums as
// they are; only the count (and through it the weight sum) sees validity.
template <bool kClim>
__device__ __forceinline__ void point(Acc& a, double w, float pf, float tf, float cf, bool in_row) {
  bool ok = in_row && __builtin_isfinite(pf) && __builtin_isfinite(tf);
  if (kClim) ok = ok && __builtin_isfinite(cf);
  const double p = (double)(ok ? pf : 0.f), t = (double)(ok ? tf : 0.f);
  a.n += ok ? 1 : 0;
  const double d = p - t;
  const double wd = w * d;
  a.s2 += wd;
  a.s3 = __builtin_fma(wd, d, a.s3);
  a.s4 += __builtin_fabs(wd);
  if (kClim) {
    const double c = (double)(ok ? cf : 0.f);
    const double pp = p - c, tp = t - c;
    const double wpp = w * pp;
    a.s5 = __builtin_fma(wpp, tp, a.s5);
    a.s6 = __builtin_fma(wpp, pp, a.s6);
    a.s7 = __builtin_fma(w * tp, tp, a.s7);
  }
}

// One workgroup = one row chunk of one plane; partial[(plane * n_chunks + chunk) * 8 + slot].
template <bool kClim>
__global__ __launch_bounds__(kThreads) void scores_kernel(const float* const* __restrict__ pred_planes,
                                                          const float* const* __restrict__ truth_planes,
                                                          const float* const* __restrict__ clim_planes, int n_lat,
                                                          int n_lon, int n_chunks, const double* __restrict__ row_w,
                                                          double* __restrict__ partial) {
  __shared__ double s_wave[kWaves][kSlots];
  const int plane = (int)(blockIdx.x / (unsigned)n_chunks), chunk = (int)(blockIdx.x % (unsigned)n_chunks);
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const gptr<const float> P = (gptr<const float>)pred_planes[plane];
  const gptr<const float> T = (gptr<const float>)truth_planes[plane];
  const gptr<const float> C = kClim ? (gptr<const float>)clim_planes[plane] : P;
  const bool vec = quads_aligned(n_lon, P, T, C);
  const int n_quads = (n_lon + 3) >> 2;
  const int rows = chunk_rows(n_lon, kChunkElems, kWaves);
  const int r_begin = chunk * rows, r_end = min(r_begin + rows, n_lat);

  Acc a;
  double s1 = 0.0;
  int count = 0;
  for (int r = r_begin + wave; r < r_end; r += kWaves) {       // wave-uniform: w is one scalar load per row
    const double w = row_w[r];
    const int64_t row0 = (int64_t)r * n_lon;
    a.n = 0;
    if (vec) {                                                 // the quad rule, p, t and c column by column
      const gptr<const f32x4> p4 = (gptr<const f32x4>)(P + row0), t4 = (gptr<const f32x4>)(T + row0),
                              c4 = (gptr<const f32x4>)(C + row0);
#pragma unroll 2
      for (int q = lane; q < n_quads; q += 64) {
        const f32x4 p = p4[q], t = t4[q], c = kClim ? c4[q] : f32x4{0.f, 0.f, 0.f, 0.f};
        point<kClim>(a, w, p.x, t.x, c.x, true);
        point<kClim>(a, w, p.y, t.y, c.y, true);
        point<kClim>(a, w, p.z, t.z, c.z, true);
        point<kClim>(a, w, p.w, t.w, c.w, true);
      }
    } else {
      for (int q = lane; q < n_quads; q += 64) {
        float p[4], t[4], c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int col = min(4 * q + k, n_lon - 1);           // clamped: the load is in the row, the guard is in_row
          p[k] = P[row0 + col];
          t[k] = T[row0 + col];
          c[k] = kClim ? C[row0 + col] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) point<kClim>(a, w, p[k], t[k], c[k], 4 * q + k < n_lon);
      }
    }
    count += a.n;
    s1 = __builtin_fma(w, (double)a.n, s1);
  }

  const double sums[kSlots] = {(double)count, s1, a.s2, a.s3, a.s4, a.s5, a.s6, a.s7};
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    if (!kClim && s >= 5) break;
    const double v = wave_sum_f64(sums[s]);
    if (lane == 0) s_wave[wave][s] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSlots) {
    const int s = (int)threadIdx.x;
    partial[(int64_t)blockIdx.x * kSlots + s] = kClim || s < 5 ? sum_waves(s_wave, s) : 0.0;
  }
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_scores_workspace_bytes(int n_planes, int n_lat, int n_lon) {
  return (size_t)chunk_plan(n_planes, n_lat, n_lon, kChunkElems, kWaves).groups * kSlots * sizeof(double);
}

extern "C" int aurora_hip_scores(const float* const* pred_planes, const float* const* truth_planes,
                                 const float* const* clim_planes, int n_planes, int n_lat, int n_lon, const double* row_w,
                                 double* sums, void* workspace, void* stream) {
  ChunkPlan plan;
  if (const int code = plan_chunks("scores", n_planes, n_lat, n_lon, kChunkElems, kWaves, &plan)) return code;
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(pred_planes && truth_planes && row_w && sums && workspace,
                   "scores: null plane array, weight, output or workspace pointer");
  AURORA_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)row_w & 7) == 0,
                   "scores: weights, output and workspace must be 8-byte aligned");
  double* const partial = (double*)workspace;
  if (clim_planes)
    hipLaunchKernelGGL(scores_kernel<true>, dim3((unsigned)plan.groups), dim3(kThreads), 0, as_stream(stream), pred_planes,
                       truth_planes, clim_planes, n_lat, n_lon, (int)plan.n_chunks, row_w, partial);
  else
    hipLaunchKernelGGL(scores_kernel<false>, dim3((unsigned)plan.groups), dim3(kThreads), 0, as_stream(stream), pred_planes,
                       truth_planes, clim_planes, n_lat, n_lon, (int)plan.n_chunks, row_w, partial);
  const int code = check_launch("scores");
  if (code != AURORA_OK) return code;
  return finish_partials("scores", partial, n_planes, (int)plan.n_chunks, kSlots, sums, as_stream(stream));
}
