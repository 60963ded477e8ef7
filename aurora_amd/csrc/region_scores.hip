// Verification sums by region on the device (aurora_amd.region_scores: weighted RMSE / bias / MAE / ACC over latitude bands,
// longitude boxes and masks).
//
// For every plane (one variable, level and batch element; n_lat x n_lon fp32, row-major) the prediction p, the truth t and,
// if given, the climatology c are read ONCE, and the eight fp64 sums of aurora_hip_scores are kept for each of up to eight
// regions.  A point belongs to region r where bit r of row_bits[row] & col_bits[col] & mask_bits[row][col] is set (no mask
// plane: every bit set).  The row byte is wave-uniform, and a row whose byte is 0 is not read at all.
//
// A lane takes quads of columns (the quad rule of planes.h, extended to the column and mask bytes: four of them are one
// 32-bit load where the float quads are one 16-byte load) and keeps the sums of EVERY region in registers, indexed by
// unrolled constants only; a point is applied to every region by select: its terms enter the regions it belongs to and +0
// enters the others.  x + (+0) = x, so a region's sums are the sums over its own points alone, in the order of the reduction
// tree of planes.h: they do not depend on which other regions share the launch or on which instantiation ran.  That only
// holds while every instantiation rounds alike, so contraction is off in this file's arithmetic and the fused multiply-adds
// that are wanted are written out.  finish_partials (n_regions x 8 sums to a chunk) is the second launch of the tree, as it
// is for scores.hip: a region's sums are the sums of aurora_hip_scores restricted to its points.
#include <type_traits>

#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlots = kSumSlots;
constexpr int kMaxRegions = 8;
constexpr int kChunkElems = kScoresChunkElems;  // target size of a row chunk (elements of one input): that of scores.hip

template <int kR, bool kClim> struct Acc {
  double s2[kR], s3[kR], s4[kR];
  double s5[kR], s6[kR], s7[kR];                // touched with a climatology only
  int n[kR];                                  // valid points of the current row, per region
};

// One point into every region.  bits: the regions the point belongs to (bit r; 0 for a point outside the row).  An invalid
// point belongs to no region, and its p, t and c are replaced by 0 so that every difference is finite.
template <int kR, bool kClim>
__device__ __forceinline__ void point(Acc<kR, kClim>& a, double w, float pf, float tf, float cf, unsigned bits) {
#pragma clang fp contract(off)
  bool ok = __builtin_isfinite(pf) && __builtin_isfinite(tf);
  if (kClim) ok = ok && __builtin_isfinite(cf);
  const unsigned in_bits = ok ? bits : 0u;
  const double p = (double)(ok ? pf : 0.f), t = (double)(ok ? tf : 0.f), c = (double)(kClim && ok ? cf : 0.f);
  const double d = p - t;
  const double wd = w * d;
  const double pp = p - c, tp = t - c;
  const double wpp = w * pp, wtp = w * tp;
#pragma unroll
  for (int k = 0; k < kR; ++k) {
    const bool in = (in_bits & (1u << k)) != 0;
    const double wdk = in ? wd : 0.0;                          // +0 for every region the point is not in
    a.n[k] += in ? 1 : 0;
    a.s2[k] = a.s2[k] + wdk;
    a.s3[k] = __builtin_fma(wdk, d, a.s3[k]);                  // (+0) d = +-0: leaves s3 as it is
    a.s4[k] = a.s4[k] + __builtin_fabs(wdk);
    if (kClim) {
      const double wppk = in ? wpp : 0.0, wtpk = in ? wtp : 0.0;
      a.s5[k] = __builtin_fma(wppk, tp, a.s5[k]);
      a.s6[k] = __builtin_fma(wppk, pp, a.s6[k]);
      a.s7[k] = __builtin_fma(wtpk, tp, a.s7[k]);
    }
  }
  __builtin_amdgcn_sched_barrier(0);   // a point at a time, as in conditional_scores.hip: interleaved points cost registers
}

// One workgroup = one row chunk of one plane; partial[((plane * n_chunks + chunk) * n_regions + region) * 8 + slot].
template <int kR, bool kClim>
__global__ __launch_bounds__(kThreads) void region_kernel(const float* const* __restrict__ pred_planes,
                                                          const float* const* __restrict__ truth_planes,
                                                          const float* const* __restrict__ clim_planes, int n_lat,
                                                          int n_lon, int n_chunks, const uint8_t* __restrict__ row_bits,
                                                          const uint8_t* __restrict__ col_bits,
                                                          const uint8_t* __restrict__ mask_bits, int n_regions,
                                                          const double* __restrict__ row_w, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double s_wave[kWaves][kR * kSlots];
  const int plane = (int)(blockIdx.x / (unsigned)n_chunks), chunk = (int)(blockIdx.x % (unsigned)n_chunks);
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const gptr<const float> P = (gptr<const float>)pred_planes[plane];
  const gptr<const float> T = (gptr<const float>)truth_planes[plane];
  const gptr<const float> C = kClim ? (gptr<const float>)clim_planes[plane] : P;
  const gptr<const uint8_t> RB = (gptr<const uint8_t>)row_bits, CB = (gptr<const uint8_t>)col_bits;
  const bool masked = mask_bits != nullptr;
  const gptr<const uint8_t> MB = masked ? (gptr<const uint8_t>)mask_bits : CB;   // an absent plane is never read
  // the quad rule over every pointer read by quads: 16 bytes of a float plane go with 4 bytes of the byte tables
  const bool vec = quads_aligned(n_lon, P, T, C) && (((uintptr_t)CB | (uintptr_t)MB) & 3) == 0;
  const unsigned live = (1u << n_regions) - 1u;                // the regions of this launch (n_regions <= kR)
  const int n_quads = (n_lon + 3) >> 2;
  const int rows = chunk_rows(n_lon, kChunkElems, kWaves);
  const int r_begin = chunk * rows, r_end = min(r_begin + rows, n_lat);

  Acc<kR, kClim> a;
  double s1[kR];
  int count[kR];
#pragma unroll
  for (int k = 0; k < kR; ++k) {
    a.s2[k] = a.s3[k] = a.s4[k] = s1[k] = 0.0, a.n[k] = count[k] = 0;
    if (kClim) a.s5[k] = a.s6[k] = a.s7[k] = 0.0;
  }

  for (int r = r_begin + wave; r < r_end; r += kWaves) {       // wave-uniform: the row byte and w are scalar loads
    const unsigned rb = (unsigned)RB[r] & live;
    if (rb == 0) continue;                                     // a row of no region: nothing of it is read
    const double w = row_w[r];
    const int64_t row0 = (int64_t)r * n_lon;
#pragma unroll
    for (int k = 0; k < kR; ++k) a.n[k] = 0;
    if (vec) {                                                 // the quad rule, p, t and c column by column
      const gptr<const f32x4> p4 = (gptr<const f32x4>)(P + row0), t4 = (gptr<const f32x4>)(T + row0),
                              c4 = (gptr<const f32x4>)(C + row0);
      const gptr<const uint32_t> cb4 = (gptr<const uint32_t>)CB, mb4 = (gptr<const uint32_t>)(MB + row0);
      const unsigned rb4 = rb * 0x01010101u;
      for (int q = lane; q < n_quads; q += 64) {
        const f32x4 p = p4[q], t = t4[q], c = kClim ? c4[q] : f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned m = cb4[q] & rb4;                             // byte k: the regions of column 4 q + k (little-endian)
        if (masked) m &= mb4[q];
        point<kR, kClim>(a, w, p.x, t.x, c.x, m & 0xffu);
        point<kR, kClim>(a, w, p.y, t.y, c.y, (m >> 8) & 0xffu);
        point<kR, kClim>(a, w, p.z, t.z, c.z, (m >> 16) & 0xffu);
        point<kR, kClim>(a, w, p.w, t.w, c.w, m >> 24);
      }
    } else {
      for (int q = lane; q < n_quads; q += 64) {                // the same points in the same order, a column at a time
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
          const int col = min(4 * q + k, n_lon - 1);           // clamped: the loads are in the row, the guard is the bits
          unsigned m = (unsigned)CB[col] & rb;
          if (masked) m &= (unsigned)MB[row0 + col];
          point<kR, kClim>(a, w, P[row0 + col], T[row0 + col], kClim ? C[row0 + col] : 0.f, 4 * q + k < n_lon ? m : 0u);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kR; ++k) {
      count[k] += a.n[k];
      s1[k] = __builtin_fma(w, (double)a.n[k], s1[k]);
    }
  }

#pragma unroll
  for (int k = 0; k < kR; ++k) {
    if (k < n_regions) {                                       // wave-uniform
      const double sums[kSlots] = {(double)count[k], s1[k], a.s2[k], a.s3[k], a.s4[k], kClim ? a.s5[k] : 0.0,
                                   kClim ? a.s6[k] : 0.0, kClim ? a.s7[k] : 0.0};
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        if (!kClim && s >= 5) break;
        const double v = wave_sum_f64(sums[s]);
        if (lane == 0) s_wave[wave][k * kSlots + s] = v;
      }
    }
  }
  __syncthreads();
  const int n_out = n_regions * kSlots;                        // <= 64 < kThreads
  if ((int)threadIdx.x < n_out)
    partial[(int64_t)blockIdx.x * n_out + threadIdx.x] =
        kClim || ((int)threadIdx.x % kSlots) < 5 ? sum_waves(s_wave, (int)threadIdx.x) : 0.0;
}

template <int kR, typename... A> void launch(bool clim, unsigned groups, hipStream_t stream, A... args) {
  if (clim) hipLaunchKernelGGL((region_kernel<kR, true>), dim3(groups), dim3(kThreads), 0, stream, args...);
  else hipLaunchKernelGGL((region_kernel<kR, false>), dim3(groups), dim3(kThreads), 0, stream, args...);
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_region_scores_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_regions) {
  if (n_regions < 1 || n_regions > kMaxRegions) return 0;
  return (size_t)chunk_plan(n_planes, n_lat, n_lon, kChunkElems, kWaves).groups * (size_t)n_regions * kSlots * sizeof(double);
}

extern "C" int aurora_hip_region_scores(const float* const* pred_planes, const float* const* truth_planes,
                                        const float* const* clim_planes, int n_planes, int n_lat, int n_lon,
                                        const uint8_t* row_bits, const uint8_t* col_bits, const uint8_t* mask_bits,
                                        int n_regions, const double* row_w, double* sums, void* workspace, void* stream) {
  ChunkPlan plan;
  if (const int code = plan_chunks("region_scores", n_planes, n_lat, n_lon, kChunkElems, kWaves, &plan)) return code;
  AURORA_CHECK_ARG(n_regions >= 1 && n_regions <= kMaxRegions, "region_scores: 1 to %d regions per call, got %d", kMaxRegions,
                   n_regions);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(pred_planes && truth_planes && row_bits && col_bits && row_w && sums && workspace,
                   "region_scores: null plane array, row or column table, weight, output or workspace pointer");
  AURORA_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)row_w & 7) == 0,
                   "region_scores: weights, output and workspace must be 8-byte aligned");
  double* const partial = (double*)workspace;
  const hipStream_t s = as_stream(stream);
  const auto run = [&](auto regions) {          // regions: the instantiation, an integral_constant
    launch<decltype(regions)::value>(clim_planes != nullptr, (unsigned)plan.groups, s, pred_planes, truth_planes, clim_planes,
                                     n_lat, n_lon, (int)plan.n_chunks, row_bits, col_bits, mask_bits, n_regions, row_w, partial);
  };
  if (n_regions <= 1) run(std::integral_constant<int, 1>{});
  else if (n_regions <= 2) run(std::integral_constant<int, 2>{});
  else if (n_regions <= 4) run(std::integral_constant<int, 4>{});
  else run(std::integral_constant<int, 8>{});
  const int code = check_launch("region_scores");
  if (code != AURORA_OK) return code;
  return finish_partials("region_scores", partial, n_planes, (int)plan.n_chunks, n_regions * kSlots, sums, s);
}
