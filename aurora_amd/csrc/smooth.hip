// Fields smoothed over a great-circle disc on the device (aurora_amd.smooth).  include/aurora_hip.h has the rule; the window
// arithmetic is smooth_window.h; this file has the two launches.
//
// Prefix.  A WAVEFRONT owns one row of one plane (a 256-thread workgroup takes four consecutive rows, as in
// probability_scores.hip and objects.hip).  It walks the row in chunks of 256 columns, a lane taking four consecutive ones
// (load4 of planes.h: one 16-byte load where the plane is aligned and n_lon % 4 == 0, four 4-byte loads otherwise -- the same
// elements in the same places, so the association below does not depend on the alignment).  A point that is not finite enters
// as value 0 and count 0.  In a chunk: the lane adds its four values in order; the lanes' totals go through an inclusive scan
// with a fixed shuffle tree (offsets 1, 2, 4, .., 32); the running sum of the chunks before is carried in a register:
//   P[j + 1] = carry + (lanes_before + in_lane_prefix),   carry' = carry + total of the chunk
// in fp64, and the same in int32 for the counts N.  The association is fixed, so the tables are repeatable bit for bit.
//
// Gather.  A workgroup owns kGatherRows target rows x 256 adjacent columns, a thread a column.  row_lo, row_count, half and w
// are wave-uniform loads; for every source row in ascending order the lane reads P and N at the ends of its window (adjacent
// lanes read adjacent addresses; a window that wraps reads a third entry) and accumulates num, den and full in fp64.  One
// fp32 store per point, no atomics, nothing reduced across threads.  Every index is clamped into its row.
#include "planes.h"
#include "smooth_window.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kPerLane = 4;
constexpr int kChunkCols = kWave * kPerLane;                   // columns of a prefix chunk
constexpr int kGatherRows = 4;                                 // target rows of a gather workgroup
constexpr int kMaxRows = 255;                                  // source rows of a target row

struct PrefixArgs {
  const float* const* planes;
  double* P;
  int32_t* N;
  int64_t n_rows;                                              // n_planes x n_lat
  int n_lat, n_lon;
};
struct GatherArgs {
  const float* const* planes;
  float* out;                                                  // n_planes x n_lat x n_lon
  const double* P;
  const int32_t* N;
  const int32_t* row_lo;
  const int32_t* row_count;
  const int32_t* half;
  const double* w;
  double min_valid;
  int n_lat, n_lon, max_rows, n_strips, n_row_blocks, wrap, keep_mask;
};

// Inclusive scan over the 64 lanes: a fixed tree, v(lane) += v(lane - o) for o = 1, 2, 4, .., 32.
template <typename T> __device__ __forceinline__ T wave_scan(T v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const T up = __shfl_up(v, o, kWave);
    if (lane >= o) v += up;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void smooth_prefix_kernel(const PrefixArgs a) {
  const int wave = (int)threadIdx.x / kWave, lane = (int)threadIdx.x % kWave;
  const int64_t row = (int64_t)blockIdx.x * kWaves + wave;    // wave-uniform
  if (row >= a.n_rows) return;
  const int64_t plane = row / a.n_lat;
  const int i = (int)(row - plane * a.n_lat);
  const int W = a.n_lon;
  const float* const base = a.planes[plane];
  const bool vec = quads_aligned(W, base);
  const float* const src = base + (int64_t)i * W;
  const gptr<double> P = (gptr<double>)(a.P + row * (int64_t)(W + 1));
  const gptr<int32_t> N = (gptr<int32_t>)(a.N + row * (int64_t)(W + 1));
  if (lane == 0) P[0] = 0.0, N[0] = 0;

  double carry = 0.0;
  int32_t carry_n = 0;
  for (int c0 = 0; c0 < W; c0 += kChunkCols) {                 // wave-uniform trip count: the shuffles see whole waves
    const int j0 = c0 + lane * kPerLane;
    float v[kPerLane];
    load4(src, (int64_t)(j0 < W ? j0 : W - 1), (int64_t)W - 1, vec && j0 < W, v);
    double s[kPerLane];
    int32_t n[kPerLane];
    double run = 0.0;
    int32_t run_n = 0;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const bool ok = j0 + k < W && __builtin_isfinite(v[k]);
      run += ok ? (double)v[k] : 0.0;
      run_n += ok ? 1 : 0;
      s[k] = run, n[k] = run_n;
    }
    const double incl = wave_scan(run, lane);
    const int32_t incl_n = wave_scan(run_n, lane);
    double before = __shfl_up(incl, 1, kWave);
    int32_t before_n = __shfl_up(incl_n, 1, kWave);
    if (lane == 0) before = 0.0, before_n = 0;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k)
      if (j0 + k < W) {
        P[j0 + k + 1] = carry + (before + s[k]);
        N[j0 + k + 1] = carry_n + (before_n + n[k]);
      }
    carry += __shfl(incl, kWave - 1, kWave);
    carry_n += __shfl(incl_n, kWave - 1, kWave);
  }
}

// Every fp64 operation is rounded on its own (contraction is off in this function, so no fma forms), as numpy does on the host.
__global__ __launch_bounds__(kThreads) void smooth_gather_kernel(const GatherArgs a) {
#pragma clang fp contract(off)
  unsigned b = blockIdx.x;
  const int strip = (int)(b % (unsigned)a.n_strips);
  b /= (unsigned)a.n_strips;
  const int row_block = (int)(b % (unsigned)a.n_row_blocks);
  const int64_t plane = (int64_t)(b / (unsigned)a.n_row_blocks);
  const int H = a.n_lat, W = a.n_lon;
  const int j = strip * kThreads + (int)threadIdx.x;
  if (j >= W) return;
  const bool wrap = a.wrap != 0;
  const gptr<const float> in = (gptr<const float>)a.planes[plane];
  const gptr<float> out = (gptr<float>)(a.out + plane * H * W);
  const int64_t stride = (int64_t)W + 1;
  const gptr<const double> P = (gptr<const double>)(a.P + plane * H * stride);
  const gptr<const int32_t> N = (gptr<const int32_t>)(a.N + plane * H * stride);
  const int i1 = min(row_block * kGatherRows + kGatherRows, H);

  for (int i = row_block * kGatherRows; i < i1; ++i) {
    // (wave-uniform: the rows of this target row, clamped into the plane)
    const int k0 = smooth_clamp(a.row_lo[i], 0, H - 1);
    const int cnt = smooth_clamp(a.row_count[i], 0, min(a.max_rows, H - k0));
    const int32_t* const half = a.half + (int64_t)i * a.max_rows;
    double num = 0.0, den = 0.0, full = 0.0;
    for (int r = 0; r < cnt; ++r) {                              // ascending source rows
      const int n = min(half[r], W);
      if (n < 0) continue;                                     // no column of this row is inside the disc
      const int k = k0 + r;
      const double wk = a.w[k];
      const SmoothWindow s = smooth_window(j, n, W, wrap);
      const gptr<const double> Pk = P + k * stride;
      const gptr<const int32_t> Nk = N + k * stride;
      double S = Pk[s.e1] - Pk[s.e0];
      int32_t C = Nk[s.e1] - Nk[s.e0];
      if (s.e2 != 0) S += Pk[s.e2], C += Nk[s.e2];               // (P[0] = 0 and N[0] = 0: the same bits as adding them)
      num += wk * S;
      den += wk * (double)C;
      full += wk * (double)smooth_full_width(n, W, wrap);
    }
    const int64_t at = (int64_t)i * W + j;
    float value = (float)(num / den);
    bool keep = den > 0.0 && !(den / full < a.min_valid) && __builtin_isfinite(value);
    if (a.keep_mask && !__builtin_isfinite(in[at])) keep = false;
    out[at] = keep ? value : __builtin_nanf("");
  }
}

size_t workspace_bytes(int64_t n_planes, int n_lat, int n_lon) {
  const int64_t entries = n_planes * n_lat * ((int64_t)n_lon + 1);
  return (size_t)((entries * 12 + 7) / 8 * 8);
}

bool sizes_ok(int n_planes, int n_lat, int n_lon) {
  return n_planes >= 1 && n_lat >= 1 && n_lon >= 1 && (int64_t)n_lat * n_lon <= 0x7fffffffll;
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_smooth_workspace_bytes(int n_planes, int n_lat, int n_lon) {
  if (!sizes_ok(n_planes, n_lat, n_lon)) return 0;
  return workspace_bytes(n_planes, n_lat, n_lon);
}

extern "C" int aurora_hip_smooth(const float* const* planes, float* out, int n_planes, int n_lat, int n_lon,
                                 const int32_t* row_lo, const int32_t* row_count, const int32_t* half, int max_rows,
                                 const double* w, int wrap, double min_valid, int keep_mask, void* workspace,
                                 size_t workspace_size, void* stream) {
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1 && n_lon >= 1, "smooth: bad sizes (planes %d, grid %d x %d)", n_planes, n_lat, n_lon);
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= 0x7fffffffll, "smooth: a plane of %d x %d points is too large", n_lat, n_lon);
  AURORA_CHECK_ARG(max_rows >= 1 && max_rows <= kMaxRows, "smooth: 1 to %d source rows per target row, got %d", kMaxRows, max_rows);
  AURORA_CHECK_ARG((wrap == 0 || wrap == 1) && (keep_mask == 0 || keep_mask == 1),
                   "smooth: the flags wrap and keep_mask must be 0 or 1, got %d and %d", wrap, keep_mask);
  AURORA_CHECK_ARG(min_valid >= 0.0 && min_valid <= 1.0, "smooth: min_valid must be in [0, 1], got %g", min_valid);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(planes && out && row_lo && row_count && half && w && workspace,
                   "smooth: null plane array, output, table or workspace pointer");
  AURORA_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)w & 7) == 0 &&
                       (((uintptr_t)row_lo | (uintptr_t)row_count | (uintptr_t)half | (uintptr_t)out) & 3) == 0,
                   "smooth: w and the workspace must be 8-byte aligned, out, row_lo, row_count and half 4-byte aligned");
  const size_t need = workspace_bytes(n_planes, n_lat, n_lon);
  AURORA_CHECK_ARG(workspace_size >= need, "smooth: the workspace has %zu bytes, %zu are needed", workspace_size, need);
  const int64_t n_rows = (int64_t)n_planes * n_lat;
  const int64_t prefix_groups = (n_rows + kWaves - 1) / kWaves;
  const int64_t n_strips = ((int64_t)n_lon + kThreads - 1) / kThreads, n_row_blocks = ((int64_t)n_lat + kGatherRows - 1) / kGatherRows;
  AURORA_CHECK_ARG(prefix_groups <= 0x7fffffff && n_strips * n_row_blocks * n_planes <= 0x7fffffff,
                   "smooth: too many planes for one launch (%d planes of %d x %d)", n_planes, n_lat, n_lon);
  const hipStream_t s = as_stream(stream);
  double* const P = (double*)workspace;
  int32_t* const N = (int32_t*)(P + n_rows * ((int64_t)n_lon + 1));

  PrefixArgs p;
  p.planes = planes, p.P = P, p.N = N, p.n_rows = n_rows, p.n_lat = n_lat, p.n_lon = n_lon;
  hipLaunchKernelGGL(smooth_prefix_kernel, dim3((unsigned)prefix_groups), dim3(kThreads), 0, s, p);
  const int code = check_launch("smooth (prefix)");
  if (code != AURORA_OK) return code;

  GatherArgs g;
  g.planes = planes, g.out = out, g.P = P, g.N = N, g.row_lo = row_lo, g.row_count = row_count, g.half = half, g.w = w;
  g.min_valid = min_valid, g.n_lat = n_lat, g.n_lon = n_lon, g.max_rows = max_rows, g.n_strips = (int)n_strips;
  g.n_row_blocks = (int)n_row_blocks, g.wrap = wrap, g.keep_mask = keep_mask;
  hipLaunchKernelGGL(smooth_gather_kernel, dim3((unsigned)(n_strips * n_row_blocks * n_planes)), dim3(kThreads), 0, s, g);
  return check_launch("smooth (gather)");
}
