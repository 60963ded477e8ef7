// Bilinear regridding of lat / lon planes on the device (Batch.regrid of a GPU-resident batch).
//
// The host builds interpolation tables once (aurora_hip_regrid_plan: per output row the two source rows and the fp64
// weight, per output column the two source columns and the weight -- the single place where the convention of the host
// path lives), and one launch of regrid_kernel then applies them to every plane of a batch.  The arithmetic is that of
// scipy's RegularGridInterpolator(method="linear") as Batch.regrid's host path runs it: fp64, all four corners summed in
// scipy's order even where a weight is zero (a NaN there poisons the result, as on the host), no fused multiply-adds;
// the result is rounded to fp32.
#include <algorithm>
#include <cmath>
#include <vector>

#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kColsPerThread = 2;               // output columns per lane: kThreads * kColsPerThread per workgroup
constexpr int kRowsPerTile = 4;                 // output rows per workgroup
constexpr int kPlanesPerGroup = 8;              // planes one workgroup sweeps with the same table entries


// scipy's evaluate_linear_2d: v00 (1-y)(1-x) + v01 (1-y) x + v10 y (1-x) + v11 y x, left to right.
__device__ __forceinline__ double bilinear(double v00, double v01, double v10, double v11, double ay0, double ay1,
                                           double bx0, double bx1) {
#pragma clang fp contract(off)
  return v00 * ay0 * bx0 + v01 * ay0 * bx1 + v10 * ay1 * bx0 + v11 * ay1 * bx1;
}

// One workgroup: kRowsPerTile output rows x kThreads * kColsPerThread output columns of up to kPlanesPerGroup planes.
// Its table entries stay in registers for the whole sweep; every store is one fp32 per lane, 64 consecutive words per
// wave instruction, so any 4-byte plane alignment is fine.  The four source values of an output point are gathered from
// two source rows that neighbouring output rows share (L2).  Table indices are clamped into the source plane.
template <typename S>
__global__ __launch_bounds__(kThreads) void regrid_kernel(const void* const* __restrict__ src_planes,
                                                          float* const* __restrict__ dst_planes, int n_planes, int n_lat,
                                                          int n_lon, const int32_t* __restrict__ rows,
                                                          const double* __restrict__ row_w, int n_rows_out,
                                                          const int32_t* __restrict__ cols,
                                                          const double* __restrict__ col_w, int n_cols_out) {
  int c_idx[kColsPerThread], c0[kColsPerThread], c1[kColsPerThread];
  double bx0[kColsPerThread], bx1[kColsPerThread];
#pragma unroll
  for (int k = 0; k < kColsPerThread; ++k) {
    const int c = (int)blockIdx.y * (kThreads * kColsPerThread) + k * kThreads + (int)threadIdx.x;
    c_idx[k] = c;
    const bool ok = c < n_cols_out;
    c0[k] = ok ? min(max(cols[2 * c], 0), n_lon - 1) : 0;
    c1[k] = ok ? min(max(cols[2 * c + 1], 0), n_lon - 1) : 0;
    const double w = ok ? col_w[c] : 0.0;
    bx0[k] = 1.0 - w;
    bx1[k] = w;
  }
  const int r_begin = (int)blockIdx.x * kRowsPerTile;
  int r0[kRowsPerTile], r1[kRowsPerTile];
  double ay0[kRowsPerTile], ay1[kRowsPerTile];
#pragma unroll
  for (int i = 0; i < kRowsPerTile; ++i) {
    const int r = min(r_begin + i, n_rows_out - 1);
    r0[i] = min(max(rows[2 * r], 0), n_lat - 1);
    r1[i] = min(max(rows[2 * r + 1], 0), n_lat - 1);
    const double w = row_w[r];
    ay0[i] = 1.0 - w;
    ay1[i] = w;
  }
  const int p_end = min((int)(blockIdx.z + 1) * kPlanesPerGroup, n_planes);
  for (int p = (int)blockIdx.z * kPlanesPerGroup; p < p_end; ++p) {
    // (the plane pointers are global memory: said so, the loads and stores are global_*, not flat_*)
    const gptr<const S> src = (gptr<const S>)src_planes[p];
    const gptr<float> dst = (gptr<float>)dst_planes[p];
    // Every load is unconditional (lanes and rows past the edge read valid clamped entries), so that all
    // 4 * kRowsPerTile * kColsPerThread gathers of a plane are in flight together; only the stores are guarded.
    float out[kRowsPerTile][kColsPerThread];
#pragma unroll
    for (int i = 0; i < kRowsPerTile; ++i) {
      const gptr<const S> s0 = src + (int64_t)r0[i] * n_lon;
      const gptr<const S> s1 = src + (int64_t)r1[i] * n_lon;
#pragma unroll
      for (int k = 0; k < kColsPerThread; ++k)
        out[i][k] = (float)bilinear((double)s0[c0[k]], (double)s0[c1[k]], (double)s1[c0[k]], (double)s1[c1[k]], ay0[i],
                                    ay1[i], bx0[k], bx1[k]);
    }
    // All eight results exist here: keeps the compiler from sinking their loads into the guarded stores below.
    static_assert(kRowsPerTile * kColsPerThread == 8, "one operand per result");
    asm volatile("" : "+v"(out[0][0]), "+v"(out[0][1]), "+v"(out[1][0]), "+v"(out[1][1]), "+v"(out[2][0]), "+v"(out[2][1]),
                 "+v"(out[3][0]), "+v"(out[3][1]));
#pragma unroll
    for (int i = 0; i < kRowsPerTile; ++i) {
      if (r_begin + i >= n_rows_out) break;
      const gptr<float> d = dst + (int64_t)(r_begin + i) * n_cols_out;
#pragma unroll
      for (int k = 0; k < kColsPerThread; ++k)
        if (c_idx[k] < n_cols_out) __builtin_nontemporal_store(out[i][k], d + c_idx[k]);
    }
  }
}

// Ascending view of a strictly monotone axis: `g` sorted ascending, `orig[i]` the index of g[i] in the given order.
bool ascending_axis(const double* x, int n, bool allow_descending, std::vector<double>& g, std::vector<int32_t>& orig) {
  bool up = true, down = allow_descending;
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(x[i])) return false;
    if (i > 0) {
      up = up && x[i] > x[i - 1];
      down = down && x[i] < x[i - 1];
    }
  }
  if (!up && !down) return false;
  g.resize(n);
  orig.resize(n);
  for (int i = 0; i < n; ++i) {
    orig[i] = up ? i : n - 1 - i;
    g[i] = x[orig[i]];
  }
  return true;
}

// scipy's find_indices on an ascending axis: the largest i with g[i] <= x, clamped to [0, n - 2] (a target on the last
// node takes the last interval; outside the axis the first / last interval extrapolates); t = (x - g[i]) / (g[i+1] - g[i]).
void locate(const std::vector<double>& g, double x, int& i, double& t) {
  const int n = (int)g.size();
  i = (int)(std::upper_bound(g.begin(), g.end(), x) - g.begin()) - 1;
  i = std::min(std::max(i, 0), n - 2);
  t = (x - g[i]) / (g[i + 1] - g[i]);
}

bool all_finite(const double* x, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return false;
  return true;
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_regrid_plan(const double* lat, int n_lat, const double* lon, int n_lon, const double* lat_new,
                                      int n_lat_new, const double* lon_new, int n_lon_new, int32_t* rows, double* row_w,
                                      int32_t* cols, double* col_w) {
  AURORA_CHECK_ARG(lat && lon && lat_new && lon_new && rows && row_w && cols && col_w,
                   "regrid_plan: null coordinate or table pointer");
  AURORA_CHECK_ARG(n_lat >= 2 && n_lon >= 2, "regrid_plan: the source grid needs n >= 2 latitudes and longitudes (got %d x %d)",
                   n_lat, n_lon);
  AURORA_CHECK_ARG(n_lat_new >= 1 && n_lon_new >= 1, "regrid_plan: empty target grid (%d x %d)", n_lat_new, n_lon_new);
  std::vector<double> g;
  std::vector<int32_t> orig;
  AURORA_CHECK_ARG(ascending_axis(lat, n_lat, true, g, orig), "regrid_plan: latitudes must be finite and strictly monotone");
  AURORA_CHECK_ARG(all_finite(lat_new, n_lat_new) && all_finite(lon_new, n_lon_new),
                   "regrid_plan: target coordinates must be finite");
  for (int k = 0; k < n_lat_new; ++k) {
    int i;
    locate(g, lat_new[k], i, row_w[k]);
    rows[2 * k] = orig[i];
    rows[2 * k + 1] = orig[i + 1];
  }
  // Longitudes: the periodic axis [lon[n-1] - 360, lon..., lon[0] + 360]; extended index j is source column (j - 1) mod n.
  std::vector<double> e(n_lon + 2);
  e[0] = lon[n_lon - 1] - 360.0;
  std::copy(lon, lon + n_lon, e.begin() + 1);
  e[n_lon + 1] = lon[0] + 360.0;
  AURORA_CHECK_ARG(ascending_axis(e.data(), n_lon + 2, false, g, orig),
                   "regrid_plan: longitudes must be finite, strictly increasing and span less than 360 degrees");
  for (int k = 0; k < n_lon_new; ++k) {
    int j;
    locate(g, lon_new[k], j, col_w[k]);
    cols[2 * k] = (j + n_lon - 1) % n_lon;
    cols[2 * k + 1] = j % n_lon;
  }
  return AURORA_OK;
}

extern "C" int aurora_hip_regrid(const void* const* src_planes, int src_dtype, float* const* dst_planes, int n_planes,
                                 int n_lat, int n_lon, const int32_t* rows, const double* row_w, int n_rows_out,
                                 const int32_t* cols, const double* col_w, int n_cols_out, void* stream) {
  AURORA_CHECK_ARG(src_planes && dst_planes && rows && row_w && cols && col_w, "regrid: null plane array or table pointer");
  AURORA_CHECK_ARG(src_dtype == AURORA_F32 || src_dtype == AURORA_F64, "regrid: source dtype must be AURORA_F32 or AURORA_F64");
  AURORA_CHECK_ARG(n_planes >= 1 && n_lat >= 1 && n_lon >= 1 && n_rows_out >= 1 && n_cols_out >= 1,
                   "regrid: sizes must be positive (planes %d, source %d x %d, output %d x %d)", n_planes, n_lat, n_lon,
                   n_rows_out, n_cols_out);
  const int64_t row_tiles = ((int64_t)n_rows_out + kRowsPerTile - 1) / kRowsPerTile;
  const int64_t col_tiles = ((int64_t)n_cols_out + kThreads * kColsPerThread - 1) / (kThreads * kColsPerThread);
  const int64_t plane_groups = ((int64_t)n_planes + kPlanesPerGroup - 1) / kPlanesPerGroup;
  AURORA_CHECK_ARG(col_tiles <= 65535 && plane_groups <= 65535, "regrid: too many output columns or planes for one launch");
  const dim3 grid((unsigned)row_tiles, (unsigned)col_tiles, (unsigned)plane_groups);
  if (src_dtype == AURORA_F32)
    hipLaunchKernelGGL(regrid_kernel<float>, grid, dim3(kThreads), 0, as_stream(stream), src_planes, dst_planes, n_planes,
                       n_lat, n_lon, rows, row_w, n_rows_out, cols, col_w, n_cols_out);
  else
    hipLaunchKernelGGL(regrid_kernel<double>, grid, dim3(kThreads), 0, as_stream(stream), src_planes, dst_planes, n_planes,
                       n_lat, n_lon, rows, row_w, n_rows_out, cols, col_w, n_cols_out);
  return check_launch("regrid");
}
