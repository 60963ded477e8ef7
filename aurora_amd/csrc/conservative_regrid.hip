// First-order conservative (area-weighted) regridding of lat / lon planes on the device (aurora_amd.conservative_regrid
// of a GPU-resident batch).
//
// The host builds the overlap tables once (aurora_amd/conservative.py: per target row the source rows its cell overlaps and
// the overlaps in sin(lat), per target column the source columns and the overlaps in degrees -- the single place where the
// cell model lives; include/aurora_hip.h has the format), and one launch of conservative_kernel applies them to every plane.
// The arithmetic is the rule of aurora_amd/conservative.py, operation for operation: fp64, each operation rounded on its
// own, rows before columns, the taps in table order; a source value that is not finite drops out of both sums; the result
// is rounded to fp32 once.
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;                   // lanes of a workgroup = target columns of a tile
constexpr int kRowsPerTile = 4;                 // target rows per workgroup
constexpr int kPlanesPerGroup = 8;              // planes one workgroup sweeps with the same column taps
constexpr int kChunk = 4 * kThreads;            // source columns whose row sums are parked in LDS at a time: a quad per lane
constexpr int kRegTaps = 8;                     // column weights a lane keeps in registers; further taps read the table
constexpr int kMaxTaps = 64;                    // taps per target cell and axis (the host refuses more)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// One workgroup: kRowsPerTile target rows x kThreads target columns of up to kPlanesPerGroup planes.
//
// The tile's target columns need the source columns [start, end) (unwrapped: source column = index mod n_lon); they are
// taken kChunk at a time.  Stage 1: lane l owns the quad of source columns 4 l .. 4 l + 3 of the chunk and runs down the row
// taps of the target row (coalesced 16-byte loads where the quad rule allows, four 4-byte ones otherwise: the same elements
// either way), accumulating cn = sum a x and cd = sum a over the finite x in registers; both are parked in LDS.  Stage 2,
// after a barrier: lane l owns target column j0 + l and adds those of its column taps that lie in the chunk, in tap order,
// to n and d, which it keeps across the chunks.  The LDS image is double-buffered, so a chunk costs one barrier.
//
// A source element is read once per target row it overlaps and per column tile, not once per target point.  A point's
// result depends on its own taps alone: not on the tile (the chunks cut a tap sequence, never reorder it), not on the
// other planes, not on pointer alignment.  Every source index is clamped or wrapped into the plane and every LDS index is
// bounded by the chunk, whatever the tables hold; only the stores are guarded.
template <typename S>
__global__ __launch_bounds__(kThreads) void conservative_kernel(
    const void* const* __restrict__ src_planes, float* const* __restrict__ dst_planes, int n_planes, int n_lat, int n_lon,
    int n_rows_out, int n_cols_out, const int32_t* __restrict__ row_first, const int32_t* __restrict__ row_count,
    const double* __restrict__ row_w, const double* __restrict__ row_measure, const int32_t* __restrict__ col_first,
    const int32_t* __restrict__ col_count, const double* __restrict__ col_w, const double* __restrict__ col_measure,
    double min_valid) {
#pragma clang fp contract(off)
  __shared__ double s_cn[2][kChunk];
  __shared__ double s_cd[2][kChunk];

  const int lane = (int)threadIdx.x;
  const int j0 = (int)blockIdx.y * kThreads;
  const int j = j0 + lane;
  const bool col_ok = j < n_cols_out;
  const int jc = min(j, n_cols_out - 1);
  const int u_max = 3 * n_lon - 1;
  const int first_j = clampi(col_first[2 * jc], 0, u_max);
  const int cnt_j = col_ok ? clampi(col_count[jc], 0, kMaxTaps) : 0;
  const int64_t woff_j = max(col_first[2 * jc + 1], 0);
  const double B_j = col_measure[jc];
  double b_reg[kRegTaps];
#pragma unroll
  for (int t = 0; t < kRegTaps; ++t) b_reg[t] = t < cnt_j ? col_w[woff_j + t] : 0.0;

  // The tile's span of source columns: first and one-past-last indices never decrease along the target columns.
  const int j_last = min(j0 + kThreads, n_cols_out) - 1;
  const int start = clampi(col_first[2 * j0], 0, u_max) & ~3;
  const int end = clampi(col_first[2 * j_last], 0, u_max) + clampi(col_count[j_last], 0, kMaxTaps);

  const float nan = __builtin_nanf("");
  int buf = 0;
  const int p_end = min((int)(blockIdx.z + 1) * kPlanesPerGroup, n_planes);
  for (int p = (int)blockIdx.z * kPlanesPerGroup; p < p_end; ++p) {
    const gptr<const S> src = (gptr<const S>)src_planes[p];
    const gptr<float> dst = (gptr<float>)dst_planes[p];
    const bool vec = quads_aligned(n_lon, src);
    for (int ii = 0; ii < kRowsPerTile; ++ii) {
      const int i = (int)blockIdx.x * kRowsPerTile + ii;
      if (i >= n_rows_out) break;               // (the same for every lane of the workgroup)
      const int r0 = clampi(row_first[2 * i], 0, n_lat - 1);
      const int r_cnt = clampi(row_count[i], 0, kMaxTaps);
      const int64_t r_off = max(row_first[2 * i + 1], 0);
      double n = 0.0, d = 0.0;
      for (int c_lo = start; c_lo < end; c_lo += kChunk) {
        // ---- stage 1: the row taps of this lane's quad of source columns
        const int u = c_lo + 4 * lane;
        if (u < end) {
          int col[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) col[k] = (u + k) % n_lon;   // (vec: u and n_lon are multiples of 4, the quad is col[0] .. + 3)
          double cn[4] = {0.0, 0.0, 0.0, 0.0}, cd[4] = {0.0, 0.0, 0.0, 0.0};
          for (int t = 0; t < r_cnt; ++t) {
            const double a = row_w[r_off + t];
            const gptr<const S> row = src + (int64_t)min(r0 + t, n_lat - 1) * n_lon;
            S x[4];
            if (vec) {
              load4<S>((const S*)row, col[0], n_lon - 1, true, x);
            } else {
#pragma unroll
              for (int k = 0; k < 4; ++k) x[k] = row[col[k]];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              if (__builtin_isfinite(x[k])) {
                cn[k] += a * (double)x[k];
                cd[k] += a;
              }
            }
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            s_cn[buf][4 * lane + k] = cn[k];
            s_cd[buf][4 * lane + k] = cd[k];
          }
        }
        __syncthreads();
        // ---- stage 2: the column taps of this lane's target column that lie in [c_lo, min(c_lo + kChunk, end))
        const int t_lo = max(0, c_lo - first_j);
        const int t_hi = min(cnt_j, min(c_lo + kChunk, end) - first_j);
        const int base = first_j - c_lo;         // tap t is LDS entry base + t, in [0, kChunk) for t_lo <= t < t_hi
#pragma unroll
        for (int t = 0; t < kRegTaps; ++t) {
          if (t >= t_lo && t < t_hi) {
            n += b_reg[t] * s_cn[buf][base + t];
            d += b_reg[t] * s_cd[buf][base + t];
          }
        }
        for (int t = max(t_lo, kRegTaps); t < t_hi; ++t) {
          const double b = col_w[woff_j + t];
          n += b * s_cn[buf][base + t];
          d += b * s_cd[buf][base + t];
        }
        buf ^= 1;                                // (the next chunk's stage 1 writes the other image: one barrier per chunk)
      }
      if (col_ok) {
        const double need = min_valid * (row_measure[i] * B_j);
        const float out = (d > 0.0 && d >= need) ? (float)(n / d) : nan;
        __builtin_nontemporal_store(out, dst + (int64_t)i * n_cols_out + j);
      }
    }
  }
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_conservative_regrid(const void* const* src_planes, int src_dtype, float* const* dst_planes,
                                              int n_planes, int n_lat, int n_lon, int n_rows_out, int n_cols_out,
                                              const int32_t* row_first, const int32_t* row_count, const double* row_w,
                                              const double* row_measure, const int32_t* col_first, const int32_t* col_count,
                                              const double* col_w, const double* col_measure, double min_valid, void* stream) {
  AURORA_CHECK_ARG(src_planes && dst_planes, "conservative_regrid: null plane array");
  AURORA_CHECK_ARG(row_first && row_count && row_w && row_measure && col_first && col_count && col_w && col_measure,
                   "conservative_regrid: null table pointer");
  AURORA_CHECK_ARG(src_dtype == AURORA_F32 || src_dtype == AURORA_F64,
                   "conservative_regrid: source dtype must be AURORA_F32 or AURORA_F64");
  AURORA_CHECK_ARG(n_planes >= 1 && n_lat >= 1 && n_lon >= 1 && n_rows_out >= 1 && n_cols_out >= 1,
                   "conservative_regrid: sizes must be positive (planes %d, source %d x %d, target %d x %d)", n_planes, n_lat,
                   n_lon, n_rows_out, n_cols_out);
  AURORA_CHECK_ARG(n_lon <= (1 << 28), "conservative_regrid: at most 2^28 source longitudes (got %d)", n_lon);
  AURORA_CHECK_ARG(min_valid > 0.0 && min_valid <= 1.0, "conservative_regrid: min_valid must be in (0, 1] (got %g)", min_valid);
  const int64_t row_tiles = ((int64_t)n_rows_out + kRowsPerTile - 1) / kRowsPerTile;
  const int64_t col_tiles = ((int64_t)n_cols_out + kThreads - 1) / kThreads;
  const int64_t plane_groups = ((int64_t)n_planes + kPlanesPerGroup - 1) / kPlanesPerGroup;
  AURORA_CHECK_ARG(col_tiles <= 65535 && plane_groups <= 65535,
                   "conservative_regrid: too many target columns or planes for one launch");
  const dim3 grid((unsigned)row_tiles, (unsigned)col_tiles, (unsigned)plane_groups);
  if (src_dtype == AURORA_F32)
    hipLaunchKernelGGL(conservative_kernel<float>, grid, dim3(kThreads), 0, as_stream(stream), src_planes, dst_planes,
                       n_planes, n_lat, n_lon, n_rows_out, n_cols_out, row_first, row_count, row_w, row_measure, col_first,
                       col_count, col_w, col_measure, min_valid);
  else
    hipLaunchKernelGGL(conservative_kernel<double>, grid, dim3(kThreads), 0, as_stream(stream), src_planes, dst_planes,
                       n_planes, n_lat, n_lon, n_rows_out, n_cols_out, row_first, row_count, row_w, row_measure, col_first,
                       col_count, col_w, col_measure, min_valid);
  return check_launch("conservative_regrid");
}
