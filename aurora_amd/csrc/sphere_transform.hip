// Spherical-harmonic analysis and synthesis of forecast planes on the device (aurora_amd.sphere_transform), on the fp64 matrix
// pipe.  THE RULE is stated in aurora_amd/sphere_transform.py and repeated in include/aurora_hip.h; the index arithmetic of the
// tables, the coefficients and the workspaces is in sphere_spectra_index.h.
//
// aurora_hip_sphere_analysis, two launches:
// 1. the zonal stage of aurora_hip_sphere_spectra without a truth (sphere_zonal_launch: the kernel lives in sphere_spectra.hip);
// 2. sphere_coefficients_kernel: the Legendre stage of sphere_spectra.hip -- one wavefront per (16 degrees l, segment of 16
//    consecutive m, 16 planes), a_lm = sum_i A[m][l][i] F_m(i) on v_mfma_f64_16x16x4_f64 with K = latitude in steps of 4, the
//    table index clamped into the array and the operand replaced by 0 where l < m, l > lmax or i >= H -- which STORES the (re,
//    im) accumulators of each m where that kernel squares them.  The planes are the tile's rows and the degrees its columns
//    (the same loads and products as in sphere_spectra.hip with the two operands exchanged), so that a lane group stores 16
//    consecutive degrees of one plane.  Every (tile, segment) pair is launched, those with l < m throughout included: the call
//    writes every element of the dense output, 0 where l < m and NaN for an invalid plane, from the zonal stage's flag words;
//    the wavefronts of (tile 0, segment 0) write `valid` and `pole_rows_dropped`.
//
// aurora_hip_sphere_synthesis, two launches:
// 1. sphere_ilegendre_kernel: G_m(i) = sum_{l = m .. lmax} b_lm P[m][l][i], a triangular batch of fp64 GEMMs: one wavefront per
//    (16 latitudes, one m, 16 planes), K = the degree from m upwards in steps of 4 (a step beyond lmax multiplies zeros, its
//    indices clamped), real and imaginary parts in two accumulators fed the same table operand; G goes to the workspace as
//    (re, im) in the layout [plane][m][i] of the analysis' F.
// 2. sphere_izonal_kernel: the folded inverse tile of zonal_idft.h per 16 grid rows; the epilogue forms E - O and E + O, rounds
//    once and writes both halves of the row with 4-byte stores; a plane whose `valid` is 0 is written as NaN.
//
// No atomics; the planes of a call share nothing but the launch; nothing is read back.
#include "sphere_spectra_index.h"
#include "sphere_zonal.h"
#include "zonal_idft.h"

namespace aurora {
namespace {

constexpr int kSteps = 4;                               // K-steps of 4 per turn of either Legendre loop
constexpr int kLatWaves = 4;                            // wavefronts (latitude tiles) per workgroup of the inverse Legendre stage

// ---- analysis, launch two ---------------------------------------------------------------------------------------------------
// grid: x = tile * n_seg + segment over the tiles of 16 degrees and ALL segments of 16 m; y = group of 16 planes; one wavefront
// per workgroup.  Lane (lg, lc): operand A is F of plane 16 y + lc, operand B the table row of degree 16 tile + lc, both at
// latitude i0 + lg; the accumulators hold planes 16 y + lg + 4 r, degree 16 tile + lc.
__global__ __launch_bounds__(64) void sphere_coefficients_kernel(const double* __restrict__ table, const f64x2* __restrict__ F,
                                                                 const int* __restrict__ flags, int H, int lmax, int n_planes,
                                                                 f64x2* __restrict__ coeff, uint8_t* __restrict__ valid,
                                                                 int32_t* __restrict__ pole_rows_dropped) {
  const int n_seg = sphere_segments(lmax);
  const int tile = (int)blockIdx.x / n_seg, seg = (int)blockIdx.x % n_seg;
  const int l0 = 16 * tile;
  const int lane = (int)threadIdx.x, lg = lane >> 4, lc = lane & 15;
  const int plane_c = min((int)blockIdx.y * 16 + lc, n_planes - 1);    // (a row beyond the planes repeats the last, unwritten)
  const int l = l0 + lc;
  const int m_begin = seg * kSphereSegment, m_end = min(m_begin + kSphereSegment, lmax + 1);

  const int n_chunks = sphere_chunks(H);
  bool invalid[4];
  int dropped[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {                                        // of the planes this lane stores
    const int p = min((int)blockIdx.y * 16 + lg + 4 * r, n_planes - 1);
    int bad = 0, n = 0;
    for (int c = 0; c < n_chunks; ++c) {
      bad |= flags[sphere_flag_offset(H, p, c, 0)];
      n += flags[sphere_flag_offset(H, p, c, 1)];
    }
    invalid[r] = bad != 0;
    dropped[r] = n;
  }

  for (int m = m_begin; m < m_end; ++m) {
    f64x4 re = {0.0, 0.0, 0.0, 0.0}, im = re;
    if (m < l0 + 16) {                                                 // (wave-uniform: a later m is above every degree of the tile)
      const bool live = l >= m && l <= lmax;
      const gptr<const double> a_row = (gptr<const double>)(table + sphere_table_offset(lmax, H, m, live ? l : m, 0));
      const gptr<const f64x2> f_p = (gptr<const f64x2>)(F + sphere_f_offset(lmax, H, 1, plane_c, 0, m, 0));
      for (int i0 = 0; i0 < H; i0 += 4 * kSteps) {                     // kSteps K-steps a turn: their loads are issued together
        double av[kSteps];
        f64x2 p[kSteps];
#pragma unroll
        for (int u = 0; u < kSteps; ++u) {
          const int i = i0 + 4 * u + lg;
          const bool in = i < H;
          const int ic = in ? i : H - 1;                               // (a step beyond the rows multiplies zeros)
          const double a = a_row[ic];
          p[u] = f_p[ic];
          av[u] = (live && in) ? a : 0.0;
          if (!in) p[u] = f64x2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < kSteps; ++u) {
          re = __builtin_amdgcn_mfma_f64_16x16x4f64(p[u].x, av[u], re, 0, 0, 0);
          im = __builtin_amdgcn_mfma_f64_16x16x4f64(p[u].y, av[u], im, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                      // plane 16 y + lg + 4 r, degree l
      const int plane = (int)blockIdx.y * 16 + lg + 4 * r;
      if (l <= lmax && plane < n_planes) {
        const double nan = __builtin_nan("");
        f64x2 v = l >= m ? f64x2{re[r], im[r]} : f64x2{0.0, 0.0};
        if (invalid[r]) v = f64x2{nan, nan};
        coeff[sphere_coeff_offset(lmax, plane, m, l)] = v;
      }
    }
  }

  if (blockIdx.x == 0 && lc == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int plane = (int)blockIdx.y * 16 + lg + 4 * r;
      if (plane < n_planes) {
        valid[plane] = invalid[r] ? 0 : 1;
        pole_rows_dropped[plane] = dropped[r];
      }
    }
  }
}

// ---- synthesis, launch one --------------------------------------------------------------------------------------------------
// grid: x = group of kLatWaves tiles of 16 latitudes (a wavefront each), y = m, z = group of 16 planes.  Lane (lg, lc): operand A
// is b_lm of plane 16 z + lc, operand B the table at latitude i0 + lc, both at degree l0 + lg; the accumulators hold planes
// 16 z + lg + 4 r, latitude i0 + lc.
__global__ __launch_bounds__(64 * kLatWaves) void sphere_ilegendre_kernel(const double* __restrict__ table,
                                                                          const f64x2* __restrict__ coeff, int H, int lmax,
                                                                          int n_planes, f64x2* __restrict__ G) {
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63, lg = lane >> 4, lc = lane & 15;
  const int i0 = ((int)blockIdx.x * kLatWaves + wave) * 16;
  if (i0 >= H) return;                                                 // (wave-uniform; the kernel has no barrier)
  const int m = (int)blockIdx.y;
  const int plane_c = min((int)blockIdx.z * 16 + lc, n_planes - 1);
  const int i = i0 + lc;
  const bool row_in = i < H;
  const gptr<const double> p_col = (gptr<const double>)(table + sphere_table_offset(lmax, H, m, m, row_in ? i : H - 1));
  const gptr<const f64x2> b_row = (gptr<const f64x2>)(coeff + sphere_coeff_offset(lmax, plane_c, m, 0));

  f64x4 re = {0.0, 0.0, 0.0, 0.0}, im = re;
  for (int l0 = m; l0 <= lmax; l0 += 4 * kSteps) {
    double av[kSteps];
    f64x2 b[kSteps];
#pragma unroll
    for (int u = 0; u < kSteps; ++u) {
      const int l = l0 + 4 * u + lg;
      const bool in = l <= lmax;
      const int lcl = in ? l : lmax;                                   // (a step beyond lmax multiplies zeros)
      const double a = p_col[(int64_t)(lcl - m) * H];
      b[u] = b_row[lcl];
      av[u] = (in && row_in) ? a : 0.0;
      if (!in) b[u] = f64x2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < kSteps; ++u) {
      re = __builtin_amdgcn_mfma_f64_16x16x4f64(b[u].x, av[u], re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f64_16x16x4f64(b[u].y, av[u], im, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int plane = (int)blockIdx.z * 16 + lg + 4 * r;
    if (row_in && plane < n_planes) G[sphere_f_offset(lmax, H, 1, plane, 0, m, i)] = f64x2{re[r], im[r]};
  }
}

// ---- synthesis, launch two --------------------------------------------------------------------------------------------------
// One workgroup = 8 wavefronts = one chunk of 32 grid rows of one plane, tile after tile, over the columns n = 0 .. N/2 in
// passes of 768.
__global__ __launch_bounds__(kThreads) void sphere_izonal_kernel(const f64x2* __restrict__ G, const uint8_t* __restrict__ valid,
                                                                 int n_lat, int N, int lmax, const double* __restrict__ twiddle,
                                                                 float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const ZonalLds lds = zonal_dft_lds(smem, N);
  const int n_chunks = sphere_chunks(n_lat);
  const int plane = (int)(blockIdx.x / (unsigned)n_chunks), chunk = (int)(blockIdx.x % (unsigned)n_chunks);
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int K = N / 2 + 1, n_coltiles = (K + 15) >> 4;                 // the columns n = 0 .. N/2
  const gptr<float> Y = (gptr<float>)(out + (int64_t)plane * n_lat * N);
  const int row_begin = chunk * kSphereChunkRows, row_end = min(row_begin + kSphereChunkRows, n_lat);

  if (valid != nullptr && valid[plane] == 0) {                         // (uniform over the workgroup)
    const float nan = __builtin_nanf("");
    for (int64_t e = (int64_t)row_begin * N + tid; e < (int64_t)row_end * N; e += kThreads) Y[e] = nan;
    return;
  }
  const gptr<const f64x2> Gp = (gptr<const f64x2>)(G + sphere_f_offset(lmax, n_lat, 1, plane, 0, 0, 0));
  zonal_dft_load_table(lds.tab, twiddle, N);

  for (int row0 = row_begin; row0 < row_end; row0 += 16) {
    for (int pass = 0; pass < n_coltiles; pass += kPassTiles) {
      const int nct = min(kColTiles, max(0, (n_coltiles - pass - wave + kWaves - 1) / kWaves));   // wave-uniform
      f64x4 acc_e[kColTiles], acc_o[kColTiles];
      zonal_idft_tile(lds, Gp, n_lat, lmax, N, row0, pass + wave, acc_e, acc_o);
#pragma unroll
      for (int c = 0; c < kColTiles; ++c) {
        if (c < nct) {
          const int n = 16 * (pass + c * kWaves + wave) + lc;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = row0 + lg + 4 * r;
            if (n < K && row < row_end) {
              const double e = acc_e[c][r], o = acc_o[c][r];
              Y[(int64_t)row * N + n] = (float)(e - o);
              if (n > 0 && 2 * n != N) Y[(int64_t)row * N + (N - n)] = (float)(e + o);
            }
          }
        }
      }
    }
  }
}

inline size_t izonal_lds_bytes(int n_lon) { return zonal_dft_lds_bytes(n_lon); }

}  // namespace
}  // namespace aurora

using namespace aurora;

static bool sphere_sizes_ok(int n_planes, int n_lat, int n_lon, int lmax) {
  return n_planes >= 1 && n_lat >= 2 && n_lon >= 2 && n_lon <= kMaxLon && lmax >= 0 && lmax <= sphere_exact_lmax(n_lat, n_lon);
}

extern "C" size_t aurora_hip_sphere_analysis_workspace_bytes(int n_planes, int n_lat, int n_lon, int lmax) {
  return sphere_sizes_ok(n_planes, n_lat, n_lon, lmax) ? (size_t)sphere_analysis_workspace_bytes(lmax, n_lat, n_planes) : 0;
}

extern "C" size_t aurora_hip_sphere_synthesis_workspace_bytes(int n_planes, int n_lat, int n_lon, int lmax) {
  return sphere_sizes_ok(n_planes, n_lat, n_lon, lmax) ? (size_t)sphere_synthesis_workspace_bytes(lmax, n_lat, n_planes) : 0;
}

// The checks the two calls share; `fn` starts the message.
static int sphere_check_sizes(const char* fn, int n_planes, int n_lat, int n_lon, int lmax) {
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 2, "%s: bad sizes (planes %d, grid %d x %d)", fn, n_planes, n_lat, n_lon);
  AURORA_CHECK_ARG(n_lon >= 2 && n_lon <= kMaxLon, "%s: n_lon must be in 2..%d, got %d", fn, kMaxLon, n_lon);
  AURORA_CHECK_ARG(lmax >= 0 && lmax <= sphere_exact_lmax(n_lat, n_lon),
                   "%s: lmax must be in 0..%d on a %d x %d grid (the quadrature is exact up to min((n_lat - 1) / 2, "
                   "(n_lon - 1) / 2)), got %d", fn, sphere_exact_lmax(n_lat, n_lon), n_lat, n_lon, lmax);
  AURORA_CHECK_ARG(sphere_table_doubles(lmax, n_lat) * 8 <= kSphereTableCap,
                   "%s: the table of lmax %d on %d rows takes %lld bytes, above the cap of 1 GiB; the largest lmax that fits "
                   "is %d", fn, lmax, n_lat, (long long)(sphere_table_doubles(lmax, n_lat) * 8), sphere_largest_lmax(n_lat));
  return AURORA_OK;
}

extern "C" int aurora_hip_sphere_analysis(const float* const* planes, int n_planes, int n_lat, int n_lon, int lmax, int pole_rows,
                                          const double* table, const double* twiddle, double* coeff, uint8_t* valid,
                                          int32_t* pole_rows_dropped, void* workspace, size_t workspace_bytes, void* stream) {
  int code = sphere_check_sizes("sphere_analysis", n_planes, n_lat, n_lon, lmax);
  if (code != AURORA_OK) return code;
  AURORA_CHECK_ARG((pole_rows & ~3) == 0, "sphere_analysis: pole_rows must be 0..3, got %d", pole_rows);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(planes && table && twiddle && coeff && valid && pole_rows_dropped && workspace,
                   "sphere_analysis: null plane array, table, output or workspace pointer");
  AURORA_CHECK_ARG((((uintptr_t)table | (uintptr_t)twiddle) & 7) == 0 && (((uintptr_t)workspace | (uintptr_t)coeff) & 15) == 0 &&
                       ((uintptr_t)pole_rows_dropped & 3) == 0,
                   "sphere_analysis: misaligned pointer (tables: 8 bytes, coefficients and workspace: 16, pole_rows_dropped: 4)");
  const size_t need = aurora_hip_sphere_analysis_workspace_bytes(n_planes, n_lat, n_lon, lmax);
  AURORA_CHECK_ARG(workspace_bytes >= need, "sphere_analysis: the workspace holds %zu bytes, %zu are needed", workspace_bytes, need);
  const int64_t zonal_groups = (int64_t)sphere_chunks(n_lat) * n_planes;
  const int64_t n_seg = sphere_segments(lmax), tiles = n_seg * n_seg, plane_groups = ((int64_t)n_planes + 15) / 16;
  AURORA_CHECK_ARG(zonal_groups <= 0x7fffffff && tiles <= 0x7fffffff && plane_groups <= 65535,
                   "sphere_analysis: too many planes for one launch (%d planes)", n_planes);
  f64x2* const F = (f64x2*)workspace;
  int* const flags = (int*)((char*)workspace + sphere_f_bytes(lmax, n_lat, 1, n_planes));
  const hipStream_t s = as_stream(stream);
  code = sphere_zonal_launch(planes, nullptr, n_planes, n_lat, n_lon, lmax, pole_rows, twiddle, F, flags, s);
  if (code != AURORA_OK) return code;
  hipLaunchKernelGGL(sphere_coefficients_kernel, dim3((unsigned)tiles, (unsigned)plane_groups), dim3(64), 0, s, table, F, flags,
                     n_lat, lmax, n_planes, (f64x2*)coeff, valid, pole_rows_dropped);
  return check_launch("sphere_analysis (legendre)");
}

extern "C" int aurora_hip_sphere_synthesis(const double* coeff, const uint8_t* valid, int n_planes, int n_lat, int n_lon, int lmax,
                                           const double* table, const double* twiddle, float* out, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  int code = sphere_check_sizes("sphere_synthesis", n_planes, n_lat, n_lon, lmax);
  if (code != AURORA_OK) return code;
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(coeff && table && twiddle && out && workspace,
                   "sphere_synthesis: null coefficient, table, output or workspace pointer");
  AURORA_CHECK_ARG((((uintptr_t)table | (uintptr_t)twiddle) & 7) == 0 && (((uintptr_t)workspace | (uintptr_t)coeff) & 15) == 0 &&
                       ((uintptr_t)out & 3) == 0,
                   "sphere_synthesis: misaligned pointer (tables: 8 bytes, coefficients and workspace: 16, out: 4)");
  const size_t need = aurora_hip_sphere_synthesis_workspace_bytes(n_planes, n_lat, n_lon, lmax);
  AURORA_CHECK_ARG(workspace_bytes >= need, "sphere_synthesis: the workspace holds %zu bytes, %zu are needed", workspace_bytes, need);
  const int64_t zonal_groups = (int64_t)sphere_chunks(n_lat) * n_planes;
  const int64_t lat_groups = ((int64_t)n_lat + 16 * kLatWaves - 1) / (16 * kLatWaves), plane_groups = ((int64_t)n_planes + 15) / 16;
  AURORA_CHECK_ARG(zonal_groups <= 0x7fffffff && plane_groups <= 65535 && lmax + 1 <= 65535,
                   "sphere_synthesis: too many planes for one launch (%d planes)", n_planes);
  once_per_device([] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sphere_izonal_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)izonal_lds_bytes(kMaxLon));
  });
  f64x2* const G = (f64x2*)workspace;
  const hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(sphere_ilegendre_kernel, dim3((unsigned)lat_groups, (unsigned)(lmax + 1), (unsigned)plane_groups),
                     dim3(64 * kLatWaves), 0, s, table, (const f64x2*)coeff, n_lat, lmax, n_planes, G);
  code = check_launch("sphere_synthesis (legendre)");
  if (code != AURORA_OK) return code;
  hipLaunchKernelGGL(sphere_izonal_kernel, dim3((unsigned)zonal_groups), dim3(kThreads), izonal_lds_bytes(n_lon), s, G, valid, n_lat,
                     n_lon, lmax, twiddle, out);
  return check_launch("sphere_synthesis (zonal)");
}
