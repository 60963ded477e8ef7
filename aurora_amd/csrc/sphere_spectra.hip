// Spherical-harmonic power spectra of forecast planes on the device (aurora_amd.sphere_spectra), on the fp64 matrix pipe.
// THE RULE is stated in aurora_amd/sphere_spectra.py and repeated in include/aurora_hip.h; the index arithmetic of the table
// and of the workspace is in sphere_spectra_index.h.  Three launches:
//
// 1. Zonal stage (sphere_zonal_kernel): F_m(i) = (1/N) sum_n x_i[n] exp(-2 pi i m n / N) for m = 0 .. lmax of every row, by the
//    folded DFT tile of zonal_dft.h, which spectra.hip multiplies with too: tile rows = 16 grid rows of the prediction or, with
//    a truth, 8 grid rows of the prediction and the SAME 8 of the truth (a row's validity is one flag for both).  Only the
//    column tiles with m <= lmax are multiplied, in one pass (lmax < 512 keeps them under the 48 of a pass).  The tile is
//    written to the workspace as (re, im) in the order [plane][field][m][i].  A non-finite value is staged as 0 and flags its
//    row: a flagged pole row is written as zeros in every field and counted, any other flagged row marks the plane invalid;
//    both go to the (plane, row chunk) flag words of the workgroup -- plain stores, no atomics.
// 2. Legendre stage (sphere_legendre_kernel): one wavefront per (16 degrees l, segment of 16 consecutive m <= l, 16 planes).  For
//    every m of its segment, a_lm = sum_i A[m][l][i] F_m(i) is a 16 x H by H x 16 GEMM on v_mfma_f64_16x16x4_f64: operand A the
//    table (rows l, K = latitude in steps of 4), operand B the planes' F (real and imaginary parts in separate accumulators fed
//    the same table operand; with a truth the truth's two accumulators sit in the same lane, so the error coefficient is a
//    difference of two accumulators of one lane).  c_m |a_lm|^2 is added in registers, m ascending, and the segment's sum goes
//    to the workspace.  A table entry with l < m, l > lmax or i >= H is never read: the index is clamped into the array and the
//    operand replaced by 0.  The segments depend on lmax alone, so the tree is a function of (H, N, lmax, has_truth).
// 3. Finish (sphere_finish_kernel): adds a (plane, field, l)'s segments in m order, writes NaN for an invalid plane, and the
//    plane's `valid` and `pole_rows_dropped` from its chunks' flag words.
//
// Every load of a plane is a 4-byte load; the planes of a call share nothing but the launch; nothing is read back.
#include "sphere_spectra_index.h"
#include "sphere_zonal.h"
#include "zonal_dft.h"

namespace aurora {
namespace {

constexpr int kSteps = 4;                               // K-steps of 4 latitudes per turn of the Legendre loop

inline size_t zonal_lds_bytes(int n_lon) { return zonal_dft_lds_bytes(n_lon) + 16 * sizeof(int); }

// ---- 1. the zonal stage ---------------------------------------------------------------------------------------------------
// pole_rows: bit 0 -- row 0 is a pole (|lat| = 90), bit 1 -- row n_lat - 1 is one.
template <bool kTruth>
__global__ __launch_bounds__(kThreads) void sphere_zonal_kernel(const float* const* __restrict__ pred_planes,
                                                                const float* const* __restrict__ truth_planes, int n_lat, int N,
                                                                int lmax, int pole_rows, const double* __restrict__ twiddle,
                                                                f64x2* __restrict__ F, int* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const ZonalLds lds = zonal_dft_lds(smem, N);
  int* const s_bad = lds.bad;
  int* const s_zero = reinterpret_cast<int*>(lds.tail);                // [16] s_bad, as the tile's epilogue reads it

  constexpr int GR = kTruth ? 8 : 16;                                  // grid rows per tile
  constexpr int NI = kTruth ? 2 : 1;
  constexpr int R = kTruth ? 2 : 4;                                    // accumulator registers per field and lane
  const int n_chunks = sphere_chunks(n_lat);
  const int plane = (int)(blockIdx.x / (unsigned)n_chunks), chunk = (int)(blockIdx.x % (unsigned)n_chunks);
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int n_coltiles = (lmax + 16) >> 4;                             // the columns m = 0 .. lmax
  const gptr<const float> P = (gptr<const float>)pred_planes[plane];
  const gptr<const float> T = kTruth ? (gptr<const float>)truth_planes[plane] : P;
  const double inv_n = 1.0 / (double)N;

  zonal_dft_load_table(lds.tab, twiddle, N);
  const int row_begin = chunk * kSphereChunkRows, row_end = min(row_begin + kSphereChunkRows, n_lat);
  int invalid = 0, dropped = 0;                                        // of the chunk: thread 0 keeps them

  for (int row0 = row_begin; row0 < row_end; row0 += GR) {
    if (tid < 16) s_bad[tid] = 0;
    __syncthreads();

    // One pass: n_lat >= 2 lmax + 1 and the table's cap of 1 GiB keep lmax below 512: at most 32 column tiles, under kPassTiles.
    const int nct = min(kColTiles, max(0, (n_coltiles - wave + kWaves - 1) / kWaves));   // wave-uniform
    f64x4 acc_re[kColTiles], acc_im[kColTiles];
    zonal_dft_tile<kTruth>(lds, P, T, n_lat, N, row0, wave, acc_re, acc_im);   // (s_bad is final)
    if (tid < 16) s_zero[tid] = s_bad[tid];
    if (tid == 0) {
      for (int g = 0; g < GR; ++g) {
        const int row = row0 + g;
        if (row < n_lat && s_bad[g]) {
          const bool pole = (row == 0 && (pole_rows & 1)) || (row == n_lat - 1 && (pole_rows & 2));
          if (pole) ++dropped;
          else invalid = 1;
        }
      }
    }
    __syncthreads();

#pragma unroll
    for (int c = 0; c < kColTiles; ++c) {
      if (c < nct) {
        const int m = 16 * (c * kWaves + wave) + lc;
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const int g = lg + 4 * i, row = row0 + g;                    // (with a truth: registers i and i + 2 of grid row g)
          if (m <= lmax && row < n_lat) {
            const bool zero = s_zero[g] != 0;
            const f64x2 vp = {zero ? 0.0 : acc_re[c][i] * inv_n, zero ? 0.0 : -(acc_im[c][i] * inv_n)};
            F[sphere_f_offset(lmax, n_lat, NI, plane, 0, m, row)] = vp;
            if (kTruth) {
              const f64x2 vt = {zero ? 0.0 : acc_re[c][i + 2] * inv_n, zero ? 0.0 : -(acc_im[c][i + 2] * inv_n)};
              F[sphere_f_offset(lmax, n_lat, NI, plane, 1, m, row)] = vt;
            }
          }
        }
      }
    }
  }
  if (tid == 0) {
    flags[sphere_flag_offset(n_lat, plane, chunk, 0)] = invalid;
    flags[sphere_flag_offset(n_lat, plane, chunk, 1)] = dropped;
  }
}

// ---- 2. the Legendre stage ------------------------------------------------------------------------------------------------
// grid: x = tile (tile + 1) / 2 + segment, over the tiles of 16 degrees and, of each, the segments 0 .. tile of m (a later
// segment holds no m <= l for any degree of the tile: it is neither launched nor added); y = group of 16 planes; one wavefront
// per workgroup.
template <bool kTruth>
__global__ __launch_bounds__(64) void sphere_legendre_kernel(const double* __restrict__ table, const f64x2* __restrict__ F,
                                                             int H, int lmax, int n_planes, double* __restrict__ partial) {
  constexpr int NI = kTruth ? 2 : 1, NO = kTruth ? 3 : 1;
  int tile = 0;
  while ((tile + 1) * (tile + 2) / 2 <= (int)blockIdx.x) ++tile;      // (at most 128 turns: lmax <= 2047)
  const int l0 = 16 * tile, seg = (int)blockIdx.x - tile * (tile + 1) / 2;
  const int lane = (int)threadIdx.x, lg = lane >> 4, lc = lane & 15;
  const int plane = (int)blockIdx.y * 16 + lc;
  const int plane_c = min(plane, n_planes - 1);                        // (a column beyond the planes repeats the last, unwritten)
  const int l = l0 + lc;                                               // operand A: this lane's degree
  const int m_begin = seg * kSphereSegment;
  const int m_end = min(min(m_begin + kSphereSegment, lmax + 1), l0 + 16);   // no degree of the tile is below a later m

  f64x4 S[NO];
#pragma unroll
  for (int f = 0; f < NO; ++f) S[f] = f64x4{0.0, 0.0, 0.0, 0.0};

  for (int m = m_begin; m < m_end; ++m) {
    const bool live = l >= m && l <= lmax;
    const gptr<const double> a_row = (gptr<const double>)(table + sphere_table_offset(lmax, H, m, live ? l : m, 0));
    const gptr<const f64x2> f_p = (gptr<const f64x2>)(F + sphere_f_offset(lmax, H, NI, plane_c, 0, m, 0));
    const gptr<const f64x2> f_t = (gptr<const f64x2>)(F + sphere_f_offset(lmax, H, NI, plane_c, NI - 1, m, 0));
    f64x4 pr = {0.0, 0.0, 0.0, 0.0}, pi = pr, tr = pr, ti = pr;
    for (int i0 = 0; i0 < H; i0 += 4 * kSteps) {                       // kSteps K-steps a turn: their loads are issued together
      double av[kSteps];
      f64x2 p[kSteps], t[kSteps];
#pragma unroll
      for (int u = 0; u < kSteps; ++u) {
        const int i = i0 + 4 * u + lg;
        const bool in = i < H;
        const int ic = in ? i : H - 1;                                 // (a step beyond the rows multiplies zeros)
        const double a = a_row[ic];
        p[u] = f_p[ic];
        if (kTruth) t[u] = f_t[ic];
        av[u] = (live && in) ? a : 0.0;
        if (!in) p[u] = t[u] = f64x2{0.0, 0.0};
      }
#pragma unroll
      for (int u = 0; u < kSteps; ++u) {
        pr = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], p[u].x, pr, 0, 0, 0);
        pi = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], p[u].y, pi, 0, 0, 0);
        if (kTruth) {
          tr = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], t[u].x, tr, 0, 0, 0);
          ti = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], t[u].y, ti, 0, 0, 0);
        }
      }
    }
    const double cm = m == 0 ? 1.0 : 2.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                      // degree l0 + lg + 4 r of plane lc; 0 where l < m
      S[0][r] += cm * (pr[r] * pr[r] + pi[r] * pi[r]);
      if (kTruth) {
        const double dr = pr[r] - tr[r], di = pi[r] - ti[r];
        S[NO - 2][r] += cm * (tr[r] * tr[r] + ti[r] * ti[r]);
        S[NO - 1][r] += cm * (dr * dr + di * di);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lr = l0 + lg + 4 * r;
    if (lr <= lmax && plane < n_planes) {
#pragma unroll
      for (int f = 0; f < NO; ++f) partial[sphere_partial_offset(lmax, NO, plane, f, seg, lr)] = S[f][r];
    }
  }
}

// ---- 3. the finish ----------------------------------------------------------------------------------------------------------
// One lane per (plane, field, l): the segments that hold an m <= l, in m order; NaN for an invalid plane; the lane of (field 0, l = 0) writes the
// plane's `valid` and `pole_rows_dropped`.
__global__ __launch_bounds__(256) void sphere_finish_kernel(const double* __restrict__ partial, const int* __restrict__ flags,
                                                           int n_planes, int n_out, int H, int lmax, double* __restrict__ power,
                                                           uint8_t* __restrict__ valid, int32_t* __restrict__ pole_rows_dropped) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_plane = (int64_t)n_out * (lmax + 1);
  if (i >= n_planes * per_plane) return;
  const int plane = (int)(i / per_plane), f = (int)((i % per_plane) / (lmax + 1)), l = (int)(i % (lmax + 1));
  const int n_seg = l / kSphereSegment + 1, n_chunks = sphere_chunks(H);   // the segments with an m <= l
  int invalid = 0, dropped = 0;
  for (int c = 0; c < n_chunks; ++c) {
    invalid |= flags[sphere_flag_offset(H, plane, c, 0)];
    dropped += flags[sphere_flag_offset(H, plane, c, 1)];
  }
  double v = 0.0;
  for (int s = 0; s < n_seg; ++s) v += partial[sphere_partial_offset(lmax, n_out, plane, f, s, l)];
  power[i] = invalid ? __builtin_nan("") : v;
  if (f == 0 && l == 0) {
    valid[plane] = invalid ? 0 : 1;
    pole_rows_dropped[plane] = dropped;
  }
}

}  // namespace

// Launch one, for this call and for aurora_hip_sphere_analysis (sphere_transform.hip), which has no copy of the kernel: the
// zonal stage of checked arguments on `s`, with a truth where truth_planes is given.  F is the workspace's f64x2 part.
int sphere_zonal_launch(const float* const* pred_planes, const float* const* truth_planes, int n_planes, int n_lat, int n_lon,
                        int lmax, int pole_rows, const double* twiddle, void* F, int* flags, hipStream_t s) {
  once_per_device([] {
    const int most = (int)zonal_lds_bytes(kMaxLon);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sphere_zonal_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sphere_zonal_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
  });
  const unsigned zonal_groups = (unsigned)((int64_t)sphere_chunks(n_lat) * n_planes);
  const size_t lds = zonal_lds_bytes(n_lon);
  if (truth_planes)
    hipLaunchKernelGGL(sphere_zonal_kernel<true>, dim3(zonal_groups), dim3(kThreads), lds, s, pred_planes, truth_planes, n_lat,
                       n_lon, lmax, pole_rows, twiddle, (f64x2*)F, flags);
  else
    hipLaunchKernelGGL(sphere_zonal_kernel<false>, dim3(zonal_groups), dim3(kThreads), lds, s, pred_planes, truth_planes, n_lat,
                       n_lon, lmax, pole_rows, twiddle, (f64x2*)F, flags);
  return check_launch("sphere_spectra (zonal)");
}

}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_sphere_spectra_workspace_bytes(int n_planes, int n_lat, int n_lon, int lmax, int has_truth) {
  if (n_planes < 1 || n_lat < 2 || n_lon < 2 || n_lon > kMaxLon || lmax < 0 || lmax > sphere_exact_lmax(n_lat, n_lon)) return 0;
  return (size_t)sphere_workspace_bytes(lmax, n_lat, has_truth ? 1 : 0, n_planes);
}

extern "C" int aurora_hip_sphere_spectra(const float* const* pred_planes, const float* const* truth_planes, int n_planes,
                                         int n_lat, int n_lon, int lmax, int pole_rows, const double* table,
                                         const double* twiddle, double* power, uint8_t* valid, int32_t* pole_rows_dropped,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 2, "sphere_spectra: bad sizes (planes %d, grid %d x %d)", n_planes, n_lat, n_lon);
  AURORA_CHECK_ARG(n_lon >= 2 && n_lon <= kMaxLon, "sphere_spectra: n_lon must be in 2..%d, got %d", kMaxLon, n_lon);
  AURORA_CHECK_ARG(lmax >= 0 && lmax <= sphere_exact_lmax(n_lat, n_lon),
                   "sphere_spectra: lmax must be in 0..%d on a %d x %d grid (the quadrature is exact up to min((n_lat - 1) / 2, "
                   "(n_lon - 1) / 2)), got %d", sphere_exact_lmax(n_lat, n_lon), n_lat, n_lon, lmax);
  AURORA_CHECK_ARG(sphere_table_doubles(lmax, n_lat) * 8 <= kSphereTableCap,
                   "sphere_spectra: the table of lmax %d on %d rows takes %lld bytes, above the cap of 1 GiB; the largest lmax "
                   "that fits is %d", lmax, n_lat, (long long)(sphere_table_doubles(lmax, n_lat) * 8), sphere_largest_lmax(n_lat));
  AURORA_CHECK_ARG((pole_rows & ~3) == 0, "sphere_spectra: pole_rows must be 0..3, got %d", pole_rows);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(pred_planes && table && twiddle && power && valid && pole_rows_dropped && workspace,
                   "sphere_spectra: null plane array, table, output or workspace pointer");
  AURORA_CHECK_ARG((((uintptr_t)power | (uintptr_t)table | (uintptr_t)twiddle) & 7) == 0 && ((uintptr_t)workspace & 15) == 0 &&
                       ((uintptr_t)pole_rows_dropped & 3) == 0,
                   "sphere_spectra: misaligned pointer (tables and power: 8 bytes, workspace: 16, pole_rows_dropped: 4)");
  const int has_truth = truth_planes != nullptr;
  const size_t need = aurora_hip_sphere_spectra_workspace_bytes(n_planes, n_lat, n_lon, lmax, has_truth);
  AURORA_CHECK_ARG(workspace_bytes >= need, "sphere_spectra: the workspace holds %zu bytes, %zu are needed", workspace_bytes, need);
  const int n_in = has_truth ? 2 : 1, n_out = has_truth ? 3 : 1;
  const int64_t zonal_groups = (int64_t)sphere_chunks(n_lat) * n_planes;
  const int64_t n_tiles = (lmax + 16) / 16, tiles = n_tiles * (n_tiles + 1) / 2, plane_groups = ((int64_t)n_planes + 15) / 16;
  const int64_t values = (int64_t)n_planes * n_out * (lmax + 1);
  AURORA_CHECK_ARG(zonal_groups <= 0x7fffffff && tiles <= 0x7fffffff && plane_groups <= 65535 && (values + 255) / 256 <= 0x7fffffff,
                   "sphere_spectra: too many planes for one launch (%d planes)", n_planes);
  f64x2* const F = (f64x2*)workspace;
  double* const partial = (double*)((char*)workspace + sphere_f_bytes(lmax, n_lat, n_in, n_planes));
  int* const flags = (int*)((char*)partial + sphere_partial_bytes(lmax, n_out, n_planes));
  const hipStream_t s = as_stream(stream);
  int code = sphere_zonal_launch(pred_planes, truth_planes, n_planes, n_lat, n_lon, lmax, pole_rows, twiddle, F, flags, s);
  if (code != AURORA_OK) return code;
  if (has_truth)
    hipLaunchKernelGGL(sphere_legendre_kernel<true>, dim3((unsigned)tiles, (unsigned)plane_groups), dim3(64), 0, s, table, F, n_lat,
                       lmax, n_planes, partial);
  else
    hipLaunchKernelGGL(sphere_legendre_kernel<false>, dim3((unsigned)tiles, (unsigned)plane_groups), dim3(64), 0, s, table, F, n_lat,
                       lmax, n_planes, partial);
  code = check_launch("sphere_spectra (legendre)");
  if (code != AURORA_OK) return code;
  hipLaunchKernelGGL(sphere_finish_kernel, dim3((unsigned)((values + 255) / 256)), dim3(256), 0, s, partial, flags, n_planes, n_out,
                     n_lat, lmax, power, valid, pole_rows_dropped);
  return check_launch("sphere_spectra (finish)");
}
