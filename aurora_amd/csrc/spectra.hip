// Zonal power spectra of forecast planes on the device (aurora_amd.spectra), on the fp64 matrix pipe.
//
// The transform of a 16-row tile -- the GEMM, the folding, the staging, the table and the passes over the column tiles -- is
// zonal_dft.h's; this file is what becomes of a tile's accumulators.
// One workgroup = 8 wavefronts = one chunk of 32 grid rows of one plane, tile after tile, over all K = N/2 + 1 wavenumbers:
// N <= 1534 takes one pass.
// Epilogue per tile: power = c_k |X|^2 / N^2 for pred, truth and pred - truth; times the band's row weight (0 for a row
// that is invalid, outside the band or beyond the grid); summed over the tile's rows in a fixed order (registers ascending,
// then an xor butterfly over the four 16-lane groups) and added to the chunk's partial by the one lane that owns
// (field, band, k) -- plain loads and stores of that lane in program order, no atomics.
// spectra_finish_kernel adds a plane's chunk partials in chunk order and divides by the band's weight sum.
//
// Row validity is the tile's: a grid row that it flagged as non-finite has weight 0 in every band.
// The tree is fixed and depends on n_lat, N and has_truth only: results are repeatable bit for bit, independent of the other
// planes of the call, and independent of pointer alignment.
#include "zonal_dft.h"

namespace aurora {
namespace {

constexpr int kChunkRows = 32;                          // grid rows per workgroup
constexpr int kMaxBands = 8;

__host__ __device__ inline int64_t chunks_per_plane(int n_lat) { return ((int64_t)n_lat + kChunkRows - 1) / kChunkRows; }
// doubles of one chunk partial: (field, band, k) sums, then per band the weight sum and the count of valid rows
__host__ __device__ inline int64_t block_doubles(int n_lon, int n_bands, int has_truth) {
  return (int64_t)(has_truth ? 3 : 1) * n_bands * (n_lon / 2 + 1) + 2 * n_bands;
}
inline size_t lds_bytes(int n_lon) { return zonal_dft_lds_bytes(n_lon) + kMaxBands * 16 * sizeof(double); }

template <bool kTruth>
__global__ __launch_bounds__(kThreads) void spectra_kernel(const float* const* __restrict__ pred_planes,
                                                           const float* const* __restrict__ truth_planes, int n_lat, int N,
                                                           int n_bands, int n_chunks, const double* __restrict__ band_w,
                                                           const double* __restrict__ twiddle, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const ZonalLds lds = zonal_dft_lds(smem, N);
  int* const s_bad = lds.bad;
  double* const s_w = reinterpret_cast<double*>(lds.tail);            // [kMaxBands][16] band weight of a tile's rows

  constexpr int GR = kTruth ? 8 : 16;                                  // grid rows per tile
  constexpr int F = kTruth ? 3 : 1;
  constexpr int R = kTruth ? 2 : 4;                                    // accumulator registers per field and lane
  const int plane = (int)(blockIdx.x / (unsigned)n_chunks), chunk = (int)(blockIdx.x % (unsigned)n_chunks);
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int J = N / 2 + 1;                                             // folded length = number of wavenumbers
  const int n_coltiles = (J + 15) >> 4;
  const gptr<const float> P = (gptr<const float>)pred_planes[plane];
  const gptr<const float> T = kTruth ? (gptr<const float>)truth_planes[plane] : P;
  double* const part = partial + (int64_t)blockIdx.x * block_doubles(N, n_bands, kTruth ? 1 : 0);
  const double n2 = (double)N * (double)N;

  zonal_dft_load_table(lds.tab, twiddle, N);
  const int row_begin = chunk * kChunkRows, row_end = min(row_begin + kChunkRows, n_lat);

  for (int row0 = row_begin; row0 < row_end; row0 += GR) {
    const bool first_tile = row0 == row_begin;
    if (tid < 16) s_bad[tid] = 0;
    __syncthreads();

    for (int pass = 0; pass < n_coltiles; pass += kPassTiles) {
      const int nct = min(kColTiles, max(0, (n_coltiles - pass - wave + kWaves - 1) / kWaves));   // wave-uniform
      f64x4 acc_re[kColTiles], acc_im[kColTiles];
      zonal_dft_tile<kTruth>(lds, P, T, n_lat, N, row0, pass + wave, acc_re, acc_im);   // (s_bad is final)
      if (pass == 0) {
        if (tid < n_bands * 16) {
          const int b = tid >> 4, g = tid & 15, row = row0 + g;
          const bool live = g < GR && row < n_lat && !s_bad[g];
          s_w[tid] = live ? band_w[(int64_t)b * n_lat + row] : 0.0;
        }
        __syncthreads();
        if (tid < n_bands) {                                           // the band's weight sum and valid rows, rows ascending
          double ws = 0.0, cnt = 0.0;
          for (int g = 0; g < GR; ++g) {
            const double w = s_w[tid * 16 + g];
            if (w > 0.0) {
              ws += w;
              cnt += 1.0;
            }
          }
          double* const tail = part + (int64_t)F * n_bands * J;
          tail[tid] = first_tile ? ws : tail[tid] + ws;
          tail[n_bands + tid] = first_tile ? cnt : tail[n_bands + tid] + cnt;
        }
      }

#pragma unroll
      for (int c = 0; c < kColTiles; ++c) {
        if (c < nct) {
          const int k = 16 * (pass + c * kWaves + wave) + lc;
          const double ck = (k == 0 || 2 * k == N) ? 1.0 : 2.0;
          double pw[F][R];
#pragma unroll
          for (int i = 0; i < R; ++i) {
            const double rp = acc_re[c][i], ip = acc_im[c][i];
            pw[0][i] = (rp * rp + ip * ip) * ck / n2;
            if (kTruth) {
              const double rt = acc_re[c][i + 2], it = acc_im[c][i + 2];
              const double dr = rp - rt, di = ip - it;
              pw[F - 2][i] = (rt * rt + it * it) * ck / n2;
              pw[F - 1][i] = (dr * dr + di * di) * ck / n2;
            }
          }
          for (int b = 0; b < n_bands; ++b) {
            double w[R];
#pragma unroll
            for (int i = 0; i < R; ++i) w[i] = s_w[b * 16 + lg + 4 * i];
#pragma unroll
            for (int f = 0; f < F; ++f) {
              double v = w[0] * pw[f][0];
#pragma unroll
              for (int i = 1; i < R; ++i) v += w[i] * pw[f][i];
              v += __shfl_xor(v, 16, 64);
              v += __shfl_xor(v, 32, 64);
              if (lg == 0 && k < J) {
                double* const dst = part + ((int64_t)f * n_bands + b) * J + k;
                *dst = first_tile ? v : *dst + v;
              }
            }
          }
        }
      }
    }
  }
}

// power[plane][field][band][k] = (sum of the chunk partials in chunk order) / (the band's weight sum); NaN and rows = 0 for
// a band without a valid row.  One lane per output value.
__global__ __launch_bounds__(256) void spectra_finish_kernel(const double* __restrict__ partial, int n_planes, int n_fields,
                                                            int n_bands, int K, int n_chunks, double* __restrict__ power,
                                                            int64_t* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_plane = (int64_t)n_fields * n_bands * K;
  if (i >= n_planes * per_plane) return;
  const int64_t plane = i / per_plane, rest = i % per_plane;
  const int f = (int)(rest / ((int64_t)n_bands * K)), b = (int)((rest / K) % n_bands), k = (int)(rest % K);
  const int64_t block = per_plane + 2 * n_bands;
  const double* p = partial + plane * n_chunks * block;
  double v = 0.0, ws = 0.0, cnt = 0.0;
  for (int c = 0; c < n_chunks; ++c, p += block) {
    v += p[rest];
    ws += p[per_plane + b];
    cnt += p[per_plane + n_bands + b];
  }
  power[i] = cnt > 0.0 ? v / ws : __builtin_nan("");
  if (f == 0 && k == 0) rows[plane * n_bands + b] = (int64_t)cnt;
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_spectra_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_bands, int has_truth) {
  if (n_planes < 1 || n_lat < 1 || n_lon < 2 || n_lon > kMaxLon || n_bands < 1 || n_bands > kMaxBands) return 0;
  return (size_t)n_planes * (size_t)chunks_per_plane(n_lat) * (size_t)block_doubles(n_lon, n_bands, has_truth ? 1 : 0) *
         sizeof(double);
}

extern "C" int aurora_hip_spectra(const float* const* pred_planes, const float* const* truth_planes, int n_planes, int n_lat,
                                  int n_lon, int n_bands, const double* band_w, const double* twiddle, double* power,
                                  int64_t* rows, void* workspace, size_t workspace_bytes, void* stream) {
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1, "spectra: bad sizes (planes %d, grid %d x %d)", n_planes, n_lat, n_lon);
  AURORA_CHECK_ARG(n_lon >= 2 && n_lon <= kMaxLon, "spectra: n_lon must be in 2..%d, got %d", kMaxLon, n_lon);
  AURORA_CHECK_ARG(n_bands >= 1 && n_bands <= kMaxBands, "spectra: n_bands must be in 1..%d, got %d", kMaxBands, n_bands);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(pred_planes && band_w && twiddle && power && rows && workspace,
                   "spectra: null plane array, weight, table, output or workspace pointer");
  AURORA_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)power | (uintptr_t)rows | (uintptr_t)band_w | (uintptr_t)twiddle) & 7) == 0,
                   "spectra: weights, table, outputs and workspace must be 8-byte aligned");
  const size_t need = aurora_hip_spectra_workspace_bytes(n_planes, n_lat, n_lon, n_bands, truth_planes != nullptr);
  AURORA_CHECK_ARG(workspace_bytes >= need, "spectra: the workspace holds %zu bytes, %zu are needed", workspace_bytes, need);
  const int64_t n_chunks = chunks_per_plane(n_lat);
  const int64_t groups = n_chunks * n_planes;
  const int K = n_lon / 2 + 1, n_fields = truth_planes ? 3 : 1;
  const int64_t values = (int64_t)n_planes * n_fields * n_bands * K;
  AURORA_CHECK_ARG(groups <= 0x7fffffff && (values + 255) / 256 <= 0x7fffffff,
                   "spectra: too many planes for one launch (%d planes x %lld row chunks)", n_planes, (long long)n_chunks);
  once_per_device([] {
    const int most = (int)lds_bytes(kMaxLon);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&spectra_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&spectra_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, most);
  });
  double* const partial = (double*)workspace;
  const size_t lds = lds_bytes(n_lon);
  if (truth_planes)
    hipLaunchKernelGGL(spectra_kernel<true>, dim3((unsigned)groups), dim3(kThreads), lds, as_stream(stream), pred_planes,
                       truth_planes, n_lat, n_lon, n_bands, (int)n_chunks, band_w, twiddle, partial);
  else
    hipLaunchKernelGGL(spectra_kernel<false>, dim3((unsigned)groups), dim3(kThreads), lds, as_stream(stream), pred_planes,
                       truth_planes, n_lat, n_lon, n_bands, (int)n_chunks, band_w, twiddle, partial);
  const int code = check_launch("spectra");
  if (code != AURORA_OK) return code;
  hipLaunchKernelGGL(spectra_finish_kernel, dim3((unsigned)((values + 255) / 256)), dim3(256), 0, as_stream(stream), partial,
                     n_planes, n_fields, n_bands, K, (int)n_chunks, power, rows);
  return check_launch("spectra (finish)");
}
