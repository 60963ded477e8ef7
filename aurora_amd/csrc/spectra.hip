// Zonal power spectra of forecast planes on the device (aurora_amd.spectra), on the fp64 matrix pipe.
//
// For every row x[0 .. N-1] of a plane (n_lat x N fp32, row-major) the real DFT X[k], k = 0 .. K-1, K = N/2 + 1, is a GEMM:
//   M          the rows of a 16-row MFMA tile: 16 grid rows of the prediction, or, with a truth, 8 grid rows of the
//              prediction (tile rows 0-7) and the SAME 8 grid rows of the truth (tile rows 8-15), so that the error spectrum
//              |X_pred - X_truth|^2 is a difference of two accumulators of one lane;
//   K-dim      longitude, FOLDED: with p[j] = x[j] + x[N-j], m[j] = x[j] - x[N-j] for 0 < j < N/2, p[j] = x[j], m[j] = 0 for
//              j = 0 and j = N/2,     Re X[k] = sum_j p[j] cos(2 pi j k / N),   -Im X[k] = sum_j m[j] sin(2 pi j k / N)
//              over j = 0 .. K-1: half the multiplications of the direct form, one extra rounding per input pair;
//   N-dim      the K cosine and the K sine columns.
// Operand A: the fp32 rows are read coalesced, converted to fp64 (exact), folded, and staged in LDS 128 folded columns at a
// time as (p, m) pairs; the next chunk's global loads are in flight while the current one is multiplied.  Operand B is never
// a matrix in memory: B[j][k] = table[(j k) mod N] from the N-entry (cos, sin) table in LDS; a lane walks j in steps of 4
// for its column k, so its index advances by (4 k) mod N with one conditional subtract.  Accumulation is the MFMA's own
// fp64 accumulator, j ascending.
//
// One workgroup = 8 wavefronts = one chunk of 32 grid rows of one plane, tile after tile.  A wavefront owns up to 6
// 16-column tiles (column tile = pass + 8 c + wave): 768 columns per pass over the rows, so N <= 1534 takes one pass and the
// rows are read once; a larger N re-reads the tile's rows (from L2) once per further pass.
// Epilogue per tile: power = c_k |X|^2 / N^2 for pred, truth and pred - truth; times the band's row weight (0 for a row
// that is invalid, outside the band or beyond the grid); summed over the tile's rows in a fixed order (registers ascending,
// then an xor butterfly over the four 16-lane groups) and added to the chunk's partial by the one lane that owns
// (field, band, k) -- plain loads and stores of that lane in program order, no atomics.
// spectra_finish_kernel adds a plane's chunk partials in chunk order and divides by the band's weight sum.
//
// Row validity comes from the inputs: while staging, a non-finite value flags its grid row and is replaced by 0.
// The tree is fixed and depends on n_lat, N and has_truth only: results are repeatable bit for bit, independent of the other
// planes of the call, and independent of pointer alignment (every global load of a plane is a 4-byte load).
#include "planes.h"

namespace aurora {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kColTiles = 6;                            // 16-column tiles per wavefront and pass
constexpr int kPassTiles = kWaves * kColTiles;          // 48 tiles = 768 columns per pass
constexpr int kChunkJ = 128;                            // folded columns staged at a time
constexpr int kAStride = 17;                            // (p, m) pairs per staged column: 16 tile rows + 1 (bank spread)
constexpr int kChunkRows = 32;                          // grid rows per workgroup
constexpr int kMaxBands = 8;
constexpr int kMaxLon = 4096;
constexpr int kStageQ = 16 * kChunkJ / kThreads;        // staged values per thread and chunk (4)


__host__ __device__ inline int64_t chunks_per_plane(int n_lat) { return ((int64_t)n_lat + kChunkRows - 1) / kChunkRows; }
// doubles of one chunk partial: (field, band, k) sums, then per band the weight sum and the count of valid rows
__host__ __device__ inline int64_t block_doubles(int n_lon, int n_bands, int has_truth) {
  return (int64_t)(has_truth ? 3 : 1) * n_bands * (n_lon / 2 + 1) + 2 * n_bands;
}
inline size_t lds_bytes(int n_lon) {
  return (size_t)(n_lon + kChunkJ * kAStride) * sizeof(f64x2) + kMaxBands * 16 * sizeof(double) + 16 * sizeof(int);
}

// One staged chunk times the table for the wavefront's six column tiles: `steps` k-steps of 4 folded columns, no branch
// inside: seven LDS reads, then twelve MFMAs that start as their operands arrive (the workgroup keeps two wavefronts on
// every SIMD, so one wavefront's reads are in flight under the other's MFMAs).  (A column tile beyond the last wavenumber is
// multiplied like the others -- its table indices stay inside the table -- and never written.)
__device__ __forceinline__ void next_operands(const f64x2* __restrict__ s_tab, int N, int (&idx)[kColTiles],
                                              const int (&step)[kColTiles], f64x2 (&tw)[kColTiles]) {
#pragma unroll
  for (int c = 0; c < kColTiles; ++c) {
    tw[c] = s_tab[idx[c]];
    const int t = idx[c] + step[c];
    idx[c] = t >= N ? t - N : t;
  }
}

__device__ __forceinline__ void multiply_step(const f64x2 av, const f64x2 (&tw)[kColTiles], f64x4 (&acc_re)[kColTiles],
                                              f64x4 (&acc_im)[kColTiles]) {
#pragma unroll
  for (int c = 0; c < kColTiles; ++c) {
    acc_re[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, tw[c].x, acc_re[c], 0, 0, 0);
    acc_im[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, tw[c].y, acc_im[c], 0, 0, 0);
  }
}

__device__ __forceinline__ void multiply_chunk(const f64x2* __restrict__ a_ptr, const f64x2* __restrict__ s_tab, int steps,
                                               int N, int (&idx)[kColTiles], const int (&step)[kColTiles],
                                               f64x4 (&acc_re)[kColTiles], f64x4 (&acc_im)[kColTiles]) {
  for (int s = 0; s < steps; ++s) {
    f64x2 tw[kColTiles];
    const f64x2 av = a_ptr[s * 4 * kAStride];
    next_operands(s_tab, N, idx, step, tw);
    multiply_step(av, tw, acc_re, acc_im);
  }
}

template <bool kTruth>
__global__ __launch_bounds__(kThreads) void spectra_kernel(const float* const* __restrict__ pred_planes,
                                                           const float* const* __restrict__ truth_planes, int n_lat, int N,
                                                           int n_bands, int n_chunks, const double* __restrict__ band_w,
                                                           const double* __restrict__ twiddle, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  f64x2* const s_tab = reinterpret_cast<f64x2*>(smem);                 // [N] (cos, sin)
  f64x2* const s_a = s_tab + N;                                        // [kChunkJ][kAStride] (p, m)
  double* const s_w = reinterpret_cast<double*>(s_a + kChunkJ * kAStride);   // [kMaxBands][16] band weight of a tile's rows
  int* const s_bad = reinterpret_cast<int*>(s_w + kMaxBands * 16);     // [16] a grid row of the tile holds a non-finite value

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

  for (int m = tid; m < N; m += kThreads) s_tab[m] = f64x2{twiddle[2 * m], twiddle[2 * m + 1]};

  // staging role of this thread: folded column jl of the chunk, tile rows sm + 4 q
  const int jl = tid & (kChunkJ - 1), sm = tid >> 7;
  const int row_begin = chunk * kChunkRows, row_end = min(row_begin + kChunkRows, n_lat);

  for (int row0 = row_begin; row0 < row_end; row0 += GR) {
    const bool first_tile = row0 == row_begin;
    if (tid < 16) s_bad[tid] = 0;
    __syncthreads();

    for (int pass = 0; pass < n_coltiles; pass += kPassTiles) {
      const int nct = min(kColTiles, max(0, (n_coltiles - pass - wave + kWaves - 1) / kWaves));   // wave-uniform
      f64x4 acc_re[kColTiles], acc_im[kColTiles];
      int idx[kColTiles], step[kColTiles];
#pragma unroll
      for (int c = 0; c < kColTiles; ++c) {
        acc_re[c] = f64x4{0.0, 0.0, 0.0, 0.0};
        acc_im[c] = f64x4{0.0, 0.0, 0.0, 0.0};
        const int k = 16 * (pass + c * kWaves + wave) + lc;
        idx[c] = (int)(((unsigned)lg * (unsigned)k) % (unsigned)N);
        step[c] = (int)((4u * (unsigned)k) % (unsigned)N);
      }

      float ga[kStageQ], gb[kStageQ];
      auto fetch = [&](int j0) {                                       // the chunk's values of this thread, raw
        const int j = j0 + jl;
        const bool has_b = j > 0 && 2 * j != N && j < J;
#pragma unroll
        for (int q = 0; q < kStageQ; ++q) {
          const int m = sm + 4 * q;
          const int row = row0 + (kTruth ? (m & 7) : m);
          const gptr<const float> src = (kTruth && m >= 8) ? T : P;
          const bool in = j < J && row < n_lat;
          const int64_t base = (int64_t)(in ? row : 0) * N;
          ga[q] = in ? src[base + j] : 0.f;
          gb[q] = (in && has_b) ? src[base + (N - j)] : 0.f;
        }
      };
      fetch(0);

      for (int j0 = 0; j0 < J; j0 += kChunkJ) {
        __syncthreads();                                               // the previous chunk has been multiplied
        {
          const int j = j0 + jl;
          const bool has_b = j > 0 && 2 * j != N && j < J;
#pragma unroll
          for (int q = 0; q < kStageQ; ++q) {
            const int m = sm + 4 * q;
            const bool ok = __builtin_isfinite(ga[q]) && __builtin_isfinite(gb[q]);
            if (!ok) s_bad[kTruth ? (m & 7) : m] = 1;
            const double a = (double)(ok ? ga[q] : 0.f), b = (double)(ok ? gb[q] : 0.f);
            s_a[jl * kAStride + m] = f64x2{a + b, has_b ? a - b : 0.0};
          }
        }
        __syncthreads();
        if (j0 + kChunkJ < J) fetch(j0 + kChunkJ);

        const int steps = (min(kChunkJ, J - j0) + 3) >> 2;
        const f64x2* a_ptr = s_a + lg * kAStride + lc;
        multiply_chunk(a_ptr, s_tab, steps, N, idx, step, acc_re, acc_im);
      }

      __syncthreads();                                                 // every row of the tile has been seen: s_bad is final
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
