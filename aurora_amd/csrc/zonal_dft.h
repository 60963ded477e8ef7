// The folded zonal DFT of a 16-row tile on the fp64 matrix pipe: the one copy that spectra.hip (spectra_kernel) and
// sphere_spectra.hip (sphere_zonal_kernel) both multiply with.  Device code: not for a host-compilable header.
//
// For every row x[0 .. N-1] of a plane (n_lat x N fp32, row-major) the real DFT X[k], k = 0 .. K-1, K = N/2 + 1, is a GEMM:
//   M          the rows of a 16-row MFMA tile: 16 grid rows of the prediction, or, with a truth, 8 grid rows of the
//              prediction (tile rows 0-7) and the SAME 8 grid rows of the truth (tile rows 8-15), so that the error spectrum
//              |X_pred - X_truth|^2 is a difference of two accumulators of one lane;
//   K-dim      longitude, FOLDED: with p[j] = x[j] + x[N-j], m[j] = x[j] - x[N-j] for 0 < j < N/2, p[j] = x[j], m[j] = 0 for
//              j = 0 and j = N/2,     Re X[k] = sum_j p[j] cos(2 pi j k / N),   -Im X[k] = sum_j m[j] sin(2 pi j k / N)
//              over j = 0 .. K-1: half the multiplications of the direct form, one extra rounding per input pair;
//   N-dim      the K cosine and the K sine columns (a caller may want only the first of them).
// Operand A: the fp32 rows are read coalesced, converted to fp64 (exact), folded, and staged in LDS 128 folded columns at a
// time as (p, m) pairs; the next chunk's global loads are in flight while the current one is multiplied.  Operand B is never
// a matrix in memory: B[j][k] = table[(j k) mod N] from the N-entry (cos, sin) table in LDS; a lane walks j in steps of 4
// for its column k, so its index advances by (4 k) mod N with one conditional subtract.  Accumulation is the MFMA's own
// fp64 accumulator, j ascending.
//
// One workgroup = 8 wavefronts works through its rows tile after tile.  A wavefront owns up to 6 16-column tiles (column
// tile = pass + 8 c + wave): 768 columns per pass over the rows, so 768 columns or fewer take one pass and the rows are read
// once; more columns re-read the tile's rows (from L2) once per further pass.
//
// Row validity comes from the inputs: while staging, a non-finite value flags its grid row in s_bad and is replaced by 0.
// The tree depends on N and kTruth only, and every global load of a plane is a 4-byte load, so a tile's accumulators do not
// depend on pointer alignment.  The tile is independent of the height of the caller's row chunk.
#pragma once
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
constexpr int kMaxLon = 4096;
constexpr int kStageQ = 16 * kChunkJ / kThreads;        // staged values per thread and chunk (4)

// The tile's share of the dynamic LDS, from its start; a kernel's own words follow at `tail`.
struct ZonalLds {
  f64x2* tab;                                           // [N] (cos, sin)
  f64x2* a;                                             // [kChunkJ][kAStride] (p, m)
  int* bad;                                             // [16] a grid row of the tile holds a non-finite value
  unsigned char* tail;
};
inline size_t zonal_dft_lds_bytes(int n_lon) { return (size_t)(n_lon + kChunkJ * kAStride) * sizeof(f64x2) + 16 * sizeof(int); }

__device__ __forceinline__ ZonalLds zonal_dft_lds(unsigned char* smem, int N) {
  f64x2* const tab = reinterpret_cast<f64x2*>(smem);
  f64x2* const a = tab + N;
  int* const bad = reinterpret_cast<int*>(a + kChunkJ * kAStride);
  return {tab, a, bad, reinterpret_cast<unsigned char*>(bad + 16)};
}

// Before the first tile, by the whole workgroup (the tile's first barrier orders it).
__device__ __forceinline__ void zonal_dft_load_table(f64x2* s_tab, const double* __restrict__ twiddle, int N) {
  for (int m = (int)threadIdx.x; m < N; m += kThreads) s_tab[m] = f64x2{twiddle[2 * m], twiddle[2 * m + 1]};
}

// One staged chunk times the table for the wavefront's six column tiles: `steps` k-steps of 4 folded columns, no branch
// inside: seven LDS reads, then twelve MFMAs that start as their operands arrive (the workgroup keeps two wavefronts on
// every SIMD, so one wavefront's reads are in flight under the other's MFMAs).  (A column tile beyond the caller's last
// column is multiplied like the others -- its table indices stay inside the table -- and never written.)
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

// The tile of the grid rows from row0 (16 of P, or with kTruth 8 of P and the same 8 of T) times the wavefront's column tiles
// tile0 + 8 c, c = 0 .. 5, tile0 = pass + wave (wave-uniform; the caller has the wave number in a scalar register already):
// on return out_re[c][i] = Re X[k], out_im[c][i] = -Im X[k] for k = 16 (tile0 + 8 c) + (lane & 15) and tile row
// (lane >> 4) + 4 i, a row beyond the grid as zeros, and s_bad is final for the tile: the caller has cleared it, with a
// barrier, before the tile's first pass.  Called by the whole workgroup.
template <bool kTruth>
__device__ __forceinline__ void zonal_dft_tile(const ZonalLds& lds, gptr<const float> P, gptr<const float> T, int n_lat, int N,
                                               int row0, int tile0, f64x4 (&out_re)[kColTiles], f64x4 (&out_im)[kColTiles]) {
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int lg = lane >> 4, lc = lane & 15;
  const int J = N / 2 + 1;                                             // folded length
  const int jl = tid & (kChunkJ - 1), sm = tid >> 7;                   // staging role: folded column jl, tile rows sm + 4 q

  // (Local accumulators, copied out once: the compiler optimises this function before it inlines it, and accumulators behind
  //  the references are memory in its loops then -- both kernels ended at 256 VGPRs with scratch that way.)
  f64x4 acc_re[kColTiles], acc_im[kColTiles];
  int idx[kColTiles], step[kColTiles];
#pragma unroll
  for (int c = 0; c < kColTiles; ++c) {
    acc_re[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    acc_im[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int k = 16 * (tile0 + c * kWaves) + lc;
    idx[c] = (int)(((unsigned)lg * (unsigned)k) % (unsigned)N);
    step[c] = (int)((4u * (unsigned)k) % (unsigned)N);
  }

  float ga[kStageQ], gb[kStageQ];
  auto fetch = [&](int j0) {                                           // the chunk's values of this thread, raw
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
    __syncthreads();                                                   // the previous chunk has been multiplied
    {
      const int j = j0 + jl;
      const bool has_b = j > 0 && 2 * j != N && j < J;
#pragma unroll
      for (int q = 0; q < kStageQ; ++q) {
        const int m = sm + 4 * q;
        const bool ok = __builtin_isfinite(ga[q]) && __builtin_isfinite(gb[q]);
        if (!ok) lds.bad[kTruth ? (m & 7) : m] = 1;
        const double a = (double)(ok ? ga[q] : 0.f), b = (double)(ok ? gb[q] : 0.f);
        lds.a[jl * kAStride + m] = f64x2{a + b, has_b ? a - b : 0.0};
      }
    }
    __syncthreads();
    if (j0 + kChunkJ < J) fetch(j0 + kChunkJ);

    const int steps = (min(kChunkJ, J - j0) + 3) >> 2;
    multiply_chunk(lds.a + lg * kAStride + lc, lds.tab, steps, N, idx, step, acc_re, acc_im);
  }
  __syncthreads();                                                     // every row of the tile has been seen: s_bad is final
#pragma unroll
  for (int c = 0; c < kColTiles; ++c) {
    out_re[c] = acc_re[c];
    out_im[c] = acc_im[c];
  }
}

}  // namespace
}  // namespace aurora
