// The inverse of zonal_dft.h's tile: a 16-row tile of grid rows from their zonal coefficients G_m(i), m = 0 .. lmax < N / 2, on
// the fp64 matrix pipe, FOLDED: for the columns n = 0 .. N/2
//     E[n] = sum_m c_m Re G_m cos(2 pi m n / N),   O[n] = sum_m c_m Im G_m sin(2 pi m n / N),   c_0 = 1, c_m = 2 otherwise,
// and the caller writes y[n] = E - O and, for 0 < n < N/2, y[N - n] = E + O: half the multiplications of the direct form.
// It is the forward tile's GEMM with other operands, and multiplies with the forward tile's own functions (next_operands,
// multiply_step, multiply_chunk), table in LDS and pass structure:
//   M      16 grid rows;
//   K-dim  the zonal wavenumber m, staged in LDS 128 at a time as the pairs (c_m Re G, c_m Im G) in the place of the forward
//          tile's folded (p, m) pairs; an m beyond lmax and a row beyond the grid are staged as zeros (their index clamped);
//   N-dim  the columns n, B[m][n] = table[(m n) mod N]: the product form of the forward tile with j = m and k = n.
// Accumulation is the MFMA's own fp64 accumulator, m ascending.  Device code: not for a host-compilable header.
#pragma once
#include "zonal_dft.h"

namespace aurora {
namespace {

// The tile of the grid rows from row0 times the wavefront's column tiles tile0 + 8 c, c = 0 .. 5: on return out_e[c][r] = E[n]
// and out_o[c][r] = O[n] for n = 16 (tile0 + 8 c) + (lane & 15) and tile row (lane >> 4) + 4 r.  G: the plane's coefficients,
// [m][i] pairs (re, im), n_lat per m.  Called by the whole workgroup; the table is in lds.tab.
__device__ __forceinline__ void zonal_idft_tile(const ZonalLds& lds, gptr<const f64x2> G, int n_lat, int lmax, int N, int row0,
                                                int tile0, f64x4 (&out_e)[kColTiles], f64x4 (&out_o)[kColTiles]) {
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int lg = lane >> 4, lc = lane & 15;
  const int J = lmax + 1;                                              // length of the m sum
  const int sr = tid & 15, sj = tid >> 4;                              // staging role: tile row sr, wavenumbers sj + 32 q of a chunk
  static_assert(kThreads / 16 * kStageQ == kChunkJ, "a chunk is staged by the workgroup in kStageQ turns");

  f64x4 acc_e[kColTiles], acc_o[kColTiles];                            // (local, copied out once: see zonal_dft_tile)
  int idx[kColTiles], step[kColTiles];
#pragma unroll
  for (int c = 0; c < kColTiles; ++c) {
    acc_e[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    acc_o[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int n = 16 * (tile0 + c * kWaves) + lc;
    idx[c] = (int)(((unsigned)lg * (unsigned)n) % (unsigned)N);
    step[c] = (int)((4u * (unsigned)n) % (unsigned)N);
  }

  f64x2 g[kStageQ];
  const int row = row0 + sr;
  auto fetch = [&](int j0) {
#pragma unroll
    for (int q = 0; q < kStageQ; ++q) {
      const int m = j0 + sj + (kThreads / 16) * q;
      const bool in = m < J && row < n_lat;
      const f64x2 v = G[(int64_t)(in ? m : 0) * n_lat + (in ? row : 0)];
      g[q] = in ? v : f64x2{0.0, 0.0};
    }
  };
  fetch(0);

  for (int j0 = 0; j0 < J; j0 += kChunkJ) {
    __syncthreads();                                                   // the previous chunk has been multiplied
#pragma unroll
    for (int q = 0; q < kStageQ; ++q) {
      const int ml = sj + (kThreads / 16) * q;
      const double cm = (j0 + ml) == 0 ? 1.0 : 2.0;
      lds.a[ml * kAStride + sr] = f64x2{cm * g[q].x, cm * g[q].y};     // (times 1 or 2: exact)
    }
    __syncthreads();
    if (j0 + kChunkJ < J) fetch(j0 + kChunkJ);

    const int steps = (min(kChunkJ, J - j0) + 3) >> 2;
    multiply_chunk(lds.a + lg * kAStride + lc, lds.tab, steps, N, idx, step, acc_e, acc_o);
  }
#pragma unroll
  for (int c = 0; c < kColTiles; ++c) {
    out_e[c] = acc_e[c];
    out_o[c] = acc_o[c];
  }
}

}  // namespace
}  // namespace aurora
