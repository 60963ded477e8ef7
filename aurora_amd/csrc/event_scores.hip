// Categorical verification on the device (aurora_amd.event_scores): for every plane, threshold and window size the three
// integer row sums behind the Fractions Skill Score and, at window size 1, the contingency table.
//
// For one plane (n_lat x n_lon fp32, row-major), threshold thr (fp32) and odd window size n = 2 h + 1:
//   valid(i,j) = pred and truth are both finite;     f = valid && pred >= thr,   o = valid && truth >= thr   (<= with `below`;
//   a NaN threshold gives no event);    cf(i,j) = sum_{|di|<=h, |dj|<=h} f(i+di, (j+dj) mod n_lon), rows outside the grid and
//   invalid points counting 0;  co likewise.  Over the VALID centre columns j of row i:
//   rowsums[(((plane T + t) S + s) n_lat + i) 3 + {0, 1, 2}] = sum_j (cf - co)^2,  sum_j cf^2,  sum_j co^2;
//   valid[plane n_lat + i] = the number of valid points of row i.
//
// One workgroup = 256 lanes = one plane, 256 consecutive EXTENDED columns (a tile of W = 256 - 2 h_max centre columns plus h_max
// halo columns on each side, wrapped modulo n_lon; h_max belongs to the largest window of the call) and a segment of 128 centre
// rows plus h_max halo rows above and below.  A lane owns one extended column and walks the rows top to bottom:
//   * each pred / truth value is loaded once per workgroup (4-byte loads, the next row's in flight under the current row's
//     work) and becomes a 16-bit word -- T pred bits, T truth bits -- in an LDS ring of 2 h_max + 2 rows; the column's valid
//     bits ride in a 64-bit shift register of the lane;
//   * per window size the lane keeps the vertical counts of its column, four thresholds to a register as bytes (<= 63 each):
//     + the bits of the entering row, - those of the leaving row (its own ring column: no barrier);
//   * per centre row and window size the counts, two thresholds to a register as 16-bit lanes, are summed horizontally by
//     doubling in LDS: W1 = the counts, W2[j] = W1[j] + W1[j+1], W4[j] = W2[j] + W2[j+2], ... and the window is put together
//     from the binary digits of n (n = 33: W32 + W1) -- log2(n) barriers instead of n reads;
//   * the three squares (and the valid flag) of the 256 lanes are added through LDS and the nonzero sums go to the tables by
//     64-bit integer vector atomics.  Integer addition is associative: the result does not depend on the order.
// No plane-sized temporary, no workspace; the tables are cleared by a small launch of their own in front (plain vector stores).
//
// Integer ranges: a vertical count <= n <= 63 (a byte); a window count <= n^2 <= 3969 (a 16-bit lane; every doubling level
// is a partial window, so it is bounded likewise); one lane's square <= 3969^2 = 15 752 961; the sum over a tile's 256 lanes
// <= 256 x 15 752 961 = 4 032 758 016 < 2^32, so the workgroup's reduction is exact in 32 bits; everything after it (the
// atomics, the tables) is 64-bit: an entry <= 4096 x 63^4 < 2^36.
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;          // extended columns of a tile; the 32-bit reduction bound above needs <= 272
constexpr int kRows = 128;             // centre rows of a workgroup
constexpr int kMaxT = 8, kMaxS = 8, kMaxN = 63, kMaxLon = 4096;
constexpr int kMaxLevels = 6;          // W1, W2, W4, W8, W16, W32: one per binary digit of the largest window size
static_assert((1 << kMaxLevels) > kMaxN && (1 << (kMaxLevels - 1)) <= kMaxN, "kMaxLevels must be the number of binary digits of kMaxN");


struct ScaleList {
  int n[kMaxS];
};

__host__ __device__ inline int levels_for(int n_max) {
  int l = 1;
  while ((2 << (l - 1)) <= n_max) ++l;
  return l;
}
inline int ring_rows_for(int h_max) { return 2 * h_max + 2; }
inline size_t lds_bytes(int h_max, int n_max, int T, int TH) {
  return (size_t)ring_rows_for(h_max) * kThreads * 2 + (size_t)levels_for(n_max) * 4 * TH * kThreads * 4 +
         (size_t)(3 * T + 1) * kThreads * 4;
}

// bit k of x (k = 0 .. 3) -> bit 0 of byte k: the products land on 16 distinct bit positions, so nothing carries
__device__ __forceinline__ uint32_t spread4(uint32_t x) { return ((x & 0xfu) * 0x00204081u) & 0x01010101u; }

// TH: registers of four thresholds each (T <= 4 TH)
template <int TH>
__global__ __launch_bounds__(kThreads) void event_scores_kernel(const float* const* __restrict__ pred_planes,
                                                                const float* const* __restrict__ truth_planes, int n_lat,
                                                                int n_lon, const float* __restrict__ thresholds, int T,
                                                                ScaleList sc, int S, int below, int tiles, int segs,
                                                                unsigned long long* __restrict__ rowsums,
                                                                unsigned long long* __restrict__ valid) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NP = 2 * TH;                                           // registers of two 16-bit lanes per field
  constexpr int NA = 2 * NP;                                           // arrays per doubling level: (field, pair)
  const int n_max = sc.n[S - 1], h_max = n_max >> 1;
  const int ring_rows = 2 * h_max + 2, levels = levels_for(n_max);
  uint16_t* const s_ring = reinterpret_cast<uint16_t*>(smem);                                    // [ring_rows][256]
  uint32_t* const s_w = reinterpret_cast<uint32_t*>(smem + (size_t)ring_rows * kThreads * 2);    // [levels][NA][256]
  uint32_t* const s_red = s_w + levels * NA * kThreads;                                          // [3 T + 1][256]

  const int tid = (int)threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int seg = (int)((blockIdx.x / (unsigned)tiles) % (unsigned)segs);
  const int64_t plane = (int64_t)(blockIdx.x / ((unsigned)tiles * (unsigned)segs));
  const int W = kThreads - 2 * h_max;
  const int col0 = tile * W;
  int g = (col0 - h_max + tid) % n_lon;                                // the grid column of this lane, wrapped
  if (g < 0) g += n_lon;
  const bool centre = tid >= h_max && tid < h_max + W && col0 + (tid - h_max) < n_lon;
  const int r0 = seg * kRows, r1 = min(r0 + kRows, n_lat);
  const int y_first = r0 - h_max, y_last = r1 - 1 + h_max;
  const gptr<const float> P = (gptr<const float>)pred_planes[plane];
  const gptr<const float> Q = (gptr<const float>)truth_planes[plane];

  float thr[kMaxT];
#pragma unroll
  for (int t = 0; t < kMaxT; ++t) thr[t] = t < T ? thresholds[plane * T + t] : __builtin_nanf("");

  // ring positions of the entering and the leaving row of every window size, relative to y_first (negative: not loaded)
  int rel_e[kMaxS], rel_l[kMaxS], pos_e[kMaxS], pos_l[kMaxS];
#pragma unroll
  for (int s = 0; s < kMaxS; ++s) {
    const int h = s < S ? sc.n[s] >> 1 : 0;
    rel_e[s] = -(h_max - h);
    rel_l[s] = -(h_max + h + 1);
    pos_e[s] = ((rel_e[s] % ring_rows) + ring_rows) % ring_rows;
    pos_l[s] = ((rel_l[s] % ring_rows) + ring_rows) % ring_rows;
  }
  int pos_y = 0;

  uint32_t cnt[kMaxS][2][TH];                                          // vertical counts: [window size][field][4 thresholds]
#pragma unroll
  for (int s = 0; s < kMaxS; ++s)
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int hh = 0; hh < TH; ++hh) cnt[s][f][hh] = 0;
  uint64_t valid_bits = 0;                                             // bit k: the point of row y - k of this column is valid

  const float nanf_ = __builtin_nanf("");
  auto in_grid = [&](int y) { return y >= 0 && y < n_lat && y <= y_last; };
  float p_next = in_grid(y_first) ? P[(int64_t)y_first * n_lon + g] : nanf_;
  float q_next = in_grid(y_first) ? Q[(int64_t)y_first * n_lon + g] : nanf_;

  for (int y = y_first; y <= y_last; ++y) {
    const float p = p_next, q = q_next;
    if (in_grid(y + 1)) {
      p_next = P[(int64_t)(y + 1) * n_lon + g];
      q_next = Q[(int64_t)(y + 1) * n_lon + g];
    } else {
      p_next = q_next = nanf_;
    }
    const bool ok = __builtin_isfinite(p) && __builtin_isfinite(q);    // (a row outside the grid arrives as NaN: no bits)
    uint32_t word = 0;
#pragma unroll
    for (int t = 0; t < 4 * TH; ++t) {
      const bool f = ok && (below ? p <= thr[t] : p >= thr[t]);
      const bool o = ok && (below ? q <= thr[t] : q >= thr[t]);
      word |= (f ? 1u : 0u) << t;
      word |= (o ? 1u : 0u) << (8 + t);
    }
    s_ring[pos_y * kThreads + tid] = (uint16_t)word;
    valid_bits = (valid_bits << 1) | (ok ? 1u : 0u);

    // vertical counts: the lane reads its own ring column, so no barrier is needed
#pragma unroll
    for (int s = 0; s < kMaxS; ++s) {
      if (s < S) {
        const uint32_t win = rel_e[s] >= 0 ? s_ring[pos_e[s] * kThreads + tid] : 0u;
        const uint32_t wout = rel_l[s] >= 0 ? s_ring[pos_l[s] * kThreads + tid] : 0u;
#pragma unroll
        for (int hh = 0; hh < TH; ++hh) {                              // (count + entering) first: no byte ever borrows
          cnt[s][0][hh] = cnt[s][0][hh] + spread4(win >> (4 * hh)) - spread4(wout >> (4 * hh));
          cnt[s][1][hh] = cnt[s][1][hh] + spread4(win >> (8 + 4 * hh)) - spread4(wout >> (8 + 4 * hh));
        }
        ++rel_e[s];
        ++rel_l[s];
        pos_e[s] = pos_e[s] + 1 == ring_rows ? 0 : pos_e[s] + 1;
        pos_l[s] = pos_l[s] + 1 == ring_rows ? 0 : pos_l[s] + 1;
      }
    }
    pos_y = pos_y + 1 == ring_rows ? 0 : pos_y + 1;

    const int i = y - h_max;                                           // the centre row whose windows are now complete
    if (i < r0) continue;                                              // (uniform)
    const bool cv = centre && ((valid_bits >> h_max) & 1u);            // a valid centre point
    __syncthreads();                                                   // the previous row's reduction has read s_red

#pragma unroll
    for (int s = 0; s < kMaxS; ++s) {
      if (s < S) {
        const int n = sc.n[s], h = n >> 1;
        uint32_t sum[NA];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
          for (int hh = 0; hh < TH; ++hh) {
            sum[f * NP + 2 * hh] = cnt[s][f][hh] & 0x00ff00ffu;            // thresholds 4 hh + 0 (low lane), 4 hh + 2
            sum[f * NP + 2 * hh + 1] = (cnt[s][f][hh] >> 8) & 0x00ff00ffu; // thresholds 4 hh + 1, 4 hh + 3
          }
        if (n > 1) {
          uint32_t cur[NA];
#pragma unroll
          for (int a = 0; a < NA; ++a) {
            cur[a] = sum[a];
            s_w[a * kThreads + tid] = cur[a];
          }
          __syncthreads();
          for (int k = 1; (1 << k) <= n; ++k) {                        // W_{2^k}[j] = W_{2^(k-1)}[j] + W_{2^(k-1)}[j + 2^(k-1)]
            const int far = tid + (1 << (k - 1));
            const uint32_t* const prev = s_w + (k - 1) * NA * kThreads;
            uint32_t* const next = s_w + k * NA * kThreads;
#pragma unroll
            for (int a = 0; a < NA; ++a) {
              cur[a] += far < kThreads ? prev[a * kThreads + far] : 0u;    // (an entry that runs off the tile is never used)
              next[a * kThreads + tid] = cur[a];
            }
            __syncthreads();
          }
#pragma unroll
          for (int a = 0; a < NA; ++a) sum[a] = 0;
          if (centre) {                                                // tid - h >= 0 and tid + h < 256 for a centre lane
            int off = tid - h;
            for (int k = kMaxLevels - 1; k >= 0; --k) {
              if ((n >> k) & 1) {
                const uint32_t* const lvl = s_w + k * NA * kThreads;
#pragma unroll
                for (int a = 0; a < NA; ++a) sum[a] += lvl[a * kThreads + off];
                off += 1 << k;
              }
            }
          }
        }
        // the squares of this lane, threshold by threshold
#pragma unroll
        for (int qd = 0; qd < NP; ++qd) {
#pragma unroll
          for (int lane = 0; lane < 2; ++lane) {
            const int t = 4 * (qd >> 1) + (qd & 1) + 2 * lane;
            if (t < T) {
              const uint32_t cf = (sum[qd] >> (16 * lane)) & 0xffffu, co = (sum[NP + qd] >> (16 * lane)) & 0xffffu;
              const uint32_t d = cf > co ? cf - co : co - cf;
              s_red[(3 * t + 0) * kThreads + tid] = cv ? d * d : 0u;
              s_red[(3 * t + 1) * kThreads + tid] = cv ? cf * cf : 0u;
              s_red[(3 * t + 2) * kThreads + tid] = cv ? co * co : 0u;
            }
          }
        }
        if (s == 0) s_red[3 * T * kThreads + tid] = cv ? 1u : 0u;
        __syncthreads();
        // four lanes per value: 64 entries each (rotated: no bank conflict), then two exchanges; 32 bits hold it (header)
        const int nv = 3 * T + (s == 0 ? 1 : 0);
        const int v = tid >> 2, part = tid & 3;
        uint32_t acc = 0;
        if (v < nv) {
          const uint32_t* const src = s_red + v * kThreads + part * 64;
#pragma unroll 8
          for (int k = 0; k < 64; ++k) acc += src[(k + tid) & 63];
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        if (v < nv && part == 0 && acc) {
          if (v == 3 * T) {
            atomicAdd(valid + plane * n_lat + i, (unsigned long long)acc);
          } else {
            const int t = v / 3, c = v - 3 * t;
            atomicAdd(rowsums + ((((plane * T + t) * S + s) * n_lat + i) * 3 + c), (unsigned long long)acc);
          }
        }
        // (the next window size writes s_w, which every lane has finished reading before the barrier above, and reaches
        //  s_red only after at least one more barrier: its n is > 1)
      }
    }
  }
}

// Clears both tables: one 8-byte vector store per entry.
__global__ __launch_bounds__(256) void event_scores_clear_kernel(unsigned long long* __restrict__ rowsums, int64_t n_rowsums,
                                                                 unsigned long long* __restrict__ valid, int64_t n_valid) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_rowsums + n_valid; i += stride) {
    if (i < n_rowsums)
      rowsums[i] = 0ull;
    else
      valid[i - n_rowsums] = 0ull;
  }
}

}  // namespace
}  // namespace aurora

using namespace aurora;

// The call needs no workspace: the tables are cleared by a launch of their own and filled by integer atomics.
extern "C" size_t aurora_hip_event_scores_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_thresholds, int n_scales) {
  (void)n_planes, (void)n_lat, (void)n_lon, (void)n_thresholds, (void)n_scales;
  return 0;
}

extern "C" int aurora_hip_event_scores(const float* const* pred_planes, const float* const* truth_planes, int n_planes,
                                       int n_lat, int n_lon, const float* thresholds, int n_thresholds, const int32_t* scales,
                                       int n_scales, int below, int64_t* rowsums, int64_t* valid, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  (void)workspace;
  const int T = n_thresholds, S = n_scales;
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1, "event_scores: bad sizes (planes %d, grid %d x %d)", n_planes, n_lat, n_lon);
  AURORA_CHECK_ARG(n_lon >= 1 && n_lon <= kMaxLon, "event_scores: n_lon must be in 1..%d, got %d", kMaxLon, n_lon);
  AURORA_CHECK_ARG(T >= 1 && T <= kMaxT, "event_scores: n_thresholds must be in 1..%d, got %d", kMaxT, T);
  AURORA_CHECK_ARG(S >= 1 && S <= kMaxS, "event_scores: n_scales must be in 1..%d, got %d", kMaxS, S);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(pred_planes && truth_planes && thresholds && scales && rowsums && valid,
                   "event_scores: null plane array, threshold, scale or output pointer");
  AURORA_CHECK_ARG(scales[0] == 1, "event_scores: scales[0] must be 1 (the contingency table), got %d", scales[0]);
  ScaleList sc = {};
  for (int s = 0; s < S; ++s) {
    const int n = scales[s];
    AURORA_CHECK_ARG(n >= 1 && n <= kMaxN && (n & 1), "event_scores: scales must be odd and in 1..%d, got scales[%d] = %d", kMaxN,
                     s, n);
    AURORA_CHECK_ARG(s == 0 || n > scales[s - 1], "event_scores: scales must be ascending and distinct (scales[%d] = %d after %d)",
                     s, n, s ? scales[s - 1] : 0);
    AURORA_CHECK_ARG(n <= n_lon, "event_scores: scales[%d] = %d is wider than the %d longitudes", s, n, n_lon);
    sc.n[s] = n;
  }
  AURORA_CHECK_ARG((((uintptr_t)rowsums | (uintptr_t)valid) & 7) == 0 && ((uintptr_t)thresholds & 3) == 0,
                   "event_scores: the outputs must be 8-byte aligned, the thresholds 4-byte aligned");
  AURORA_CHECK_ARG(workspace_bytes >= aurora_hip_event_scores_workspace_bytes(n_planes, n_lat, n_lon, T, S),
                   "event_scores: the workspace is too small");
  const int n_max = sc.n[S - 1], h_max = n_max >> 1;
  const int W = kThreads - 2 * h_max;
  const int64_t tiles = ((int64_t)n_lon + W - 1) / W, segs = ((int64_t)n_lat + kRows - 1) / kRows;
  const int64_t groups = tiles * segs * n_planes;
  AURORA_CHECK_ARG(groups <= 0x7fffffff, "event_scores: too many planes for one launch (%d planes x %lld row segments x %lld tiles)",
                   n_planes, (long long)segs, (long long)tiles);
  {
    // the dynamic LDS limit of both forms, raised once per device; a failure is reported, not left to a later launch error
    static bool raised[64] = {false};
    bool& done = raised[current_device() & 63];
    if (!done) {
      const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&event_scores_kernel<1>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kMaxN >> 1, kMaxN, 4, 1));
      const hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void*>(&event_scores_kernel<2>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kMaxN >> 1, kMaxN, kMaxT, 2));
      if (e1 != hipSuccess || e2 != hipSuccess) {
        (void)hipGetLastError();
        set_error("event_scores: the device refused %zu bytes of dynamic LDS per workgroup: %s", lds_bytes(kMaxN >> 1, kMaxN, kMaxT, 2),
                  hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        return AURORA_E_LAUNCH;
      }
      done = true;
    }
  }
  unsigned long long* const rs = reinterpret_cast<unsigned long long*>(rowsums);
  unsigned long long* const vd = reinterpret_cast<unsigned long long*>(valid);
  const int64_t n_rowsums = (int64_t)n_planes * T * S * n_lat * 3, n_valid = (int64_t)n_planes * n_lat;
  const int64_t clear_groups = (n_rowsums + n_valid + 255) / 256;
  hipLaunchKernelGGL(event_scores_clear_kernel, dim3((unsigned)(clear_groups < 4096 ? clear_groups : 4096)), dim3(256), 0,
                     as_stream(stream), rs, n_rowsums, vd, n_valid);
  int code = check_launch("event_scores (clearing the tables)");
  if (code != AURORA_OK) return code;
  const int TH = T <= 4 ? 1 : 2;
  const size_t lds = lds_bytes(h_max, n_max, T, TH);
  if (TH == 1)
    hipLaunchKernelGGL(event_scores_kernel<1>, dim3((unsigned)groups), dim3(kThreads), lds, as_stream(stream), pred_planes,
                       truth_planes, n_lat, n_lon, thresholds, T, sc, S, below ? 1 : 0, (int)tiles, (int)segs, rs, vd);
  else
    hipLaunchKernelGGL(event_scores_kernel<2>, dim3((unsigned)groups), dim3(kThreads), lds, as_stream(stream), pred_planes,
                       truth_planes, n_lat, n_lon, thresholds, T, sc, S, below ? 1 : 0, (int)tiles, (int)segs, rs, vd);
  return check_launch("event_scores");
}
