// Per-point quantile maps of an ENSEMBLE and the map of the truth's rank on the device (aurora_amd.ensemble_quantiles:
// the median, the 10 % and 90 % maps, where the truth fell outside the ensemble).
//
// For every plane (one variable, level and batch element; n_lat x n_lon fp32, row-major) the M member planes (and the
// truth plane, if there is one) are read ONCE, and n_q quantile planes (and one int8 rank plane) are written.  The rule
// (include/aurora_hip.h has it in full): a point is valid where all M members are finite; its values are sorted by the
// integer key of sortnet.h; for quantile i, with (j, g) = the library's (floor, fraction) of (M - 1) q_i and
// hi = min(j + 1, M - 1),
//     value = (float)(a + g (b - a)),  a = (double)x_(j), b = (double)x_(hi),
// the three fp64 operations rounded one by one (never an fma: the numpy path has none, and the two agree bit for bit);
// an invalid point gives NaN.  rank = #{m : x_m < y}, compared as stored; -1 where y or a member is not finite.
//
// A point's M values live in registers, as in ensemble_scores.hip: the kernel is a template on the member-count BUCKET,
// the slots past M hold +inf, and every loop over members is unrolled over the bucket with a wave-uniform `m < M` guard.
// x_(j) and x_(hi) are picked from the sorted registers by a wave-uniform switch over j (j comes from the kernel's
// arguments, so it lives in a scalar register): a branch, not an indexed array, so nothing goes to scratch.  Buckets up to
// 16 take a quad of columns per lane (the quad rule of planes.h, over the member, truth AND output pointers); buckets 32
// and 64 take one column.  One workgroup = one row chunk of one plane, a wave takes every fourth row of it.  One launch:
// no workspace, no atomics, no reduction across threads; every output element is written by exactly one lane.
#include <cmath>

#include "planes.h"
#include "sortnet.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxQuantiles = 8;

// Target size of a row chunk (elements of one input), as in ensemble_scores.hip.
constexpr int chunk_elems(int bucket) { return bucket <= 8 ? 40960 : 16384; }

// What the library makes of the host's q: passed to the kernel BY VALUE (no table is uploaded: a call is capturable).
struct Spec {
  int n;
  int j[kMaxQuantiles];                         // floor((M - 1) q), at most M - 1
  double g[kMaxQuantiles];                      // (M - 1) q - j
};

// v[j] and v[min(j + 1, N - 1)] of a register array for a wave-uniform j in [0, N): one scalar branch per call.
template <int N, int P> __device__ __forceinline__ void pick(const float (&v)[P][N], int j, float (&a)[P], float (&b)[P]) {
#define AURORA_PICK(K)                                  \
  case K:                                               \
    _Pragma("unroll") for (int p = 0; p < P; ++p) {     \
      a[p] = v[p][K];                                   \
      b[p] = v[p][(K) + 1 < N ? (K) + 1 : N - 1];       \
    }                                                   \
    break;
#define AURORA_PICK4(K) AURORA_PICK(K) AURORA_PICK((K) + 1) AURORA_PICK((K) + 2) AURORA_PICK((K) + 3)
#define AURORA_PICK16(K) AURORA_PICK4(K) AURORA_PICK4((K) + 4) AURORA_PICK4((K) + 8) AURORA_PICK4((K) + 12)
  if constexpr (N == 4) {
    switch (j) { AURORA_PICK4(0) }
  } else if constexpr (N == 8) {
    switch (j) { AURORA_PICK4(0) AURORA_PICK4(4) }
  } else if constexpr (N == 16) {
    switch (j) { AURORA_PICK16(0) }
  } else if constexpr (N == 32) {
    switch (j) { AURORA_PICK16(0) AURORA_PICK16(16) }
  } else {
    static_assert(N == 64, "the buckets are 4, 8, 16, 32 and 64");
    switch (j) { AURORA_PICK16(0) AURORA_PICK16(16) AURORA_PICK16(32) AURORA_PICK16(48) }
  }
#undef AURORA_PICK16
#undef AURORA_PICK4
#undef AURORA_PICK
}

// a + g (b - a) in fp64, every operation rounded on its own, then one rounding to fp32.
__device__ __forceinline__ float interpolate(float af, float bf, double g) {
#pragma clang fp contract(off)
  const double a = (double)af, b = (double)bf;
  const double d = b - a;
  const double t = g * d;
  return (float)(a + t);
}

// One workgroup = one row chunk of one plane.  MB: the bucket; PPL: points per lane and item (4: a quad of columns, 1: a
// column).
template <int MB, int PPL>
__global__ __launch_bounds__(kThreads) void ensemble_quantiles_kernel(const float* const* __restrict__ member_planes,
                                                                      const float* const* __restrict__ truth_planes,
                                                                      int n_members, int n_planes, int n_lat, int n_lon,
                                                                      int n_chunks, const Spec spec,
                                                                      float* __restrict__ quantiles,
                                                                      signed char* __restrict__ rank) {
  static_assert(PPL == 1 || PPL == 4, "an item is a column or a quad of columns");
  const int plane = (int)(blockIdx.x / (unsigned)n_chunks), chunk = (int)(blockIdx.x % (unsigned)n_chunks);
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int M = __builtin_amdgcn_readfirstlane(n_members);
  const int n_q = __builtin_amdgcn_readfirstlane(spec.n);
  const bool has_truth = truth_planes != nullptr;
  const gptr<const float> T = has_truth ? (gptr<const float>)truth_planes[plane] : nullptr;
  const float* const* __restrict__ members = member_planes + plane;          // member m: members[m * n_planes]
  const int64_t n_points = (int64_t)n_lat * n_lon;
  const gptr<float> Q = (gptr<float>)quantiles + (int64_t)plane * n_q * n_points;   // map i of the plane: Q + i n_points
  const gptr<signed char> R = has_truth ? (gptr<signed char>)rank + (int64_t)plane * n_points : nullptr;
  bool vec = false;
  if (PPL == 4) {                        // the quad rule over T, the M member pointers and the n_q output planes
    uintptr_t bits = (uintptr_t)T | (uintptr_t)(n_lon & 3) | (uintptr_t)Q | (uintptr_t)(n_q > 1 ? n_points * 4 : 0);
    for (int m = 0; m < M; ++m) bits |= (uintptr_t)members[(int64_t)m * n_planes];
    vec = (bits & 15) == 0;
  }
  const bool rank_vec = vec && ((uintptr_t)R & 3) == 0;          // (four int8 ranks of a quad as one 4-byte store)
  const int n_items = PPL == 4 ? (n_lon + 3) >> 2 : n_lon;
  const int rows = chunk_rows(n_lon, chunk_elems(MB), kWaves);
  const int r_begin = chunk * rows, r_end = min(r_begin + rows, n_lat);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");

  for (int r = r_begin + wave; r < r_end; r += kWaves) {
    const int64_t row0 = (int64_t)r * n_lon;
    for (int i0 = 0; i0 < n_items; i0 += 64) {
      const bool in = i0 + lane < n_items;
      const int item = in ? i0 + lane : n_items - 1;             // clamped: the load is in the row, the guard is `in`
      float x[PPL][MB], y[PPL];
      int col[PPL];
      bool in_row[PPL];
#pragma unroll
      for (int p = 0; p < PPL; ++p) {
        col[p] = PPL == 1 ? item : min(4 * item + p, n_lon - 1);
        in_row[p] = in && (PPL == 1 || 4 * item + p < n_lon);
        y[p] = 0.0f;
      }
      if (PPL == 1) {
        if (has_truth) y[0] = T[row0 + item];
#pragma unroll
        for (int m = 0; m < MB; ++m)
          x[0][m] = m < M ? ((gptr<const float>)members[(int64_t)m * n_planes])[row0 + item] : inf;
      } else if (vec) {                                          // the quad rule, written out for the `m < M` guards
        if (has_truth) {
          const f32x4 t = ((gptr<const f32x4>)(T + row0))[item];
#pragma unroll
          for (int p = 0; p < PPL; ++p) y[p] = t[p];
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          f32x4 q = {inf, inf, inf, inf};
          if (m < M) q = ((gptr<const f32x4>)((gptr<const float>)members[(int64_t)m * n_planes] + row0))[item];
#pragma unroll
          for (int p = 0; p < PPL; ++p) x[p][m] = q[p];
        }
      } else {
        if (has_truth) {
#pragma unroll
          for (int p = 0; p < PPL; ++p) y[p] = T[row0 + col[p]];
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          const gptr<const float> P = (gptr<const float>)members[(int64_t)(m < M ? m : 0) * n_planes];
#pragma unroll
          for (int p = 0; p < PPL; ++p) x[p][m] = m < M ? P[row0 + col[p]] : inf;
        }
      }

      // validity and rank from the values as stored, then the sort
      bool ok[PPL];
      int below[PPL];
#pragma unroll
      for (int p = 0; p < PPL; ++p) {
        unsigned top = 0u;                                       // the largest |bits|: NaN and inf are >= 0x7f800000
        int n = 0;
#pragma unroll
        for (int m = 0; m < MB; ++m)
          if (m < M) {
            top = max(top, (unsigned)__float_as_int(x[p][m]) & 0x7fffffffu);
            n += x[p][m] < y[p] ? 1 : 0;
          }
        ok[p] = top < 0x7f800000u;
        below[p] = ok[p] && ((unsigned)__float_as_int(y[p]) & 0x7fffffffu) < 0x7f800000u ? n : -1;
        sort_ascending<MB>(x[p]);
      }

      for (int i = 0; i < n_q; ++i) {                            // wave-uniform: j and g are scalars
        const int j = __builtin_amdgcn_readfirstlane(spec.j[i]);
        const double g = spec.g[i];
        float a[PPL], b[PPL], v[PPL];
        pick<MB, PPL>(x, j, a, b);
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
          const float hi = j + 1 < M ? b[p] : a[p];              // hi = min(j + 1, M - 1): never a padding slot
          v[p] = ok[p] ? interpolate(a[p], hi, g) : nan;
        }
        const gptr<float> out = Q + i * n_points + row0;
        bool stored = false;
        if constexpr (PPL == 4) {
          if (vec) {
            if (in) ((gptr<f32x4>)out)[item] = f32x4{v[0], v[1], v[2], v[3]};
            stored = true;
          }
        }
        if (!stored) {
#pragma unroll
          for (int p = 0; p < PPL; ++p)
            if (in_row[p]) out[col[p]] = v[p];
        }
      }
      if (has_truth) {
        bool stored = false;
        if constexpr (PPL == 4) {
          if (rank_vec) {
            const unsigned packed = ((unsigned)below[0] & 0xffu) | (((unsigned)below[1] & 0xffu) << 8) |
                                    (((unsigned)below[2] & 0xffu) << 16) | ((unsigned)below[3] << 24);
            if (in) ((gptr<unsigned>)(R + row0))[item] = packed;
            stored = true;
          }
        }
        if (!stored) {
#pragma unroll
          for (int p = 0; p < PPL; ++p)
            if (in_row[p]) R[row0 + col[p]] = (signed char)below[p];
        }
      }
    }
  }
}

template <int MB, int PPL>
void launch(unsigned groups, void* stream, const float* const* member_planes, const float* const* truth_planes, int n_members,
            int n_planes, int n_lat, int n_lon, int n_chunks, const Spec& spec, float* quantiles, int8_t* rank) {
  hipLaunchKernelGGL((ensemble_quantiles_kernel<MB, PPL>), dim3(groups), dim3(kThreads), 0, as_stream(stream), member_planes,
                     truth_planes, n_members, n_planes, n_lat, n_lon, n_chunks, spec, quantiles, (signed char*)rank);
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_ensemble_quantiles(const float* const* member_planes, const float* const* truth_planes, int n_members,
                                             int n_planes, int n_lat, int n_lon, const double* q, int n_q, float* quantiles,
                                             int8_t* rank, void* stream) {
  AURORA_CHECK_ARG(n_members >= 2 && n_members <= kMaxMembers, "ensemble_quantiles: n_members must be in 2..%d, got %d",
                   kMaxMembers, n_members);
  AURORA_CHECK_ARG(n_q >= 1 && n_q <= kMaxQuantiles, "ensemble_quantiles: n_q must be in 1..%d, got %d", kMaxQuantiles, n_q);
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1 && n_lon >= 1, "ensemble_quantiles: bad sizes (planes %d, grid %d x %d)",
                   n_planes, n_lat, n_lon);
  AURORA_CHECK_ARG(q, "ensemble_quantiles: null q");
  Spec spec{};
  spec.n = n_q;
  for (int i = 0; i < n_q; ++i) {
    AURORA_CHECK_ARG(std::isfinite(q[i]) && q[i] >= 0.0 && q[i] <= 1.0, "ensemble_quantiles: q[%d] = %g is not in [0, 1]", i,
                     q[i]);
    const double h = (double)(n_members - 1) * q[i];             // as numpy forms the index of method="linear"
    const int j = std::min((int)std::floor(h), n_members - 1);
    spec.j[i] = j;
    spec.g[i] = h - (double)j;
  }
  AURORA_CHECK_ARG((truth_planes == nullptr) == (rank == nullptr),
                   "ensemble_quantiles: rank must be given with truth_planes and null without them");
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(member_planes && quantiles, "ensemble_quantiles: null plane array or output pointer");
  AURORA_CHECK_ARG(((uintptr_t)quantiles & 3) == 0, "ensemble_quantiles: quantiles must be 4-byte aligned");
  const int bucket = bucket_of(n_members);
  const int64_t n_chunks = chunks_per_plane(n_lat, n_lon, chunk_elems(bucket), kWaves);
  const int64_t groups = n_chunks * n_planes;
  AURORA_CHECK_ARG(groups <= 0x7fffffff, "ensemble_quantiles: too many planes for one launch (%d planes x %lld row chunks)",
                   n_planes, (long long)n_chunks);
#define AURORA_QUANTILES_LAUNCH(MB, PPL)                                                                                 \
  launch<MB, PPL>((unsigned)groups, stream, member_planes, truth_planes, n_members, n_planes, n_lat, n_lon, (int)n_chunks, \
                  spec, quantiles, rank)
  switch (bucket) {
    case 4: AURORA_QUANTILES_LAUNCH(4, 4); break;
    case 8: AURORA_QUANTILES_LAUNCH(8, 4); break;
    case 16: AURORA_QUANTILES_LAUNCH(16, 4); break;
    case 32: AURORA_QUANTILES_LAUNCH(32, 1); break;
    default: AURORA_QUANTILES_LAUNCH(64, 1); break;
  }
#undef AURORA_QUANTILES_LAUNCH
  return check_launch("ensemble_quantiles");
}
