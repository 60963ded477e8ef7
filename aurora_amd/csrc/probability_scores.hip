// Event probabilities of an ENSEMBLE against truth on the device (aurora_amd.probability_scores: Brier score and its
// decomposition, reliability diagram, ROC).
//
// For every plane (one variable, level and batch element; n_lat x n_lon fp32, row-major) the M member planes and the
// truth plane are read ONCE.  A point is valid where the truth and all M members are finite; for each of the T
// thresholds of the plane a valid point has k = #{m : x_m >= thr} in 0..M and o = [y >= thr] (both <= with `below`; a
// NaN threshold: k = 0, o = 0), and the whole output is, per row i of the plane, the number of its valid points with
// each (t, o, k): rows[(((plane n_lat + i) T + t) 2 + o) (M + 1) + k], int32 (include/aurora_hip.h).  Only integer
// arithmetic decides the output, so it is exact and does not depend on any order of addition or of the members.
//
// Mapping.  A wavefront owns a row: a 256-thread workgroup takes four consecutive rows of one plane, the grid is n_planes x
// ceil(n_lat / 4), and the plane index, its thresholds and its pointers are wave-uniform (scalar loads).  A lane takes a
// quad of columns per step (the quad rule and load_quad of planes.h) and STREAMS the members past it in a runtime loop
// unrolled by four: per member `ok &= finite(x)` and a byte-packed counter gets `+= (x >= thr_t) << 8 (t mod 4)` (k <= 64
// fits a byte; thresholds 0..3 share one register, 4..7 a second one that only the T > 4 instantiation carries).  No
// member-count bucket, no template on M; slots t >= T hold a NaN threshold and are never binned.
// Each wave keeps its row's T x 2 x (M + 1) bins in LDS (at most 4,160 bytes), clears them, adds to them with LDS
// integer atomics (ds_add_u32, whose order cannot change a sum) and stores them contiguously with plain vector stores:
// no global atomics, no clearing launch, no workspace, ONE launch.
// Most points fall into the corner bins (o = 0, k = 0) and (o = 1, k = M), where the 64 lanes of a step would add to one
// LDS address.  kCornerBallot takes those two bins by __ballot + popcount into scalar registers, added once per row by one
// lane per threshold, and sends only the remaining lanes through the atomic; AURORA_PROBABILITY_PLAIN_ATOMICS builds the
// plain form (every valid lane an LDS atomic) for tools/probability_scores_bench.py, which times the two side by side.
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxMembers = 64;
constexpr int kMaxT = 8;
constexpr int kMaxBins = kMaxT * 2 * (kMaxMembers + 1);       // of one row
#ifdef AURORA_PROBABILITY_PLAIN_ATOMICS
constexpr bool kCornerBallot = false;
#else
constexpr bool kCornerBallot = true;
#endif

template <bool BELOW> __device__ __forceinline__ bool event(float x, float thr) { return BELOW ? x <= thr : x >= thr; }

// One member's quad: validity and the byte-packed exceedance counts of its four points.
template <int TT, bool BELOW>
__device__ __forceinline__ void tally(const f32x4 q, const float (&thr)[TT], bool (&ok)[4], uint32_t (&cnt)[4][TT / 4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    ok[p] = ok[p] && __builtin_isfinite(q[p]);
#pragma unroll
    for (int t = 0; t < TT; ++t) cnt[p][t >> 2] += (uint32_t)event<BELOW>(q[p], thr[t]) << (8 * (t & 3));
  }
}

__device__ __forceinline__ void lds_add(int* p, int v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);    // result unused: ds_add_u32
}

// One row of one plane by one wave into its `bins` ([t][o][k], cleared by the caller).
template <int TT, bool BELOW, bool VEC>
__device__ __forceinline__ void bin_row(const float* const* __restrict__ members, int64_t member_stride, gptr<const float> truth,
                                        int64_t row0, int n_lon, int M, int T, const float (&thr)[TT], int lane, int* bins) {
  const int n_items = (int)(((int64_t)n_lon + 3) >> 2);
  const int M1 = M + 1;
  int corner0[TT] = {}, cornerM[TT] = {};                       // wave-uniform (scalar registers)
  for (int i0 = 0; i0 < n_items; i0 += 64) {                    // wave-uniform trip count: ballots see whole waves
    const bool in = i0 + lane < n_items;
    const int item = in ? i0 + lane : n_items - 1;              // clamped: the load is in the row, the guard is `in`
    unsigned col[4];
    bool ok[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const unsigned c = 4u * (unsigned)item + (unsigned)p;
      ok[p] = in && c < (unsigned)n_lon;
      col[p] = min(c, (unsigned)n_lon - 1u);
    }
    const f32x4 y = load_quad<VEC>(truth + row0, item, col);
    uint32_t cnt[4][TT / 4] = {};
#pragma unroll
    for (int p = 0; p < 4; ++p) ok[p] = ok[p] && __builtin_isfinite(y[p]);
    int m = 0;
    for (; m + 4 <= M; m += 4) {                                // four members' loads in flight
      f32x4 q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = load_quad<VEC>((gptr<const float>)members[(m + u) * member_stride] + row0, item, col);
#pragma unroll
      for (int u = 0; u < 4; ++u) tally<TT, BELOW>(q[u], thr, ok, cnt);
    }
    for (; m < M; ++m) tally<TT, BELOW>(load_quad<VEC>((gptr<const float>)members[m * member_stride] + row0, item, col), thr, ok, cnt);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int t = 0; t < TT; ++t)
        if (t < T) {                                            // wave-uniform
          const int k = (int)((cnt[p][t >> 2] >> (8 * (t & 3))) & 0xffu);
          const bool o = event<BELOW>(y[p], thr[t]);
          int* const bin = bins + (t * 2 + (o ? 1 : 0)) * M1 + k;
          if (kCornerBallot) {
            const bool c0 = ok[p] && !o && k == 0, cM = ok[p] && o && k == M;
            corner0[t] += __builtin_popcountll(__ballot(c0));
            cornerM[t] += __builtin_popcountll(__ballot(cM));
            if (ok[p] && !c0 && !cM) lds_add(bin, 1);
          } else if (ok[p]) {
            lds_add(bin, 1);
          }
        }
  }
  if (kCornerBallot) {                                          // lane t adds the two corner counts of threshold t
    int v0 = 0, vM = 0;
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      v0 = lane == t ? corner0[t] : v0;
      vM = lane == t ? cornerM[t] : vM;
    }
    if (lane < T) {
      lds_add(bins + (lane * 2) * M1, v0);
      lds_add(bins + (lane * 2 + 1) * M1 + M, vM);
    }
  }
}

// One workgroup = four consecutive rows of one plane, a wave each.  TT: threshold slots carried (4 or 8, >= T).
template <int TT, bool BELOW>
__global__ __launch_bounds__(kThreads) void probability_scores_kernel(const float* const* __restrict__ member_planes,
                                                                      const float* const* __restrict__ truth_planes,
                                                                      int n_members, int n_planes, int n_lat, int n_lon,
                                                                      int n_groups, const float* __restrict__ thresholds,
                                                                      int n_thresholds, int32_t* __restrict__ rows) {
  __shared__ int s_bins[kWaves][kMaxBins];
  const int plane = (int)(blockIdx.x / (unsigned)n_groups), group = (int)(blockIdx.x % (unsigned)n_groups);
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int M = __builtin_amdgcn_readfirstlane(n_members), T = __builtin_amdgcn_readfirstlane(n_thresholds);
  const int row = group * kWaves + wave;
  const bool mine = row < n_lat;                                // (wave-uniform; the barriers below are outside it)
  const int n_bins = T * 2 * (M + 1);
  int* const bins = s_bins[wave];
  if (mine)
    for (int j = lane; j < n_bins; j += 64) bins[j] = 0;
  __syncthreads();
  if (mine) {
    float thr[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) thr[t] = t < T ? thresholds[(int64_t)plane * T + t] : __builtin_nanf("");
    const gptr<const float> truth = (gptr<const float>)truth_planes[plane];
    const float* const* __restrict__ members = member_planes + plane;        // member m: members[m * n_planes]
    uintptr_t bits = (uintptr_t)truth | (uintptr_t)(n_lon & 3);   // the quad rule over truth and the M member pointers
    for (int m = 0; m < M; ++m) bits |= (uintptr_t)members[(int64_t)m * n_planes];
    const int64_t row0 = (int64_t)row * n_lon;
    if ((bits & 15) == 0)
      bin_row<TT, BELOW, true>(members, n_planes, truth, row0, n_lon, M, T, thr, lane, bins);
    else
      bin_row<TT, BELOW, false>(members, n_planes, truth, row0, n_lon, M, T, thr, lane, bins);
  }
  __syncthreads();
  if (mine) {
    int32_t* const out = rows + ((int64_t)plane * n_lat + row) * n_bins;
    for (int j = lane; j < n_bins; j += 64) out[j] = bins[j];
  }
}

template <int TT, bool BELOW>
void launch(unsigned groups, void* stream, const float* const* member_planes, const float* const* truth_planes, int n_members,
            int n_planes, int n_lat, int n_lon, int n_groups, const float* thresholds, int n_thresholds, int32_t* rows) {
  hipLaunchKernelGGL((probability_scores_kernel<TT, BELOW>), dim3(groups), dim3(kThreads), 0, as_stream(stream), member_planes,
                     truth_planes, n_members, n_planes, n_lat, n_lon, n_groups, thresholds, n_thresholds, rows);
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_probability_scores(const float* const* member_planes, const float* const* truth_planes, int n_members,
                                             int n_planes, int n_lat, int n_lon, const float* thresholds, int n_thresholds,
                                             int below, int32_t* rows, void* stream) {
  AURORA_CHECK_ARG(n_members >= 2 && n_members <= kMaxMembers, "probability_scores: n_members must be in 2..%d, got %d",
                   kMaxMembers, n_members);
  AURORA_CHECK_ARG(n_thresholds >= 1 && n_thresholds <= kMaxT, "probability_scores: n_thresholds must be in 1..%d, got %d", kMaxT,
                   n_thresholds);
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1 && n_lon >= 1, "probability_scores: bad sizes (planes %d, grid %d x %d)", n_planes,
                   n_lat, n_lon);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(member_planes && truth_planes && thresholds && rows,
                   "probability_scores: null plane array, threshold or output pointer");
  AURORA_CHECK_ARG((((uintptr_t)rows | (uintptr_t)thresholds) & 3) == 0,
                   "probability_scores: rows and thresholds must be 4-byte aligned");
  const int64_t n_groups = ((int64_t)n_lat + kWaves - 1) / kWaves;
  const int64_t groups = n_groups * n_planes;
  AURORA_CHECK_ARG(groups <= 0x7fffffff, "probability_scores: too many planes for one launch (%d planes x %lld row groups)",
                   n_planes, (long long)n_groups);
#define AURORA_PROBABILITY_LAUNCH(TT, BELOW)                                                                                \
  launch<TT, BELOW>((unsigned)groups, stream, member_planes, truth_planes, n_members, n_planes, n_lat, n_lon, (int)n_groups, \
                    thresholds, n_thresholds, rows)
  if (n_thresholds <= 4) {
    if (below) AURORA_PROBABILITY_LAUNCH(4, true); else AURORA_PROBABILITY_LAUNCH(4, false);
  } else {
    if (below) AURORA_PROBABILITY_LAUNCH(8, true); else AURORA_PROBABILITY_LAUNCH(8, false);
  }
#undef AURORA_PROBABILITY_LAUNCH
  return check_launch("probability_scores");
}
