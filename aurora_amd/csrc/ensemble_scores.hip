// Verification sums of an ENSEMBLE against truth on the device (aurora_amd.ensemble_scores: CRPS, ensemble-mean RMSE /
// bias / MAE, spread, rank histogram).
//
// For every plane (one variable, level and batch element; n_lat x n_lon fp32, row-major) the M member planes and the
// truth plane are read ONCE and reduced to eight fp64 sums and M + 2 integer counts over the points where the truth
// and all M members are finite (include/aurora_hip.h has the table).  Everything is formed in fp64 from the
// differences to truth d_m = (double)x_m - (double)y; nothing is accumulated in fp32.
//
// A point's M values live in registers.  The kernel is a template on a member-count BUCKET (4, 8, 16, 32, 64): the slots
// past M hold +inf, so they sort last, and every loop over members is unrolled over the bucket with a wave-uniform
// `m < M` guard, so every register index is a compile-time constant (no scratch).  Per point:
//   pass 1, member order   sd = sum d_m (e = sd / M), any x_m == y (a tie); the point is valid iff sd is finite
//                          (a NaN or an infinity in any input makes some d_m, and with it sd, NaN or infinite);
//   sort                   the fp32 values x_m by Batcher's odd-even merge network (sortnet.h; x -> x - y is
//                          monotone, so the d_m are then ascending too);
//   pass 2, sorted order   sum |d_(k)|, sum (2k - M - 1) d_(k)  (= M^2 g / 2), sum (d_(k) - e)^2, and for the
//                          histogram one ballot per k: the number of valid points of the wave with x_(k) < y, added
//                          up in scalar registers (two 16-bit counts each, flushed to lane k of a vector register).  Only sorted values enter S5, S6 and the counts, so they do not depend
//                          on the order of the members, bit for bit.
// Buckets up to 16 take a quad of columns per lane (the quad rule of planes.h); buckets 32 and 64 take one column.
//
// The fp64 sums go through the reduction tree of planes.h, four waves to a workgroup, with a chunk size that depends on
// the bucket; the integer counts ride along (they are wave sums from the start: popcounts of ballots).
// ensemble_finish_kernel is the tree's second launch in place of finish_partials: it adds the sums by the plane rule of
// planes.h, over partials that are partial_bytes apart, and also turns the cumulative counts #{points : x_(k) < y} into the
// M + 1 bins.  No atomics of any kind.
#include "planes.h"
#include "sortnet.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlots = kSumSlots;
// Target size of a row chunk (elements of one input): that of scores.hip where a point is cheap, smaller chunks (more
// workgroups to balance) where a point costs hundreds of instructions.
constexpr int chunk_elems(int bucket) { return bucket <= 8 ? 40960 : 16384; }

// Bytes of one workgroup's partial: eight doubles, then bucket + 2 counts (valid points, #{x_(k) < y} for k < bucket,
// ties) padded to whole doubles.
__host__ __device__ constexpr int64_t partial_bytes(int bucket) { return kSlots * 8 + ((bucket + 2) * 4 + 7) / 8 * 8; }

// ---- accumulators ---------------------------------------------------------------------------------------------------
struct Acc {                                    // per lane
  double s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
};
template <int MB> struct Counts {               // per wave
  int valid = 0, ties = 0, row = 0;             // wave-uniform (scalar registers); row: valid points of the current row
  // #{valid points of the wave : x_(k) < y} since the last flush, wave-uniform, two 16-bit counts to a register (k in
  // the low half, k + MB / 2 in the high half: 64 whole registers would not fit the scalar file) ...
  unsigned packed[MB / 2] = {};
  int below = 0;                                // ... and, flushed, in lane k: the same count over the wave's whole share
  // A flush is due before a 16-bit count can overflow: every kFlushPoints points of the wave at the latest.
  static constexpr int kFlushPoints = 32768;
  __device__ __forceinline__ void flush(int lane) {
#pragma unroll
    for (int j = 0; j < MB / 2; ++j) {
      const int lo = lane == j ? (int)(packed[j] & 0xffffu) : 0;
      below += lane == j + MB / 2 ? (int)(packed[j] >> 16) : lo;
      packed[j] = 0;
    }
  }
};
struct Scale {                                  // wave-uniform constants of M
  int M;
  double inv_m, g_scale, inv_m1;                // 1 / M, 2 / M^2, 1 / (M - 1)
};

__device__ __forceinline__ int lanes(bool b) { return __builtin_popcountll(__ballot(b)); }

// One point: v[0 .. M) the members in member order (v[M ..] = +inf), yf the truth.  An invalid point (outside the row,
// or any input not finite) adds exactly +0 to every sum and nothing to any count.
template <int MB>
__device__ __forceinline__ void point(Acc& a, Counts<MB>& c, const Scale& sc, double w, float (&v)[MB], float yf, bool in_row) {
  const double y = (double)yf;
  double sd = 0.0;
  bool tie = false;
#pragma unroll
  for (int m = 0; m < MB; ++m)
    if (m < sc.M) {
      sd += (double)v[m] - y;
      tie = tie || v[m] == yf;
    }
  const bool ok = in_row && __builtin_isfinite(sd);
  const double e = sd * sc.inv_m;
  sort_ascending<MB>(v);
  const float y_cmp = ok ? yf : -__builtin_inff();           // nothing is below -inf: an invalid point counts nowhere
  double sa = 0.0, sg = 0.0, sv = 0.0;
#pragma unroll
  for (int k = 0; k < MB; ++k)
    if (k < sc.M) {
      const double d = (double)v[k] - y;
      sa += __builtin_fabs(d);
      sg = __builtin_fma((double)(2 * k + 1 - sc.M), d, sg);
      const double t = d - e;
      sv = __builtin_fma(t, t, sv);
      c.packed[k % (MB / 2)] += (unsigned)lanes(v[k] < y_cmp) << (k < MB / 2 ? 0 : 16);
    }
  c.row += lanes(ok);
  c.ties += lanes(ok && tie);
  const double ez = ok ? e : 0.0, az = ok ? sa * sc.inv_m : 0.0, gz = ok ? sg * sc.g_scale : 0.0,
               vz = ok ? sv * sc.inv_m1 : 0.0;
  const double we = w * ez;
  a.s2 += we;
  a.s3 = __builtin_fma(we, ez, a.s3);
  a.s4 += __builtin_fabs(we);
  a.s5 = __builtin_fma(w, az, a.s5);
  a.s6 = __builtin_fma(w, gz, a.s6);
  a.s7 = __builtin_fma(w, vz, a.s7);
}

// One workgroup = one row chunk of one plane.  MB: the bucket; PPL: points per lane and item (4: a quad of columns, 1: a
// column).  partial: per workgroup partial_bytes(MB) bytes.
template <int MB, int PPL>
__global__ __launch_bounds__(kThreads) void ensemble_scores_kernel(const float* const* __restrict__ member_planes,
                                                                   const float* const* __restrict__ truth_planes,
                                                                   int n_members, int n_planes, int n_lat, int n_lon,
                                                                   int n_chunks, const double* __restrict__ row_w,
                                                                   char* __restrict__ partial) {
  static_assert(PPL == 1 || PPL == 4, "an item is a column or a quad of columns");
  __shared__ double s_wave[kWaves][kSlots];
  __shared__ int s_counts[kWaves][MB + 2];
  const int plane = (int)(blockIdx.x / (unsigned)n_chunks), chunk = (int)(blockIdx.x % (unsigned)n_chunks);
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int M = __builtin_amdgcn_readfirstlane(n_members);
  const Scale sc{M, 1.0 / (double)M, 2.0 / ((double)M * (double)M), 1.0 / (double)(M - 1)};
  const gptr<const float> T = (gptr<const float>)truth_planes[plane];
  const float* const* __restrict__ members = member_planes + plane;          // member m: members[m * n_planes]
  bool vec = false;
  if (PPL == 4) {                                                // the quad rule over T and the M member pointers
    uintptr_t bits = (uintptr_t)T | (uintptr_t)(n_lon & 3);
    for (int m = 0; m < M; ++m) bits |= (uintptr_t)members[(int64_t)m * n_planes];
    vec = (bits & 15) == 0;
  }
  const int n_items = PPL == 4 ? (n_lon + 3) >> 2 : n_lon;
  const int rows = chunk_rows(n_lon, chunk_elems(MB), kWaves);
  const int r_begin = chunk * rows, r_end = min(r_begin + rows, n_lat);
  const float inf = __builtin_inff();
  constexpr int kBlock = Counts<MB>::kFlushPoints / PPL;       // items between two flushes of the packed counts

  Acc a;
  Counts<MB> c;
  double s1 = 0.0;
  for (int r = r_begin + wave; r < r_end; r += kWaves) {       // wave-uniform: w is one scalar load per row
    const double w = row_w[r];
    const int64_t row0 = (int64_t)r * n_lon;
    c.row = 0;
    for (int block = 0; block < n_items; block += kBlock) {    // (a flush per row where n_items <= kBlock)
    const int block_end = min(block + kBlock, n_items);
    for (int i0 = block; i0 < block_end; i0 += 64) {           // wave-uniform trip count: ballots see whole waves
      const bool in = i0 + lane < n_items;
      const int item = in ? i0 + lane : n_items - 1;           // clamped: the load is in the row, the guard is `in`
      float x[PPL][MB], y[PPL];
      bool in_row[PPL];
      if (PPL == 1) {
        y[0] = T[row0 + item];
        in_row[0] = in;
#pragma unroll
        for (int m = 0; m < MB; ++m)
          x[0][m] = m < M ? ((gptr<const float>)members[(int64_t)m * n_planes])[row0 + item] : inf;
      } else if (vec) {                                        // the quad rule, written out for the `m < M` guards
        const f32x4 t = ((gptr<const f32x4>)(T + row0))[item];
#pragma unroll
        for (int p = 0; p < PPL; ++p) y[p] = t[p], in_row[p] = in;
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          f32x4 q = {inf, inf, inf, inf};
          if (m < M) q = ((gptr<const f32x4>)((gptr<const float>)members[(int64_t)m * n_planes] + row0))[item];
#pragma unroll
          for (int p = 0; p < PPL; ++p) x[p][m] = q[p];
        }
      } else {
        int col[PPL];
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
          col[p] = min(4 * item + p, n_lon - 1);
          in_row[p] = in && 4 * item + p < n_lon;
          y[p] = T[row0 + col[p]];
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          const gptr<const float> P = (gptr<const float>)members[(int64_t)(m < M ? m : 0) * n_planes];
#pragma unroll
          for (int p = 0; p < PPL; ++p) x[p][m] = m < M ? P[row0 + col[p]] : inf;
        }
      }
#pragma unroll
      for (int p = 0; p < PPL; ++p) point<MB>(a, c, sc, w, x[p], y[p], in_row[p]);
    }
    c.flush(lane);
    }
    c.valid += c.row;
    s1 = __builtin_fma(w, (double)c.row, s1);                  // (wave-uniform: the wave's sum as it stands)
  }

  const double sums[kSlots] = {(double)c.valid, s1, wave_sum_f64(a.s2), wave_sum_f64(a.s3), wave_sum_f64(a.s4),
                               wave_sum_f64(a.s5), wave_sum_f64(a.s6), wave_sum_f64(a.s7)};
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < kSlots; ++s) s_wave[wave][s] = sums[s];
    s_counts[wave][0] = c.valid;
    s_counts[wave][MB + 1] = c.ties;
  }
  if (lane < MB) s_counts[wave][1 + lane] = c.below;
  __syncthreads();
  char* const mine = partial + (int64_t)blockIdx.x * partial_bytes(MB);
  const int t = (int)threadIdx.x;
  if (t < kSlots) {
    ((double*)mine)[t] = sum_waves(s_wave, t);
  } else if (t >= 64 && t < 64 + MB + 2) {                     // (the second wave: both stores go out side by side)
    int v = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) v += s_counts[k][t - 64];
    ((int*)(mine + kSlots * 8))[t - 64] = v;
  }
}

// One lane per (plane, output): the eight sums, the M + 1 bins, the ties; partials added in chunk order.
__global__ __launch_bounds__(kThreads) void ensemble_finish_kernel(const char* __restrict__ partial, int n_members,
                                                                   int bucket, int n_planes, int n_chunks,
                                                                   double* __restrict__ sums, int64_t* __restrict__ hist) {
  const int per_plane = kSlots + n_members + 2;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)n_planes * per_plane) return;
  const int64_t plane = i / per_plane;
  const int j = (int)(i % per_plane);
  const int64_t stride = partial_bytes(bucket);
  const char* p = partial + plane * n_chunks * stride;
  if (j < kSlots) {
    double v = ((const double*)p)[j];           // the plane stage of planes.h: partial 0, then += partial 1, 2, ...
    for (int k = 1; k < n_chunks; ++k) v += ((const double*)(p + k * stride))[j];
    sums[plane * kSlots + j] = v;
    return;
  }
  // counts of a partial: [0] valid points, [1 + k] #{x_(k) < y}, [bucket + 1] ties.  With C(0) = valid, C(b) = #{x_(b-1) < y}
  // and C(M + 1) = 0, bin b (exactly b members below the truth) holds C(b) - C(b + 1) points.
  const int b = j - kSlots;
  const int first = b <= n_members ? b : bucket + 1, second = b < n_members ? b + 1 : -1;
  int64_t v = 0;
  for (int k = 0; k < n_chunks; ++k) {
    const int* cnt = (const int*)(p + k * stride + kSlots * 8);
    v += cnt[first];
    if (second >= 0) v -= cnt[second];
  }
  hist[plane * (n_members + 2) + b] = v;
}

template <int MB, int PPL>
void launch(unsigned groups, void* stream, const float* const* member_planes, const float* const* truth_planes, int n_members,
            int n_planes, int n_lat, int n_lon, int n_chunks, const double* row_w, char* partial) {
  hipLaunchKernelGGL((ensemble_scores_kernel<MB, PPL>), dim3(groups), dim3(kThreads), 0, as_stream(stream), member_planes,
                     truth_planes, n_members, n_planes, n_lat, n_lon, n_chunks, row_w, partial);
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_ensemble_scores_workspace_bytes(int n_members, int n_planes, int n_lat, int n_lon) {
  if (n_members < 2 || n_members > kMaxMembers) return 0;
  const int bucket = bucket_of(n_members);
  return (size_t)chunk_plan(n_planes, n_lat, n_lon, chunk_elems(bucket), kWaves).groups * (size_t)partial_bytes(bucket);
}

extern "C" int aurora_hip_ensemble_scores(const float* const* member_planes, const float* const* truth_planes, int n_members,
                                          int n_planes, int n_lat, int n_lon, const double* row_w, double* sums,
                                          int64_t* hist, void* workspace, void* stream) {
  AURORA_CHECK_ARG(n_members >= 2 && n_members <= kMaxMembers, "ensemble_scores: n_members must be in 2..%d, got %d",
                   kMaxMembers, n_members);
  const int bucket = bucket_of(n_members);
  ChunkPlan plan;
  if (const int code = plan_chunks("ensemble_scores", n_planes, n_lat, n_lon, chunk_elems(bucket), kWaves, &plan)) return code;
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(member_planes && truth_planes && row_w && sums && hist && workspace,
                   "ensemble_scores: null plane array, weight, output or workspace pointer");
  AURORA_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)sums | (uintptr_t)hist | (uintptr_t)row_w) & 7) == 0,
                   "ensemble_scores: weights, outputs and workspace must be 8-byte aligned");
  // (a wave's counts are 32-bit: at most chunk_rows x n_lon points of a workgroup)
  AURORA_CHECK_ARG((int64_t)chunk_rows(n_lon, chunk_elems(bucket), kWaves) * n_lon <= 0x7fffffff, "ensemble_scores: n_lon %d is too long a row",
                   n_lon);
  char* const partial = (char*)workspace;
#define AURORA_ENSEMBLE_LAUNCH(MB, PPL)                                                                          \
  launch<MB, PPL>((unsigned)plan.groups, stream, member_planes, truth_planes, n_members, n_planes, n_lat, n_lon, \
                  (int)plan.n_chunks, row_w, partial)
  switch (bucket) {
    case 4: AURORA_ENSEMBLE_LAUNCH(4, 4); break;
    case 8: AURORA_ENSEMBLE_LAUNCH(8, 4); break;
    case 16: AURORA_ENSEMBLE_LAUNCH(16, 4); break;
    case 32: AURORA_ENSEMBLE_LAUNCH(32, 1); break;
    default: AURORA_ENSEMBLE_LAUNCH(64, 1); break;
  }
#undef AURORA_ENSEMBLE_LAUNCH
  const int code = check_launch("ensemble_scores");
  if (code != AURORA_OK) return code;
  const int64_t outputs = (int64_t)n_planes * (kSlots + n_members + 2);
  hipLaunchKernelGGL(ensemble_finish_kernel, dim3((unsigned)((outputs + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     as_stream(stream), partial, n_members, bucket, n_planes, (int)plan.n_chunks, sums, hist);
  return check_launch("ensemble_scores (finish)");
}
