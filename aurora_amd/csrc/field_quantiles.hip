// Spatial quantiles of planes on the device (aurora_amd.field_quantiles: the plane's 0.9 / 0.99 quantile by area or by count,
// the percentile thresholds of event_scores, objects and conditional_scores; the rule is stated in
// aurora_amd/field_quantiles.py and include/aurora_hip.h).
//
// An exact multi-target radix SELECT over the 32-bit key K(v) of objects.hip (ascending with the value, -0 below +0), most
// significant byte first, 8 bits per pass, four passes.  Every q becomes one integer TARGET (kind = area: a cumulative sum of
// row units) or two (kind = count: the cumulative counts j + 1 and hi + 1), and a target is found as the smallest key whose
// cumulative weight reaches it.  A fixed sequence of launches on the caller's stream:
//
//   zero      the histograms of all four passes in the workspace.
//   pass 0    every plane is read once; per plane one histogram of the key's top byte by COUNT and, with units, one by UNIT.
//             Their totals are n (valid) and W.
//   pick 0    one workgroup per plane: q -> targets (on the device: n and W are only known here), each target's bin and what
//             remains of it inside that bin; the targets' DISTINCT prefixes get one histogram slot each for the next pass.
//   pass p    p = 1, 2, 3: the planes are read again; a point whose key starts with one of the plane's distinct prefixes enters
//             that prefix' histogram of the next byte, with the weight of the kind.
//   pick p    as pick 0; pick 3 has the whole key: it inverts K, interpolates (count) and writes values, valid and total.
//
// A workgroup owns a row chunk of a plane and a wave a row at a time (the row's unit is one scalar), accumulates in LDS and
// flushes its non-zero bins with 64-bit integer vector atomics.  A realistic field sits in one or two bins of the top byte
// (all of a 2 m temperature in kelvin shares sign and exponent), so the lanes of a wave that share a bin are combined by
// ballot before the LDS atomic, as tabulate_kernel of objects.hip combines the lanes that share an object: kRounds leaders,
// then whatever is left goes one atomic per lane -- left over are the lanes of a SPREAD digit, which do not contend.
//
// Everything accumulated is an integer: the histograms, and with them every result, do not depend on the order of the
// atomics, on the other planes of the call or (the quad rule of planes.h) on pointer alignment.  Order between the phases is
// the order of the launches: no kernel spins or waits on a value that another workgroup writes in the same launch, and every
// loop is bounded by n_lat, n_lon, 256 or the number of targets (the ballot loop by kRounds).
#include <cmath>

#include "field_quantiles_pick.h"
#include "planes.h"

namespace aurora {
namespace {

using namespace fq;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunkElems = 40960;               // target size of a row chunk, as scores.hip
constexpr int kRounds = 3;                       // leaders per point before the lanes go one by one
constexpr int64_t kMaxPoints = 0x7ffffffell, kMaxAreaPoints = 1ll << 30;   // (the unit sum stays within int64, as objects)

// What the library makes of the host's q: passed to the kernels BY VALUE (no table is uploaded: a call is capturable).
struct Spec {
  int n;
  double q[kMaxQ];
};

// A plane's select between two passes.  rem[t] == 0: a dead target (no valid point, or W = 0); its result is NaN.
struct PlaneState {
  int64_t n, W;                                  // valid points; sum of unit over them (n without units)
  int64_t rem[kMaxTargets];                      // what is left of the target inside its prefix
  uint32_t prefix[kMaxTargets];                  // the bytes of the key found so far, the first one highest
  int32_t slot[kMaxTargets];                     // the target's histogram in the coming pass
  uint32_t distinct[kMaxTargets];                // the prefix of every slot
  int32_t n_distinct, pad;
};

// The workspace: the histograms of pass 0 (two per plane), of passes 1 .. 3 (n_targets per plane each), the states.
struct Layout {
  int64_t hist[4];                               // offsets in int64 words
  int64_t hist_words, state_word, words;
};
Layout layout_of(int64_t n_planes, int n_q) {
  const int64_t nt = 2 * n_q;                    // of kind = count; kind = area uses half of it
  Layout l;
  l.hist[0] = 0;
  l.hist[1] = n_planes * 2 * kBins;
  for (int p = 2; p < 4; ++p) l.hist[p] = l.hist[p - 1] + n_planes * nt * kBins;
  l.hist_words = l.hist[3] + n_planes * nt * kBins;
  l.state_word = l.hist_words;
  l.words = l.state_word + n_planes * (int64_t)(sizeof(PlaneState) / 8);
  return l;
}
static_assert(sizeof(PlaneState) % 8 == 0, "the states follow the histograms in int64 words");

__device__ __forceinline__ uint32_t value_key_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

__global__ __launch_bounds__(kThreads) void quantile_zero_kernel(int64_t* __restrict__ words, int64_t n_words) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_words; i += stride) words[i] = 0;   // bounded by n_words
}

// ---- a pass -----------------------------------------------------------------------------------------------------------------
// One point of every lane: `idx` is its LDS bin (-1: none).  The lanes that share the bin of a leader are added by the leader.
// FIRST with units: the bin pair (idx, 256 + idx) takes (count, count x unit).
template <bool kFirst>
__device__ __forceinline__ void add_point(int64_t* s_hist, int idx, int lane, int64_t weight, bool pair) {
  bool active = idx >= 0;
  uint64_t todo = __ballot(active);
#pragma unroll
  for (int round = 0; round < kRounds; ++round) {
    if (!todo) break;                              // wave-uniform
    const int leader = __builtin_ctzll(todo);
    const int i0 = __shfl(idx, leader, 64);
    const uint64_t sel = __ballot(active && idx == i0);
    todo &= ~sel;
    if (lane == leader) {
      const int64_t n = __builtin_popcountll(sel);
      __hip_atomic_fetch_add(s_hist + i0, kFirst ? n : n * weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (kFirst && pair) __hip_atomic_fetch_add(s_hist + kBins + i0, n * weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    active = active && !((sel >> lane) & 1);
  }
  if (active) {
    __hip_atomic_fetch_add(s_hist + idx, kFirst ? (int64_t)1 : weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (kFirst && pair) __hip_atomic_fetch_add(s_hist + kBins + idx, weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// One workgroup = one row chunk of one plane.  kFirst: pass 0 (the top byte of every valid point; `states` is not read);
// otherwise pass `pass` in 1 .. 3 over the plane's distinct prefixes.  hist: this pass' histograms, `slots` of them per plane.
template <bool kFirst>
__global__ __launch_bounds__(kThreads) void quantile_pass_kernel(const float* const* __restrict__ planes, int n_lat, int n_lon,
                                                                 int n_chunks, const int64_t* __restrict__ unit, int pass,
                                                                 int slots, const PlaneState* __restrict__ states,
                                                                 int64_t* __restrict__ hist) {
  __shared__ int64_t s_hist[kMaxTargets * kBins];
  const int plane = (int)(blockIdx.x / (unsigned)n_chunks), chunk = (int)(blockIdx.x % (unsigned)n_chunks);
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const bool has_unit = unit != nullptr;
  int D = kFirst ? (has_unit ? 2 : 1) : __builtin_amdgcn_readfirstlane(states[plane].n_distinct);
  if (D == 0) return;                              // no live target (uniform over the workgroup, before any barrier)
  uint32_t prefix[kMaxTargets];
#pragma unroll
  for (int d = 0; d < kMaxTargets; ++d) prefix[d] = !kFirst && d < D ? states[plane].distinct[d] : 0u;
  for (int i = (int)threadIdx.x; i < D * kBins; i += kThreads) s_hist[i] = 0;   // bounded by 16 x 256
  __syncthreads();

  const gptr<const float> P = (gptr<const float>)planes[plane];
  const bool vec = quads_aligned(n_lon, P);
  const int n_quads = (n_lon + 3) >> 2;
  const int rows = chunk_rows(n_lon, kChunkElems, kWaves);
  const int r_begin = chunk * rows, r_end = min(r_begin + rows, n_lat);
  const int shift = kFirst ? 24 : 32 - 8 * pass;   // the prefix is key >> shift, the digit the byte below it

  for (int r = r_begin + wave; r < r_end; r += kWaves) {      // wave-uniform: the unit is one scalar load per row
    const int64_t weight = has_unit ? unit[r] : 1;
    const gptr<const float> row = P + (int64_t)r * n_lon;
    for (int q0 = 0; q0 < n_quads; q0 += 64) {                // bounded by n_lon
      const bool in = q0 + lane < n_quads;
      const int item = in ? q0 + lane : n_quads - 1;          // clamped: the load is in the row, the guard is `in`
      int col[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) col[k] = min(4 * item + k, n_lon - 1);
      const f32x4 v = vec ? load_quad<true>(row, item, col) : load_quad<false>(row, item, col);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t u = __float_as_uint(v[k]);
        const bool ok = in && 4 * item + k < n_lon && (u & 0x7fffffffu) < 0x7f800000u;
        const uint32_t key = value_key_bits(u);
        int idx = -1;
        if (kFirst) {
          idx = ok ? (int)(key >> 24) : -1;
        } else {
          const uint32_t top = key >> shift;
          const int digit = (int)((key >> (shift - 8)) & 255u);
#pragma unroll
          for (int d = 0; d < kMaxTargets; ++d) {
            if (d >= D) break;                                // wave-uniform
            idx = ok && top == prefix[d] ? d * kBins + digit : idx;
          }
        }
        add_point<kFirst>(s_hist, idx, lane, weight, has_unit);
      }
    }
  }
  __syncthreads();
  int64_t* const out = hist + (int64_t)plane * slots * kBins;  // D <= slots
  for (int i = (int)threadIdx.x; i < D * kBins; i += kThreads) {   // bounded by 16 x 256
    const int64_t c = s_hist[i];
    if (c != 0) __hip_atomic_fetch_add(out + i, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- a pick -----------------------------------------------------------------------------------------------------------------
// a + g (b - a) in fp64, every operation rounded on its own, then one rounding to fp32 (as ensemble_quantiles.hip).
__device__ __forceinline__ float interpolate(float af, float bf, double g) {
#pragma clang fp contract(off)
  const double a = (double)af, b = (double)bf;
  const double d = b - a;
  const double t = g * d;
  return (float)(a + t);
}

// One workgroup per plane; thread t < n_targets owns target t.  hist: the histograms of pass `pass`, `slots` per plane.
__global__ __launch_bounds__(kThreads) void quantile_pick_kernel(const int64_t* __restrict__ hist, int pass, int slots,
                                                                 int has_unit,
                                                                 const Spec spec, PlaneState* __restrict__ states,
                                                                 float* __restrict__ values, int64_t* __restrict__ valid,
                                                                 int64_t* __restrict__ total) {
  __shared__ int64_t s_hist[kMaxTargets * kBins];
  __shared__ int64_t s_rem[kMaxTargets];
  __shared__ uint32_t s_prefix[kMaxTargets];
  const int plane = (int)blockIdx.x, t = (int)threadIdx.x;
  PlaneState* const st = states + plane;
  const int n_q = spec.n;
  const int n_targets = has_unit ? n_q : 2 * n_q;
  const int D = pass == 0 ? (has_unit ? 2 : 1) : st->n_distinct;
  const int64_t* const in = hist + (int64_t)plane * slots * kBins;
  for (int i = t; i < D * kBins; i += kThreads) s_hist[i] = in[i];   // bounded by 16 x 256
  __syncthreads();

  int64_t n = 0, W = 0;
  if (pass == 0) {
    for (int b = 0; b < kBins; ++b) {                          // every thread adds the same 256 integers
      n += s_hist[b];
      W += has_unit ? s_hist[kBins + b] : s_hist[b];
    }
  } else {
    n = st->n, W = st->W;
  }
  if (t < n_targets) {
    int64_t rem = 0;
    uint32_t prefix = 0;
    int slot = has_unit ? 1 : 0;                               // of pass 0: the histogram of the kind's weight
    if (pass == 0) {
      if (has_unit) {
        rem = W > 0 ? area_target(W, spec.q[t]) : 0;
      } else if (n > 0) {
        int64_t j, hi;
        double g;
        count_index(n, spec.q[t >> 1], &j, &hi, &g);
        rem = ((t & 1) ? hi : j) + 1;
      }
    } else {
      rem = st->rem[t], prefix = st->prefix[t], slot = st->slot[t];
    }
    if (rem != 0) {                                            // then 0 <= slot < D
      int64_t before;
      const int bin = pick_bin(s_hist + slot * kBins, rem, &before);
      prefix = (prefix << 8) | (uint32_t)bin;
      rem -= before;                                           // >= 1: the bin holds the target
    }
    s_rem[t] = rem, s_prefix[t] = prefix;
  }
  __syncthreads();

  if (pass < 3) {
    if (t == 0) {
      uint32_t distinct[kMaxTargets];
      int32_t slot[kMaxTargets];
      const int n_distinct = distinct_prefixes(s_prefix, s_rem, n_targets, distinct, slot);
      st->n = n, st->W = W, st->n_distinct = n_distinct, st->pad = 0;
      for (int k = 0; k < kMaxTargets; ++k) {                  // bounded by the number of targets
        const bool live = k < n_targets;
        st->rem[k] = live ? s_rem[k] : 0;
        st->prefix[k] = live ? s_prefix[k] : 0u;
        st->slot[k] = live ? slot[k] : -1;
        st->distinct[k] = k < n_distinct ? distinct[k] : 0u;
      }
    }
    return;
  }
  // the key is complete
  if (t < n_q) {
    float v = __builtin_nanf("");
    if (has_unit) {
      if (s_rem[t] != 0) v = __uint_as_float(key_to_bits(s_prefix[t]));
    } else if (n > 0) {
      int64_t j, hi;
      double g;
      count_index(n, spec.q[t], &j, &hi, &g);
      v = interpolate(__uint_as_float(key_to_bits(s_prefix[2 * t])), __uint_as_float(key_to_bits(s_prefix[2 * t + 1])), g);
    }
    values[(int64_t)plane * n_q + t] = v;
  }
  if (t == 0) valid[plane] = n, total[plane] = W;
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" size_t aurora_hip_field_quantiles_workspace_bytes(int n_planes, int n_q) {
  if (n_planes < 1 || n_q < 1 || n_q > kMaxQ) return 0;
  return (size_t)layout_of(n_planes, n_q).words * 8;
}

extern "C" int aurora_hip_field_quantiles(const float* const* planes, int n_planes, int n_lat, int n_lon, const int64_t* unit,
                                          const double* q, int n_q, float* values, int64_t* valid, int64_t* total,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  ChunkPlan plan;
  if (const int code = plan_chunks("field_quantiles", n_planes, n_lat, n_lon, kChunkElems, kWaves, &plan)) return code;
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= (unit ? kMaxAreaPoints : kMaxPoints),
                   "field_quantiles: a grid of %d x %d points is beyond the %s", n_lat, n_lon,
                   unit ? "2^30 whose unit sum fits an int64" : "2^31 - 2 that are supported");
  AURORA_CHECK_ARG(n_q >= 1 && n_q <= kMaxQ, "field_quantiles: n_q must be in 1..%d, got %d", kMaxQ, n_q);
  AURORA_CHECK_ARG(q, "field_quantiles: null q");
  Spec spec{};
  spec.n = n_q;
  for (int i = 0; i < n_q; ++i) {
    AURORA_CHECK_ARG(std::isfinite(q[i]) && q[i] >= 0.0 && q[i] <= 1.0, "field_quantiles: q[%d] = %g is not in [0, 1]", i, q[i]);
    spec.q[i] = q[i];
  }
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(planes && values && valid && total && workspace,
                   "field_quantiles: null plane array, output or workspace pointer");
  AURORA_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)valid & 7) == 0 && ((uintptr_t)total & 7) == 0 &&
                       ((uintptr_t)unit & 7) == 0 && ((uintptr_t)values & 3) == 0,
                   "field_quantiles: unit, valid, total and workspace must be 8-byte aligned, values 4-byte aligned");
  const Layout l = layout_of(n_planes, n_q);
  AURORA_CHECK_ARG(workspace_bytes >= (size_t)l.words * 8, "field_quantiles: the workspace has %zu bytes, %zu are needed",
                   workspace_bytes, (size_t)l.words * 8);
  int64_t* const words = (int64_t*)workspace;
  PlaneState* const states = (PlaneState*)(words + l.state_word);
  const hipStream_t s = as_stream(stream);
  const int has_unit = unit ? 1 : 0, n_targets = 2 * n_q;      // slots per plane of the passes 1 .. 3
  const unsigned zero_groups = (unsigned)(l.hist_words / kThreads + 1 < 4096 ? l.hist_words / kThreads + 1 : 4096);
  int code;
  hipLaunchKernelGGL(quantile_zero_kernel, dim3(zero_groups), dim3(kThreads), 0, s, words, l.hist_words);
  if ((code = check_launch("field_quantiles (zero)")) != AURORA_OK) return code;
  for (int pass = 0; pass < 4; ++pass) {
    const int slots = pass == 0 ? 2 : n_targets;
    int64_t* const hist = words + l.hist[pass];
    if (pass == 0)
      hipLaunchKernelGGL(quantile_pass_kernel<true>, dim3((unsigned)plan.groups), dim3(kThreads), 0, s, planes, n_lat, n_lon,
                         (int)plan.n_chunks, unit, pass, slots, (const PlaneState*)states, hist);
    else
      hipLaunchKernelGGL(quantile_pass_kernel<false>, dim3((unsigned)plan.groups), dim3(kThreads), 0, s, planes, n_lat, n_lon,
                         (int)plan.n_chunks, unit, pass, slots, (const PlaneState*)states, hist);
    if ((code = check_launch("field_quantiles (pass)")) != AURORA_OK) return code;
    hipLaunchKernelGGL(quantile_pick_kernel, dim3((unsigned)n_planes), dim3(kThreads), 0, s, (const int64_t*)hist, pass, slots,
                       has_unit, spec, states, values, valid, total);
    if ((code = check_launch("field_quantiles (pick)")) != AURORA_OK) return code;
  }
  return AURORA_OK;
}
