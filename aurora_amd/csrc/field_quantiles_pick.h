// The integer side of aurora_hip_field_quantiles (field_quantiles.hip) between two passes of its radix select: what q asks
// for as integer targets, which bin of a 256-bin histogram holds a target, and the inverse of the key.  Plain C++ without a
// device construct, so that the same text also compiles for the host (tools/probes/field_quantiles_pick_host.cpp runs it
// under the sanitizers).
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define AURORA_FQ_HD __host__ __device__ __forceinline__
#else
#define AURORA_FQ_HD inline
#endif

namespace aurora {
namespace fq {

constexpr int kBins = 256;                       // 8 bits per pass, most significant first
constexpr int kMaxQ = 8;
constexpr int kMaxTargets = 2 * kMaxQ;           // kind = count: x_(j) and x_(hi) of every q

// kind = count: (j, g) of the rule for n >= 1 valid points, the expression of aurora_hip_ensemble_quantiles with n for M.
// One multiplication and one subtraction in fp64, each rounded on its own.
AURORA_FQ_HD void count_index(int64_t n, double q, int64_t* j, int64_t* hi, double* g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double h = (double)(n - 1) * q;
  int64_t f = (int64_t)__builtin_floor(h);
  if (f > n - 1) f = n - 1;
  *j = f;
  *hi = f + 1 < n - 1 ? f + 1 : n - 1;
  *g = h - (double)f;
}

// kind = area: target = min(max((int64)ceil(q (double)W), 1), W) for W >= 1.
AURORA_FQ_HD int64_t area_target(int64_t W, double q) {
  int64_t t = (int64_t)__builtin_ceil(q * (double)W);
  if (t < 1) t = 1;
  return t < W ? t : W;
}

// The first bin b of hist[0 .. 255] with hist[0] + ... + hist[b] >= rem, and *before = hist[0] + ... + hist[b - 1].
// 1 <= rem <= the histogram's total is the caller's; otherwise the last bin is returned.  256 iterations, no early exit.
AURORA_FQ_HD int pick_bin(const int64_t* hist, int64_t rem, int64_t* before) {
  int bin = kBins - 1;
  int64_t cum = 0, b4 = 0;
  bool found = false;
  for (int b = 0; b < kBins; ++b) {
    const int64_t next = cum + hist[b];
    const bool here = !found && next >= rem;
    bin = here ? b : bin;
    b4 = here ? cum : b4;
    found = found || here;
    cum = next;
  }
  if (!found) b4 = cum - hist[kBins - 1];
  *before = b4;
  return bin;
}

// The float32 bits whose key is k (K = ~u where u has the sign bit, else u | 0x80000000).
AURORA_FQ_HD uint32_t key_to_bits(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// Targets that share a prefix share a histogram in the next pass: slot[t] = the index of prefix[t] among the DISTINCT
// prefixes of the live targets in order of first appearance (-1 for a dead target, rem[t] == 0); returns their number.
AURORA_FQ_HD int distinct_prefixes(const uint32_t* prefix, const int64_t* rem, int n_targets, uint32_t* distinct,
                                          int32_t* slot) {
  int n = 0;
  for (int t = 0; t < n_targets; ++t) {          // bounded by the number of targets, twice
    slot[t] = -1;
    if (rem[t] == 0) continue;
    int d = 0;
    while (d < n && distinct[d] != prefix[t]) ++d;
    if (d == n) distinct[n++] = prefix[t];
    slot[t] = d;
  }
  return n;
}

}  // namespace fq
}  // namespace aurora
