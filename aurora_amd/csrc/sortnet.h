// Sorting a point's member values in registers, shared by ensemble_scores.hip and ensemble_quantiles.hip: Batcher's
// odd-even merge network on integer keys.  Every index is a compile-time constant, so an array sorted here stays in
// registers.
#pragma once

#include <utility>

#include "common.h"

namespace aurora {

// ---- Batcher's odd-even merge sort for N = 2^k inputs as a table of compare-exchange pairs ----------------------------
template <int N> struct SortNet {
  int count = 0;
  unsigned char lo[N * 11] = {}, hi[N * 11] = {};        // (N log N (log N + 1) / 4 pairs at most: 672 for N = 64)
};
template <int N> constexpr SortNet<N> make_sort_net() {
  SortNet<N> s{};
  for (int p = 1; p < N; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j <= N - 1 - k; j += 2 * k)
        for (int i = 0; i < k && i <= N - j - k - 1; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            s.lo[s.count] = (unsigned char)(i + j);
            s.hi[s.count] = (unsigned char)(i + j + k);
            ++s.count;
          }
  return s;
}
template <int N> struct Net { static constexpr SortNet<N> v = make_sort_net<N>(); };

// The network runs on integer keys: key(x) = bits ^ (0x7fffffff where the sign is set) orders as the floats do (-0 just
// below +0, +inf above every finite value), is its own inverse, and integer min / max need no NaN handling (fp32 min /
// max cost a canonicalising instruction per operand here, which doubled the network).
__device__ __forceinline__ int sort_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

template <int N, int I> __device__ __forceinline__ int compare_exchange(int (&v)[N]) {
  constexpr int a = Net<N>::v.lo[I], b = Net<N>::v.hi[I];
  const int lo = min(v[a], v[b]), hi = max(v[a], v[b]);
  v[a] = lo;
  v[b] = hi;
  return 0;
}
template <int N, size_t... I> __device__ __forceinline__ void sort_keys(int (&v)[N], std::index_sequence<I...>) {
  const int done[] = {compare_exchange<N, (int)I>(v)...};
  (void)done;
}
template <int N> __device__ __forceinline__ void sort_ascending(float (&v)[N]) {
  int key[N];
#pragma unroll
  for (int k = 0; k < N; ++k) key[k] = sort_key(__float_as_int(v[k]));
  sort_keys<N>(key, std::make_index_sequence<Net<N>::v.count>{});
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = __int_as_float(sort_key(key[k]));
}

// The member-count bucket: the smallest of 4, 8, 16, 32, 64 that holds M; the slots past M hold +inf and sort last.
constexpr int kMaxMembers = 64;
constexpr int bucket_of(int n_members) {
  return n_members <= 4 ? 4 : n_members <= 8 ? 8 : n_members <= 16 ? 16 : n_members <= 32 ? 32 : 64;
}

}  // namespace aurora
