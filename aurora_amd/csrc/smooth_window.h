// The window arithmetic of aurora_amd.smooth (include/aurora_hip.h has the rule): which entries of a row's exclusive prefix
// table make the sum over the columns j - n .. j + n, on a full circle (wrap) and on a regional grid (clip).  Plain C++ with
// no dependency: the gather kernel of smooth.hip and the host program tools/probes/smooth_window_host.cpp include this one
// file, so the case split is written once.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AURORA_SMOOTH_HD __host__ __device__ inline
#else
#define AURORA_SMOOTH_HD inline
#endif

namespace aurora {

// sum = (P[e1] - P[e0]) + P[e2] over a table P[0 .. W] with P[0] = 0; every index is in [0, W].  e2 = 0 where the window
// does not wrap: P[0] is exactly 0 and a prefix is never -0, so the kernel may leave that term out and get the same bits.
struct SmoothWindow {
  int e0, e1, e2;
};

AURORA_SMOOTH_HD int smooth_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The columns of a source row that a window of half width n >= 0 around column j counts on a grid of W columns: 2 n + 1, on
// a full circle at most the whole row.  (Columns clipped off a regional grid stay counted: they are invalid, not absent.)
AURORA_SMOOTH_HD int smooth_full_width(int n, int W, bool wrap) {
  const int full = 2 * n + 1;
  return wrap && full > W ? W : full;
}

// The window of column j (0 <= j < W) with half width n (0 <= n; on a full circle n <= W / 2), W >= 1.
AURORA_SMOOTH_HD SmoothWindow smooth_window(int j, int n, int W, bool wrap) {
  const int lo = j - n, hi = j + n + 1;
  SmoothWindow s;
  if (!wrap) {                                   // regional: clip into the row
    s.e0 = smooth_clamp(lo, 0, W), s.e1 = smooth_clamp(hi, 0, W), s.e2 = 0;
  } else if (2 * n + 1 >= W) {                   // the whole row
    s.e0 = 0, s.e1 = W, s.e2 = 0;
  } else if (lo < 0) {                           // over the western edge: lo + W .. W - 1 and 0 .. hi - 1
    s.e0 = smooth_clamp(lo + W, 0, W), s.e1 = W, s.e2 = smooth_clamp(hi, 0, W);
  } else if (hi > W) {                           // over the eastern edge: lo .. W - 1 and 0 .. hi - W - 1
    s.e0 = smooth_clamp(lo, 0, W), s.e1 = W, s.e2 = smooth_clamp(hi - W, 0, W);
  } else {
    s.e0 = smooth_clamp(lo, 0, W), s.e1 = smooth_clamp(hi, 0, W), s.e2 = 0;
  }
  return s;
}

}  // namespace aurora
