// The window arithmetic of aurora_amd.extrema (include/aurora_hip.h has the rule): which two entries of a row's DOUBLING
// TABLES give the minimum over the columns j - n .. j + n, on a full circle (wrap) and on a regional grid (clip).  Plain C++
// with no dependency: the filter kernel of extrema.hip and the host program tools/probes/extrema_window_host.cpp include this
// one file, so the case split is written once.
//
// The tables of a row of W entries: m[0][c] is the entry of column c, and
//   m[l + 1][c] = min(m[l][c], m[l][p])   with p = extrema_partner(c, l, W, wrap),   m[l + 1][c] = m[l][c] where p < 0,
// so m[l][c] is the minimum over the 2^l columns from c eastwards -- around the circle on a full circle (2^l <= W is all that
// is ever asked for), up to the end of the row on a regional grid.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AURORA_EXTREMA_HD __host__ __device__ inline
#else
#define AURORA_EXTREMA_HD inline
#endif

namespace aurora {

// min(m[level - back][a], m[level - back][b]) is the minimum over the window; a and b are in [0, W - 1].  `level` depends on
// n alone: it is the step of the doubling at which every column of a target row is answered.  `back` is 0 or 1: on a regional
// grid a window that is clipped to less than 2^level columns reads the table before, which the doubling still holds.
struct ExtremaWindow {
  int level, back, a, b;
};

AURORA_EXTREMA_HD int extrema_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// floor(log2(v)) for v >= 1.
AURORA_EXTREMA_HD int extrema_log2(int v) { return 31 - __builtin_clz((unsigned)(v < 1 ? 1 : v)); }

// Is the window of EVERY column the whole row?  (Then the row's extreme answers, and no table is needed.)
AURORA_EXTREMA_HD bool extrema_whole_row(int n, int W, bool wrap) { return wrap ? 2 * n + 1 >= W : n >= W - 1; }

// The step at which a target row with half width n >= 0 is answered: floor(log2(2 n + 1)).
AURORA_EXTREMA_HD int extrema_level(int n) { return extrema_log2(2 * n + 1); }

// The second entry of the doubling step l -> l + 1 at column c, or -1 for none (past the end of a regional row).
AURORA_EXTREMA_HD int extrema_partner(int c, int l, int W, bool wrap) {
  const int p = c + (1 << l);
  if (p < W) return p;
  return wrap ? extrema_clamp(p - W, 0, W - 1) : -1;
}

// The window of column j (0 <= j < W) with half width n >= 0 where extrema_whole_row(n, W, wrap) is false, W >= 1.
AURORA_EXTREMA_HD ExtremaWindow extrema_window(int j, int n, int W, bool wrap) {
  ExtremaWindow q;
  q.level = extrema_level(n);
  if (wrap) {                                    // 2 n + 1 < W: the window is 2 n + 1 >= 2^level columns, around the circle
    int a = j - n, b = j + n + 1 - (1 << q.level);
    if (a < 0) a += W;
    if (b < 0) b += W;
    if (b >= W) b -= W;
    q.back = 0, q.a = extrema_clamp(a, 0, W - 1), q.b = extrema_clamp(b, 0, W - 1);
  } else {                                       // clipped into the row: n + 1 or more columns, so at least 2^(level - 1)
    const int lo = extrema_clamp(j - n, 0, W - 1), hi = extrema_clamp(j + n, 0, W - 1);
    const int own = extrema_log2(hi - lo + 1);
    q.back = own < q.level ? 1 : 0;
    const int l = q.level - q.back;
    q.a = lo, q.b = extrema_clamp(hi + 1 - (1 << l), lo, W - 1);
  }
  return q;
}

}  // namespace aurora
