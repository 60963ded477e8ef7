// The parts of aurora_hip_link_extrema (links.hip) that decide a result, apart from the kernel so that a host program can run
// the very same text (tools/probes/link_extrema_host.cpp does, under the sanitizers, against a brute-force double loop): which
// rows of a table are live, the point of a row, the key of a pair and the scan of one staged tile by one row.  THE RULE is stated
// in aurora_amd/links.py; the key itself is `key_of` of nearest_event_search.h.  Plain C++ without a device construct.
#pragma once

#include <stdint.h>

#include "nearest_event_search.h"

namespace aurora {
namespace links {

constexpr int kThreads = 256;                    // rows of a chunk: a thread owns one row of its side
constexpr int kTile = 1024;                      // rows of the other side staged at a time: 24 bytes each
constexpr int kMaxLon = ne::kMaxLon;             // cd fits LDS: 32 KiB at 4096 longitudes
constexpr int kMaxPoints = 65536;                // of `extrema`
constexpr uint64_t kInfBits = 0x7FF0000000000000ull;

// A row of a side, gathered: the sine and cosine of its latitude, its flat index and its column; col = -1 where it is not live.
struct Point {
  double s, c;
  int32_t flat, col;
};

// The best partner so far: the smallest (key, row) among keys <= key_max.  +inf and -1: none.
struct Best {
  double key;
  int32_t row;
};

AURORA_NE_HD int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// THE RULE, point 2: the rows below min(count, max_points) can be live (a count below 0 counts as 0).
AURORA_NE_HD int rows_of(int count, int max_points) { return clamp_int(count, 0, max_points); }

// The point of a table row: the flat index is clamped into the grid BEFORE it addresses s or c.  `s` and `c` hold n_lat entries.
AURORA_NE_HD Point point_of(int64_t flat, bool live, const double* s, const double* c, int n_lat, int n_lon) {
  const int64_t last = (int64_t)n_lat * n_lon - 1;
  const int32_t at = (int32_t)(flat < 0 ? 0 : (flat > last ? last : flat));
  const int i = at / n_lon;
  Point p;
  p.s = s[i], p.c = c[i], p.flat = at, p.col = live ? at - i * n_lon : -1;
  return p;
}

// THE RULE, point 3: 0 exactly for one and the same grid point, else key_of over the gap of the columns.  Both columns are
// inside the row, so the gap is inside cd.
AURORA_NE_HD double pair_key(const Point& p, double sk, double ck, int32_t flat_k, int32_t col_k, const double* cd, int n_lon,
                             bool wrap) {
  if (flat_k == p.flat) return 0.0;
  return ne::key_of(p.s, p.c, sk, ck, cd[ne::gap_of(p.col, col_k, n_lon, wrap)]);
}

// One live row `p` against the n staged rows q0 .. q0 + n - 1 of the other side (THE RULE, point 4).  Rows are taken in
// ascending order and only a strictly smaller key replaces the best, so of equal keys the smallest row wins.
AURORA_NE_HD void scan_tile(Best& best, const Point& p, const double* ts, const double* tc, const int32_t* tflat,
                            const int32_t* tcol, int n, int q0, const double* cd, int n_lon, bool wrap, double key_max) {
  for (int e = 0; e < n; ++e) {
    const int32_t col = tcol[e];
    if (col < 0) continue;                       // not live
    const double key = pair_key(p, ts[e], tc[e], tflat[e], col, cd, n_lon, wrap);
    if (key <= key_max && key < best.key) best.key = key, best.row = q0 + e;
  }
}

// What a row stores: the bits of its key and the partner's row; the bits of +inf and -1 for none.
AURORA_NE_HD int64_t key_bits_of(const Best& best) {
  if (best.row < 0) return (int64_t)kInfBits;
  union {
    double d;
    int64_t i;
  } u;
  u.d = best.key;
  return u.i;
}

}  // namespace links
}  // namespace aurora
