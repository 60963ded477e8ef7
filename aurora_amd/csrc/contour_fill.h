// The window and word arithmetic of aurora_amd.closed_contours (include/aurora_hip.h has the rule): a candidate's WINDOW -- the
// source rows of its disc plus one ring row above and below, the disc's columns plus one ring column on either side -- as rows of
// 64-bit words, bit b of word w being local column 64 w + b, and the bounded flood fill on such rows.  Plain C++ with no
// dependency: the kernel of contours.hip and the host program tools/probes/contour_fill_host.cpp include this one file, so the
// shifts, the carries between words and the seam are written once.
//
// Two kinds of window.  LINEAR: local column l is the global column first + l -- taken mod W on a full circle (where the ring
// columns may name one global column twice: they hold no member, so nothing is filled twice), and no column at all outside
// 0 .. W - 1 on a regional grid.  CYCLIC (a full circle whose widest row of the disc is the whole row): local column l IS the
// global column l, width = W, and column W - 1 joins column 0.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AURORA_CONTOUR_HD __host__ __device__ inline
#else
#define AURORA_CONTOUR_HD inline
#endif

namespace aurora {

// The LDS budget of the three bitmaps of a workgroup (passable member, passable non-member, reached): 156 KiB of the CU's
// 160 KiB; the rest is the kernel's static LDS.
constexpr int kContourLdsBudget = 156 * 1024;

// Bytes of the three bitmaps for windows of up to max_rows source rows and max_words words a row.
AURORA_CONTOUR_HD int64_t contour_lds_bytes(int max_rows, int max_words) { return 3 * 8 * (int64_t)(max_rows + 2) * max_words; }

struct ContourWindow {
  int rows;     // local rows: the source rows of the disc and the two ring rows (set by the caller)
  int words;    // 64-bit words of a local row
  int width;    // local columns
  int first;    // linear: the global column of local column 0 before it is wrapped (-1 or more on a regional grid)
  int cyclic;   // 1: the local row is the whole circle
};

// The window of a candidate in column j0 whose widest disc row has half width n_max >= 0 (at most W).
AURORA_CONTOUR_HD ContourWindow contour_window(int j0, int n_max, int W, bool wrap) {
  ContourWindow q;
  q.rows = 0;
  if (wrap && 2 * n_max + 1 >= W) {
    q.cyclic = 1, q.first = 0, q.width = W;
  } else {
    int lo = j0 - n_max - 1, hi = j0 + n_max + 1;
    if (!wrap) {                                   // clipped to the columns -1 .. W: the ring beyond a regional row is empty
      lo = lo < -1 ? -1 : lo;
      hi = hi > W ? W : hi;
    }
    q.cyclic = 0, q.first = lo, q.width = hi - lo + 1;
  }
  q.words = (q.width + 63) >> 6;
  return q;
}

// The most words any window of a target row with widest half width n_max can have, whatever the column: what the host sums up
// into max_words.
AURORA_CONTOUR_HD int contour_row_words(int n_max, int W, bool wrap) {
  int width;
  if (wrap) width = 2 * n_max + 1 >= W ? W : 2 * n_max + 3;
  else width = 2 * n_max + 3 < W + 2 ? 2 * n_max + 3 : W + 2;
  return (width + 63) >> 6;
}

// The global column of local column l, or -1 where there is none.
AURORA_CONTOUR_HD int contour_column(const ContourWindow& q, int l, int W, bool wrap) {
  if (l >= q.width) return -1;
  if (q.cyclic) return l;
  int c = q.first + l;
  if (!wrap) return c >= 0 && c < W ? c : -1;
  if (c < 0) c += W;
  if (c >= W) c -= W;
  return c >= 0 && c < W ? c : -1;
}

// Is local column l (which names a column) within n columns of the candidate's column j0?  n = -1: never.
AURORA_CONTOUR_HD bool contour_is_member(const ContourWindow& q, int l, int j0, int n, int W) {
  int d = q.cyclic ? l - j0 : q.first + l - j0;
  if (d < 0) d = -d;
  if (q.cyclic && W - d < d) d = W - d;
  return d <= n;
}

AURORA_CONTOUR_HD uint64_t contour_reverse(uint64_t v) {
  v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
  v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
  v = ((v >> 4) & 0x0f0f0f0f0f0f0f0full) | ((v & 0x0f0f0f0f0f0f0f0full) << 4);
  v = ((v >> 8) & 0x00ff00ff00ff00ffull) | ((v & 0x00ff00ff00ff00ffull) << 8);
  v = ((v >> 16) & 0x0000ffff0000ffffull) | ((v & 0x0000ffff0000ffffull) << 16);
  return (v >> 32) | (v << 32);
}

// The bits of `a` from every bit of s (a subset of a) upwards to the end of its run of ones in a: the addition carries through
// the run and clears it; a seed further up in a run that a lower seed has cleared is set again by its own addition, hence | s.
AURORA_CONTOUR_HD uint64_t contour_run_up(uint64_t s, uint64_t a) { return (a & ~(a + s)) | s; }

// THE HORIZONTAL SHORTCUT: every run of ones of `a` that holds a bit of s (a subset of a), whole -- within the word; a run that
// goes on in the next word is picked up there by the next sweep.
AURORA_CONTOUR_HD uint64_t contour_run_fill(uint64_t s, uint64_t a) {
  return contour_run_up(s, a) | contour_reverse(contour_run_up(contour_reverse(s), contour_reverse(a)));
}

// Word w of row r of a bitmap, dilated by one column to either side: the carries between words, and on a cyclic window the seam
// (the top column, bit (width - 1) & 63 of the last word, joins bit 0 of word 0).  ld(r, w) is the word.  Bits past the width
// may be set in the result; every caller masks it with a bitmap that has none there.
template <typename Load>
AURORA_CONTOUR_HD uint64_t contour_spread(const Load& ld, int r, int w, const ContourWindow& q) {
  const uint64_t mid = ld(r, w);
  const int last = q.words - 1, top = (q.width - 1) & 63;
  uint64_t out = mid | (mid << 1) | (mid >> 1);
  if (w > 0) out |= ld(r, w - 1) >> 63;
  else if (q.cyclic) out |= (ld(r, last) >> top) & 1ull;
  if (w < last) out |= ld(r, w + 1) << 63;
  else if (q.cyclic) out |= (ld(r, 0) & 1ull) << top;
  return out;
}

// The bits of word w of row r (1 <= r <= rows - 2) that have a neighbour -- 8: the ring of eight; else the four -- or
// themselves in the bitmap.
template <typename Load>
AURORA_CONTOUR_HD uint64_t contour_dilate(const Load& ld, int r, int w, const ContourWindow& q, bool eight) {
  uint64_t s = contour_spread(ld, r, w, q);
  if (eight) s |= contour_spread(ld, r - 1, w, q) | contour_spread(ld, r + 1, w, q);
  else s |= ld(r - 1, w) | ld(r + 1, w);
  return s;
}

// One step of R |= A & dilate(R) for word w of row r, with the horizontal shortcut; `a` is the word of A.  The result holds the
// word's own bits of R (R is a subset of A), and only bits of the fill: a bit of A next to a bit of R, and the run it is in.
template <typename Load>
AURORA_CONTOUR_HD uint64_t contour_reach(const Load& reached, uint64_t a, int r, int w, const ContourWindow& q, bool eight) {
  return contour_run_fill(contour_dilate(reached, r, w, q, eight) & a, a);
}

// The bits of word w of a row of a REGIONAL window whose points are on the edge of the grid: all of them in row 0 and row
// H - 1 (`edge_row`), else the columns 0 and W - 1.
AURORA_CONTOUR_HD uint64_t contour_edge(const ContourWindow& q, int w, bool edge_row, int W) {
  if (edge_row) return ~0ull;
  uint64_t m = 0;
  const int west = -q.first, east = W - 1 - q.first;              // the local columns of the global columns 0 and W - 1
  if (west >= 0 && (west >> 6) == w) m |= 1ull << (west & 63);
  if (east >= 0 && (east >> 6) == w) m |= 1ull << (east & 63);
  return m;
}

}  // namespace aurora
