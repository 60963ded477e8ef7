// The parts of aurora_hip_nearest_event (nearest_event.hip) that decide a result, apart from the kernels so that a host program
// can run the very same text (tools/probes/nearest_event_host.cpp does, under the sanitizers, against a brute force): the row
// candidate of a column from the event bits of its row, the key of a candidate, the visit of one source row by one target
// point, and the stop test of the row walk.  THE RULE is stated in aurora_amd/distances.py.  Plain C++ without a device construct.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define AURORA_NE_HD __host__ __device__ __forceinline__
#else
#define AURORA_NE_HD inline
#endif

namespace aurora {
namespace ne {

constexpr int kMaxLon = 4096;                    // 64 chunks of 64 columns: a column fits the int16 of the candidate map
constexpr int kNone = 1 << 20;                   // "no event on this side": farther than any column, and still far from overflow

// ---- the row candidate ------------------------------------------------------------------------------------------------------
// A row is cut into chunks of 64 columns; bit b of the mask of chunk c is set where column 64 c + b holds an event.
// The last / first event column of a chunk (mask != 0).
AURORA_NE_HD int chunk_last(uint64_t mask, int c) { return 64 * c + 63 - __builtin_clzll(mask); }
AURORA_NE_HD int chunk_first(uint64_t mask, int c) { return 64 * c + __builtin_ctzll(mask); }

// The nearest event WEST of column j = 64 c + lane, itself included, and the nearest EAST of it, itself included, as columns of
// the unrolled row: west_before is the last event column of the chunks before c (on a wrapping grid, failing that, the last
// event column of the row minus W), east_after the first of the chunks after c (failing that, the first of the row plus W);
// -kNone / +kNone where there is none.
AURORA_NE_HD int west_of(uint64_t mask, int c, int lane, int west_before) {
  const uint64_t m = mask & (~0ull >> (63 - lane));          // bits 0 .. lane
  return m ? chunk_last(m, c) : west_before;
}
AURORA_NE_HD int east_of(uint64_t mask, int c, int lane, int east_after) {
  const uint64_t m = mask >> lane;                           // bits lane .. 63, moved down
  return m ? 64 * c + lane + __builtin_ctzll(m) : east_after;
}

// THE RULE, point 3: of the two the one with the smaller gap, and of two at the same gap the smaller column of the grid; -1
// where the row has no event.  (Every other event of the row is farther west than `west` or farther east than `east`, and on a
// wrapping grid its gap min(d, W - d) is no smaller than the smaller of the two walks.)
AURORA_NE_HD int candidate(int j, int west, int east, int n_lon) {
  const bool hw = west > -kNone, he = east < kNone;
  if (!hw && !he) return -1;
  const int wc = west < 0 ? west + n_lon : west, ec = east >= n_lon ? east - n_lon : east;   // columns of the grid
  if (!he) return wc;
  if (!hw) return ec;
  const int dw = j - west, de = east - j;
  return dw < de ? wc : (de < dw ? ec : (wc < ec ? wc : ec));
}

// ---- the key ----------------------------------------------------------------------------------------------------------------
// THE RULE, point 4: 1 - (s_i s_k + (c_i c_k) cd[d]), every operation rounded on its own.  Contraction is switched off for this
// function (the pragma below), so no fma can form on the device or on the host; numpy has none either.  Negative results are 0.
AURORA_NE_HD double key_of(double si, double ci, double sk, double ck, double cd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double m1 = si * sk;
  const double m2 = ci * ck;
  const double m3 = m2 * cd;
  const double a = m1 + m3;
  const double key = 1.0 - a;
  return key < 0.0 ? 0.0 : key;
}

// ---- the stop test of the row walk --------------------------------------------------------------------------------------------
// A point walks the rows outward from its own.  Let key0 = key_of(.., cd = 1) of a row k, the ZERO-GAP key, and `bound` the
// smaller of the best key so far and key_max.  If key0 - kMargin > bound, no row at k or beyond it in that direction can win or
// tie.  Why:
//   (a) cd[d] <= 1 and c >= 0, and a rounded product, sum or difference is monotone in each operand, so in floating point
//       key_of(i, k', d) >= key_of(i, k', 0) for every gap d: every candidate of a row is at least its zero-gap key.  (This is
//       also why a single row may be skipped, without any margin, when its own key0 > bound.)
//   (b) key_of(i, k', 0) is within E = 3.5 x 2^-53 < 3.9e-16 of K = 1 - (s_i s_k' + c_i c_k') taken exactly on the table values:
//       two products of magnitude <= 1 (half an ulp each: 2^-54), the product by cd = 1 exact, a sum of magnitude <= 2 (2^-53),
//       a difference of magnitude <= 2 (2^-53); clamping at 0 moves no value by more than that.
//   (c) K is within N < 1.4e-15 of the true 1 - cos(lat_i - lat_k'): an entry of s or c is off by t <= 4.6e-16 (the degree to
//       radian product, relative 2^-52 of an angle <= pi / 2: 3.5e-16; a library sine or cosine to an ulp: 1.1e-16; clamping a
//       cosine at 0 only moves it towards the true value), and |s| + |c| <= sqrt 2 on either side: N <= 2 sqrt 2 t + t^2.
//   (d) the true 1 - cos(lat_i - lat_k') does not decrease as k' moves away from i: latitudes are strictly monotone and within
//       [-90, 90], so |lat_i - lat_k'| grows and stays within [0, 180] degrees.
//   So for k' at or beyond k: key_of(i, k', d) >= key_of(i, k, 0) - 2 (E + N) > key0 - 3.6e-15.  kMargin = 2^-46 = 1.42e-14 is
//   four times that; at a quarter of a degree two neighbouring rows differ by 1e-5 in key at one row's distance, so the margin
//   costs no extra row there.
constexpr double kMargin = 1.0 / 70368744177664.0;                 // 2^-46
AURORA_NE_HD bool stops(double key0, double bound) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return key0 - kMargin > bound;
}

// ---- one source row seen from one target point ------------------------------------------------------------------------------
struct Best {
  double key;                                    // +inf: none yet
  int32_t index;                                 // flat index i W + j of the event, -1: none yet
};

AURORA_NE_HD int gap_of(int j, int col, int n_lon, bool wrap) {
  const int d = j > col ? j - col : col - j;
  return wrap && n_lon - d < d ? n_lon - d : d;
}

// Target (i, j) takes the candidate `col` (>= 0) of source row k: THE RULE, points 4 to 6.  cd: the table of W cosines.
AURORA_NE_HD void visit(Best& best, int i, int j, int k, int col, double si, double ci, double sk, double ck, const double* cd,
                        int n_lon, bool wrap, double key_max) {
  const double key = (k == i && col == j) ? 0.0 : key_of(si, ci, sk, ck, cd[gap_of(j, col, n_lon, wrap)]);
  const int32_t index = (int32_t)(k * n_lon + col);
  if (key > key_max) return;
  if (key < best.key || (key == best.key && index < best.index)) best.key = key, best.index = index;
}

}  // namespace ne
}  // namespace aurora
