// Host check of aurora_amd/csrc/extrema_window.h, the window arithmetic of aurora_hip_extrema: every width 1..130, every half
// width 0..W / 2 (regional: ..W - 1), every column, on a full circle and on a regional grid.  The doubling tables of a row of
// composites (one entry in sixteen is the all-ones sentinel of an invalid point) are built by extrema_partner up to the level
// that extrema_level asks for, and the two entries that extrema_window names must EQUAL the minimum of a brute-force loop over
// the member columns; a window that is the whole row (extrema_whole_row) must be every column.  Every table index and level is
// checked before it is used.  Build with the address and undefined-behaviour sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aurora_amd/csrc \
//       tools/probes/extrema_window_host.cpp -o tools/probes/extrema_window_host && tools/probes/extrema_window_host
#include <cstdint>
#include <cstdio>
#include <vector>

#include "extrema_window.h"

int main() {
  using namespace aurora;
  const uint64_t kNone = ~(uint64_t)0;
  long checked = 0, whole = 0, failures = 0;
  for (int W = 1; W <= 130; ++W) {
    std::vector<uint64_t> x(W);
    uint32_t state = 54321u + (uint32_t)W;
    for (int j = 0; j < W; ++j) {
      state = state * 1664525u + 1013904223u;
      const bool ok = (state >> 28) != 0;                       // one point in sixteen is invalid
      x[j] = ok ? ((uint64_t)((state >> 8) & 0xff) << 32) | (uint32_t)j : kNone;   // few distinct keys: ties go to the column
    }
    for (int wrap = 0; wrap < 2; ++wrap) {
      // the tables, one level more than any window of this row can ask for
      std::vector<std::vector<uint64_t>> m(1, x);
      const int top = extrema_level(wrap ? W / 2 : W - 1);
      for (int l = 0; l < top; ++l) {
        std::vector<uint64_t> next(W);
        for (int c = 0; c < W; ++c) {
          const int p = extrema_partner(c, l, W, wrap != 0);
          if (p >= W) {
            std::printf("FAIL partner W %d wrap %d l %d c %d: %d\n", W, wrap, l, c, p);
            ++failures;
          }
          next[c] = p >= 0 && p < W && m[l][p] < m[l][c] ? m[l][p] : m[l][c];
        }
        m.push_back(next);
      }
      const int n_max = wrap ? W / 2 : W - 1;
      for (int n = 0; n <= n_max; ++n)
        for (int j = 0; j < W; ++j) {
          uint64_t want = kNone;
          int width = 0;
          if (wrap) {                                           // distinct columns within gap n on the circle
            for (int l = 0; l < W; ++l) {
              const int d = l > j ? l - j : j - l, gap = d < W - d ? d : W - d;
              if (gap <= n) want = x[l] < want ? x[l] : want, ++width;
            }
          } else {
            for (int l = j - n; l <= j + n; ++l)
              if (l >= 0 && l < W) want = x[l] < want ? x[l] : want, ++width;
          }
          ++checked;
          if (extrema_whole_row(n, W, wrap != 0)) {
            ++whole;
            if (width != W) {
              std::printf("FAIL whole row W %d wrap %d n %d j %d: %d members\n", W, wrap, n, j, width);
              ++failures;
            }
            continue;
          }
          const ExtremaWindow q = extrema_window(j, n, W, wrap != 0);
          const int l = q.level - q.back;
          if (q.level != extrema_level(n) || q.back < 0 || q.back > 1 || l < 0 || l >= (int)m.size() || q.a < 0 || q.a >= W ||
              q.b < 0 || q.b >= W) {
            std::printf("FAIL index W %d wrap %d n %d j %d: level %d back %d a %d b %d\n", W, wrap, n, j, q.level, q.back, q.a, q.b);
            ++failures;
            continue;
          }
          const uint64_t got = m[l][q.a] < m[l][q.b] ? m[l][q.a] : m[l][q.b];
          if (got != want) {
            std::printf("FAIL W %d wrap %d n %d j %d: %llx (loop %llx)\n", W, wrap, n, j, (unsigned long long)got,
                        (unsigned long long)want);
            ++failures;
          }
        }
    }
  }
  std::printf("extrema_window: %ld windows checked (W 1..130, n 0..W / 2 on a full circle, 0..W - 1 regional; %ld of them the "
              "whole row), %ld failures\n", checked, whole, failures);
  return failures ? 1 : 0;
}
