// Host check of aurora_amd/csrc/smooth_window.h, the window arithmetic of aurora_hip_smooth: every width 1..130, every half
// width -1..W / 2 (regional: ..W - 1), every column, on a full circle and on a regional grid, against a brute-force loop over
// the columns.  The values are small integers, so fp64 prefix sums and their differences are exact and must EQUAL the loop.
// Every table index is checked against [0, W] before it is used.  Build with the address and undefined-behaviour sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aurora_amd/csrc \
//       tools/probes/smooth_window_host.cpp -o tools/probes/smooth_window_host && tools/probes/smooth_window_host
#include <cstdint>
#include <cstdio>
#include <vector>

#include "smooth_window.h"

int main() {
  using namespace aurora;
  long checked = 0, failures = 0;
  for (int W = 1; W <= 130; ++W) {
    std::vector<double> x(W), P(W + 1);
    std::vector<int32_t> ok(W), N(W + 1);
    uint32_t state = 12345u + (uint32_t)W;
    for (int j = 0; j < W; ++j) {
      state = state * 1664525u + 1013904223u;
      ok[j] = (state >> 28) != 0;                               // one point in sixteen is invalid
      x[j] = ok[j] ? (double)((int)((state >> 8) & 0xffff) - 32768) : 0.0;
    }
    P[0] = 0.0, N[0] = 0;
    for (int j = 0; j < W; ++j) P[j + 1] = P[j] + x[j], N[j + 1] = N[j] + ok[j];
    for (int wrap = 0; wrap < 2; ++wrap) {
      const int n_max = wrap ? W / 2 : W - 1;
      for (int n = -1; n <= n_max; ++n)
        for (int j = 0; j < W; ++j) {
          double sum = 0.0;
          int32_t count = 0;
          int width = 0;
          if (n >= 0) {
            if (wrap) {                                         // distinct columns within gap n on the circle
              for (int l = 0; l < W; ++l) {
                const int d = l > j ? l - j : j - l, gap = d < W - d ? d : W - d;
                if (gap <= n) sum += x[l], count += ok[l], ++width;
              }
            } else {
              for (int l = j - n; l <= j + n; ++l) {
                ++width;                                        // a column off the grid counts, as invalid
                if (l >= 0 && l < W) sum += x[l], count += ok[l];
              }
            }
          }
          double S = 0.0;
          int32_t C = 0;
          int F = 0;
          if (n >= 0) {                                         // (n = -1: the kernel skips the row)
            const SmoothWindow s = smooth_window(j, n, W, wrap != 0);
            if (s.e0 < 0 || s.e0 > W || s.e1 < 0 || s.e1 > W || s.e2 < 0 || s.e2 > W || s.e0 > s.e1) {
              std::printf("FAIL index W %d wrap %d n %d j %d: e0 %d e1 %d e2 %d\n", W, wrap, n, j, s.e0, s.e1, s.e2);
              ++failures;
              continue;
            }
            S = (P[s.e1] - P[s.e0]) + P[s.e2];
            C = (N[s.e1] - N[s.e0]) + N[s.e2];
            F = smooth_full_width(n, W, wrap != 0);
          }
          ++checked;
          if (S != sum || C != count || F != width) {
            std::printf("FAIL W %d wrap %d n %d j %d: sum %.0f (loop %.0f) count %d (%d) width %d (%d)\n", W, wrap, n, j, S, sum, C,
                        count, F, width);
            ++failures;
          }
        }
    }
  }
  std::printf("smooth_window: %ld windows checked (W 1..130, n -1..W / 2 on a full circle, -1..W - 1 regional), %ld failures\n",
              checked, failures);
  return failures ? 1 : 0;
}
