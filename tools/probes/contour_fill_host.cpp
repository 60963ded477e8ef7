// Host check of aurora_amd/csrc/contour_fill.h, the word arithmetic of aurora_hip_closed_contours: every window width 1..130 (one,
// two and three words, every position of the last bit), linear and cyclic (the seam), connectivity 4 and 8, three densities of
// passable members.  The fill -- contour_reach swept over the member rows in place until nothing changes, as the kernel does
// -- must EQUAL a per-bit breadth-first fill; the exits -- the reached bits under contour_dilate of the non-member bitmap --
// must equal a per-bit count; contour_run_fill must equal a per-bit walk along the run; and the sweeps must stay within
// |members| + 1.  Every word index is checked before it is used.  Build with the address and undefined-behaviour sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aurora_amd/csrc \
//       tools/probes/contour_fill_host.cpp -o tools/probes/contour_fill_host && tools/probes/contour_fill_host
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "contour_fill.h"

namespace {

struct Rng {
  uint32_t s;
  uint32_t next() { return s = s * 1664525u + 1013904223u; }
  bool chance(int per_256) { return (int)((next() >> 24) & 255u) < per_256; }
};

struct Bitmap {
  int rows, words;
  std::vector<uint64_t> w;
  Bitmap(int r, int n) : rows(r), words(n), w((size_t)r * n, 0) {}
  bool get(int r, int l) const { return (w[(size_t)r * words + (l >> 6)] >> (l & 63)) & 1; }
  void set(int r, int l) { w[(size_t)r * words + (l >> 6)] |= 1ull << (l & 63); }
};

}  // namespace

int main() {
  using namespace aurora;
  long windows = 0, run_checks = 0, failures = 0, most_sweeps = 0;
  const int kRows = 7;                                           // five member rows and the two ring rows
  for (int width = 1; width <= 130; ++width)
    for (int cyclic = 0; cyclic < 2; ++cyclic)
      for (int eight = 0; eight < 2; ++eight)
        for (int density = 0; density < 3; ++density) {
          ContourWindow q;
          q.rows = kRows, q.width = width, q.words = (width + 63) >> 6, q.first = 0, q.cyclic = cyclic;
          Rng g{12345u + 977u * (uint32_t)width + 31u * (uint32_t)cyclic + 7u * (uint32_t)eight + (uint32_t)density};
          Bitmap A(kRows, q.words), X(kRows, q.words), R(kRows, q.words);
          const int per_256 = density == 0 ? 110 : (density == 1 ? 170 : 235);
          long members = 0;
          for (int r = 0; r < kRows; ++r)
            for (int l = 0; l < width; ++l) {
              const bool ring = r == 0 || r == kRows - 1 || (!cyclic && (l == 0 || l == width - 1));
              if (ring) {
                if (g.chance(128)) X.set(r, l);
              } else if (g.chance(per_256)) {
                A.set(r, l), ++members;
              } else if (g.chance(64)) {
                X.set(r, l);                                     // a passable non-member inside the rows (outside the disc)
              }
            }
          const int seed_row = 1 + (int)(g.next() % (kRows - 2)), seed_col = (int)(g.next() % (uint32_t)width);
          if (!A.get(seed_row, seed_col)) A.set(seed_row, seed_col), ++members;
          if (X.get(seed_row, seed_col)) X.w[(size_t)seed_row * q.words + (seed_col >> 6)] &= ~(1ull << (seed_col & 63));
          R.set(seed_row, seed_col);

          // the kernel's sweeps, serially
          long bad_index = 0;
          const auto reached = [&](int r, int w) -> uint64_t {
            if (r < 0 || r >= kRows || w < 0 || w >= q.words) return ++bad_index, 0;
            return R.w[(size_t)r * q.words + w];
          };
          const auto outside = [&](int r, int w) -> uint64_t {
            if (r < 0 || r >= kRows || w < 0 || w >= q.words) return ++bad_index, 0;
            return X.w[(size_t)r * q.words + w];
          };
          long sweeps = 0;
          for (bool changed = true; changed;) {
            changed = false, ++sweeps;
            for (int r = 1; r < kRows - 1; ++r)
              for (int w = 0; w < q.words; ++w) {
                const size_t at = (size_t)r * q.words + w;
                const uint64_t now = contour_reach(reached, A.w[at], r, w, q, eight != 0);
                if ((now & R.w[at]) != R.w[at] || (now & ~A.w[at])) {
                  std::printf("FAIL reach width %d cyclic %d eight %d: loses a bit or leaves A\n", width, cyclic, eight);
                  ++failures;
                }
                if (now != R.w[at]) R.w[at] = now, changed = true;
              }
          }
          most_sweeps = sweeps > most_sweeps ? sweeps : most_sweeps;
          if (sweeps > members + 1) {
            std::printf("FAIL sweeps width %d cyclic %d eight %d: %ld sweeps for %ld members\n", width, cyclic, eight, sweeps, members);
            ++failures;
          }

          // per bit: a breadth-first fill, and the exits
          const auto column = [&](int l, int* out) {              // the column next to l - 1 / l + 1, false for none
            if (l >= 0 && l < width) return *out = l, true;
            if (!cyclic) return false;
            return *out = l < 0 ? l + width : l - width, true;
          };
          std::vector<char> F((size_t)kRows * width, 0);
          std::vector<std::pair<int, int>> queue{{seed_row, seed_col}};
          F[(size_t)seed_row * width + seed_col] = 1;
          long want_points = 1, want_exits = 0;
          for (size_t head = 0; head < queue.size(); ++head)
            for (int dr = -1; dr <= 1; ++dr)
              for (int dl = -1; dl <= 1; ++dl) {
                if ((dr == 0 && dl == 0) || (!eight && dr != 0 && dl != 0)) continue;
                const int r = queue[head].first + dr;
                int l;
                if (r < 0 || r >= kRows || !column(queue[head].second + dl, &l)) continue;
                if (A.get(r, l) && !F[(size_t)r * width + l]) F[(size_t)r * width + l] = 1, queue.push_back({r, l}), ++want_points;
              }
          for (const auto& p : queue) {
            bool open = false;
            for (int dr = -1; dr <= 1; ++dr)
              for (int dl = -1; dl <= 1; ++dl) {
                if ((dr == 0 && dl == 0) || (!eight && dr != 0 && dl != 0)) continue;
                const int r = p.first + dr;
                int l;
                if (r < 0 || r >= kRows || !column(p.second + dl, &l)) continue;
                open = open || X.get(r, l);
              }
            want_exits += open;
          }
          long points = 0, exits = 0;
          bool same = true;
          for (int r = 0; r < kRows; ++r) {
            for (int l = 0; l < width; ++l) same = same && R.get(r, l) == (F[(size_t)r * width + l] != 0);
            for (int w = 0; w < q.words; ++w) {
              const uint64_t f = R.w[(size_t)r * q.words + w];
              points += __builtin_popcountll(f);
              if (f && r >= 1 && r < kRows - 1) exits += __builtin_popcountll(f & contour_dilate(outside, r, w, q, eight != 0));
              if (w == q.words - 1 && (width & 63) && (f >> (width & 63))) same = false;                // a bit past the width
            }
          }
          ++windows;
          if (!same || points != want_points || exits != want_exits || bad_index) {
            std::printf("FAIL width %d cyclic %d eight %d density %d: points %ld (per bit %ld), exits %ld (per bit %ld), %ld bad "
                        "indices\n", width, cyclic, eight, density, points, want_points, exits, want_exits, bad_index);
            ++failures;
          }

          // the horizontal shortcut, word by word: every run of A that holds a seed bit, whole
          for (int trial = 0; trial < 8; ++trial) {
            const uint64_t a = ((uint64_t)g.next() << 32 | g.next()) | ((uint64_t)g.next() << 32 | g.next());
            const uint64_t s = a & ((uint64_t)g.next() << 32 | g.next()) & ((uint64_t)g.next() << 32 | g.next());
            uint64_t want = 0;
            for (int b = 0; b < 64; ++b)
              if ((s >> b) & 1) {
                for (int u = b; u < 64 && ((a >> u) & 1); ++u) want |= 1ull << u;
                for (int d = b; d >= 0 && ((a >> d) & 1); --d) want |= 1ull << d;
              }
            ++run_checks;
            if (contour_run_fill(s, a) != want) {
              std::printf("FAIL run_fill a %llx s %llx: %llx (per bit %llx)\n", (unsigned long long)a, (unsigned long long)s,
                          (unsigned long long)contour_run_fill(s, a), (unsigned long long)want);
              ++failures;
            }
          }
        }
  // the two windows the LDS budget is stated for
  if (contour_lds_bytes(71, 23) != 40296 || contour_lds_bytes(107, 57) != 149112 || contour_lds_bytes(107, 57) > kContourLdsBudget ||
      contour_lds_bytes(120, 64) <= kContourLdsBudget) {
    std::printf("FAIL the LDS arithmetic\n");
    ++failures;
  }
  std::printf("contour_fill: %ld windows filled (widths 1..130, linear and cyclic, connectivity 4 and 8, three densities; at most "
              "%ld sweeps), %ld run fills, %ld failures\n", windows, most_sweeps, run_checks, failures);
  return failures ? 1 : 0;
}
