// Host check of aurora_amd/csrc/links_scan.h, the per-pair and per-tile logic of aurora_hip_link_extrema: every max_points pair
// Ma, Mb in 1..130, on a full circle and on a regional grid of 7 x 12 points whose first and last rows are the poles, with counts
// below, at and above max_points (and 0), keep masks on every other case, and now and then a flat index outside the grid.  Each
// direction is run the way the kernel runs it -- the other side staged by point_of into tiles that are exactly as long as the
// rows they hold (so the address sanitizer sees any read past a tile), at a tile length of 7 and at kTile, one scan_tile per live
// row and tile -- and every stored (key bits, row) must EQUAL that of a brute-force double loop that writes THE RULE of
// aurora_amd/links.py out on its own.  Build with the address and undefined-behaviour sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aurora_amd/csrc \
//       tools/probes/link_extrema_host.cpp -o tools/probes/link_extrema_host && tools/probes/link_extrema_host
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "links_scan.h"

namespace {

using namespace aurora;

constexpr int H = 7, W = 12;
const double kPi = 3.14159265358979323846;

struct Side {
  std::vector<int64_t> table;                     // 2 per row: flat index, (unused) key
  std::vector<uint8_t> keep;
  int count, m;
  bool masked;
};

uint32_t next(uint32_t& state) { return state = state * 1664525u + 1013904223u; }

Side make(int m, uint32_t& state, bool masked) {
  Side s;
  s.m = m, s.masked = masked;
  const uint32_t pick = next(state) >> 8;
  s.count = pick % 5 == 0 ? 0 : (pick % 5 == 1 ? m + 1 + (int)(pick % 7) : (int)(pick % (uint32_t)(m + 1)));
  s.table.resize(2 * (size_t)m), s.keep.resize(m);
  for (int r = 0; r < m; ++r) {
    const uint32_t v = next(state) >> 8;
    int64_t flat = (int64_t)(v % (H * W));
    if (v % 97 == 0) flat = -3 - (int64_t)(v % 11);           // outside the grid: clamped to the first point
    if (v % 89 == 0) flat = H * W + (int64_t)(v % 1000);       // ... to the last
    s.table[2 * r] = flat, s.table[2 * r + 1] = 0x5a5a;
    s.keep[r] = (next(state) >> 8) % 4 != 0;
  }
  return s;
}

bool live(const Side& s, int r) { return r < (s.count < 0 ? 0 : (s.count > s.m ? s.m : s.count)) && (!s.masked || s.keep[r]); }

int64_t bits(double key) {
  int64_t i;
  std::memcpy(&i, &key, 8);
  return i;
}

// THE RULE, written out: the brute force
void brute(const Side& mine, const Side& other, const std::vector<double>& s, const std::vector<double>& c,
           const std::vector<double>& cd, bool wrap, double key_max, std::vector<int64_t>& out) {
  out.assign(2 * (size_t)mine.m, 0);
  const auto clamp = [](int64_t f) { return (int)(f < 0 ? 0 : (f > H * W - 1 ? H * W - 1 : f)); };
  for (int r = 0; r < mine.m; ++r) {
    double best = INFINITY;
    int row = -1;
    if (live(mine, r)) {
      const int fa = clamp(mine.table[2 * r]);
      for (int q = 0; q < other.m; ++q) {
        if (!live(other, q)) continue;
        const int fb = clamp(other.table[2 * q]);
        double key = 0.0;
        if (fa != fb) {
          int gap = std::abs(fa % W - fb % W);
          if (wrap && W - gap < gap) gap = W - gap;
          volatile double m1 = s[fa / W] * s[fb / W];
          volatile double m2 = c[fa / W] * c[fb / W];
          volatile double m3 = m2 * cd[gap];
          volatile double sum = m1 + m3;
          volatile double k = 1.0 - sum;
          key = k < 0.0 ? 0.0 : k;
        }
        if (key <= key_max && key < best) best = key, row = q;
      }
    }
    out[2 * r] = row < 0 ? (int64_t)links::kInfBits : bits(best), out[2 * r + 1] = row;
  }
}

// one direction as the kernel runs it, with tiles of `tile` rows
void scan(const Side& mine, const Side& other, const std::vector<double>& s, const std::vector<double>& c,
          const std::vector<double>& cd, bool wrap, double key_max, int tile, std::vector<int64_t>& out) {
  out.assign(2 * (size_t)mine.m, 0);
  const int n_mine = links::rows_of(mine.count, mine.m), n_other = links::rows_of(other.count, other.m);
  std::vector<links::Best> best(mine.m);
  for (auto& b : best) b.key = INFINITY, b.row = -1;
  for (int q0 = 0; q0 < n_other; q0 += tile) {
    const int n = n_other - q0 < tile ? n_other - q0 : tile;
    std::vector<double> ts(n), tc(n);                           // exactly n entries: a read past the tile is a report
    std::vector<int32_t> tflat(n), tcol(n);
    for (int e = 0; e < n; ++e) {
      const int q = q0 + e;
      const links::Point t = links::point_of(other.table[2 * q], !other.masked || other.keep[q] != 0, s.data(), c.data(), H, W);
      ts[e] = t.s, tc[e] = t.c, tflat[e] = t.flat, tcol[e] = t.col;
    }
    for (int r = 0; r < n_mine; ++r) {
      const bool is = !mine.masked || mine.keep[r] != 0;
      if (!is) continue;
      const links::Point p = links::point_of(mine.table[2 * r], true, s.data(), c.data(), H, W);
      links::scan_tile(best[r], p, ts.data(), tc.data(), tflat.data(), tcol.data(), n, q0, cd.data(), W, wrap, key_max);
    }
  }
  for (int r = 0; r < mine.m; ++r) out[2 * r] = links::key_bits_of(best[r]), out[2 * r + 1] = best[r].row;
}

}  // namespace

int main() {
  long cases = 0, rows = 0, linked = 0, failures = 0;
  for (int wrap = 0; wrap < 2; ++wrap) {
    std::vector<double> s(H), c(H), cd(W);
    const double step = wrap ? 360.0 / W : 25.0;
    for (int i = 0; i < H; ++i) {
      const double lat = (90.0 - 30.0 * i) * kPi / 180.0;
      s[i] = std::sin(lat), c[i] = std::cos(lat) < 0.0 ? 0.0 : std::cos(lat);
    }
    for (int d = 0; d < W; ++d) cd[d] = d == 0 ? 1.0 : std::cos(d * step * kPi / 180.0);
    const double key_maxes[3] = {1.0 - std::cos(0.6), 1.0 - cd[1], INFINITY};      // (the second IS a key of the grid: <= keeps it)
    for (int ma = 1; ma <= 130; ++ma) {
      for (int mb = 1; mb <= 130; ++mb) {
        uint32_t state = 12345u + 131u * (uint32_t)ma + 17161u * (uint32_t)mb + (uint32_t)wrap;
        const bool masked = ((ma + mb) & 1) != 0;
        const Side a = make(ma, state, masked), b = make(mb, state, masked);
        const double key_max = key_maxes[(ma + 2 * mb) % 3];
        const int tile = (ma * 7 + mb) % 4 == 0 ? links::kTile : 7;
        std::vector<int64_t> want, got;
        for (int back = 0; back < 2; ++back) {
          const Side& mine = back ? b : a;
          const Side& other = back ? a : b;
          brute(mine, other, s, c, cd, wrap != 0, key_max, want);
          scan(mine, other, s, c, cd, wrap != 0, key_max, tile, got);
          for (int r = 0; r < mine.m; ++r) {
            ++rows;
            linked += want[2 * r + 1] >= 0;
            if (want[2 * r] != got[2 * r] || want[2 * r + 1] != got[2 * r + 1]) {
              if (++failures <= 10)
                std::printf("FAIL wrap %d Ma %d Mb %d back %d row %d: (%llx, %lld) against (%llx, %lld)\n", wrap, ma, mb, back, r,
                            (unsigned long long)got[2 * r], (long long)got[2 * r + 1], (unsigned long long)want[2 * r],
                            (long long)want[2 * r + 1]);
            }
          }
        }
        ++cases;
      }
    }
  }
  std::printf("link_extrema: %ld table pairs checked (Ma, Mb 1..130, a full circle and a regional grid of %d x %d with pole rows, "
              "counts 0, below and above max_points, keep masks on every other pair, tiles of 7 and of %d rows), %ld rows, %ld "
              "of them linked, %ld failures\n", cases, H, W, links::kTile, rows, linked, failures);
  return failures ? 1 : 0;
}
