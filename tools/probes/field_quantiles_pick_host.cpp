// The between-pass logic of aurora_amd/csrc/field_quantiles_pick.h on the host, against a sort: the same count_index,
// area_target, pick_bin, distinct_prefixes and key_to_bits that field_quantiles.hip runs between its passes, driven by
// histograms made here the way its passes make them (per distinct prefix, of the next byte, by count or by unit).  Checks
// that every target ends on the key a full sort finds and that no slot or bin index leaves its table.  No GPU.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/probes/field_quantiles_pick_host.cpp -o fq_pick_host && ./fq_pick_host
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../aurora_amd/csrc/field_quantiles_pick.h"

namespace {

using namespace aurora::fq;

struct Point {
  uint32_t key;
  int64_t unit;
};

// The select as the kernels run it: targets, then four rounds of (histograms per distinct prefix, pick).
std::vector<uint32_t> select(const std::vector<Point>& pts, const std::vector<double>& q, bool area, int64_t* n_out, int64_t* W_out) {
  const int n_q = (int)q.size(), n_targets = area ? n_q : 2 * n_q;
  int64_t n = (int64_t)pts.size(), W = 0;
  for (const Point& p : pts) W += area ? p.unit : 1;
  *n_out = n, *W_out = W;
  int64_t rem[kMaxTargets] = {};
  uint32_t prefix[kMaxTargets] = {}, distinct[kMaxTargets] = {};
  int32_t slot[kMaxTargets];
  for (int t = 0; t < n_targets; ++t) {
    if (area) {
      rem[t] = W > 0 ? area_target(W, q[t]) : 0;
    } else if (n > 0) {
      int64_t j, hi;
      double g;
      count_index(n, q[t >> 1], &j, &hi, &g);
      rem[t] = ((t & 1) ? hi : j) + 1;
    }
  }
  int n_distinct = distinct_prefixes(prefix, rem, n_targets, distinct, slot);   // pass 0: every live target shares prefix 0
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    std::vector<int64_t> hist((size_t)n_distinct * kBins, 0);                     // exactly as many slots as the pass fills
    for (const Point& p : pts)
      for (int d = 0; d < n_distinct; ++d)
        if (pass == 0 || (p.key >> (shift + 8)) == distinct[d]) hist[(size_t)d * kBins + ((p.key >> shift) & 255u)] += area ? p.unit : 1;
    for (int t = 0; t < n_targets; ++t) {
      if (rem[t] == 0) continue;
      int64_t before;
      const int bin = pick_bin(hist.data() + (size_t)slot[t] * kBins, rem[t], &before);
      prefix[t] = (prefix[t] << 8) | (uint32_t)bin;
      rem[t] -= before;
    }
    n_distinct = distinct_prefixes(prefix, rem, n_targets, distinct, slot);
  }
  std::vector<uint32_t> keys(n_targets, 0);
  for (int t = 0; t < n_targets; ++t) keys[t] = rem[t] ? prefix[t] : 0xffffffffu;   // (0xffffffff: the key of a NaN, "dead")
  return keys;
}

int check(std::vector<Point> pts, const std::vector<double>& q, bool area, const char* what) {
  int64_t n, W;
  const std::vector<uint32_t> got = select(pts, q, area, &n, &W);
  std::stable_sort(pts.begin(), pts.end(), [](const Point& a, const Point& b) { return a.key < b.key; });
  int bad = 0;
  for (size_t t = 0; t < got.size(); ++t) {
    uint32_t want = 0xffffffffu;
    if (area && W > 0) {
      const int64_t target = area_target(W, q[t]);
      int64_t cum = 0;
      for (const Point& p : pts)
        if ((cum += p.unit) >= target) {
          want = p.key;
          break;
        }
    } else if (!area && n > 0) {
      int64_t j, hi;
      double g;
      count_index(n, q[t >> 1], &j, &hi, &g);
      if (j < 0 || hi >= n || g < 0.0 || g >= 1.0 + 1e-9) ++bad;
      want = pts[(t & 1) ? hi : j].key;
    }
    if (got[t] != want) {
      std::printf("MISMATCH %s area %d n %lld target %zu: key %08x, the sort says %08x\n", what, (int)area, (long long)n, t, got[t], want);
      ++bad;
    }
  }
  return bad;
}

uint32_t key_of(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace

int main() {
  int bad = 0, cases = 0;
  std::mt19937 g(11);
  const std::vector<std::vector<double>> qs = {{0.5}, {0.5, 0.9, 0.99}, {0.99, 0.0, 0.5, 0.5, 1.0, 0.25, 0.001, 0.75}, {0.0, 1.0}};
  for (int trial = 0; trial < 300; ++trial) {
    const int n = trial < 4 ? trial : 1 + (int)(g() % 3000);
    const int kind = trial % 6;              // what the keys look like
    std::vector<Point> pts(n);
    for (Point& p : pts) {
      float v = 0.f;
      switch (kind) {
        case 0: v = 5e4f + (float)((int)(g() % 100000) - 50000) * 0.01f; break;            // one top byte, as a real field
        case 1: v = (g() & 1) ? 1.f : -1.f; break;                                          // two keys
        case 2: v = 273.15f; break;                                                         // one key
        case 3: v = (float)((int)(g() % 81) - 40) * 1.4e-45f; break;                        // denormals and +-0
        case 4: { uint32_t u = g(); if ((u & 0x7f800000u) == 0x7f800000u) u &= ~0x00800000u; std::memcpy(&v, &u, 4); } break;   // any finite bits
        default: v = (float)(g() % 7); break;                                               // heavy ties
      }
      p.key = key_of(v);
      p.unit = (g() % 5 == 0) ? 0 : (int64_t)(g() % 6000000000ull);                         // rows of unit 0 among the others
      uint32_t back = key_to_bits(p.key), u;
      std::memcpy(&u, &v, 4);
      if (back != u) ++bad;
    }
    for (const auto& q : qs)
      for (int area = 0; area < 2; ++area, ++cases) bad += check(pts, q, area != 0, "random");
  }
  {  // every point on a row of unit 0: W = 0, every target dead
    std::vector<Point> pts(50, Point{key_of(1.f), 0});
    bad += check(pts, qs[1], true, "unit 0");
    ++cases;
  }
  std::printf("%d cases, %d mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
