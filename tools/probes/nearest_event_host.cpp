// The search of aurora_amd/csrc/nearest_event_search.h on the host, against a brute force: the same west_of / east_of /
// candidate, key_of, stops and visit that nearest_event.hip runs, driven by loops that do serially what the kernels do by
// lanes (a mask per chunk, the last event before and the first after a chunk, the walk outward inside the extent with the stop
// test and the single-row skip).  Random and hand-drawn rows and planes, wrapping and regional, ascending and descending, with
// and without key_max.  Checks (1) every row candidate against a scan over all events of the row, (2) index and key of every
// point against the minimum over ALL row candidates without any stop or skip, bit for bit, and (3) the key against the minimum
// over ALL events of the plane, which the candidate rule must not miss.  No GPU.
//
//   c++ -std=c++17 -O1 -g tools/probes/nearest_event_host.cpp -o nearest_event_host && ./nearest_event_host
//   (and with -fsanitize=address,undefined)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../aurora_amd/csrc/nearest_event_search.h"

namespace {

using namespace aurora;
const double kPi = 3.14159265358979323846;

struct Grid {
  int H, W;
  bool wrap;
  std::vector<double> s, c, cd;
};

Grid grid_of(int H, int W, bool wrap, bool ascending, bool poles) {
  Grid g{H, W, wrap, {}, {}, {}};
  const double top = poles ? 90.0 : 80.0;
  for (int i = 0; i < H; ++i) {
    double lat = H == 1 ? 37.5 : top - 2 * top * i / (H - 1);
    if (ascending) lat = -lat;
    g.s.push_back(std::sin(lat * kPi / 180));
    g.c.push_back(std::fmax(std::cos(lat * kPi / 180), 0.0));
  }
  const double step = wrap ? 360.0 / W : 0.5;
  for (int d = 0; d < W; ++d) g.cd.push_back(d ? std::cos(d * step * kPi / 180) : 1.0);
  return g;
}

// What rows_kernel writes: the candidates of one row, and whether it has an event.
bool candidates_of(const uint8_t* ev, const Grid& g, int16_t* cand) {
  const int n_chunks = (g.W + 63) / 64;
  std::vector<uint64_t> mask(64, 0);
  for (int j = 0; j < g.W; ++j)
    if (ev[j]) mask[j / 64] |= 1ull << (j % 64);
  std::vector<int> west(64, -ne::kNone), east(64, ne::kNone);
  int seen = -ne::kNone, row_first = ne::kNone;
  for (int c = 0; c < 64; ++c) {                     // the exclusive prefix maximum of the lanes
    west[c] = seen;
    if (mask[c]) seen = ne::chunk_last(mask[c], c);
  }
  const int row_last = seen;
  seen = ne::kNone;
  for (int c = 63; c >= 0; --c) {                    // the exclusive suffix minimum
    east[c] = seen;
    if (mask[c]) seen = ne::chunk_first(mask[c], c);
  }
  row_first = seen;
  const bool any = row_first < ne::kNone;
  for (int c = 0; c < n_chunks; ++c) {
    int wb = west[c], ea = east[c];
    if (g.wrap && any) {
      if (wb == -ne::kNone) wb = row_last - g.W;
      if (ea == ne::kNone) ea = row_first + g.W;
    }
    for (int lane = 0; lane < 64; ++lane) {
      const int j = 64 * c + lane;
      if (j < g.W) cand[j] = (int16_t)ne::candidate(j, ne::west_of(mask[c], c, lane, wb), ne::east_of(mask[c], c, lane, ea), g.W);
    }
  }
  return any;
}

// What one lane of search_kernel does.
ne::Best search(const Grid& g, const int16_t* cand, const uint8_t* flag, int lo, int hi, int i, int j, double key_max, long* visits) {
  ne::Best best{std::numeric_limits<double>::infinity(), -1};
  const double si = g.s[i], ci = g.c[i];
  int ku = i < hi ? i : hi, kd = i + 1 > lo ? i + 1 : lo;
  bool up = ku >= lo, down = kd <= hi;
  while (up || down) {
    for (int dir = 0; dir < 2; ++dir) {
      bool& walking = dir ? down : up;
      int& k = dir ? kd : ku;
      if (!walking) continue;
      const double sk = g.s[k], ck = g.c[k];
      const double key0 = ne::key_of(si, ci, sk, ck, 1.0);
      const double bound = best.key < key_max ? best.key : key_max;
      if (ne::stops(key0, bound)) {
        walking = false;
        continue;
      }
      if (flag[k] && !(key0 > bound)) {
        ne::visit(best, i, j, k, cand[(size_t)k * g.W + j], si, ci, sk, ck, g.cd.data(), g.W, g.wrap, key_max);
        ++*visits;
      }
      k += dir ? 1 : -1;
      walking = dir ? k <= hi : k >= lo;
    }
  }
  return best;
}

long check(const char* name, const Grid& g, const std::vector<uint8_t>& ev, double key_max) {
  const int H = g.H, W = g.W;
  long bad = 0, visits = 0;
  std::vector<int16_t> cand((size_t)H * W);
  std::vector<uint8_t> flag(H);
  int lo = H, hi = -1;
  for (int k = 0; k < H; ++k) {
    flag[k] = candidates_of(&ev[(size_t)k * W], g, &cand[(size_t)k * W]);
    if (flag[k]) lo = lo < k ? lo : k, hi = k;
    for (int j = 0; j < W; ++j) {                    // (1) the candidate against a scan over the row
      int want = -1, want_gap = 1 << 30;
      for (int e = 0; e < W; ++e)
        if (ev[(size_t)k * W + e] && ne::gap_of(j, e, W, g.wrap) < want_gap) want = e, want_gap = ne::gap_of(j, e, W, g.wrap);
      bad += cand[(size_t)k * W + j] != want;
    }
  }
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < W; ++j) {
      const ne::Best got = search(g, cand.data(), flag.data(), lo, hi, i, j, key_max, &visits);
      ne::Best rows{std::numeric_limits<double>::infinity(), -1};   // (2) every row candidate, no stop, no skip
      double all = std::numeric_limits<double>::infinity();         // (3) every event
      for (int k = 0; k < H; ++k) {
        if (flag[k]) ne::visit(rows, i, j, k, cand[(size_t)k * W + j], g.s[i], g.c[i], g.s[k], g.c[k], g.cd.data(), W, g.wrap, key_max);
        for (int e = 0; e < W; ++e)
          if (ev[(size_t)k * W + e]) {
            const double key = (k == i && e == j) ? 0.0 : ne::key_of(g.s[i], g.c[i], g.s[k], g.c[k], g.cd[ne::gap_of(j, e, W, g.wrap)]);
            if (key <= key_max && key < all) all = key;
          }
      }
      bad += got.index != rows.index || std::memcmp(&got.key, &rows.key, 8) != 0 || got.key != all;
    }
  std::printf("%-28s %3d x %4d %s key_max %-8.3g visits per point %6.2f  %ld mismatches\n", name, H, W, g.wrap ? "wrap    " : "regional",
              key_max, (double)visits / ((double)H * W), bad);
  return bad;
}

}  // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  std::mt19937 rng(7);
  long bad = 0;
  const int widths[] = {1, 2, 63, 64, 65, 129, 257}, heights[] = {1, 2, 24};
  for (int H : heights)
    for (int W : widths)
      for (int form = 0; form < 4; ++form) {
        const Grid g = grid_of(H, W, form & 1, form & 2, !(form & 2));
        std::vector<uint8_t> ev((size_t)H * W);
        for (auto& e : ev) e = rng() % 100 < 4;
        bad += check("random, 4 % events", g, ev, inf);
        bad += check("random, 4 % events", g, ev, 0.02);
      }
  {                                                  // hand-drawn: nothing, everything, one corner, the pole rows, the seam
    const Grid g = grid_of(24, 130, true, false, true), r = grid_of(24, 130, false, true, true);
    std::vector<uint8_t> ev(24 * 130, 0);
    bad += check("empty", g, ev, inf);
    ev[0] = 1;
    bad += check("one event in a corner", g, ev, inf) + check("one event in a corner", r, ev, inf) + check("one event in a corner", g, ev, 0.003);
    ev[0] = 0, ev[23 * 130 + 129] = 1;
    bad += check("one event in the last corner", g, ev, inf) + check("one event in the last corner", r, ev, inf);
    ev[3] = ev[40] = ev[23 * 130 + 17] = 1;
    bad += check("events in the pole rows", g, ev, inf) + check("events in the pole rows", r, ev, inf);
    std::fill(ev.begin(), ev.end(), 1);
    bad += check("full", g, ev, inf);
    const Grid seam = grid_of(5, 12, true, false, false);
    std::vector<uint8_t> two(5 * 12, 0);
    two[2 * 12 + 2] = two[2 * 12 + 10] = 1;
    bad += check("two columns either side", seam, two, inf);
    two[0 * 12 + 6] = two[4 * 12 + 6] = 1;
    bad += check("north and south", seam, two, inf);
  }
  {                                                  // a band of events: many rows within the margin of each other's keys
    const Grid g = grid_of(40, 70, true, false, true);
    std::vector<uint8_t> ev(40 * 70, 0);
    for (int k = 10; k < 30; ++k)
      for (int j = 0; j < 70; ++j) ev[k * 70 + j] = (j + k) % 7 == 0;
    bad += check("a lattice", g, ev, inf) + check("a lattice", g, ev, 0.001);
  }
  std::printf("nearest_event_host: %ld mismatches\n", bad);
  return bad != 0;
}
