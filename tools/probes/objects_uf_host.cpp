// The union-find loops of aurora_amd/csrc/objects_uf.h on the host, against a flood fill: the same uf_find, uf_unite and
// uf_unite_point that objects.hip runs, over std::atomic parents, with the points dealt to several threads in shuffled order
// (so that unions race as workgroups do) and then flattened concurrently.  Checks that every loop ends and that every point's
// root is the smallest flat index of its flood-filled object.  No GPU.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/probes/objects_uf_host.cpp -o objects_uf_host && ./objects_uf_host
//   (or -fsanitize=thread)
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "../../aurora_amd/csrc/objects_uf.h"

namespace {

struct HostParents {
  std::atomic<int32_t>* p;
  bool event(int32_t i) const { return p[i].load(std::memory_order_relaxed) >= 0; }
  int32_t load(int32_t i) const { return p[i].load(std::memory_order_relaxed); }
  void store(int32_t i, int32_t v) const { p[i].store(v, std::memory_order_relaxed); }
  int32_t fetch_min(int32_t i, int32_t v) const {
    int32_t old = p[i].load(std::memory_order_relaxed);
    while (old > v && !p[i].compare_exchange_weak(old, v, std::memory_order_relaxed)) {
    }
    return old;
  }
};

// The object of every event by flood fill, as its smallest flat index.
std::vector<int32_t> flood(const std::vector<char>& ev, int H, int W, bool eight, bool wrap) {
  std::vector<int32_t> first(ev.size(), -1), stack;
  for (int32_t s = 0; s < (int32_t)ev.size(); ++s) {
    if (!ev[s] || first[s] >= 0) continue;
    first[s] = s, stack.assign(1, s);
    while (!stack.empty()) {
      const int32_t x = stack.back();
      stack.pop_back();
      const int i = x / W, j = x % W;
      for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj) {
          if ((!di && !dj) || (!eight && di && dj)) continue;
          int a = i + di, b = j + dj;
          if (a < 0 || a >= H) continue;
          if (b < 0 || b >= W) {
            if (!wrap) continue;
            b = (b + W) % W;
          }
          const int32_t y = a * W + b;
          if (ev[y] && first[y] < 0) first[y] = s, stack.push_back(y);
        }
    }
  }
  return first;
}

int check(const std::vector<char>& ev, int H, int W, bool eight, bool wrap, unsigned seed, int n_threads) {
  const int32_t N = H * W;
  std::vector<std::atomic<int32_t>> parent(N);
  std::vector<int32_t> points;
  for (int i = 0; i < H; ++i)
    for (int j = 0, start = 0; j < W; ++j) {      // the runs, as rows_kernel leaves them
      if (!ev[i * W + j]) {
        parent[i * W + j] = -1;
        continue;
      }
      if (j == 0 || !ev[i * W + j - 1]) start = j;
      parent[i * W + j] = i * W + start;
      points.push_back(i * W + j);
    }
  std::mt19937 g(seed);
  std::shuffle(points.begin(), points.end(), g);
  const HostParents mem{parent.data()};
  auto deal = [&](auto&& body) {
    std::vector<std::thread> ts;
    for (int t = 0; t < n_threads; ++t)
      ts.emplace_back([&, t] {
        for (size_t k = t; k < points.size(); k += n_threads) body(points[k]);
      });
    for (auto& t : ts) t.join();
  };
  deal([&](int32_t x) { aurora::uf_unite_point(mem, x / W, x % W, W, eight, wrap); });
  deal([&](int32_t x) {
    const int32_t r = aurora::uf_find(mem, x);
    if (r != mem.load(x)) mem.store(x, r);
  });
  const std::vector<int32_t> want = flood(ev, H, W, eight, wrap);
  for (int32_t x = 0; x < N; ++x)
    if (parent[x].load() != want[x]) {
      std::printf("MISMATCH %d x %d eight %d wrap %d seed %u: point %d has root %d, flood fill says %d\n", H, W, eight, wrap,
                  seed, x, parent[x].load(), want[x]);
      return 1;
    }
  return 0;
}

}  // namespace

int main() {
  int bad = 0, cases = 0;
  std::mt19937 g(7);
  for (int trial = 0; trial < 400; ++trial) {
    const int H = 1 + g() % 40, W = 1 + g() % 70;
    const double density = (1 + g() % 9) / 10.0;
    std::vector<char> ev(H * W);
    for (auto& e : ev) e = (g() % 1000) < density * 1000;
    for (int eight = 0; eight < 2; ++eight)
      for (int wrap = 0; wrap < 2; ++wrap, ++cases) bad += check(ev, H, W, eight, wrap, trial, 1 + trial % 8);
  }
  {  // a one-point-wide serpentine (long parent chains), a comb and a checkerboard
    const int H = 33, W = 70;
    std::vector<char> snake(H * W, 0), comb(H * W, 0), board(H * W, 0);
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j) {
        snake[i * W + j] = i % 2 == 0 || j == (i % 4 == 1 ? W - 1 : 0);
        comb[i * W + j] = i == H - 1 || j % 2 == 0;
        board[i * W + j] = (i + j) % 2;
      }
    for (const auto* ev : {&snake, &comb, &board})
      for (int eight = 0; eight < 2; ++eight)
        for (int wrap = 0; wrap < 2; ++wrap)
          for (unsigned seed = 0; seed < 8; ++seed, ++cases) bad += check(*ev, H, W, eight, wrap, seed, 8);
  }
  std::printf("%d cases, %d mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
