// The hash aggregation of aurora_amd/csrc/pairs_hash.h on the host, against a std::map: the same pairs_insert, pairs_find and
// pairs_home that object_matches.hip runs, over std::atomic words, single-threaded and with the contributions dealt to several
// threads in shuffled order (so that claims of one slot race as wavefronts do).  Checks that every loop ends, that every key
// that found a slot holds exactly the sums of the map, and the three edges: a table exactly full, a table one key too small
// (the overflow word set, every stored sum still right) and a probe chain that wraps past slot C - 1.  No GPU.
//
//   c++ -std=c++17 -O1 -g -pthread tools/probes/object_pairs_host.cpp -o object_pairs_host && ./object_pairs_host
//   (and with -fsanitize=address,undefined, and with -fsanitize=thread)
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../../aurora_amd/csrc/pairs_hash.h"

namespace {

struct HostTable {
  std::atomic<uint64_t>* w;
  uint64_t load(int64_t i) const { return w[i].load(std::memory_order_relaxed); }
  uint64_t cas(int64_t i, uint64_t expected, uint64_t desired) const {
    w[i].compare_exchange_strong(expected, desired, std::memory_order_relaxed);
    return expected;                               // the value found
  }
  void fetch_add(int64_t i, uint64_t v) const { w[i].fetch_add(v, std::memory_order_relaxed); }
};

struct Contribution {
  uint64_t key;
  int64_t points, units;
};

typedef std::map<uint64_t, std::pair<int64_t, int64_t>> Sums;

// Inserts `todo` into a fresh table of 2^log2c slots with n_threads threads and compares with the map.
//   expect_overflow < 0: whatever happens must be consistent;  0: every key must be stored;  1: the overflow word must be set.
// With one thread every key that holds a slot must have the sums of ALL its contributions (none is dropped once a key is in);
// with racing threads too: a key that is in the table is found by every later walk, and a walk that fails has passed C slots
// of other keys, which an earlier or later walk for the same key would pass as well -- once the table is full of other keys.
int check(const char* what, const std::vector<Contribution>& todo, int log2c, int n_threads, unsigned seed, int expect_overflow) {
  const int64_t C = (int64_t)1 << log2c;
  std::vector<std::atomic<uint64_t>> words(aurora::pairs_table_words(log2c));
  for (auto& x : words) x.store(0);
  const HostTable mem{words.data()};
  std::vector<Contribution> order(todo);
  if (n_threads > 1) {
    std::mt19937 g(seed);
    std::shuffle(order.begin(), order.end(), g);
  }
  std::vector<std::atomic<int64_t>> dropped(1);
  dropped[0] = 0;
  std::vector<std::thread> ts;
  for (int t = 0; t < n_threads; ++t)
    ts.emplace_back([&, t] {
      for (size_t k = t; k < order.size(); k += n_threads)
        if (!aurora::pairs_insert(mem, log2c, order[k].key, order[k].points, order[k].units)) dropped[0].fetch_add(1);
    });
  for (auto& t : ts) t.join();
  Sums want;
  for (const auto& c : todo) want[c.key].first += c.points, want[c.key].second += c.units;
  const bool overflow = aurora::pairs_overflowed(mem, log2c);
  int bad = 0;
  int64_t stored = 0;
  for (int64_t s = 0; s < C; ++s) {
    const uint64_t key = mem.load(s);
    if (!key) {
      if (mem.load(C + s) || mem.load(2 * C + s)) ++bad, std::printf("%s: an empty slot %lld has sums\n", what, (long long)s);
      continue;
    }
    ++stored;
    const auto it = want.find(key);
    if (it == want.end()) {
      ++bad, std::printf("%s: slot %lld holds the key %llx, which nobody inserted\n", what, (long long)s, (unsigned long long)key);
      continue;
    }
    if (aurora::pairs_find(mem, log2c, key) != s)
      ++bad, std::printf("%s: the key %llx is stored twice or cannot be found\n", what, (unsigned long long)key);
    if ((int64_t)mem.load(C + s) != it->second.first || (int64_t)mem.load(2 * C + s) != it->second.second)
      ++bad, std::printf("%s: the key %llx has sums %lld / %lld, the map says %lld / %lld\n", what, (unsigned long long)key,
                         (long long)mem.load(C + s), (long long)mem.load(2 * C + s), (long long)it->second.first,
                         (long long)it->second.second);
  }
  const int64_t distinct = (int64_t)want.size();
  if (stored != std::min(distinct, C)) ++bad, std::printf("%s: %lld keys stored, %lld expected\n", what, (long long)stored, (long long)std::min(distinct, C));
  if (overflow != (distinct > C)) ++bad, std::printf("%s: overflow word %d with %lld keys for %lld slots\n", what, overflow, (long long)distinct, (long long)C);
  if (overflow != (dropped[0].load() > 0)) ++bad, std::printf("%s: overflow word %d but %lld contributions dropped\n", what, overflow, (long long)dropped[0].load());
  if (expect_overflow >= 0 && overflow != (expect_overflow == 1)) ++bad, std::printf("%s: overflow word %d, expected %d\n", what, overflow, expect_overflow);
  if (!overflow)
    for (const auto& kv : want)
      if (aurora::pairs_find(mem, log2c, kv.first) < 0) ++bad, std::printf("%s: the key %llx is missing\n", what, (unsigned long long)kv.first);
  if (aurora::pairs_find(mem, log2c, aurora::pairs_key(0x7fffffff, 0x7fffffff)) >= 0) ++bad, std::printf("%s: found a key that was never inserted\n", what);
  return bad;
}

// n distinct keys, each `repeat` times with varying sums, drawn from labels up to (ma, mb).
std::vector<Contribution> random_keys(std::mt19937& g, int n, int repeat, int ma, int mb) {
  std::map<uint64_t, int> seen;
  std::vector<Contribution> out;
  while ((int)seen.size() < n) {                   // bounded: n <= ma * mb / 2 in every call below
    const uint64_t key = aurora::pairs_key(1 + (int32_t)(g() % ma), 1 + (int32_t)(g() % mb));
    if (seen.emplace(key, 1).second)
      for (int r = 0; r < repeat; ++r) out.push_back({key, 1 + (int64_t)(g() % 64), (int64_t)(g() % 1000000007) << 8});
  }
  return out;
}

// n distinct keys whose home slot in a table of 2^log2c slots is one of the last `window` slots: their chain wraps past C - 1.
std::vector<Contribution> wrapping_keys(int n, int log2c, int window) {
  const int64_t C = (int64_t)1 << log2c;
  std::vector<Contribution> out;
  for (int32_t ka = 1; (int)out.size() < n && ka < 4096; ++ka)
    for (int32_t kb = 1; (int)out.size() < n && kb < 4096; ++kb)
      if (aurora::pairs_home(aurora::pairs_key(ka, kb), log2c) >= C - window) out.push_back({aurora::pairs_key(ka, kb), 1, 4294967296ll});
  return out;
}

}  // namespace

int main() {
  int bad = 0, cases = 0;
  std::mt19937 g(11);
  if (aurora::pairs_log2c(1) != 6 || aurora::pairs_log2c(32) != 6 || aurora::pairs_log2c(33) != 7 || aurora::pairs_log2c(4096) != 13 ||
      aurora::pairs_log2c(8192) != 14 || aurora::pairs_table_words(6) != 193)
    ++bad, std::printf("pairs_log2c / pairs_table_words are off\n");
  for (int trial = 0; trial < 200; ++trial, ++cases) {   // random loads, below and above the table's size
    const int log2c = 6 + trial % 4, C = 1 << log2c;
    const int n = 1 + (int)(g() % (C + C / 4));
    bad += check("random", random_keys(g, n, 1 + trial % 5, 300, 300), log2c, 1 + trial % 8, trial, -1);
  }
  for (int threads : {1, 2, 8})
    for (unsigned seed = 0; seed < 4; ++seed) {
      const int log2c = 7, C = 1 << log2c;
      bad += check("one key, many adders", random_keys(g, 1, 4000, 50, 50), log2c, threads, seed, 0), ++cases;
      bad += check("exactly full", random_keys(g, C, 3, 300, 300), log2c, threads, seed, 0), ++cases;
      bad += check("one key too small", random_keys(g, C + 1, 3, 300, 300), log2c, threads, seed, 1), ++cases;
      const std::vector<Contribution> chain = wrapping_keys(40, log2c, 2);
      if ((int)chain.size() != 40) ++bad, std::printf("found %zu keys at home in the last two slots\n", chain.size());
      bad += check("a chain that wraps", chain, log2c, threads, seed, 0), ++cases;
      std::vector<Contribution> both = wrapping_keys(C, log2c, 1);   // every key at home in slot C - 1: the whole table is one chain
      bad += check("one chain, exactly full", both, log2c, threads, seed, 0), ++cases;
      both.push_back({aurora::pairs_key(4097, 1), 1, 1});
      bad += check("one chain, one key too many", both, log2c, threads, seed, 1), ++cases;
    }
  std::printf("%d cases, %d mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
