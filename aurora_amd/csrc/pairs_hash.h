// The bounded, lock-free hash aggregation of object_matches.hip, apart from the kernels so that a host program can run the very
// same loops (tools/probes/object_pairs_host.cpp does, single- and multi-threaded, against a std::map).
//
// One TABLE per (plane, threshold) item: C = 2^log2c slots, C = max(64, pow2ceil(2 max_pairs)), as 3 C + 1 words of 64 bits:
//     word s             the KEY of slot s: 0 = empty, else (ka << 32) | kb  (never 0: ka >= 1)
//     word C + s         the POINTS of slot s: the number of points that carry the key
//     word 2 C + s       the UNITS of slot s: the sum of their area units
//     word 3 C           the OVERFLOW word: not 0 once a contribution found no slot
// all zero before the first insert.  THE HOME SLOT of a key is
//     home = (key * 0x9E3779B97F4A7C15) >> (64 - log2c)          (the product modulo 2^64)
// and a key lives in the first slot from home, walking upwards and wrapping from slot C - 1 to slot 0, that was empty when the
// key arrived (linear probing).  A key word changes once, from 0 to its key, and never again; nothing is ever removed.
//
// Mem: load(i), cas(i, expected, desired) -> the value found, and fetch_add(i, v) on word i, atomic per word, relaxed.  The two
// sums are only ever added to, and integer addition commutes, so the sums do not depend on the order of the adds and need no
// ordering with the compare-and-swap that claimed the slot: whoever reads them does so after every insert has finished (the
// next launch; a joined thread).  A load may return 0 for a slot that another thread has claimed by now: the compare-and-swap
// that follows acts on the current value and says what it was.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define AURORA_PH_HD __host__ __device__ __forceinline__
#else
#define AURORA_PH_HD inline
#endif

namespace aurora {

constexpr int kPairsMinLog2C = 6;                  // C >= 64
constexpr int kPairsMaxPairs = 8192;               // so C <= 16384

// log2 C for a table of up to max_pairs pairs: C = max(64, pow2ceil(2 max_pairs)).
AURORA_PH_HD int pairs_log2c(int max_pairs) {
  int l = kPairsMinLog2C;
  while (((int64_t)1 << l) < 2 * (int64_t)max_pairs) ++l;   // bounded: l <= 32
  return l;
}

AURORA_PH_HD int64_t pairs_table_words(int log2c) { return 3 * ((int64_t)1 << log2c) + 1; }

AURORA_PH_HD uint64_t pairs_key(int32_t ka, int32_t kb) { return ((uint64_t)(uint32_t)ka << 32) | (uint64_t)(uint32_t)kb; }

AURORA_PH_HD int64_t pairs_home(uint64_t key, int log2c) { return (int64_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - log2c)); }

// Has a contribution of this table been dropped?  (Then the item's result is "overflow" whatever else the table holds.)
template <typename Mem> AURORA_PH_HD bool pairs_overflowed(const Mem& m, int log2c) {
  return m.load(3 * ((int64_t)1 << log2c)) != 0;
}

// Add (points, units) to the sums of `key` (not 0).  False if the table had no slot for it: the overflow word is set and
// the contribution is dropped.
template <typename Mem> AURORA_PH_HD bool pairs_insert(const Mem& m, int log2c, uint64_t key, int64_t points, int64_t units) {
  const int64_t C = (int64_t)1 << log2c;
  int64_t s = pairs_home(key, log2c);
  // TERMINATION: at most C iterations whatever the other threads do -- every iteration either returns or moves to the next
  // slot, and the walk stops after C of them.  No iteration waits for a value that another thread has yet to write: a slot is
  // either seen to hold the key, claimed by ONE compare-and-swap whose returned value decides, or left behind for good (a key
  // word that is neither 0 nor the key never becomes either).
  for (int64_t n = 0; n < C; ++n) {
    uint64_t k = m.load(s);
    if (k == 0) {
      k = m.cas(s, 0, key);                        // the value found: 0 = this thread claimed the slot
      if (k == 0) k = key;
    }
    if (k == key) {
      m.fetch_add(C + s, (uint64_t)points);
      m.fetch_add(2 * C + s, (uint64_t)units);
      return true;
    }
    s = (s + 1) & (C - 1);
  }
  if (m.load(3 * C) == 0) m.cas(3 * C, 0, 1);      // C slots, every one another key's: the table is full
  return false;
}

// The slot that holds `key`, or -1.  Only after every insert has finished (the keys no longer change).
template <typename Mem> AURORA_PH_HD int64_t pairs_find(const Mem& m, int log2c, uint64_t key) {
  const int64_t C = (int64_t)1 << log2c;
  int64_t s = pairs_home(key, log2c);
  for (int64_t n = 0; n < C; ++n) {                // bounded by C
    const uint64_t k = m.load(s);
    if (k == key) return s;
    if (k == 0) return -1;                         // an insert of `key` would have claimed this slot
    s = (s + 1) & (C - 1);
  }
  return -1;
}

}  // namespace aurora
