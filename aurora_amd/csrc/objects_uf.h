// The lock-free union-find of objects.hip, apart from the kernels so that a host program can run the very same loops
// (tools/probes/objects_uf_host.cpp does, single- and multi-threaded, against a flood fill).
//
// parent[] holds one int32 per point of a plane: -1 for background, else the flat index of another point of the same
// object.  THE INVARIANT: parent[x] <= x at all times -- it is set up with the start of x's run (<= x), and the only later
// writes are fetch_min with a smaller index (uf_unite) and the store of x's root (the flatten pass).  A root is a point with
// parent[x] == x; since a larger index always hangs under a smaller one, the root of a finished object is its first point.
//
// Mem: load(i) and fetch_min(i, v) on parent[i], atomic per element, relaxed.  A load may return an OLDER value of
// parent[i] than another thread has written by now: every value parent[i] ever had is a point of i's object that is <= i,
// so a stale value costs steps and never correctness -- the fetch_min itself acts on the current value and says what it was.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define AURORA_UF_HD __host__ __device__ __forceinline__
#else
#define AURORA_UF_HD inline
#endif

namespace aurora {

// The root of x as far as this thread can see it.
template <typename Mem> AURORA_UF_HD int32_t uf_find(const Mem& m, int32_t x) {
  // TERMINATION: every iteration either returns or moves to p < x, so there are at most x iterations whatever the other
  // threads do; nothing here waits for a value that another thread has yet to write.
  for (;;) {
    const int32_t p = m.load(x);
    if (p >= x || p < 0) return x;   // p == x: a root.  (p > x and p < 0 cannot happen for an event point; they end the walk)
    x = p;
  }
}

// Join the objects of a and b.
template <typename Mem> AURORA_UF_HD void uf_unite(const Mem& m, int32_t a, int32_t b) {
  // TERMINATION: every iteration either returns or replaces the larger of (a, b) by a strictly smaller index (old < a, then
  // uf_find only goes down), so a + b falls strictly and is bounded below by 0: at most a + b iterations, whatever the
  // other threads do.  No iteration waits for another thread.
  for (;;) {
    a = uf_find(m, a);
    b = uf_find(m, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = m.fetch_min(a, b);   // b < a, so parent[a] <= a stays true
    if (old == a) return;                    // a was a root, and hangs under b now
    a = old;                                 // a had been hung elsewhere meanwhile (old < a): join THAT point with b
  }
}

// The unions that the event point (row, j) of an n_lon-wide plane owes: every contact with the row above that its left
// neighbour does not already carry, and the seam.  Mem::event(i): is point i an event (parent[i] >= 0: that never changes once
// the runs are set up).  Every index is within the plane: row - 1 >= 0 where the row above is read, columns within 0 .. n_lon - 1.
template <typename Mem> AURORA_UF_HD void uf_unite_point(const Mem& m, int row, int j, int n_lon, bool eight, bool wrap) {
  const int32_t row0 = row * n_lon, up0 = row0 - n_lon, x = row0 + j;
  if (row > 0) {                                    // no neighbours beyond a pole
    const bool left = j > 0 && m.event(x - 1);
    if (m.event(up0 + j)) {
      // the point above; its row neighbours are in its run.  Carried already where the left neighbour and the point above
      // THAT are both events: those two are in contact, and each is in the run of its right neighbour.
      if (!(left && m.event(up0 + j - 1))) uf_unite(m, x, up0 + j);
    } else if (eight) {
      // the diagonals, wrapped in longitude; the one on the left is carried by an event left neighbour (which is right below
      // it), the one on the right by an event right neighbour.
      const int ja = j > 0 ? j - 1 : (wrap ? n_lon - 1 : -1);
      const int jc = j + 1 < n_lon ? j + 1 : (wrap ? 0 : -1);
      if (ja >= 0 && !left && m.event(up0 + ja)) uf_unite(m, x, up0 + ja);
      const bool right = j + 1 < n_lon && m.event(x + 1);
      if (jc >= 0 && !right && m.event(up0 + jc)) uf_unite(m, x, up0 + jc);
    }
  }
  if (wrap && j == n_lon - 1 && j > 0 && m.event(row0)) uf_unite(m, x, row0);   // the seam
}

}  // namespace aurora
