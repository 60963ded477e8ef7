// Linking the extrema of two steps on the device (aurora_amd.link_extrema).  aurora_amd/links.py has THE RULE and
// include/aurora_hip.h the contract; the per-pair and per-tile logic is links_scan.h; this file has the one launch.
//
// A 256-thread workgroup owns (a chunk of 256 rows of one side, a plane, a direction): direction 0 searches the rows of b for
// every row of a (forward), direction 1 the rows of a for every row of b (backward).  A thread owns ONE row of its side and
// keeps its point (s, c, flat index, column) and the best (key, row) so far in registers.  The other side is staged through LDS
// in tiles of kTile rows, every entry gathered by its row first -- s[i], c[i], flat index, column, column -1 where the row is
// not live -- so the inner loop reads LDS alone: four broadcast reads of the tile entry (every thread is at the same entry) and
// one gathered read of cd, which sits in LDS for the whole launch.  The loop runs over the min(count, max_points) rows of the
// other side, not over max_points.  A workgroup whose chunk lies past the rows of its side stores "none" and exits at once.
// No atomics, no workspace, nothing reduced across threads: a row's result is two plain 8-byte stores by its own thread.
//
// Every flat index read from a table is clamped into the grid before it addresses s, c or cd (links_scan.h: point_of), and
// every count into 0 .. max_points.
#include "planes.h"
#include "links_scan.h"

namespace aurora {
namespace {

using links::kThreads;
using links::kTile;

struct LinkArgs {
  const int64_t* table_a;
  const int64_t* table_b;
  const int32_t* count_a;
  const int32_t* count_b;
  const uint8_t* keep_a;                                       // or null: every row is kept
  const uint8_t* keep_b;
  int64_t* forward;
  int64_t* backward;
  const double* s;
  const double* c;
  const double* cd;
  double key_max;
  int ma, mb, n_chunks, n_lat, n_lon, wrap;
};

__global__ __launch_bounds__(kThreads) void link_extrema_kernel(const LinkArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];        // cd (n_lon) | s (kTile) | c (kTile) | flat, col (kTile each)
  const int tid = (int)threadIdx.x;
  unsigned g = blockIdx.x;
  const int chunk = (int)(g % (unsigned)a.n_chunks);
  g /= (unsigned)a.n_chunks;
  const bool back = (g & 1u) != 0;                               // workgroup-uniform, like everything up to `r`
  const int64_t plane = (int64_t)(g >> 1);
  const int m_mine = back ? a.mb : a.ma, m_other = back ? a.ma : a.mb;
  const int r0 = chunk * kThreads;
  if (r0 >= m_mine) return;                                      // (the grid is sized by the larger side)

  const gptr<const int64_t> t_mine = (gptr<const int64_t>)(back ? a.table_b : a.table_a) + plane * 2 * m_mine;
  const gptr<const int64_t> t_other = (gptr<const int64_t>)(back ? a.table_a : a.table_b) + plane * 2 * m_other;
  const uint8_t* const keep_mine = back ? a.keep_b : a.keep_a;
  const uint8_t* const keep_other = back ? a.keep_a : a.keep_b;
  const gptr<const uint8_t> k_mine = (gptr<const uint8_t>)keep_mine + plane * m_mine;
  const gptr<const uint8_t> k_other = (gptr<const uint8_t>)keep_other + plane * m_other;
  const gptr<int64_t> out = (gptr<int64_t>)(back ? a.backward : a.forward) + plane * 2 * m_mine;
  const int n_mine = links::rows_of(((gptr<const int32_t>)(back ? a.count_b : a.count_a))[plane], m_mine);
  const int n_other = links::rows_of(((gptr<const int32_t>)(back ? a.count_a : a.count_b))[plane], m_other);
  const int r = r0 + tid;

  if (r0 >= n_mine || n_other == 0) {                            // nothing to search for, or nothing to find
    if (r < m_mine) out[2 * r] = (int64_t)links::kInfBits, out[2 * r + 1] = -1;
    return;
  }

  const int H = a.n_lat, W = a.n_lon;
  const bool wrap = a.wrap != 0;
  double* const cd = lds;
  double* const ts = cd + W;
  double* const tc = ts + kTile;
  int32_t* const tflat = (int32_t*)(tc + kTile);
  int32_t* const tcol = tflat + kTile;
  for (int d = tid; d < W; d += kThreads) cd[d] = ((gptr<const double>)a.cd)[d];

  const bool live = r < n_mine && (keep_mine == nullptr || k_mine[r] != 0);
  const links::Point p = links::point_of(r < n_mine ? t_mine[2 * r] : 0, live, a.s, a.c, H, W);
  links::Best best;
  best.key = __builtin_inf(), best.row = -1;

  for (int q0 = 0; q0 < n_other; q0 += kTile) {                  // workgroup-uniform trip count: the barriers see every thread
    const int n = min(kTile, n_other - q0);
    __syncthreads();                                             // the tile before this one is read; the first time: cd is whole
    for (int e = tid; e < n; e += kThreads) {
      const int q = q0 + e;
      const links::Point t = links::point_of(t_other[2 * q], keep_other == nullptr || k_other[q] != 0, a.s, a.c, H, W);
      ts[e] = t.s, tc[e] = t.c, tflat[e] = t.flat, tcol[e] = t.col;
    }
    __syncthreads();
    if (live) links::scan_tile(best, p, ts, tc, tflat, tcol, n, q0, cd, W, wrap, a.key_max);
  }
  if (r < m_mine) out[2 * r] = links::key_bits_of(best), out[2 * r + 1] = best.row;
}

size_t lds_bytes(int n_lon) { return (size_t)n_lon * 8 + (size_t)kTile * 24; }      // <= 56 KiB

bool apart(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return q == nullptr || a + np <= b || b + nq <= a;
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_link_extrema(const int64_t* table_a, const int32_t* count_a, const uint8_t* keep_a, int max_points_a,
                                       const int64_t* table_b, const int32_t* count_b, const uint8_t* keep_b, int max_points_b,
                                       int n_planes, const double* tables, int n_lat, int n_lon, int wrap, double key_max,
                                       int64_t* forward, int64_t* backward, void* stream) {
  AURORA_CHECK_ARG(n_planes >= 0 && n_lat >= 1 && n_lon >= 1, "link_extrema: bad sizes (planes %d, grid %d x %d)", n_planes, n_lat, n_lon);
  AURORA_CHECK_ARG(n_lon <= links::kMaxLon, "link_extrema: the grid has %d longitudes; 1 to %d are supported", n_lon, links::kMaxLon);
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= 0x7fffffffll, "link_extrema: a plane of %d x %d points is too large", n_lat, n_lon);
  AURORA_CHECK_ARG(max_points_a >= 1 && max_points_a <= links::kMaxPoints && max_points_b >= 1 && max_points_b <= links::kMaxPoints,
                   "link_extrema: max_points must be in 1..%d, got %d and %d", links::kMaxPoints, max_points_a, max_points_b);
  AURORA_CHECK_ARG(wrap == 0 || wrap == 1, "link_extrema: the flag wrap must be 0 or 1, got %d", wrap);
  AURORA_CHECK_ARG(key_max >= 0.0, "link_extrema: key_max must be a number >= 0 (+inf: no limit), got %g", key_max);
  if (n_planes == 0) return AURORA_OK;
  AURORA_CHECK_ARG(table_a && count_a && table_b && count_b && tables && forward && backward,
                   "link_extrema: null table, count, coordinate table or output pointer");
  AURORA_CHECK_ARG((((uintptr_t)table_a | (uintptr_t)table_b | (uintptr_t)tables | (uintptr_t)forward | (uintptr_t)backward) & 7) == 0 &&
                       (((uintptr_t)count_a | (uintptr_t)count_b) & 3) == 0,
                   "link_extrema: the tables and the outputs must be 8-byte aligned, the counts 4-byte aligned");
  const size_t n = (size_t)n_planes, ta = n * max_points_a * 16, tb = n * max_points_b * 16;
  const struct {
    const void* at;
    size_t bytes;
  } inputs[] = {{table_a, ta}, {table_b, tb}, {count_a, n * 4}, {count_b, n * 4}, {keep_a, n * max_points_a},
                {keep_b, n * max_points_b}, {tables, ((size_t)2 * n_lat + n_lon) * 8}};
  bool clear = apart(forward, ta, backward, tb);
  for (const auto& in : inputs) clear = clear && apart(forward, ta, in.at, in.bytes) && apart(backward, tb, in.at, in.bytes);
  AURORA_CHECK_ARG(clear, "link_extrema: forward and backward must not overlap each other or an input");
  const int m = max_points_a > max_points_b ? max_points_a : max_points_b;
  const int n_chunks = (m + kThreads - 1) / kThreads;
  AURORA_CHECK_ARG((int64_t)n_chunks * 2 * n_planes <= 0x7fffffffll, "link_extrema: too many planes for one launch (%d planes of %d rows)",
                   n_planes, m);

  LinkArgs a;
  a.table_a = table_a, a.table_b = table_b, a.count_a = count_a, a.count_b = count_b, a.keep_a = keep_a, a.keep_b = keep_b;
  a.forward = forward, a.backward = backward, a.s = tables, a.c = tables + n_lat, a.cd = tables + 2 * (size_t)n_lat;
  a.key_max = key_max, a.ma = max_points_a, a.mb = max_points_b, a.n_chunks = n_chunks, a.n_lat = n_lat, a.n_lon = n_lon, a.wrap = wrap;
  hipLaunchKernelGGL(link_extrema_kernel, dim3((unsigned)((int64_t)n_chunks * 2 * n_planes)), dim3(kThreads), lds_bytes(n_lon),
                     as_stream(stream), a);
  return check_launch("link_extrema");
}
