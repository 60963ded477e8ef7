// Index arithmetic of aurora_hip_sphere_spectra (sphere_spectra.hip): the triangularly packed analysis table and the
// workspace; at the end, of aurora_hip_sphere_analysis and aurora_hip_sphere_synthesis (sphere_transform.hip).  Plain integer functions that compile for the host alone too: tools/probes/sphere_spectra_index_host.cpp checks
// every offset against a triple loop under the address and undefined-behaviour sanitizers.
//
// Table (doubles): A[m][l][i] for 0 <= m <= l <= lmax, 0 <= i < H; m outermost, then l from m upwards, then the latitude:
//   offset(m, l, i) = (rows_before(m) + (l - m)) H + i,     rows_before(m) = m (lmax + 1) - m (m - 1) / 2,
// (lmax + 1)(lmax + 2) / 2 rows of H doubles in all.
//
// Workspace (bytes, 16-byte aligned), three parts one after the other:
//   F        n_planes x n_in x (lmax + 1) x H pairs (re, im) of doubles, [plane][field][m][i]: n_in = 1, or 2 with a truth;
//   partial  n_planes x n_out x n_seg x (lmax + 1) doubles, [plane][field][segment of m][l]: n_out = 1, or 3 with a truth;
//            a segment is kSphereSegment consecutive m;
//   flags    n_planes x n_chunks x 2 int32, [plane][row chunk]{invalid, pole rows dropped}: a chunk is kSphereChunkRows rows.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AURORA_SPHERE_HD __host__ __device__
#else
#define AURORA_SPHERE_HD
#endif

namespace aurora {

constexpr int kSphereSegment = 16;             // consecutive m that one wavefront of the Legendre stage sums
constexpr int kSphereChunkRows = 32;           // grid rows per workgroup of the zonal stage
constexpr int64_t kSphereTableCap = (int64_t)1 << 30;   // bytes

AURORA_SPHERE_HD inline int64_t sphere_rows_before(int lmax, int m) {
  return (int64_t)m * (lmax + 1) - (int64_t)m * (m - 1) / 2;
}
AURORA_SPHERE_HD inline int64_t sphere_table_offset(int lmax, int H, int m, int l, int i) {
  return (sphere_rows_before(lmax, m) + (l - m)) * H + i;
}
AURORA_SPHERE_HD inline int64_t sphere_table_doubles(int lmax, int H) {
  return (int64_t)(lmax + 1) * (lmax + 2) / 2 * H;
}
// The largest lmax >= 0 whose table for H rows stays within the cap, or -1 where not even lmax = 0 does.
inline int sphere_largest_lmax(int H) {
  int lmax = -1;
  while (lmax < 4096 && sphere_table_doubles(lmax + 1, H) * 8 <= kSphereTableCap) ++lmax;
  return lmax;
}
// The largest degree the quadrature of H rows and N longitudes resolves exactly.
AURORA_SPHERE_HD inline int sphere_exact_lmax(int H, int N) {
  const int a = (H - 1) / 2, b = (N - 1) / 2;
  return a < b ? a : b;
}

AURORA_SPHERE_HD inline int sphere_segments(int lmax) { return (lmax + kSphereSegment) / kSphereSegment; }
AURORA_SPHERE_HD inline int sphere_chunks(int H) { return (H + kSphereChunkRows - 1) / kSphereChunkRows; }

// F, in pairs of doubles from the start of the workspace
AURORA_SPHERE_HD inline int64_t sphere_f_offset(int lmax, int H, int n_in, int plane, int field, int m, int i) {
  return (((int64_t)plane * n_in + field) * (lmax + 1) + m) * H + i;
}
AURORA_SPHERE_HD inline int64_t sphere_f_bytes(int lmax, int H, int n_in, int n_planes) {
  return 16 * sphere_f_offset(lmax, H, n_in, n_planes, 0, 0, 0);
}
// partial, in doubles from the start of its part
AURORA_SPHERE_HD inline int64_t sphere_partial_offset(int lmax, int n_out, int plane, int field, int seg, int l) {
  return (((int64_t)plane * n_out + field) * sphere_segments(lmax) + seg) * (lmax + 1) + l;
}
AURORA_SPHERE_HD inline int64_t sphere_partial_bytes(int lmax, int n_out, int n_planes) {
  return 8 * sphere_partial_offset(lmax, n_out, n_planes, 0, 0, 0);
}
// flags, in int32 from the start of their part
AURORA_SPHERE_HD inline int64_t sphere_flag_offset(int H, int plane, int chunk, int which) {
  return ((int64_t)plane * sphere_chunks(H) + chunk) * 2 + which;
}
AURORA_SPHERE_HD inline int64_t sphere_flag_bytes(int H, int n_planes) { return 4 * sphere_flag_offset(H, n_planes, 0, 0); }

AURORA_SPHERE_HD inline int64_t sphere_workspace_bytes(int lmax, int H, int has_truth, int n_planes) {
  const int64_t b = sphere_f_bytes(lmax, H, has_truth ? 2 : 1, n_planes) + sphere_partial_bytes(lmax, has_truth ? 3 : 1, n_planes) +
                    sphere_flag_bytes(H, n_planes);
  return (b + 15) / 16 * 16;
}

// ---- aurora_hip_sphere_analysis and aurora_hip_sphere_synthesis (sphere_transform.hip) ------------------------------------
// tools/probes/sphere_transform_index_host.cpp checks these the same way.
//
// Coefficients (pairs (re, im) of doubles), dense: n_planes x (lmax + 1) x (lmax + 1), [plane][m][l]; l < m holds zeros.
// Synthesis table (doubles): P[m][l][i], packed exactly like the analysis table -- sphere_table_offset is its offset too.
// Workspace of the analysis: F with n_in = 1, then the flags; of the synthesis: G, in the layout [plane][m][i] of F with
// n_in = 1 (sphere_f_offset).
AURORA_SPHERE_HD inline int64_t sphere_coeff_offset(int lmax, int plane, int m, int l) {
  return ((int64_t)plane * (lmax + 1) + m) * (lmax + 1) + l;
}
AURORA_SPHERE_HD inline int64_t sphere_coeff_bytes(int lmax, int n_planes) { return 16 * sphere_coeff_offset(lmax, n_planes, 0, 0); }
AURORA_SPHERE_HD inline int64_t sphere_analysis_workspace_bytes(int lmax, int H, int n_planes) {
  return (sphere_f_bytes(lmax, H, 1, n_planes) + sphere_flag_bytes(H, n_planes) + 15) / 16 * 16;
}
AURORA_SPHERE_HD inline int64_t sphere_synthesis_workspace_bytes(int lmax, int H, int n_planes) {
  return sphere_f_bytes(lmax, H, 1, n_planes);
}

}  // namespace aurora
