// Host check of aurora_amd/csrc/sphere_spectra_index.h, the index arithmetic of aurora_hip_sphere_spectra: for every lmax in
// 1..40 and H in 2..90, every (m, l, i) offset of the packed table must equal the running count of a plain triple loop (m
// outermost, l from m, then i) and end at sphere_table_doubles; every F, partial and flag offset of the workspace, with and
// without a truth, for 3 planes, must equal the count of its own loop, the three parts must follow each other without overlap
// inside sphere_workspace_bytes, and a table of exactly the stated size is filled through the offsets (the sanitizer sees any
// index outside it).  Build with the address and undefined-behaviour sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aurora_amd/csrc \
//       tools/probes/sphere_spectra_index_host.cpp -o tools/probes/sphere_spectra_index_host && tools/probes/sphere_spectra_index_host
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sphere_spectra_index.h"

int main() {
  using namespace aurora;
  long checked = 0, failures = 0;
  const int n_planes = 3;
  for (int lmax = 1; lmax <= 40; ++lmax)
    for (int H = 2; H <= 90; ++H) {
      std::vector<unsigned char> table((size_t)sphere_table_doubles(lmax, H), 0);
      int64_t next = 0;
      for (int m = 0; m <= lmax; ++m)
        for (int l = m; l <= lmax; ++l)
          for (int i = 0; i < H; ++i, ++next, ++checked) {
            const int64_t at = sphere_table_offset(lmax, H, m, l, i);
            if (at != next || at < 0 || at >= (int64_t)table.size()) {
              if (++failures < 10) std::printf("FAIL table lmax %d H %d (m %d, l %d, i %d): %lld, loop %lld\n", lmax, H, m, l, i,
                                               (long long)at, (long long)next);
            } else {
              ++table[(size_t)at];
            }
          }
      if (next != sphere_table_doubles(lmax, H)) ++failures, std::printf("FAIL table size lmax %d H %d\n", lmax, H);
      for (unsigned char c : table) failures += c != 1;
      for (int truth = 0; truth < 2; ++truth) {
        const int n_in = truth ? 2 : 1, n_out = truth ? 3 : 1;
        int64_t f = 0, p = 0, g = 0;
        for (int plane = 0; plane < n_planes; ++plane) {
          for (int field = 0; field < n_in; ++field)
            for (int m = 0; m <= lmax; ++m)
              for (int i = 0; i < H; ++i, ++f, ++checked) failures += sphere_f_offset(lmax, H, n_in, plane, field, m, i) != f;
          for (int field = 0; field < n_out; ++field)
            for (int seg = 0; seg < sphere_segments(lmax); ++seg)
              for (int l = 0; l <= lmax; ++l, ++p, ++checked) failures += sphere_partial_offset(lmax, n_out, plane, field, seg, l) != p;
          for (int chunk = 0; chunk < sphere_chunks(H); ++chunk)
            for (int which = 0; which < 2; ++which, ++g, ++checked) failures += sphere_flag_offset(H, plane, chunk, which) != g;
        }
        const int64_t fb = sphere_f_bytes(lmax, H, n_in, n_planes), pb = sphere_partial_bytes(lmax, n_out, n_planes),
                      gb = sphere_flag_bytes(H, n_planes), all = sphere_workspace_bytes(lmax, H, truth, n_planes);
        if (fb != 16 * f || pb != 8 * p || gb != 4 * g || all < fb + pb + gb || all % 16 || all - (fb + pb + gb) >= 16 ||
            fb != (int64_t)16 * (lmax + 1) * H * n_in * n_planes || sphere_segments(lmax) * kSphereSegment < lmax + 1 ||
            (sphere_segments(lmax) - 1) * kSphereSegment > lmax || sphere_chunks(H) * kSphereChunkRows < H) {
          ++failures;
          std::printf("FAIL workspace lmax %d H %d truth %d\n", lmax, H, truth);
        }
      }
    }
  const bool cap = sphere_largest_lmax(721) >= 360 && sphere_table_doubles(sphere_largest_lmax(1441), 1441) * 8 <= kSphereTableCap &&
                   sphere_table_doubles(sphere_largest_lmax(1441) + 1, 1441) * 8 > kSphereTableCap && sphere_exact_lmax(721, 1440) == 360 &&
                   sphere_exact_lmax(720, 1440) == 359 && sphere_exact_lmax(2, 4) == 0;
  if (!cap) ++failures, std::printf("FAIL cap / exact lmax\n");
  std::printf("sphere_spectra_index: %ld offsets checked (lmax 1..40, H 2..90; table, F, partials and flags, with and without a "
              "truth), largest lmax under the cap at 721 rows %d, %ld failures\n", checked, sphere_largest_lmax(721), failures);
  return failures ? 1 : 0;
}
