// Host check of the part of aurora_amd/csrc/sphere_spectra_index.h that aurora_hip_sphere_analysis and
// aurora_hip_sphere_synthesis add: for every lmax in 1..40 and 3 planes, every dense coefficient offset (plane, m, l) must equal
// the running count of a plain triple loop and end at sphere_coeff_bytes / 16, and a buffer of exactly that size is filled
// through the offsets (the sanitizer sees any index outside it); for every H in 2..90 besides, the synthesis table -- packed
// like the analysis table -- is walked the way the inverse Legendre stage walks it (the column of latitude i of m, then
// (l - m) H further per degree) against the count of the loop m, l, i; the workspace of the analysis must hold F and the flags
// one after the other without overlap, that of the synthesis G alone, in the [plane][m][i] order of F.  Build with the address
// and undefined-behaviour sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I aurora_amd/csrc \
//       tools/probes/sphere_transform_index_host.cpp -o tools/probes/sphere_transform_index_host && tools/probes/sphere_transform_index_host
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sphere_spectra_index.h"

int main() {
  using namespace aurora;
  long checked = 0, failures = 0;
  const int n_planes = 3;
  for (int lmax = 1; lmax <= 40; ++lmax) {
    std::vector<unsigned char> coeff((size_t)(sphere_coeff_bytes(lmax, n_planes) / 16), 0);
    int64_t next = 0;
    for (int plane = 0; plane < n_planes; ++plane)
      for (int m = 0; m <= lmax; ++m)
        for (int l = 0; l <= lmax; ++l, ++next, ++checked) {
          const int64_t at = sphere_coeff_offset(lmax, plane, m, l);
          if (at != next || at < 0 || at >= (int64_t)coeff.size()) {
            if (++failures < 10) std::printf("FAIL coeff lmax %d (plane %d, m %d, l %d): %lld, loop %lld\n", lmax, plane, m, l,
                                             (long long)at, (long long)next);
          } else {
            ++coeff[(size_t)at];
          }
        }
    if (next * 16 != sphere_coeff_bytes(lmax, n_planes) || next != (int64_t)n_planes * (lmax + 1) * (lmax + 1))
      ++failures, std::printf("FAIL coeff size lmax %d\n", lmax);
    for (unsigned char c : coeff) failures += c != 1;

    for (int H = 2; H <= 90; ++H) {
      std::vector<unsigned char> table((size_t)sphere_table_doubles(lmax, H), 0);
      int64_t t = 0;
      for (int m = 0; m <= lmax; ++m)
        for (int l = m; l <= lmax; ++l)
          for (int i = 0; i < H; ++i, ++t, ++checked) {
            const int64_t at = sphere_table_offset(lmax, H, m, m, i) + (int64_t)(l - m) * H;   // the inverse Legendre stage's walk
            if (at != t || at < 0 || at >= (int64_t)table.size()) {
              if (++failures < 10) std::printf("FAIL table lmax %d H %d (m %d, l %d, i %d): %lld, loop %lld\n", lmax, H, m, l, i,
                                               (long long)at, (long long)t);
            } else {
              ++table[(size_t)at];
            }
          }
      for (unsigned char c : table) failures += c != 1;
      int64_t g = 0;
      for (int plane = 0; plane < n_planes; ++plane)
        for (int m = 0; m <= lmax; ++m)
          for (int i = 0; i < H; ++i, ++g, ++checked) failures += sphere_f_offset(lmax, H, 1, plane, 0, m, i) != g;
      const int64_t fb = sphere_f_bytes(lmax, H, 1, n_planes), gb = sphere_flag_bytes(H, n_planes),
                    wa = sphere_analysis_workspace_bytes(lmax, H, n_planes), ws = sphere_synthesis_workspace_bytes(lmax, H, n_planes);
      if (fb != 16 * g || ws != fb || wa < fb + gb || wa % 16 || wa - (fb + gb) >= 16 || ws % 16 ||
          gb != (int64_t)8 * n_planes * sphere_chunks(H)) {
        ++failures;
        std::printf("FAIL workspace lmax %d H %d\n", lmax, H);
      }
    }
  }
  const bool sizes = sphere_coeff_bytes(360, 1) == (int64_t)16 * 361 * 361 && sphere_synthesis_workspace_bytes(360, 721, 69) == (int64_t)69 * 16 * 361 * 721;
  if (!sizes) ++failures, std::printf("FAIL production sizes\n");
  std::printf("sphere_transform_index: %ld offsets checked (lmax 1..40, H 2..90, 3 planes; coefficients, the synthesis table's walk, G "
              "and the two workspaces), coefficients of one plane at lmax 360 %lld bytes, %ld failures\n", checked,
              (long long)sphere_coeff_bytes(360, 1), failures);
  return failures ? 1 : 0;
}
