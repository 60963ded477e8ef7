// Derived fields on the device (aurora_amd.diagnostics): relative vorticity, divergence and wind speed of a wind, and the
// vertical integrals of moisture (total column water vapour, integrated vapour transport).  include/aurora_hip.h has the
// arithmetic; this file has the two launches.
//
// Wind group.  The unit of work is one WAVEFRONT: a strip of 256 columns (a lane = four consecutive columns: load4 / store4
// of planes.h) times 16 rows, which the wave walks from north to south with a rolling three-row window of u and v in
// registers: a row is loaded once by the wave and serves as row i + 1, then i, then i - 1.  The two halo rows of a chunk are
// the neighbouring wave's (the four waves of a workgroup own consecutive chunks, so they come out of the L1 / L2 and not out
// of HBM a second time).  East and west neighbours inside a lane's four columns are registers; the two across its edges are
// two more 4-byte loads of the row the wave has just fetched (overlapping loads: cache hits).  Nothing is shared between
// lanes, so there is no LDS and no barrier, and nothing is reduced, so there is no tree to fix: a point's result depends on
// its own stencil alone.  An item whose vo and div entries are both NULL takes a plain elementwise loop and reads no
// neighbour rows.
//
// Column group.  A lane owns four consecutive points of the plane and walks the levels in level order, four levels in
// flight, with the three sums of each point in fp64 registers.
#include "planes.h"

namespace aurora {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kPerLane = 4;
constexpr int kStripCols = kWave * kPerLane;                  // columns of a wave
constexpr int kWaveRows = 16;                                  // rows a wave walks
constexpr int kBlockRows = kWaveRows * (kThreads / kWave);     // rows of a workgroup
constexpr int kChunk = kThreads * kPerLane;                    // points of a workgroup (column group)
constexpr int kGroup = 4;                                      // levels in flight
constexpr int kMaxLevels = 64;

struct WindArgs {
  const float* const* u;
  const float* const* v;
  float* const* vo;
  float* const* div;
  float* const* ws;
  const double* rows;     // n_lat x (A, m0, m1, m2)
  double L;
  int n_lat, n_lon, n_strips, n_row_blocks, wrap;
};
struct ColumnArgs {
  const float* const* q;
  const float* const* u;
  const float* const* v;
  float* const* tcwv;
  float* const* ivtu;
  float* const* ivtv;
  float* const* ivt;
  const double* level_w;
  int64_t n_points;
  int n_levels, n_chunks;
};

// Rounded to fp32 once; a result that is not finite (as fp32) is stored as NaN.
__device__ __forceinline__ float result(double x) {
  const float r = (float)x;
  return __builtin_isfinite(r) ? r : __builtin_nanf("");
}
__device__ __forceinline__ float wind_speed(float u, float v) { return result(wind_speed_f64(u, v)); }

__global__ __launch_bounds__(kThreads) void diagnostics_wind_kernel(const WindArgs a) {
  unsigned b = blockIdx.x;
  const int strip = (int)(b % (unsigned)a.n_strips);
  b /= (unsigned)a.n_strips;
  const int row_block = (int)(b % (unsigned)a.n_row_blocks), item = (int)(b / (unsigned)a.n_row_blocks);
  const int wave = (int)threadIdx.x / kWave, lane = (int)threadIdx.x % kWave;
  const int n = a.n_lon, last_col = n - 1, last_row = a.n_lat - 1;
  const int r0 = row_block * kBlockRows + wave * kWaveRows;
  const int j0 = strip * kStripCols + lane * kPerLane;
  if (r0 > last_row || j0 > last_col) return;
  const int r1 = r0 + kWaveRows < a.n_lat ? r0 + kWaveRows : a.n_lat;
  const int cnt = n - j0 < kPerLane ? n - j0 : kPerLane;

  // (wave-uniform: the item's pointers)
  const float* const U = a.u[item];
  const float* const V = a.v[item];
  float* const VO = a.vo ? a.vo[item] : nullptr;
  float* const DIV = a.div ? a.div[item] : nullptr;
  float* const WS = a.ws ? a.ws[item] : nullptr;
  const bool rows16 = (n & 3) == 0;                            // every row of an aligned plane starts on 16 bytes
  const bool vec_in = rows16 && ((((uintptr_t)U | (uintptr_t)V) & 15) == 0);
  const bool vec_vo = rows16 && ((uintptr_t)VO & 15) == 0, vec_div = rows16 && ((uintptr_t)DIV & 15) == 0;
  const bool vec_ws = rows16 && ((uintptr_t)WS & 15) == 0;
  const int64_t N = n;
  const int64_t row_last = last_col;                           // clamp inside a row: relative to the row's first element

  if (!VO && !DIV) {                                           // wind speed alone: no neighbour rows
    if (!WS) return;
#pragma unroll 4
    for (int i = r0; i < r1; ++i) {
      float u[kPerLane], v[kPerLane], s[kPerLane];
      load4(U + i * N, j0, row_last, vec_in, u);
      load4(V + i * N, j0, row_last, vec_in, v);
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) s[k] = wind_speed(u[k], v[k]);
      store4(WS + i * N, j0, cnt, vec_ws, s);
    }
    return;
  }

  // the columns across the lane's edges: the west neighbour of its first column and the east neighbour of its last one
  // (wrapped; without wrap the first and last column of the row do not use them)
  const int wj = j0 == 0 ? last_col : j0 - 1;
  const int ej = j0 + cnt - 1 == last_col ? 0 : j0 + kPerLane;   // (not the row's end: cnt == 4 and j0 + 4 <= last_col)
  const bool wrap = a.wrap != 0;
  const double L = a.L, L2 = 2.0 * a.L;

  float up[kPerLane], uc[kPerLane], un[kPerLane], vp[kPerLane], vc[kPerLane], vn[kPerLane];
  {
    const int im = r0 > 0 ? r0 - 1 : 0;                         // a row that does not exist: the clamped index
    load4(U + im * N, j0, row_last, vec_in, up);
    load4(V + im * N, j0, row_last, vec_in, vp);
    load4(U + r0 * N, j0, row_last, vec_in, uc);
    load4(V + r0 * N, j0, row_last, vec_in, vc);
  }
  for (int i = r0; i < r1; ++i) {
    const int ip = i < last_row ? i + 1 : last_row;
    load4(U + ip * N, j0, row_last, vec_in, un);
    load4(V + ip * N, j0, row_last, vec_in, vn);
    const gptr<const float> ug = (gptr<const float>)(U + i * N), vg = (gptr<const float>)(V + i * N);
    const float uw = ug[wj], ue = ug[ej], vw = vg[wj], ve = vg[ej];
    const double A = a.rows[4 * i], m0 = a.rows[4 * i + 1], m1 = a.rows[4 * i + 2], m2 = a.rows[4 * i + 3];

    float o_vo[kPerLane], o_div[kPerLane], o_ws[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const int j = j0 + k;
      const bool first = j == 0, last = j == last_col;
      // f[j - 1] and f[j + 1]: wrapped, or at the ends of a regional row the column itself (one-sided, factor 2 L)
      const float u_w = first ? (wrap ? uw : uc[k]) : (k == 0 ? uw : uc[k > 0 ? k - 1 : 0]);
      const float v_w = first ? (wrap ? vw : vc[k]) : (k == 0 ? vw : vc[k > 0 ? k - 1 : 0]);
      const float u_e = last ? (wrap ? ue : uc[k]) : (k == kPerLane - 1 ? ue : uc[k < kPerLane - 1 ? k + 1 : k]);
      const float v_e = last ? (wrap ? ve : vc[k]) : (k == kPerLane - 1 ? ve : vc[k < kPerLane - 1 ? k + 1 : k]);
      const double Lk = !wrap && (first || last) ? L2 : L;
      const double dv = ((double)v_e - (double)v_w) * Lk, du = ((double)u_e - (double)u_w) * Lk;
      const double mu = m0 * (double)up[k] + m1 * (double)uc[k] + m2 * (double)un[k];
      const double mv = m0 * (double)vp[k] + m1 * (double)vc[k] + m2 * (double)vn[k];
      o_vo[k] = result(A * (dv - mu));
      o_div[k] = result(A * (du + mv));
      o_ws[k] = wind_speed(uc[k], vc[k]);
    }
    if (VO) store4(VO + i * N, j0, cnt, vec_vo, o_vo);
    if (DIV) store4(DIV + i * N, j0, cnt, vec_div, o_div);
    if (WS) store4(WS + i * N, j0, cnt, vec_ws, o_ws);
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) up[k] = uc[k], uc[k] = un[k], vp[k] = vc[k], vc[k] = vn[k];
  }
}

__global__ __launch_bounds__(kThreads) void diagnostics_column_kernel(const ColumnArgs a) {
  const int item = (int)(blockIdx.x / (unsigned)a.n_chunks), chunk = (int)(blockIdx.x % (unsigned)a.n_chunks);
  const int64_t i0 = (int64_t)chunk * kChunk + (int64_t)threadIdx.x * kPerLane;
  if (i0 >= a.n_points) return;
  const int64_t left = a.n_points - i0, last = a.n_points - 1;
  const int cnt = left < kPerLane ? (int)left : kPerLane;
  const int C = a.n_levels;

  // (wave-uniform: the item's pointers)
  float* const TCWV = a.tcwv ? a.tcwv[item] : nullptr;
  float* const IVTU = a.ivtu ? a.ivtu[item] : nullptr;
  float* const IVTV = a.ivtv ? a.ivtv[item] : nullptr;
  float* const IVT = a.ivt ? a.ivt[item] : nullptr;
  const bool need_u = a.u != nullptr && (IVTU || IVT), need_v = a.v != nullptr && (IVTV || IVT);
  const float* const* const Q = a.q + (int64_t)item * C;
  const float* const* const U = need_u ? a.u + (int64_t)item * C : nullptr;
  const float* const* const V = need_v ? a.v + (int64_t)item * C : nullptr;
  const bool points16 = (a.n_points & 3) == 0;
  uintptr_t bits = 0;
  for (int c = 0; c < C; ++c) {
    bits |= (uintptr_t)Q[c];
    if (need_u) bits |= (uintptr_t)U[c];
    if (need_v) bits |= (uintptr_t)V[c];
  }
  const bool vec_in = points16 && (bits & 15) == 0;

  double st[kPerLane] = {}, su[kPerLane] = {}, sv[kPerLane] = {};
  for (int c0 = 0; c0 < C; c0 += kGroup) {
    float q[kGroup][kPerLane], u[kGroup][kPerLane], v[kGroup][kPerLane];
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) q[g][k] = u[g][k] = v[g][k] = 0.f;
      if (c0 + g < C) {
        load4(Q[c0 + g], i0, last, vec_in, q[g]);
        if (need_u) load4(U[c0 + g], i0, last, vec_in, u[g]);
        if (need_v) load4(V[c0 + g], i0, last, vec_in, v[g]);
      }
    }
#pragma unroll
    for (int g = 0; g < kGroup; ++g)
      if (c0 + g < C) {                                        // in level order
        const double w = a.level_w[c0 + g];
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
          const double wq = w * (double)q[g][k];
          st[k] += wq;
          su[k] += wq * (double)u[g][k];
          sv[k] += wq * (double)v[g][k];
        }
      }
  }

  float o[kPerLane];
  if (TCWV) {
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) o[k] = result(st[k]);
    store4(TCWV, i0, cnt, points16 && ((uintptr_t)TCWV & 15) == 0, o);
  }
  if (IVTU) {
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) o[k] = result(su[k]);
    store4(IVTU, i0, cnt, points16 && ((uintptr_t)IVTU & 15) == 0, o);
  }
  if (IVTV) {
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) o[k] = result(sv[k]);
    store4(IVTV, i0, cnt, points16 && ((uintptr_t)IVTV & 15) == 0, o);
  }
  if (IVT) {
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) o[k] = result(__builtin_sqrt(su[k] * su[k] + sv[k] * sv[k]));
    store4(IVT, i0, cnt, points16 && ((uintptr_t)IVT & 15) == 0, o);
  }
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_diagnostics(const float* const* wind_u, const float* const* wind_v, float* const* vo_planes,
                                      float* const* div_planes, float* const* ws_planes, int n_wind, const double* row_table,
                                      double L, int wrap, const float* const* q_planes, const float* const* col_u,
                                      const float* const* col_v, float* const* tcwv_planes, float* const* ivtu_planes,
                                      float* const* ivtv_planes, float* const* ivt_planes, int n_cols, int n_levels,
                                      const double* level_w, int n_lat, int n_lon, void* stream) {
  AURORA_CHECK_ARG(n_wind >= 0 && n_cols >= 0, "diagnostics: negative item counts (wind %d, columns %d)", n_wind, n_cols);
  AURORA_CHECK_ARG(n_lat >= 2 && n_lon >= 2, "diagnostics: the grid must have at least 2 latitudes and 2 longitudes, got %d x %d",
                   n_lat, n_lon);
  AURORA_CHECK_ARG((int64_t)n_lat * n_lon <= 0x7fffffff, "diagnostics: a plane of %d x %d points is too large", n_lat, n_lon);
  const int64_t n_strips = (n_lon + kStripCols - 1) / kStripCols, n_row_blocks = (n_lat + kBlockRows - 1) / kBlockRows;
  const int64_t n_chunks = ((int64_t)n_lat * n_lon + kChunk - 1) / kChunk;
  if (n_wind > 0) {
    AURORA_CHECK_ARG(wind_u && wind_v, "diagnostics: %d wind items but a null u or v plane table", n_wind);
    AURORA_CHECK_ARG(vo_planes || div_planes || ws_planes, "diagnostics: %d wind items but no output table", n_wind);
    AURORA_CHECK_ARG(!(vo_planes || div_planes) || (row_table && ((uintptr_t)row_table & 7) == 0 && L == L),
                     "diagnostics: vorticity and divergence need an 8-byte aligned row table and a longitude factor");
    AURORA_CHECK_ARG(n_strips * n_row_blocks * n_wind <= 0x7fffffff, "diagnostics: too many wind items for one launch (%d)",
                     n_wind);
  }
  if (n_cols > 0) {
    AURORA_CHECK_ARG(n_levels >= 2 && n_levels <= kMaxLevels, "diagnostics: a vertical integral takes 2..%d levels, got %d",
                     kMaxLevels, n_levels);
    AURORA_CHECK_ARG(q_planes && level_w && ((uintptr_t)level_w & 7) == 0,
                     "diagnostics: %d columns but a null q plane table or null / misaligned level weights", n_cols);
    AURORA_CHECK_ARG(tcwv_planes || ivtu_planes || ivtv_planes || ivt_planes, "diagnostics: %d columns but no output table",
                     n_cols);
    AURORA_CHECK_ARG(col_u || !(ivtu_planes || ivt_planes), "diagnostics: ivtu and ivt need the u plane table of the columns");
    AURORA_CHECK_ARG(col_v || !(ivtv_planes || ivt_planes), "diagnostics: ivtv and ivt need the v plane table of the columns");
    AURORA_CHECK_ARG(n_chunks * n_cols <= 0x7fffffff, "diagnostics: too many columns for one launch (%d)", n_cols);
  }
  const hipStream_t q = as_stream(stream);
  if (n_wind > 0) {
    WindArgs a;
    a.u = wind_u, a.v = wind_v, a.vo = vo_planes, a.div = div_planes, a.ws = ws_planes, a.rows = row_table, a.L = L;
    a.n_lat = n_lat, a.n_lon = n_lon, a.n_strips = (int)n_strips, a.n_row_blocks = (int)n_row_blocks, a.wrap = wrap;
    hipLaunchKernelGGL(diagnostics_wind_kernel, dim3((unsigned)(n_strips * n_row_blocks * n_wind)), dim3(kThreads), 0, q, a);
    const int code = check_launch("diagnostics (wind)");
    if (code != AURORA_OK) return code;
  }
  if (n_cols > 0) {
    ColumnArgs a;
    a.q = q_planes, a.u = col_u, a.v = col_v, a.tcwv = tcwv_planes, a.ivtu = ivtu_planes, a.ivtv = ivtv_planes;
    a.ivt = ivt_planes, a.level_w = level_w, a.n_points = (int64_t)n_lat * n_lon, a.n_levels = n_levels;
    a.n_chunks = (int)n_chunks;
    hipLaunchKernelGGL(diagnostics_column_kernel, dim3((unsigned)(n_chunks * n_cols)), dim3(kThreads), 0, q, a);
    return check_launch("diagnostics (columns)");
  }
  return AURORA_OK;
}
