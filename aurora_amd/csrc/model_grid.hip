// The model handle of libaurora_hip.so: what depends on the grid, the pressure levels or the time -- Fourier expansions,
// position / scale tables of the patch grid, window token tables and a band's halo plans, aurora_hip_precompute and
// aurora_hip_set_time.  Host code only; every launch goes through the operator ABI of this same library.
#include "model.h"

namespace aurora {

namespace {
constexpr double PI = 3.14159265358979323846;

// ---- host-side tables ----------------------------------------------------------------------------
double polygon_area_km2(const double (*poly)[2], int n_in) {   // aurora/area.py:12-48, incl. its way of closing the ring
  std::vector<std::array<double, 2>> pts;
  for (int i = 0; i < n_in; ++i) pts.push_back({poly[i][0], poly[i][1]});
  pts.push_back({poly[n_in - 1][0], poly[n_in - 1][1]});
  const int n = (int)pts.size();
  const double R = 6378137.0 / 1000.0, rad = PI / 180.0;
  double total = 0.0;
  for (int i = 0; i < n; ++i)
    total += (pts[(i + 2) % n][1] * rad - pts[i][1] * rad) * sin(pts[(i + 1) % n][0] * rad);
  return fabs(total * R * R / 2);
}

void expansion_range(Expansion kind, double& lower, double& upper, bool& check) {
  const double delta = 0.01, R = 6378137.0 / 1000.0;
  switch (kind) {
    case POS: lower = delta; upper = 720.0; check = true; break;
    case SCALE: {
      const double poly[4][2] = {{90, 0}, {90, delta}, {90 - delta, delta}, {90 - delta, 0}};
      lower = polygon_area_km2(poly, 4); upper = 4 * PI * R * R; check = true; break;
    }
    case LEAD_TIME: lower = 1.0 / 60; upper = 24.0 * 7 * 3; check = true; break;
    case LEVELS: lower = 0.01; upper = 1e5; check = true; break;
    default: lower = 1.0; upper = 24 * 365.25; check = false; break;
  }
}

// Fourier position / scale features of the patch grid (posencoding.py:61-192): [L][D] each, L = Hp * Wp.
// Patch-mean position and patch root area in fp32 like the reference, the trigonometry in fp64 (the reference's fp32
// torch kernels are not reproducible bit for bit outside torch; callers who need that pass the encodings in).
void pos_scale_tables(const double* lat, const double* lon, int Hp, int Wp, int P, int D, float* pos_out, float* scale_out) {
  const int64_t Lp = (int64_t)Hp * Wp;
  std::vector<double> mid_lat(Hp), mid_lon(Wp), area_lat(Hp), area_lon(Wp);
  const float rad = (float)(PI / 180.0);
  for (int hp = 0; hp < Hp; ++hp) {
    float sum = 0.f, mx = -INFINITY, mn = INFINITY;
    for (int i = 0; i < P; ++i) {
      const float v = (float)lat[hp * P + i];
      for (int j = 0; j < P; ++j) sum += v;   // avg_pool2d sums the P x P window of the broadcast grid in fp32
      mx = fmaxf(mx, v); mn = fminf(mn, v);
    }
    REQUIRE(mx > mn, "latitudes of a patch must differ");
    mid_lat[hp] = (double)(sum / (float)(P * P));
    area_lat[hp] = (double)((float)sin((double)(mx * rad)) - (float)sin((double)(mn * rad)));
  }
  for (int wp = 0; wp < Wp; ++wp) {
    float sum = 0.f, mx = -INFINITY, mn = INFINITY;
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < P; ++j) sum += (float)lon[wp * P + j];
    for (int j = 0; j < P; ++j) {
      const float v = (float)lon[wp * P + j];
      mx = fmaxf(mx, v); mn = fminf(mn, v);
    }
    REQUIRE(mx > mn, "longitudes of a patch must differ");
    mid_lon[wp] = (double)(sum / (float)(P * P));
    area_lon[wp] = (double)(mx * rad - mn * rad);
  }
  std::vector<double> xs(Lp), ys(Lp), ra(Lp);
  for (int hp = 0; hp < Hp; ++hp)
    for (int wp = 0; wp < Wp; ++wp) {
      const int64_t l = (int64_t)hp * Wp + wp;
      // avg_pool2d over a P x P patch of a separable grid: mean over rows of the (constant per row) latitudes
      xs[l] = mid_lat[hp];
      ys[l] = mid_lon[wp];
      const float area = (float)(6371.0 * 6371.0 * PI) * (float)area_lat[hp] * (float)area_lon[wp];
      REQUIRE(area > 0, "patch areas must be positive");
      ra[l] = (double)sqrtf(area);
    }
  std::vector<float> half((size_t)Lp * (D / 2));
  fourier(POS, xs.data(), Lp, D / 2, half.data());
  for (int64_t l = 0; l < Lp; ++l) memcpy(&pos_out[(size_t)l * D], &half[(size_t)l * (D / 2)], (D / 2) * 4);
  fourier(POS, ys.data(), Lp, D / 2, half.data());
  for (int64_t l = 0; l < Lp; ++l) memcpy(&pos_out[(size_t)l * D + D / 2], &half[(size_t)l * (D / 2)], (D / 2) * 4);
  fourier(SCALE, ra.data(), Lp, D, scale_out);
}

}  // namespace

// Fourier features (aurora/model/fourier.py:45-92, 112-126): [sin(2 pi x / lambda_j) | cos(...)], lambda log-spaced,
// evaluated in fp64 and cast to fp32 like `encoding.float()` upstream.
void fourier(Expansion kind, const double* x, int64_t n, int d, float* out) {
  double lower, upper;
  bool check;
  expansion_range(kind, lower, upper, check);
  REQUIRE(d % 2 == 0, "The dimensionality must be a multiple of two.");
  const int h = d / 2;
  std::vector<double> w(h);
  const double a = log10(lower), b = log10(upper), step = h > 1 ? (b - a) / (h - 1) : 0.0;
  for (int j = 0; j < h; ++j) w[j] = 2 * PI / pow(10.0, j == h - 1 && h > 1 ? b : a + j * step);
  for (int64_t i = 0; i < n; ++i) {
    const double ax = fabs(x[i]);
    REQUIRE(!check || x[i] == 0 || (lower <= ax && ax <= upper),
            "The input tensor is not within the configured range `[%g, %g]`.", lower, upper);
    for (int j = 0; j < h; ++j) {
      const double pr = x[i] * w[j];
      out[i * d + j] = (float)sin(pr);
      out[i * d + h + j] = (float)cos(pr);
    }
  }
}

const DevTables& tables_for(Model& m, int stage, bool shifted) {
  auto key = std::make_pair(stage, (int)shifted);
  auto it = m.tables.find(key);
  if (it == m.tables.end()) {
    const WindowTables t = window_tables(m.stage_res[stage], m.window, shifted);
    REQUIRE(t.n_tok <= 144, "windows of more than 144 tokens are not supported");
    DevTables d;
    d.n_windows = t.n_windows;
    d.n_tok = t.n_tok;
    d.tok = DevBuf(t.tok.size() * 4);
    upload(d.tok.p, t.tok.data(), t.tok.size() * 4);
    d.has_grp = !t.grp.empty();
    if (d.has_grp) {
      d.grp = DevBuf(t.grp.size());
      upload(d.grp.p, t.grp.data(), t.grp.size());
    }
    it = m.tables.emplace(key, std::move(d)).first;
  }
  return it->second;
}

// The attention plan of one block flavour of this rank's band, on the device.
const DevPlan& plan_for(Model& m, int stage, bool shifted) {
  auto key = std::make_pair(stage, (int)shifted);
  auto it = m.plans.find(key);
  if (it == m.plans.end()) {
    BandPlan p;
    if (!band_plan(m.stage_res[stage], m.window, shifted, m.band.rank, m.rows[stage], p)) throw Fail{AURORA_E_ARG};
    REQUIRE(p.n_tok <= 144, "windows of more than 144 tokens are not supported");
    DevPlan d;
    d.n_windows = p.n_windows; d.n_tok = p.n_tok; d.n_own = p.n_own; d.n_halo = p.n_halo; d.n_interior = p.n_interior;
    d.tok = DevBuf(p.tok.size() * 4);
    upload(d.tok.p, p.tok.data(), p.tok.size() * 4);
    d.has_grp = !p.grp.empty();
    if (d.has_grp) {
      d.grp = DevBuf(p.grp.size());
      upload(d.grp.p, p.grp.data(), p.grp.size());
    }
    std::vector<int32_t> both;
    for (int side = 0; side < 2; ++side) {
      d.recv_off[side] = p.recv_off[side]; d.recv_cnt[side] = p.recv_cnt[side];
      d.send_cnt[side] = (int)p.send_idx[side].size();
      both.insert(both.end(), p.send_idx[side].begin(), p.send_idx[side].end());
    }
    REQUIRE(d.recv_cnt[0] == 0 || d.recv_cnt[1] == 0 || d.recv_off[1] == d.recv_off[0] + d.recv_cnt[0],
            "band plan: the halo rows of the two neighbours are not adjacent");
    if (!both.empty()) {
      d.send_idx = DevBuf(both.size() * 4);
      upload(d.send_idx.p, both.data(), both.size() * 4);
    }
    it = m.plans.emplace(key, std::move(d)).first;
  }
  return it->second;
}

// ---- the stages of aurora_hip_precompute -----------------------------------------------------------
namespace {

// Token grids of the whole forecast (swin3d.py:868-882) and this rank's rows (all, or a latitude band): returns the first.
int band_rows_of(Model& m, const aurora_hip_grid* g) {
  const int P = m.P;
  REQUIRE(g->n_lon % P == 0, "Width of the data must be a multiple of the patch size.");
  REQUIRE(g->n_lat % P == 0 || g->n_lat % P == 1, "There can at most be one latitude too many.");
  const int H = g->n_lat - g->n_lat % P, W = g->n_lon;
  m.full_Hp = H / P; m.Wp = W / P; m.n_lon = W;
  m.stage_res = stage_resolutions(Res{m.Cl, m.full_Hp, m.Wp}, m.n_stages);
  m.merge_pad.clear(); m.tables.clear(); m.plans.clear(); m.embed_packs.clear();
  for (int s = 0; s + 1 < m.n_stages; ++s) m.merge_pad.push_back({m.stage_res[s].h % 2, m.stage_res[s].w % 2});
  m.merge_pad.push_back({0, 0});
  int h0 = 0;
  m.Hp = m.full_Hp;
  m.rows.clear();
  if (m.sharded()) {
    if (!band_rows(m.stage_res, m.window, m.band.world, m.rows)) throw Fail{AURORA_E_ARG};
    h0 = m.rows[0][m.band.rank][0];
    m.Hp = m.rows[0][m.band.rank][1] - h0;
  }
  m.n_lat = m.Hp * P;
  return h0;
}

// Position + scale embedding of the band's patch rows (posencoding.py:61-192), from the caller's encodings or the grid.
void pos_scale_table(Model& m, Launcher& L, const aurora_hip_grid* g, int h0) {
  const int D = m.D;
  const int64_t Lp_full = (int64_t)m.full_Hp * m.Wp, Lp = (int64_t)m.Hp * m.Wp;
  std::vector<float> pos((size_t)Lp_full * D), scale((size_t)Lp_full * D);
  if (g->pos_encoding && g->scale_encoding) {
    memcpy(pos.data(), g->pos_encoding, pos.size() * 4);
    memcpy(scale.data(), g->scale_encoding, scale.size() * 4);
  } else {
    REQUIRE(g->lat && g->lon, "precompute: latitudes / longitudes (or the encodings themselves) are required");
    pos_scale_tables(g->lat, g->lon, m.full_Hp, m.Wp, m.P, D, pos.data(), scale.data());
  }
  DevBuf d_pos((size_t)Lp * D * 4), d_scale((size_t)Lp * D * 4), pe((size_t)Lp * D * 4);
  upload(d_pos.p, pos.data() + (size_t)h0 * m.Wp * D, (size_t)Lp * D * 4);       // the band's patch rows
  upload(d_scale.p, scale.data() + (size_t)h0 * m.Wp * D, (size_t)Lp * D * 4);
  m.pos_scale = DevBuf((size_t)Lp * D * 4);
  L.linear(LinearOp(d_pos.p, D, m.W("encoder.pos_embed.weight"), D, m.W("encoder.pos_embed.bias"), pe.p, D, Lp, D, D, AURORA_F32));
  L.linear(LinearOp(d_scale.p, D, m.W("encoder.scale_embed.weight"), D, m.W("encoder.scale_embed.bias"), m.pos_scale.p, D, Lp, D, D,
                    AURORA_F32).residual(pe.f(), D));
  hip_ok(hipStreamSynchronize(as_stream(L.stream)), "precompute sync");
}

// First queries of a decoder Perceiver: the level queries through to_q (and its LayerNorm).
void first_queries(Model& m, Launcher& L, const Resampler& rs, DevBuf& q) {
  const int C = m.n_levels, D = m.D;
  const auto& d0 = rs.layers[0];
  q = DevBuf((size_t)C * d0.inner * 4);
  L.linear(LinearOp(m.dec_queries.p, 2 * D, d0.to_q, 2 * D, nullptr, q.p, d0.inner, C, d0.inner, 2 * D, AURORA_F32));
  if (d0.ln_q_w)
    L.layernorm(q.p, d0.inner, d0.ln_q_w, d0.ln_q_b, nullptr, 0, 0, q.f(), d0.inner, nullptr, 0, C, d0.inner, 1e-5f, AURORA_F32);
}

// Pressure levels: per-level patch-embedding bias, decoder queries and the score rows made from them (encoder.py:318-330,
// decoder.py:176-200).  The operands of these launches go to `scratch`.
void level_tables(Model& m, Launcher& L, const aurora_hip_grid* g, std::vector<DevBuf>& scratch) {
  const int C = g->n_levels, D = m.D;
  REQUIRE(C >= 1 && C <= 32 && g->levels, "precompute: 1..32 pressure levels are required");
  m.n_levels = C;
  m.levels.assign(C, 0.0);
  for (int c = 0; c < C; ++c) m.levels[c] = g->levels_float32 ? (double)(float)g->levels[c] : g->levels[c];
  std::vector<float> enc((size_t)C * D), dec((size_t)C * 2 * D);
  fourier(LEVELS, m.levels.data(), C, D, enc.data());
  fourier(LEVELS, m.levels.data(), C, 2 * D, dec.data());
  DevBuf d_enc = to_device(enc), d_dec = to_device(dec);
  m.enc_bias = DevBuf((size_t)C * D * 4);
  if (m.level_condition.empty()) {
    L.linear(LinearOp(d_enc.p, D, m.W("encoder.atmos_levels_embed.weight"), D, m.W("encoder.atmos_levels_embed.bias"), m.enc_bias.p,
                      D, C, D, D, AURORA_F32).residual(m.W("encoder.atmos_token_embeds.bias"), 0));
  } else {   // every level has its own patch embedding, bias included (levelcond.py:36-69)
    DevBuf pb((size_t)C * D * 4);
    for (int c = 0; c < C; ++c)
      hip_ok(hipMemcpy(pb.f() + (size_t)c * D, m.W("encoder.atmos_token_embeds.layers." + level_to_str(m.levels[c]) + ".bias"),
                       (size_t)D * 4, hipMemcpyDeviceToDevice), "copy");
    L.linear(LinearOp(d_enc.p, D, m.W("encoder.atmos_levels_embed.weight"), D, m.W("encoder.atmos_levels_embed.bias"), m.enc_bias.p,
                      D, C, D, D, AURORA_F32).residual(pb.f(), D));
    hip_ok(hipStreamSynchronize(as_stream(L.stream)), "precompute sync");
  }
  m.dec_queries = DevBuf((size_t)C * 2 * D * 4);
  L.linear(LinearOp(d_dec.p, 2 * D, m.W("decoder.atmos_levels_embed.weight"), 2 * D, m.W("decoder.atmos_levels_embed.bias"),
                    m.dec_queries.p, 2 * D, C, 2 * D, 2 * D, AURORA_F32));
  first_queries(m, L, m.dec_rs, m.dec_q);
  if (m.has_alt) first_queries(m, L, m.dec_rs_alt, m.dec_q_alt);
  hip_ok(hipStreamSynchronize(as_stream(L.stream)), "precompute sync");
  score_weights(m, m.dec_rs, m.dec_q.f(), C, m.perceiver_heads);
  if (m.has_alt) score_weights(m, m.dec_rs_alt, m.dec_q_alt.f(), C, m.perceiver_heads);
  scratch.push_back(std::move(d_enc));
  scratch.push_back(std::move(d_dec));
}

// What a decoder Perceiver can put out, whatever the inputs: every layer returns LN2(.) + LN1(.) + its residual, the
// first residual being the level queries (max |q| = `qmax`) -- |LN(x) g + b| <= sqrt(D) max|g| + max|b|.  Decides whether
// the output may leave in the fp16-pair layout for the output heads' two-term GEMM (step.hip).
float output_bound(const Resampler& rs, float qmax) {
  float b = qmax;
  for (const auto& ly : rs.layers) {
    const float rt = sqrtf((float)ly.dim);
    b += absmax(ly.ln1_w, ly.dim) * rt + absmax(ly.ln1_b, ly.dim) + absmax(ly.ln2_w, ly.dim) * rt + absmax(ly.ln2_b, ly.dim);
  }
  return b;
}
// The bounds that depend on the level set: of the decoder Perceivers' outputs and of the atmospheric level bias.
void output_bounds(Model& m) {
  const float qmax = absmax(m.dec_queries.f(), (size_t)m.n_levels * 2 * m.D);
  m.dec_out_bound = output_bound(m.dec_rs, qmax);
  m.dec_out_bound_alt = m.has_alt ? output_bound(m.dec_rs_alt, qmax) : 0.f;
  m.enc_bias_max = absmax(m.enc_bias.f(), (size_t)m.n_levels * m.D);
}

// Normalisation statistics: loc, scale, 1/scale (computed in fp64) per variable (and level).
void normalisation_stats(Model& m, const aurora_hip_grid* g) {
  const int C = m.n_levels;
  const int ns = (int)m.surf_inputs.size(), nst = (int)m.static_vars.size(), na = (int)m.atmos_vars.size();
  REQUIRE(g->surf_loc && g->surf_scale && g->atmos_loc && g->atmos_scale && (nst == 0 || (g->static_loc && g->static_scale)),
          "precompute: normalisation statistics are required");
  std::vector<float> hs;
  m.surf_stat_off.clear(); m.static_stat_off.clear(); m.atmos_stat_off.clear(); m.static_lvl_stat_off.clear(); m.static_loc.clear();
  auto push1 = [&](std::vector<size_t>& offs, double loc, double sc) {
    offs.push_back(hs.size());
    hs.push_back((float)loc); hs.push_back((float)sc); hs.push_back((float)(1.0 / sc)); hs.push_back(0.f);
  };
  auto pushC = [&](std::vector<size_t>& offs, const double* loc, const double* sc, int stride) {   // C x loc | scale | 1/scale
    offs.push_back(hs.size());
    for (int c = 0; c < C; ++c) hs.push_back((float)loc[c * stride]);
    for (int c = 0; c < C; ++c) hs.push_back((float)sc[c * stride]);
    for (int c = 0; c < C; ++c) hs.push_back((float)(1.0 / sc[c * stride]));
    while (hs.size() % 4) hs.push_back(0.f);
  };
  for (int v = 0; v < ns; ++v) push1(m.surf_stat_off, g->surf_loc[v], g->surf_scale[v]);
  for (int v = 0; v < nst; ++v) {
    push1(m.static_stat_off, g->static_loc[v], g->static_scale[v]);
    m.static_loc.push_back(g->static_loc[v]);
  }
  for (int v = 0; v < na; ++v) pushC(m.atmos_stat_off, g->atmos_loc + (size_t)v * C, g->atmos_scale + (size_t)v * C, 1);
  // static variables fed at every level keep their surface statistics; dynamic planes are not normalised
  for (int v = 0; v < nst; ++v) pushC(m.static_lvl_stat_off, g->static_loc + v, g->static_scale + v, 0);
  const double zero = 0.0, one = 1.0;
  std::vector<size_t> identity;
  pushC(identity, &zero, &one, 0);
  m.one_stat_off = identity[0];
  m.stats = to_device(hs);
}

// A band's halo plans, and the staging each side of an exchange needs.
void halo_staging(Model& m) {
  m.staging_need = 0;
  if (!m.sharded()) return;
  for (int s = 0; s < m.n_stages; ++s)
    for (int sh = 0; sh < 2; ++sh) {
      const DevPlan& pl = plan_for(m, s, sh != 0);
      const int64_t row_bytes = (int64_t)m.stage_dim(s) * (int64_t)m.bbs();   // the block's input rows travel (step.hip)
      m.staging_need = std::max(m.staging_need, (int64_t)std::max(pl.send_cnt[0] + pl.send_cnt[1], pl.recv_cnt[0] + pl.recv_cnt[1]) * row_bytes);
    }
}

}  // namespace

}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_pos_scale_encoding(const double* lat, const double* lon, int n_lat, int n_lon, int patch_size,
                                             int embed_dim, float* pos_out, float* scale_out) {
  GUARDED({
    REQUIRE(lat && lon && pos_out && scale_out, "pos_scale_encoding: null argument");
    REQUIRE(patch_size > 0 && n_lon % patch_size == 0 && n_lat >= patch_size && embed_dim % 4 == 0,
            "pos_scale_encoding: bad grid %d x %d for patch size %d / embed_dim %d", n_lat, n_lon, patch_size, embed_dim);
    pos_scale_tables(lat, lon, n_lat / patch_size, n_lon / patch_size, patch_size, embed_dim, pos_out, scale_out);
  })
}

extern "C" int aurora_hip_precompute(aurora_hip_model* mp, const aurora_hip_grid* g, void* stream) {
  GUARDED({
    REQUIRE(mp && g, "precompute: null argument");
    Model& m = *mp;
    REQUIRE(m.finalized, "precompute: call aurora_hip_finalize after packing the weights");
    Launcher L{m, stream};
    const int h0 = band_rows_of(m, g);
    pos_scale_table(m, L, g, h0);
    std::vector<DevBuf> scratch;   // operands of level_tables' launches: not freed before the bounds are taken
    level_tables(m, L, g, scratch);
    output_bounds(m);
    if (!m.level_condition.empty()) build_atmos_heads(m, true);   // level-conditioned heads depend on the level set
    normalisation_stats(m, g);
    halo_staging(m);
    m.have_grid = true;
    m.generation += 1;
  })
}

namespace {
// Civil date of a day count since 1970-01-01 (proleptic Gregorian; H. Hinnant's days_from_civil inverse).
void civil_from_days(int64_t z, int& y, int& mth, int& d) {
  z += 719468;
  const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  const unsigned doe = (unsigned)(z - era * 146097);
  const unsigned yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const unsigned mp = (5 * doy + 2) / 153;
  d = (int)(doy - (153 * mp + 2) / 5 + 1);
  mth = (int)(mp < 10 ? mp + 3 : mp - 9);
  y = (int)(yoe + era * 400 + (mth <= 2));
}
}  // namespace

extern "C" int aurora_hip_set_time_ex(aurora_hip_model* mp, const double* time_hours, const int32_t* calendar, int B, void* stream) {
  GUARDED({
    REQUIRE(mp && time_hours && B >= 1, "set_time: bad argument");
    Model& m = *mp;
    std::vector<double> t(B);
    // the reference converts the timestamps to a float32 tensor before expanding (encoder.py:359-362)
    for (int b = 0; b < B; ++b) t[b] = (double)(float)time_hours[b];
    if (m.abs_B < B) {
      hip_ok(hipDeviceSynchronize(), "set_time");
      m.abs_enc = DevBuf((size_t)B * m.D * 4);
      m.dyn_planes = DevBuf((size_t)6 * B * 4);
      m.abs_B = B;
      m.generation += 1;
    }
    const size_t n_abs = (size_t)B * m.D, n_dyn = (size_t)6 * m.abs_B, bytes = (n_abs + n_dyn) * 4;
    auto& slot = m.pinned[m.pinned_next++ & 3];
    if (slot.done) hip_ok(hipEventSynchronize(slot.done), "set_time");   // the copy that used this slot four uploads ago
    else hip_ok(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming), "set_time");
    if (slot.bytes < bytes) {
      if (slot.host) (void)hipHostFree(slot.host);
      hip_ok(hipHostMalloc((void**)&slot.host, bytes, hipHostMallocDefault), "set_time");
      slot.bytes = bytes;
    }
    fourier(ABS_TIME, t.data(), B, m.D, slot.host);
    // time of day / day of week / "day of year" planes of the dynamic variables (encoder.py:226-246: the last really is the
    // day of the MONTH over 365.25), plane i of batch element b at [i][b]
    float* dyn = slot.host + n_abs;
    for (size_t i = 0; i < n_dyn; ++i) dyn[i] = 0.f;
    for (int b = 0; b < B; ++b) {
      int hour, weekday, day;
      if (calendar) { hour = calendar[3 * b]; weekday = calendar[3 * b + 1]; day = calendar[3 * b + 2]; }
      else {
        const double hrs = time_hours[b];
        const int64_t days = (int64_t)floor(hrs / 24.0);
        hour = (int)floor(hrs - 24.0 * (double)days);
        weekday = (int)(((days % 7) + 7 + 3) % 7);   // 1970-01-01 was a Thursday; Monday = 0
        int y, mo;
        civil_from_days(days, y, mo, day);
      }
      const double vals[6] = {cos(2 * PI * hour / 24), sin(2 * PI * hour / 24), cos(2 * PI * weekday / 7), sin(2 * PI * weekday / 7),
                              cos(2 * PI * day / 365.25), sin(2 * PI * day / 365.25)};
      for (int i = 0; i < 6; ++i) dyn[(size_t)i * m.abs_B + b] = (float)vals[i];
    }
    hip_ok(hipMemcpyAsync(m.abs_enc.p, slot.host, n_abs * 4, hipMemcpyHostToDevice, as_stream(stream)), "set_time");
    hip_ok(hipMemcpyAsync(m.dyn_planes.p, dyn, n_dyn * 4, hipMemcpyHostToDevice, as_stream(stream)), "set_time");
    hip_ok(hipEventRecord(slot.done, as_stream(stream)), "set_time");
  })
}

extern "C" int aurora_hip_set_time(aurora_hip_model* mp, const double* time_hours, int B, void* stream) {
  return aurora_hip_set_time_ex(mp, time_hours, nullptr, B, stream);
}
