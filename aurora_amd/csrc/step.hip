// The launch sequence of ONE FORECAST STEP (aurora_hip_step): encoder (encoder.py:198-366), 3D Swin U-net
// (swin3d.py:884-936, 440-509), decoder (decoder.py:168-276), for every model class -- the ERA5 family and the
// air-pollution / ocean-wave variants (aurora.py:726-796, 854-932; levelcond.py:36-69) -- on one device or on one
// latitude band of a sharded forecast (halo exchange through the host's transport callbacks, include/aurora_hip.h).
// Host code only; every launch goes through the operator ABI of this same library.  `run_step` at the end names the
// stages in order; each stage is a function over `Step`.
#include <algorithm>

#include "model.h"
#include "resampler_space.h"

namespace aurora {

namespace {

// Where the guard word of a resampler call comes from.  The context is as unbounded as the model inputs, so the linears that
// read it, or averages of its value projection, pick their operand split on the device: |ctx| <= a * word + c.  `scan`: this
// call measures max |ctx| into the word itself (a = 1, c = 0), else the caller measured the word upstream and derived the
// bound.  `pairs`: the context arrives as fp16 pairs, and `limit_kv` is the limit the caller wrote them under.
struct CtxGuard { float* word; float a, c, limit_kv; bool pairs, scan; };
// The context linears of the encoder's level aggregation with the patch embedding folded in (model_weights.hip:compose_front):
// one ComposedCtx per layer, read over the `levels` row blocks (`rows` each) of the unfolded input, level c with its own bias
// row and -- `groups` > 1 -- its own weight.  `embed_l1`, `embed_bias_max`: of the embedding, for the bound the stages gave.
struct ComposedFront { const ComposedCtx* layers; int levels, groups; int64_t rows; float embed_l1, embed_bias_max; };

// One call of the PerceiverResampler (perceiver.py:212-233) for all grid columns `g` at once.  ctx: (ctx_rows, ctx_dim), key j of
// column (b, l) at row b*kv_bstride + j*kv_lstride + l.  First layer: the latents `latents0` (and so the queries `q0`) are
// shared by every column.  `out_pairs`: the last layer's result leaves as fp16 pairs where that layer can write them.
// `front` (or null): the context is the unfolded input, read through the composed weights.
struct ResamplerCall {
  const Resampler* rs;
  const float* ctx;
  int64_t ctx_rows;
  int ctx_dim;
  const float *q0, *latents0;
  PerceiverCols g;
  float eps;
  bool out_pairs;
  const ComposedFront* front;
  CtxGuard guard;
};

// What the stages of layer `i` of a call share: its workspace (resampler_space.h), the guard word and to_out's limit.
struct ResamplerLayer {
  const ResamplerCall& call;
  size_t i;
  const Resampler::Layer& ly;
  LayerSpace sp;
  const float* lat;             // the previous layer's result (null in the first)
  const float* word;            // the call's guard word, and the limit to_out's activation operand is held to against it
  float lim_out;
  float *y, *lat1;              // the regions Y, L and S of the layer's workspace, and the arena mark behind Y
  char* S;
  size_t after_y;
  float *kv, *qb, *att, *P, *o; // what lives in them, in launch order: set and explained in `resampler_layer`
  void* Vp;
  const float* q;               // the queries of this layer, `q_stride` rows apart from column to column
  int64_t q_stride;
};

// The workspace of layer `i` of the call (taken from the arena: Y, L, S in this order) and the limit of its to_out guard.
ResamplerLayer resampler_layer(Model& m, const ResamplerCall& c, size_t i, const float* lat) {
  const Resampler& rs = *c.rs;
  const auto& ly = rs.layers[i];
  LayerShape sh{};
  sh.layer = i;
  sh.dim = ly.dim; sh.inner = ly.inner; sh.hidden = ly.hidden; sh.head_dim = ly.head_dim; sh.heads = c.g.heads;
  sh.n_vs = rs.n_vs; sh.vs_lq = rs.vs_lq;
  sh.ln_k = ly.ln_k_w != nullptr; sh.to_out_s = ly.to_out_s != nullptr; sh.fc1_s = ly.fc1_s != nullptr; sh.fc2_s = ly.fc2_s != nullptr;
  sh.f16_mode = ly.f16_mode;
  sh.reassoc_out = m.reassoc_out;
  sh.out_supported = aurora_hip_perceiver_out_supported(c.g.Lq, c.g.Lk, c.g.heads, ly.head_dim, ly.dim) != 0;
  sh.B = c.g.B; sh.cols = c.g.cols; sh.ctx_rows = c.ctx_rows; sh.Lq = c.g.Lq; sh.Lk = c.g.Lk;
  const LayerSpace sp = layer_space(sh);
  const CtxGuard& gd = c.guard;
  // |att| <= max |v| <= (largest L1 row norm of W_v) * max |ctx|: the context's guard word, a tighter limit.
  // (composed: |v| <= v_l1 max|input| + max|bias| of the COMPOSED value rows, never looser than the above: model.h)
  const float lim_out = c.front ? composed_value_bound(ly.v_l1, c.front->embed_l1, c.front->embed_bias_max, c.front->layers[i].v_l1,
                                                       c.front->layers[i].vb_max).word_limit()
                                : (F16_SAFE / ly.v_l1 - gd.c) / gd.a;
  ResamplerLayer r{c, i, ly, sp, lat, gd.word, lim_out};
  // Y: the attention output (`att`; re-associated: the value rows `Vp` as fp16 pairs) until fc2 writes the layer's result there
  r.y = (float*)m.arena.take(sp.unit);
  r.after_y = m.arena.top;
  r.Vp = r.y;
  // L: LayerNorm 1's output, the MLP's input and residual
  r.lat1 = (float*)m.arena.take(sp.unit);
  // S: k | v (or v | scores) with the projected queries behind it; then to_out's result (k | v and q are dead) -- the softmax
  // weights P of the re-associated form lie behind both --; then the MLP's hidden layer in row chunks (to_out's result is dead)
  r.S = (char*)m.arena.take(sp.s_bytes);
  r.kv = r.o = (float*)r.S;
  r.qb = (float*)(r.S + round256(sp.kv_bytes));
  r.P = (float*)(r.S + sp.p_off);
  r.att = sp.att_in_y ? r.y : (float*)(r.S + sp.att_off);   // (wider than Y: in S, behind everything it coexists with)
  // first layer: the queries are shared by every column
  r.q = i > 0 ? r.qb : c.q0;
  r.q_stride = i > 0 ? c.g.Lq : 0;
  return r;
}

// Stage 1: k | v (or v | scores) of every context row.  The one place that knows the forms a context comes in.
void project_context(Launcher& L, const ResamplerLayer& r) {
  const ResamplerCall& c = r.call;
  const CtxGuard& gd = c.guard;
  const auto& ly = r.ly;
  const int kv_ld = r.sp.kv_ld;
  REQUIRE(!gd.pairs || ly.to_kv_s, "resampler: a pair-layout context needs pre-split to_kv weights");
  if (c.front) {
    // `ctx` is the unfolded, normalised input itself (fp32: the two-term kernel splits it, as the embedding did), so the
    // guard word bounds this linear's activation operand directly; one strided-batch launch over the levels
    const ComposedFront& f = *c.front;
    const ComposedCtx& cc = f.layers[r.i];
    REQUIRE(cc.N == kv_ld && f.levels * f.rows == c.ctx_rows, "resampler: composed context weights of another shape");
    L.guarded_linear(LinearOp(c.ctx, c.ctx_dim, cc.w.f(), c.ctx_dim, cc.bias.f(), r.kv, kv_ld, f.rows, kv_ld, c.ctx_dim, AURORA_F32)
                         .batched(f.levels, f.rows * c.ctx_dim, f.groups > 1 ? (int64_t)kv_ld * c.ctx_dim : 0, kv_ld, f.rows * kv_ld),
                     cc.ws.p, 0, ly.f16_mode, r.word, F16_SAFE);
  } else {
    // |ctx| <= a * word + c < F16_SAFE  <=>  word < (F16_SAFE - c) / a; a context in pairs comes with its own limit
    const bool scores = r.sp.scores;
    L.guarded_linear(LinearOp(c.ctx, c.ctx_dim, scores ? c.rs->vs_w.f() : ly.to_kv, c.ctx_dim, nullptr, r.kv, kv_ld, c.ctx_rows, kv_ld,
                              c.ctx_dim, AURORA_F32),
                     scores ? c.rs->vs_ws.p : ly.to_kv_s, gd.pairs ? AURORA_F32_A_SPLIT : 0, ly.f16_mode, r.word,
                     gd.pairs ? gd.limit_kv : (F16_SAFE - gd.c) / gd.a);
  }
}

// Stage 2: LayerNorm over the K half, in place (perceiver.py:144-147)
void norm_keys(Launcher& L, const ResamplerLayer& r) {
  const int inner = r.ly.inner;
  if (r.ly.ln_k_w)
    L.layernorm(r.kv, 2 * inner, r.ly.ln_k_w, r.ly.ln_k_b, nullptr, 0, 0, r.kv, 2 * inner, nullptr, 0, r.call.ctx_rows, inner, 1e-5f,
                AURORA_F32);
}

// Stage 3, layers after the first: the queries of the previous layer's result, with their LayerNorm
void project_queries(Launcher& L, const ResamplerLayer& r) {
  if (r.i == 0) return;
  const auto& ly = r.ly;
  const int inner = ly.inner;
  const int64_t n_rows = r.call.g.n_rows();
  L.linear(LinearOp(r.lat, ly.dim, ly.to_q, ly.dim, nullptr, r.qb, inner, n_rows, inner, ly.dim, AURORA_F32));
  if (ly.ln_q_w) L.layernorm(r.qb, inner, ly.ln_q_w, ly.ln_q_b, nullptr, 0, 0, r.qb, inner, nullptr, 0, n_rows, inner, 1e-5f, AURORA_F32);
}

// Stage 4, plain: attention, then to_out.  With pre-split to_out weights the attention writes fp16 pairs iff the guard holds,
// and to_out multiplies them without splitting anything.  `skip`: as the fall-back behind the re-associated pair -- attention
// output in fp32, to_out on three bf16 terms, both retiring at once iff the guard HOLDS.
void attend_plain(Launcher& L, const ResamplerLayer& r, bool skip) {
  const PerceiverCols& g = r.call.g;
  const auto& ly = r.ly;
  const int inner = ly.inner;
  const bool pairs = !skip && r.sp.att_pairs;
  const float* pair_word = pairs ? r.word : nullptr;
  const float pair_limit = skip ? 0.f : r.lim_out, skip_limit = skip ? r.lim_out : 0.f;
  const float* skip_word = skip ? r.word : nullptr;
  if (pairs) L.m.note_guard(r.word, r.lim_out);
  if (r.sp.scores) L.perceiver_attention_scores(g, ly.head_dim, r.kv, r.sp.kv_ld, inner, r.att, pair_word, pair_limit, skip_word, skip_limit);
  else L.perceiver_attention(g, ly.head_dim, r.q, r.q_stride, r.kv, r.att, pair_word, pair_limit, skip_word, skip_limit);
  LinearOp to_out(r.att, inner, ly.to_out, inner, nullptr, r.o, ly.dim, g.n_rows(), ly.dim, inner, AURORA_F32);
  if (skip) L.linear(to_out.f32_mode(1).guarded_by(r.word, r.lim_out));
  else L.guarded_linear(to_out, ly.to_out_s, pairs ? AURORA_F32_A_SPLIT : 0, ly.f16_mode, r.word, r.lim_out);
}

// Stage 4, re-associated (perceiver_out.hip): the softmax weights and the value rows, to_out of the value rows combined in
// registers -- and, for values outside fp16's range (the same word decides, on the device), the plain pair instead; inside
// the range both of its launches retire at once.
void attend_reassociated(Launcher& L, const ResamplerLayer& r) {
  const PerceiverCols& g = r.call.g;
  const auto& ly = r.ly;
  const LayerSpace& sp = r.sp;
  // (the launch that writes P reads k | v, and to_out's result lands on [0, unit) while P is read)
  REQUIRE(sp.p_off >= sp.kv_bytes && sp.p_off >= sp.unit && sp.p_off + sp.p_bytes <= sp.s_bytes,
          "resampler: the softmax weights overlap k | v or to_out's result in the scratch region");
  for (int k = 0; k < 3; ++k) L.m.note_guard(r.word, r.lim_out);   // probs, perceiver_out and the plain attention behind them
  L.perceiver_probs(g, ly.head_dim, sp.scores ? nullptr : r.q, r.kv, sp.kv_ld, ly.inner, r.P, r.Vp, r.word, r.lim_out);
  L.perceiver_out(g, ly.head_dim, r.Vp, ly.to_out_s, ly.inner, r.P, r.o, ly.dim, r.word, r.lim_out);
  attend_plain(L, r, true);
}

// Stage 5, the MLP half: LayerNorm 1 of to_out's result (+ residual: the previous layer's result, or the shared latents) into
// `lat1`, fc1 -> fc2 in row chunks through the scratch region into `y`, LayerNorm 2 in place (or, `y_pairs`, to the fp16-pair
// layout).
void resampler_mlp(Launcher& L, const ResamplerLayer& r) {
  const ResamplerCall& c = r.call;
  const auto& ly = r.ly;
  const LayerSpace& sp = r.sp;
  const int Dd = ly.dim;
  const int64_t n_rows = c.g.n_rows();
  const float* res = r.i == 0 ? c.latents0 : r.lat;
  const int64_t res_mod = r.i == 0 ? c.g.Lq : 0;
  float *lat1 = r.lat1, *y = r.y;
  if (sp.pairs) L.layernorm_split(r.o, Dd, ly.ln1_w, ly.ln1_b, res, Dd, res_mod, 0, nullptr, 0, lat1, Dd, n_rows, Dd, c.eps);
  else L.layernorm(r.o, Dd, ly.ln1_w, ly.ln1_b, res, Dd, res_mod, lat1, Dd, nullptr, 0, n_rows, Dd, c.eps, AURORA_F32);
  // fc1 sees a LayerNorm output (|x| <= sqrt(D) * gain), fc2 its GELU: bounded whatever the inputs are.  Row chunks of the
  // pair fc1 -> fc2, so that the hidden layer of a chunk fits the scratch region (to_out's result is dead by now).
  float* hid = (float*)r.S;
  const int64_t chunk_rows = sp.chunk_rows;
  REQUIRE(chunk_rows >= 1 && (size_t)chunk_rows * sp.hid_row <= sp.s_bytes, "resampler: scratch region too small for the MLP");
  const int all = 2 | AURORA_F32_A_SPLIT | AURORA_F32_W_SPLIT;
  for (int64_t r0 = 0; r0 < n_rows; r0 += chunk_rows) {
    const int64_t nr = std::min(chunk_rows, n_rows - r0);
    LinearOp fc1(lat1 + (size_t)r0 * Dd, Dd, sp.pairs ? ly.fc1_s : ly.fc1_w, Dd, ly.fc1_b, hid, ly.hidden, nr, ly.hidden, Dd, AURORA_F32);
    LinearOp fc2(hid, ly.hidden, sp.pairs ? ly.fc2_s : ly.fc2_w, ly.hidden, ly.fc2_b, y + (size_t)r0 * Dd, Dd, nr, Dd, ly.hidden, AURORA_F32);
    L.linear(fc1.activation(AURORA_ACT_GELU).f32_mode(sp.pairs ? all | AURORA_F32_C_SPLIT : ly.f16_mode));
    L.linear(fc2.f32_mode(sp.pairs ? all : ly.f16_mode));
  }
  // (`y_pairs`: the LAST layer's result leaves in the fp16-pair layout, in place -- a row is in registers before any of
  // it is written --, for a consumer that multiplies it without splitting anything: the decoder's output heads)
  const bool y_pairs = c.out_pairs && sp.pairs && r.i + 1 == c.rs->layers.size();
  if (sp.pairs) L.layernorm_split(y, Dd, ly.ln2_w, ly.ln2_b, lat1, Dd, 0, 1, y_pairs ? nullptr : y, Dd, y_pairs ? y : nullptr, Dd, n_rows, Dd, c.eps);
  else L.layernorm(y, Dd, ly.ln2_w, ly.ln2_b, lat1, Dd, 0, y, Dd, nullptr, 0, n_rows, Dd, c.eps, AURORA_F32);
}

// The layers of a resampler call as their stages.  Returns the last layer's result (B*cols*Lq, D).
float* resampler(Model& m, Launcher& L, const ResamplerCall& c) {
  // (the words were cleared at the start of the step)
  if (c.guard.scan)
    timed(m, L.stream, K_ABSMAX, 0.0, [&] { return aurora_hip_absmax_fold(c.ctx, c.ctx_rows * c.ctx_dim, c.guard.word, L.stream); });
  float* lat = nullptr;
  for (size_t i = 0; i < c.rs->layers.size(); ++i) {
    const ResamplerLayer r = resampler_layer(m, c, i, lat);
    project_context(L, r);
    norm_keys(L, r);
    project_queries(L, r);
    if (r.sp.reassoc) attend_reassociated(L, r);
    else attend_plain(L, r, false);
    resampler_mlp(L, r);
    m.arena.top = r.after_y;   // temporaries of this layer are dead (a previous layer's result stays below y)
    lat = r.y;
  }
  return lat;
}

inline int index_of(const std::vector<std::string>& v, const std::string& s) {
  const auto it = std::find(v.begin(), v.end(), s);
  return it == v.end() ? -1 : (int)(it - v.begin());
}

// patchify descriptor of one input channel (embed.hip): where its pixels come from, its normalisation, its transform
aurora_patch_var channel_desc(const Model& m, const aurora_hip_step_io& io, const Channel& ch, bool atmos_level, int C) {
  const float* st = m.stats.f();
  aurora_patch_var d{};
  d.transform = ch.transform; d.tw0 = ch.tw0; d.tw1 = ch.tw1; d.tb = ch.tb;
  switch (ch.kind) {
    case SRC_SURF:
      d.src = io.surf[ch.src];
      d.stride_b = io.surf_strides[0]; d.stride_t = io.surf_strides[1]; d.stride_h = io.surf_strides[2]; d.stride_w = io.surf_strides[3];
      d.loc = st + m.surf_stat_off[ch.src]; d.inv_scale = d.loc + 2;
      break;
    case SRC_STATIC:   // broadcast over batch / history (/ level)
      d.src = io.stat[ch.src];
      d.stride_h = io.static_strides[0]; d.stride_w = io.static_strides[1];
      if (atmos_level) { d.loc = st + m.static_lvl_stat_off[ch.src]; d.inv_scale = d.loc + 2 * C; }
      else { d.loc = st + m.static_stat_off[ch.src]; d.inv_scale = d.loc + 2; }
      break;
    case SRC_DYN:      // one constant plane per batch element (encoder.py:226-246), identity normalisation
      d.src = m.dyn_planes.f() + (size_t)ch.src * m.abs_B;
      d.stride_b = 1;
      d.loc = st + m.one_stat_off; d.inv_scale = d.loc + 2 * C;
      break;
    case SRC_ATMOS:
      d.src = io.atmos[ch.src];
      d.stride_b = io.atmos_strides[0]; d.stride_t = io.atmos_strides[1]; d.stride_c = io.atmos_strides[2];
      d.stride_h = io.atmos_strides[3]; d.stride_w = io.atmos_strides[4];
      d.loc = st + m.atmos_stat_off[ch.src]; d.inv_scale = d.loc + 2 * C;
      break;
  }
  return d;
}

bool channel_present(const aurora_hip_step_io& io, const Channel& ch) {
  switch (ch.kind) {
    case SRC_SURF: return io.surf[ch.src] != nullptr;
    case SRC_STATIC: return io.stat != nullptr && io.stat[ch.src] != nullptr;
    case SRC_ATMOS: return io.atmos[ch.src] != nullptr;
    default: return true;
  }
}

// What every stage of a step reads, computed once (run_step).  Lp: patches per level (of this rank's rows); bf / bb / es:
// the backbone runs in bf16, its dtype code, its element size.
struct Step {
  Model& m;
  Launcher L;
  const aurora_hip_step_io& io;
  int B, T, P, D, Hp, Wp, Cl, C, PP;
  int64_t Lp;
  bool sharded;
  int rank, world;
  bool clamp_now, bf;
  int bb;
  size_t es;
  // token grid of this rank at a stage: the whole grid, or its band of latitude rows
  Res local_res(int stage) const {
    Res r = m.stage_res[stage];
    if (sharded) r.h = m.rows[stage][rank][1] - m.rows[stage][rank][0];
    return r;
  }
};

// `launch(descriptors, count, index of the first)` for descriptors that travel as kernel arguments: at most 32 per launch
template <typename V, typename F>
void in_launches_of_32(Step& s, int kind, const std::vector<V>& descs, F&& launch) {
  for (size_t i = 0; i < descs.size(); i += 32)
    timed(s.m, s.L.stream, kind, 0.0, [&] { return launch(descs.data() + i, (int)std::min<size_t>(32, descs.size() - i), (int)i); });
}

// Input of a patch embedding (surface, or all atmospheric levels): the weights packed for the channels this step carries,
// and the arena rows `A` ((n_lvl B Lp, Kpad)) those channels are normalised and unfolded into by `patchify` -- which folds
// max |A| into `word` when the embedding runs guarded.
const EmbedPack& embed_input(Step& s, bool atmos, float*& A) {
  const std::vector<Channel>& channels = atmos ? s.m.atmos_channels : s.m.surf_channels;
  std::vector<char> present(channels.size());
  for (size_t i = 0; i < present.size(); ++i) present[i] = channel_present(s.io, channels[i]);
  const EmbedPack& p = embed_pack(s.m, atmos ? 1 : 0, s.T, present);
  A = (float*)s.m.arena.take((size_t)(atmos ? s.C : 1) * s.B * s.Lp * p.Kpad * 4);
  return p;
}
void patchify(Step& s, const EmbedPack& p, bool atmos, float* A, float* word) {
  const std::vector<Channel>& channels = atmos ? s.m.atmos_channels : s.m.surf_channels;
  std::vector<aurora_patch_var> descs;
  for (int ci : p.channels) descs.push_back(channel_desc(s.m, s.io, channels[ci], atmos, s.C));
  in_launches_of_32(s, K_PATCHIFY, descs, [&](const aurora_patch_var* d, int n, int i0) {
    return aurora_hip_patchify_absmax(d, n, A, p.Kpad, i0 * s.T * s.PP, p.K, s.B, s.T, atmos ? s.C : 1, s.Hp, s.Wp, s.P, AURORA_F32, word,
                                      s.L.stream);
  });
}

// ---- surface level: normalise + unfold, patch embedding, MLP, LayerNorm.  Returns xs0 + LN(MLP(xs0)) (B Lp, D). ----
const float* encode_surface(Step& s) {
  Model& m = s.m;
  Launcher& L = s.L;
  Arena& A = m.arena;
  const int D = s.D;
  const int64_t R = s.B * s.Lp;
  float* A_s;
  const EmbedPack& ps = embed_input(s, false, A_s);
  const int Kpad_s = ps.Kpad;
  const bool surf_guarded = m.surf_chain && ps.ws.p != nullptr;
  float* word = m.ctx_max.f() + 2;   // max |normalised surface input|, folded in by patchify when the chain is guarded
  patchify(s, ps, false, A_s, surf_guarded ? word : nullptr);
  float* xs0 = (float*)A.take((size_t)R * D * 4);
  const int hid_s = (int)m.T_("encoder.surf_mlp.net.0.weight").shape[0];
  float* hid = (float*)A.take((size_t)R * hid_s * 4);
  float* y = (float*)A.take((size_t)R * D * 4);
  const LinearOp embed = LinearOp(A_s, Kpad_s, ps.w.f(), Kpad_s, m.W("encoder.surf_token_embeds.bias"), xs0, D, R, D, Kpad_s, AURORA_F32)
                             .residual(m.W("encoder.surf_level_encoding"), 0);
  const LinearOp fc1 = LinearOp(xs0, D, m.W("encoder.surf_mlp.net.0.weight"), D, m.W("encoder.surf_mlp.net.0.bias"), hid, hid_s, R, hid_s,
                                D, AURORA_F32).activation(AURORA_ACT_GELU);
  const LinearOp fc2(hid, hid_s, m.W("encoder.surf_mlp.net.2.weight"), hid_s, m.W("encoder.surf_mlp.net.2.bias"), y, D, R, D, hid_s, AURORA_F32);
  // Guarded like the atmospheric chain: max |normalised input| once, then every linear takes two fp16 terms iff the
  // bound that word implies for ITS activation operand is inside fp16's range -- embedding: the input itself; first
  // MLP linear: |xs0| <= l1_e * w + c; second: |GELU(h)| <= |h| <= l1_0 * (l1_e * w + c) + |b0| -- else three bf16 terms.
  if (surf_guarded) {
    const float l1e = ps.l1;
    const float lim_e = F16_SAFE, lim_0 = (F16_SAFE - m.surf_c) / l1e, lim_2 = ((F16_SAFE - m.surf_b0) / m.surf_l1_0 - m.surf_c) / l1e;
    L.guarded_pair(embed, ps.ws.p, 0, word, lim_e);
    L.guarded_pair(fc1, m.surf_w0_s.p, 0, word, lim_0);
    L.guarded_pair(fc2, m.surf_w2_s.p, 0, word, lim_2);
  } else {
    L.linear(embed);
    L.linear(fc1);
    L.linear(fc2);
  }
  L.layernorm(y, D, m.W("encoder.surf_norm.weight"), m.W("encoder.surf_norm.bias"), xs0, D, 0, y, D, nullptr, 0, R, D, 1e-5f,
              AURORA_F32);   // xs0 + LN(MLP(xs0)), in place
  return y;
}

// ---- atmospheric levels: normalise + unfold, patch embedding, level aggregation (Perceiver resampler over the level
// axis).  Returns the latent levels (B Lp (Cl - 1), D). ----
const float* encode_levels(Step& s) {
  Model& m = s.m;
  Launcher& L = s.L;
  const int B = s.B, D = s.D, C = s.C;
  float* A_a;
  const EmbedPack& pa = embed_input(s, true, A_a);
  const int Kpad_a = pa.Kpad;
  bool chain = pa.ws.p != nullptr;
  for (const auto& ly : m.enc_rs.layers) chain = chain && ly.f16_mode == 2 && ly.to_kv_s != nullptr;
  const bool composed = !pa.composed.empty();
  m.front_composed = composed;
  float* word = m.ctx_max.f() + 1;   // max |normalised atmospheric input|, folded in by patchify when the chain is guarded
  patchify(s, pa, true, A_a, chain || composed ? word : nullptr);
  const int64_t R = (int64_t)B * s.Lp;
  // the level aggregation: three latent queries per column over its C levels, level c of column (b, l) at row c R + b Lp + l
  ResamplerCall call{};
  call.rs = &m.enc_rs;
  call.ctx_rows = (int64_t)C * R;
  call.q0 = m.enc_q0.f();
  call.latents0 = m.W("encoder.atmos_latents");
  call.g.B = B; call.g.cols = s.Lp; call.g.kv_bstride = s.Lp; call.g.kv_lstride = R;
  call.g.Lq = s.Cl - 1; call.g.Lk = C; call.g.heads = m.perceiver_heads;
  call.eps = m.ln_eps;
  call.out_pairs = false;
  // The embedding folded into the level aggregation's context linears: no embedding launch, no embeddings in the arena --
  // the resampler reads the unfolded input with the composed weights.  The guard is the same word, one link shorter: the
  // activation operand of the context linear is the input itself (limit F16_SAFE), and the attention output's bound comes
  // from the composed value rows.  Format and kernels still switch together on that word.
  if (composed) {
    REQUIRE(pa.composed.size() == m.enc_rs.layers.size(), "encoder: composed context weights for %zu of %zu layers",
            pa.composed.size(), m.enc_rs.layers.size());
    const ComposedFront front{pa.composed.data(), C, pa.groups, R, pa.l1, m.enc_bias_max};
    call.ctx = A_a;
    call.ctx_dim = Kpad_a;
    call.front = &front;
    call.guard = CtxGuard{word, 1.0f, 0.0f, F16_SAFE, false, false};
    return resampler(m, L, call);
  }
  float* xa = (float*)m.arena.take((size_t)C * B * s.Lp * D * 4);
  // The patch embedding and the level aggregation's to_kv as one guarded chain: max |normalised input| is measured
  // once (a third of the bytes of the embeddings the resampler would otherwise scan), and if it is inside fp16's range
  // -- together with the bound it implies for the embeddings, |x| <= l1 * max|input| + max|bias| -- the embedding runs
  // on two fp16 terms and writes fp16 PAIRS, which to_kv multiplies without splitting anything; otherwise both run on
  // three bf16 terms over fp32 buffers.  One word and one limit decide format and kernels together.
  // All C levels are ONE strided-batch launch: level c reads rows [c R, (c + 1) R) of the unfolded input, its own bias
  // (level embedding + patch bias) and -- level-conditioned models (levelcond.py:36-69) -- its own weight.
  const int64_t sw = pa.groups > 1 ? (int64_t)D * Kpad_a : 0;
  const LinearOp embed = LinearOp(A_a, Kpad_a, pa.w.f(), Kpad_a, m.enc_bias.f(), xa, D, R, D, Kpad_a, AURORA_F32)
                             .batched(C, R * Kpad_a, sw, D, R * D);
  call.ctx = xa;
  call.ctx_dim = D;
  call.front = nullptr;
  if (chain) {
    const float l1 = pa.l1, cb = m.enc_bias_max;
    call.guard = CtxGuard{word, l1, cb, std::min(F16_SAFE, (F16_SAFE - cb) / l1), true, false};
    L.guarded_pair(embed, pa.ws.p, AURORA_F32_C_SPLIT, call.guard.word, call.guard.limit_kv);
  } else {
    L.linear(embed);
    call.guard = CtxGuard{m.ctx_max.f(), 1.0f, 0.0f, F16_SAFE, false, true};   // the resampler scans the embeddings itself
  }
  return resampler(m, L, call);
}

// ---- assemble tokens + position / scale / time embeddings into the residual stream (and its bf16 shadow) ----
void assemble(Step& s, const float* xs1, const float* lat, float* x_f, void* x_b) {
  Model& m = s.m;
  const int B = s.B, D = s.D;
  float* time_emb = (float*)m.arena.take((size_t)B * D * 4);
  s.L.linear(LinearOp(m.abs_enc.f(), D, m.W("encoder.absolute_time_embed.weight"), D, m.W("encoder.absolute_time_embed.bias"), time_emb,
                      D, B, D, D, AURORA_F32).residual(m.lead_emb.f(), 0));
  timed(m, s.L.stream, K_ASSEMBLE, 0.0, [&] {
    return aurora_hip_assemble_tokens(xs1, lat, m.pos_scale.f(), time_emb, x_f, x_b, B, s.Cl, s.Lp, D, s.bb, s.L.stream);
  });
}

// ================= backbone (swin3d.py:884-936) =================
// The windows [w0, w0 + n_windows) of an attention table over q | k | v (rows of 3 dim, or head planes `plane_stride` apart).
void window_attention(Step& s, const Block& blk, const void* qkv, int64_t plane_stride, void* ao, const int32_t* tok, const uint8_t* grp,
                      int n_windows, int n_tok, int64_t Lq, int64_t Lo) {
  // algorithmic bytes: q, k, v read + o written once over the (padded) windows
  timed(s.m, s.L.stream, K_WINDOW_ATTENTION, 4.0 * s.B * n_windows * n_tok * blk.dim * s.es, [&] {
    return aurora_hip_window_attention_planes(qkv, plane_stride, blk.qkv_b, ao, tok, grp, s.B, Lq, Lo, blk.dim, blk.heads, n_windows,
                                              n_tok, s.bb, s.L.stream);
  });
}

// The qkv linear of `M` rows.  bf16 blocks: q | k | v in head planes (head h: [rows][q | k | v = 192]) -- what the attention
// gathers per (token, head) is then 384 contiguous bytes, and a window's runs of consecutive tokens are contiguous in DRAM
// (m.qkv_planes, AURORA_QKV_PLANES=0 at creation: rows of 3 dim).  Same bytes, same arithmetic; the planes of a band have
// own + halo rows.
void qkv_linear(Step& s, const Block& blk, const void* a_in, const void* w, void* qkv, int64_t plane_stride, int64_t M) {
  const int dim = blk.dim;
  if (s.bf && s.m.qkv_planes) s.L.linear_planes(a_in, dim, w, dim, blk.qkv_b, qkv, plane_stride, blk.heads, M, 3 * dim, dim);
  else s.L.linear(LinearOp(a_in, dim, w, dim, blk.qkv_b, qkv, 3 * dim, M, 3 * dim, dim, s.bb));
}

// Attention of a block on one device.  Returns its output (M, dim), taken from the arena like q | k | v below it.
void* attention_whole(Step& s, const Block& blk, const void* w_qkv, int stage, const void* a_in, int64_t Ls) {
  Arena& A = s.m.arena;
  const int dim = blk.dim;
  const int64_t M = s.B * Ls;
  void* qkv = A.take((size_t)M * 3 * dim * s.es);
  const int64_t plane_stride = s.bf && s.m.qkv_planes ? M * 192 : 0;   // elements
  qkv_linear(s, blk, a_in, w_qkv, qkv, plane_stride, M);
  const DevTables& tb = tables_for(s.m, stage, blk.shifted);
  void* ao = A.take((size_t)M * dim * s.es);
  window_attention(s, blk, qkv, plane_stride, ao, (const int32_t*)tb.tok.p, tb.has_grp ? (const uint8_t*)tb.grp.p : nullptr, tb.n_windows,
                   tb.n_tok, Ls, Ls);
  return ao;
}

// A band, ahead of its qkv GEMM: pack the halo rows and post the exchange.
// What travels is the INPUT of the block, not k | v: the halo rows' activations (dim wide: half the bytes of k | v, a third
// of q | k | v) leave before this rank's own qkv GEMM is even launched, so the transfer has that GEMM and the interior
// windows to hide under; the receiver projects the halo rows to k | v itself (a small GEMM straight into the halo region
// of `qkv`: no placement copy).  A halo row is only ever a key / value -- its own rank computes its queries.
void post_halo(Step& s, const DevPlan& pl, const void* a_in, int dim) {
  Model& m = s.m;
  void* stream = s.L.stream;
  const int64_t row_bytes = (int64_t)dim * s.es;
  const int n_send = pl.send_cnt[0] + pl.send_cnt[1], n_recv = pl.recv_cnt[0] + pl.recv_cnt[1];
  REQUIRE(m.dry || (std::max(n_send, n_recv) * row_bytes <= m.staging_bytes && m.stage_send && m.stage_recv),
          "band staging buffers are missing or too small");
  if (n_send > 0)   // one launch packs the rows for both neighbours: the previous rank's first, the next rank's behind
    timed(m, stream, K_GATHER, 0.0, [&] {
      return aurora_hip_gather_rows(a_in, row_bytes, (const int32_t*)pl.send_idx.p, m.stage_send, row_bytes, n_send, row_bytes, stream);
    });
  aurora_hip_halo_msg sends[2], recvs[2];
  int ns = 0, nr = 0;
  for (int side = 0; side < 2; ++side) {
    const int peer = side == 0 ? s.rank - 1 : s.rank + 1;
    if (pl.send_cnt[side] > 0)
      sends[ns++] = aurora_hip_halo_msg{peer, 0, (side == 0 ? 0 : pl.send_cnt[0]) * row_bytes, pl.send_cnt[side] * row_bytes};
    if (pl.recv_cnt[side] > 0)
      recvs[nr++] = aurora_hip_halo_msg{peer, 0, (side == 0 ? 0 : pl.recv_cnt[0]) * row_bytes, pl.recv_cnt[side] * row_bytes};
  }
  if (!m.dry) {
    const int rc = m.band.post(m.band.user, sends, ns, recvs, nr, stream);
    REQUIRE(rc == 0, "the host's halo `post` callback failed (%d)", rc);
  }
}

// A band, behind its qkv GEMM: wait for the halo rows, project them to k | v, attend.
// The halo rows were posted ahead of the qkv GEMM, so the transfer has that whole GEMM to hide under.  By default ALL
// windows then run in one launch behind the halo projection: a band's interior / boundary launches are latency-bound
// (~15 us each for a few hundred workgroups), two of them cost a rank 0.4 ms per step.  `split_attention`
// (AURORA_BAND_SPLIT_ATTENTION=1 at creation) keeps the interior windows as a launch of their own in front of `wait`, for
// transports that need those extra microseconds of cover.
void attend_behind_halo(Step& s, const Block& blk, const DevPlan& pl, const void* w_qkv, char* qkv, int64_t plane_stride, void* ao,
                        int64_t Ls, int64_t Lq) {
  Model& m = s.m;
  const int dim = blk.dim;
  const size_t es = s.es;
  const int32_t* tok = (const int32_t*)pl.tok.p;
  const uint8_t* grp = pl.has_grp ? (const uint8_t*)pl.grp.p : nullptr;
  const int w0 = (m.split_attention && pl.n_interior > 0) ? pl.n_interior : 0;
  if (w0 > 0) window_attention(s, blk, qkv, plane_stride, ao, tok, grp, w0, pl.n_tok, Lq, Ls);
  if (!m.dry) {
    const int rc = m.band.wait(m.band.user, s.L.stream);
    REQUIRE(rc == 0, "the host's halo `wait` callback failed (%d)", rc);
  }
  // k | v of the received rows: rows [dim, 3 dim) of the qkv weight, written into columns [dim, 3 dim) of the halo rows
  const char* w_kv = (const char*)w_qkv + (size_t)dim * dim * es;
  const int n_recv = pl.recv_cnt[0] + pl.recv_cnt[1];
  const int first = pl.recv_cnt[0] > 0 ? pl.recv_off[0] : pl.recv_off[1];   // the two neighbours' halo rows are adjacent
  if (n_recv > 0 && s.bf && m.qkv_planes)   // k | v of rows Ls + first ... of every head's plane (64 elements into the row: behind q)
    s.L.linear_planes(m.stage_recv, dim, w_kv, dim, blk.qkv_b + dim, qkv + ((size_t)(Ls + first) * 192 + 64) * es, plane_stride,
                      blk.heads, n_recv, 2 * dim, dim);
  else if (n_recv > 0)
    s.L.linear(LinearOp(m.stage_recv, dim, w_kv, dim, blk.qkv_b + dim, qkv + ((size_t)(Ls + first) * 3 * dim + dim) * es, 3 * dim, n_recv,
                        2 * dim, dim, s.bb));
  if (pl.n_windows > w0)
    window_attention(s, blk, qkv, plane_stride, ao, tok + (size_t)w0 * pl.n_tok, grp ? grp + (size_t)w0 * pl.n_tok : nullptr,
                     pl.n_windows - w0, pl.n_tok, Lq, Ls);
}

// Attention of a block on a latitude band: the attention table indexes [own rows | halo rows]; outputs are written for
// owned tokens only.  Returns its output (M, dim), taken from the arena like q | k | v below it.
void* attention_band(Step& s, const Block& blk, const void* w_qkv, int stage, const void* a_in, int64_t Ls) {
  Arena& A = s.m.arena;
  const int dim = blk.dim;
  const int64_t M = s.B * Ls;
  const bool planes = s.bf && s.m.qkv_planes;
  const DevPlan& pl = plan_for(s.m, stage, blk.shifted);
  REQUIRE(pl.n_own == Ls, "band plan of stage %d holds %d rows, the step %lld", stage, pl.n_own, (long long)Ls);
  const int64_t Lq = Ls + pl.n_halo;
  char* qkv = (char*)A.take((size_t)Lq * 3 * dim * s.es);
  REQUIRE(!planes || s.B == 1, "a latitude band runs one batch element");
  const int64_t plane_stride = planes ? Lq * 192 : 0;   // elements
  void* ao = A.take((size_t)M * dim * s.es);
  const bool exchange = pl.n_halo > 0 || pl.send_cnt[0] > 0 || pl.send_cnt[1] > 0;
  if (exchange) post_halo(s, pl, a_in, dim);
  qkv_linear(s, blk, a_in, w_qkv, qkv, plane_stride, M);
  if (exchange)
    attend_behind_halo(s, blk, pl, w_qkv, qkv, plane_stride, ao, Ls, Lq);
  else
    window_attention(s, blk, qkv, plane_stride, ao, (const int32_t*)pl.tok.p, pl.has_grp ? (const uint8_t*)pl.grp.p : nullptr,
                     pl.n_windows, pl.n_tok, Lq, Ls);
  return ao;
}

// One Swin block of `stage` on the residual stream xf (and its bf16 shadow xb): attention, proj + AdaLN, fc1, fc2 + AdaLN.
// `final_out`: where the block's result goes instead of xf (leading dimension final_ld; no shadow then).
void block(Step& s, const Block& blk, const void* w_qkv, const void* w_proj, int stage, float* xf, void* xb, float* final_out,
           int64_t final_ld) {
  Model& m = s.m;
  Launcher& L = s.L;
  Arena& A = m.arena;
  const Res res = s.local_res(stage);
  const int64_t Ls = (int64_t)res.c * res.h * res.w, M = (int64_t)s.B * Ls;
  const int dim = blk.dim, bb = s.bb;
  const size_t es = s.es;
  const void* a_in = s.bf ? xb : (const void*)xf;
  const size_t mark = A.top;
  void* ao = s.sharded ? attention_band(s, blk, w_qkv, stage, a_in, Ls) : attention_whole(s, blk, w_qkv, stage, a_in, Ls);
  // D = 512 under autocast: the linear, its AdaLN and the residual add are ONE launch (a workgroup owns whole rows)
  // m.fuse_ln (AURORA_FUSE_LN when the handle was created): 0 never, 1 (default) by the fill rule below, 2 always
  const int fuse_env = m.fuse_ln;
  // (a row-owning tile is 128 rows: only when the launch fills its rounds of one tile per CU -- a latitude band's
  // 270 tiles on 256 CUs would take two rounds for the work of 1.05)
  const int64_t ln_tiles = (M + 127) / 128, cus = device_cus();
  const bool fills = (double)ln_tiles >= 0.85 * (double)(((ln_tiles + cus - 1) / cus) * cus);
  const bool fuse = s.bf && dim == 512 && (fuse_env == 2 || (fuse_env == 1 && fills));
  auto fused = [&](const void* a, const void* w, const float* bias, int K_, const float* gain, const float* shift, float* xo,
                   int64_t ldo, void* xbo) {
    timed(m, L.stream, K_LINEAR_LN, 2.0 * (double)M * dim * K_, [&] {
      return aurora_hip_linear_layernorm(a, K_, w, K_, bias, gain, shift, xf, dim, xo, ldo, xbo, dim, M, dim, K_, 1e-5f, L.stream);
    });
  };
  if (fuse) {
    fused(ao, w_proj, blk.proj_b, dim, blk.gain1, blk.shift1, xf, dim, xb);
  } else {
    void* y = A.take((size_t)M * dim * es);
    L.linear(LinearOp(ao, dim, w_proj, dim, blk.proj_b, y, dim, M, dim, dim, bb));
    L.layernorm(y, dim, blk.gain1, blk.shift1, xf, dim, 0, xf, dim, xb, dim, M, dim, 1e-5f, bb);
  }
  A.top = mark;
  void* hid = A.take((size_t)M * blk.hidden * es);
  L.linear(LinearOp(a_in, dim, blk.fc1_w, dim, blk.fc1_b, hid, blk.hidden, M, blk.hidden, dim, bb).activation(AURORA_ACT_GELU));
  float* xo = final_out ? final_out : xf;
  const int64_t ldo = final_out ? final_ld : dim;
  void* xbo = final_out ? nullptr : xb;
  if (fuse) {
    fused(hid, blk.fc2_w, blk.fc2_b, blk.hidden, blk.gain2, blk.shift2, xo, ldo, xbo);
  } else {
    void* y2 = A.take((size_t)M * dim * es);
    L.linear(LinearOp(hid, blk.hidden, blk.fc2_w, blk.hidden, blk.fc2_b, y2, dim, M, dim, blk.hidden, bb));
    L.layernorm(y2, dim, blk.gain2, blk.shift2, xf, dim, 0, xo, ldo, xbo, dim, M, dim, 1e-5f, bb);
  }
  A.top = mark;
}

// Patch merging behind stage i: the residual stream moves to the coarser grid (xf / xb then point at the new buffers).
void merge_stage(Step& s, int i, float*& xf, void*& xb) {
  Model& m = s.m;
  Arena& A = m.arena;
  const Res g = m.stage_res[i], r = s.local_res(i);
  REQUIRE(g.h > 1 && g.w > 1, "grid (%d, %d, %d) too small to merge", g.c, g.h, g.w);
  const int dim = m.stage_dim(i);
  const int H2 = (r.h + 1) / 2, W2 = (r.w + 1) / 2;
  REQUIRE(H2 == s.local_res(i + 1).h, "band rows of stages %d / %d do not nest", i, i + 1);
  const int64_t M2 = (int64_t)s.B * r.c * H2 * W2;
  float* nf = (float*)A.take((size_t)M2 * 2 * dim * 4);
  void* nb = s.bf ? A.take((size_t)M2 * 2 * dim * 2) : nullptr;
  const size_t mark = A.top;
  void* mg = A.take((size_t)M2 * 4 * dim * s.es);
  timed(m, s.L.stream, K_MERGE_LN, 0.0, [&] {
    return aurora_hip_merge_ln(xf, m.merges[i].ln_w, m.merges[i].ln_b, mg, s.B, r.c, r.h, r.w, dim, 1e-5f, s.bb, s.L.stream);
  });
  LinearOp reduce(mg, 4 * dim, m.merges[i].w, 4 * dim, nullptr, s.bf ? nb : (void*)nf, 2 * dim, M2, 2 * dim, 4 * dim, s.bb);
  if (s.bf) reduce.second_output(nf, 2 * dim);
  s.L.linear(reduce);
  A.top = mark;
  xf = nf;
  xb = nb;
}

// Patch splitting behind decoder layer i (stage idx = n - 1 - i): the residual stream moves to the finer grid.
void split_stage(Step& s, int i, const std::vector<float*>& skips, float*& xf, void*& xb) {
  Model& m = s.m;
  Arena& A = m.arena;
  const int n = m.n_stages, idx = n - 1 - i, B = s.B;
  const Res r = s.local_res(idx);
  const int dim = m.stage_dim(idx);
  const void* a_in = s.bf ? xb : (const void*)xf;
  // the odd bottom row of the finer stage belongs to the last band only
  const int crop_h = (s.sharded && s.rank != s.world - 1) ? 0 : m.merge_pad[idx - 1][0], crop_w = m.merge_pad[idx - 1][1];
  const int Ho = 2 * r.h - crop_h, Wo = 2 * r.w - crop_w;
  REQUIRE(Ho == s.local_res(idx - 1).h && Wo == s.local_res(idx - 1).w, "band rows of stages %d / %d do not nest", idx - 1, idx);
  const int64_t M1 = (int64_t)B * r.c * r.h * r.w, M2 = (int64_t)B * r.c * Ho * Wo;
  float* nf = (float*)A.take((size_t)M2 * (dim / 2) * 4);
  void* nb = s.bf ? A.take((size_t)M2 * (dim / 2) * 2) : nullptr;
  const size_t mark = A.top;
  void* y1 = A.take((size_t)M1 * 2 * dim * s.es);
  s.L.linear(LinearOp(a_in, dim, m.splits[i].w1, dim, nullptr, y1, 2 * dim, M1, 2 * dim, dim, s.bb));
  void* sp = A.take((size_t)M2 * (dim / 2) * s.es);
  timed(m, s.L.stream, K_SPLIT_LN, 0.0, [&] {
    return aurora_hip_split_ln(y1, m.splits[i].ln_w, m.splits[i].ln_b, sp, B, r.c, r.h, r.w, dim / 2, crop_h, crop_w, 1e-5f, s.bb,
                               s.L.stream);
  });
  // additive skip after the intermediate decoder stages (swin3d.py:930-932)
  const float* res_ = (i > 0 && i < n - 1) ? skips[idx - 1] : nullptr;
  LinearOp expand(sp, dim / 2, m.splits[i].w2, dim / 2, nullptr, s.bf ? nb : (void*)nf, dim / 2, M2, dim / 2, dim / 2, s.bb);
  if (s.bf) expand.second_output(nf, dim / 2);
  s.L.linear(expand.residual(res_, dim / 2));
  A.top = mark;
  xf = nf;
  xb = nb;
}

// ================= decoder (decoder.py:168-276) =================
// An output variable with every optional feature off (engine/lib.py:unpatch_var): plain de-normalisation of head column col0.
aurora_unpatch_var plain_unpatch(float* dst, const float* loc, int n_lvl, bool clamp_min0, int col0) {
  aurora_unpatch_var d{};
  d.dst = dst; d.loc = loc; d.scale = loc + n_lvl; d.clamp_min0 = clamp_min0; d.col0 = col0;
  d.mod_col0 = d.angle_col0 = d.dens_col0 = -1;
  return d;
}

// difference prediction (aurora.py:761-779): y + (1 + y_mod) * normalised previous state of the same variable
void diff_fields(const Step& s, aurora_unpatch_var& d, const std::string& name, const std::vector<std::string>& heads, bool atmos,
                 int src, int n_lvl) {
  const Model& m = s.m;
  const aurora_hip_step_io& io = s.io;
  const auto it = m.diff_index.find(name);
  const int mod = index_of(heads, name + "_mod");
  if (m.variant != 1 || it == m.diff_index.end() || mod < 0) return;
  d.mod_col0 = mod * s.PP;
  const int idx = it->second;
  if (atmos) {
    d.prev = io.atmos[src] + (int64_t)idx * io.atmos_strides[1];
    d.prev_sb = io.atmos_strides[0]; d.prev_sc = io.atmos_strides[2]; d.prev_sh = io.atmos_strides[3];
    REQUIRE(io.atmos_strides[4] == 1, "difference prediction needs unit longitude stride");
  } else {
    d.prev = io.surf[src] + (int64_t)idx * io.surf_strides[1];
    d.prev_sb = io.surf_strides[0]; d.prev_sc = 0; d.prev_sh = io.surf_strides[2];
    REQUIRE(io.surf_strides[3] == 1, "difference prediction needs unit longitude stride");
  }
  REQUIRE(idx < s.T, "difference prediction of '%s' refers to history index %d, %d states given", name.c_str(), idx, s.T);
  d.inv_scale = d.loc + 2 * n_lvl;
}

// unpatchify descriptor of surface output `v` (surface input `src`), decoded from the heads `hs`
aurora_unpatch_var surf_unpatch(const Step& s, const HeadGroup& hs, size_t v, int src) {
  const Model& m = s.m;
  const aurora_hip_step_io& io = s.io;
  const std::string& name = m.surf_out[v];
  aurora_unpatch_var d = plain_unpatch(io.out_surf[v], m.stats.f() + m.surf_stat_off[src], 1, s.clamp_now && index_of(m.pos_surf, name) >= 0, 0);
  const int plain = index_of(hs.names, name);
  if (m.variant == 2 && plain < 0) {   // a direction: atan2 of its sin / cos heads (aurora.py:914-932)
    d.col0 = index_of(hs.names, name + "_sin") * s.PP;
    d.angle_col0 = index_of(hs.names, name + "_cos") * s.PP;
  } else {
    REQUIRE(plain >= 0, "no decoder head for '%s'", name.c_str());
    d.col0 = plain * s.PP;
  }
  diff_fields(s, d, name, hs.names, false, src, 1);
  const int dens = m.variant == 2 ? index_of(hs.names, name + "_density") : -1;
  if (dens >= 0) {   // keep the value only over water and where the density head says "present"
    const int wmb = index_of(m.static_vars, "wmb");
    REQUIRE(wmb >= 0 && io.stat && io.stat[wmb], "the ocean-wave variant needs the static variable 'wmb'");
    REQUIRE(io.static_strides[1] == 1, "the water-body mask needs unit longitude stride");
    d.dens_col0 = dens * s.PP;
    d.mask = io.stat[wmb];
    d.mask_sh = io.static_strides[0];
    d.mask_thresh = (float)m.static_loc[wmb];   // normalised value > 0
  }
  return d;
}

// unpatchify descriptor of atmospheric variable `v`, decoded from head `hi` of the group `hg`
aurora_unpatch_var atmos_unpatch(const Step& s, const HeadGroup& hg, size_t hi, int v) {
  const Model& m = s.m;
  const std::string& name = hg.names[hi];
  aurora_unpatch_var d = plain_unpatch(s.io.out_atmos[v], m.stats.f() + m.atmos_stat_off[v], s.C,
                                       s.clamp_now && index_of(m.pos_atmos, name) >= 0, (int)hi * s.PP);
  diff_fields(s, d, name, hg.names, true, v, s.C);
  if (m.variant == 1 && m.use_lora && name == "so2")   // aurora.py:781-794
    for (int c = 0; c < s.C; ++c)
      if (m.levels[c] >= 850) d.clamp_max1_levels |= 1u << c;
  return d;
}

// ---- surface heads on latent level 0, and their unpatchify ----
void decode_surface(Step& s, const float* x_cat) {
  Model& m = s.m;
  const int B = s.B, D2 = 2 * s.D;
  const int64_t Lp = s.Lp;
  const HeadGroup& hs = m.head_surf;
  const int n_s = (int)hs.names.size() * s.PP, ld_s = round_up(n_s, 4);
  float* y_s = (float*)m.arena.take((size_t)B * Lp * ld_s * 4);
  for (int b = 0; b < B; ++b)
    s.L.linear(LinearOp(x_cat + (size_t)b * s.Cl * Lp * D2, D2, hs.w.f(), D2, hs.b.f(), y_s + (size_t)b * Lp * ld_s, ld_s, Lp, n_s, D2,
                        AURORA_F32));
  std::vector<aurora_unpatch_var> ud;
  for (size_t v = 0; v < m.surf_out.size(); ++v) {
    const int src = index_of(m.surf_inputs, m.surf_out[v]);
    REQUIRE(src >= 0, "surface output '%s' is not a surface input", m.surf_out[v].c_str());
    if (s.io.out_surf[v] == nullptr || s.io.surf[src] == nullptr) continue;
    ud.push_back(surf_unpatch(s, hs, v, src));
  }
  in_launches_of_32(s, K_UNPATCHIFY, ud, [&](const aurora_unpatch_var* d, int n, int) {
    return aurora_hip_unpatchify(y_s, ld_s, d, n, B, 1, s.Hp, s.Wp, s.P, s.L.stream);
  });
}

// One Perceiver group of the level de-aggregation: resampler -> heads (one strided-batch launch over the levels when every
// level has its own head, levelcond.py:36-69) -> unpatchify with the post-decoder hooks fused.
void decode_group(Step& s, const HeadGroup& hg, const Resampler& rs, const float* q, float out_bound, bool scan_ctx, const float* ctx) {
  Model& m = s.m;
  const int B = s.B, C = s.C, Cl = s.Cl, D2 = 2 * s.D;
  const int64_t Lp = s.Lp;
  const size_t gmark = m.arena.top;
  // The output heads have few columns (80 at patch size 4, 500 at 10): on the native-fp32 128 x 128 kernel they ran at
  // 77 TFLOP/s.  When the Perceiver's output is bounded inside fp16's range by its LayerNorm parameters alone (it is: a few
  // hundred), its last LayerNorm writes fp16 pairs and the heads -- rows zero-padded to the 256-column tile, weights
  // pre-split -- run on the VALU-free two-term kernel instead.
  const auto& last_ly = rs.layers.back();
  const bool last_pairs = last_ly.fc1_s && last_ly.fc2_s && last_ly.dim % 32 == 0;
  const bool two_term = hg.n_pad > 0 && last_pairs && out_bound < F16_SAFE;
  // one query per level and column over the Cl - 1 latent levels, latent level j of column (b, l) at row b (Cl - 1) Lp + j Lp + l
  ResamplerCall call{};
  call.rs = &rs;
  call.ctx = ctx;
  call.ctx_rows = (int64_t)B * (Cl - 1) * Lp;
  call.ctx_dim = D2;
  call.q0 = q;
  call.latents0 = m.dec_queries.f();
  call.g.B = B; call.g.cols = Lp; call.g.kv_bstride = (int64_t)(Cl - 1) * Lp; call.g.kv_lstride = Lp;
  call.g.Lq = C; call.g.Lk = Cl - 1; call.g.heads = m.perceiver_heads;
  call.eps = m.ln_eps;
  call.out_pairs = two_term;
  call.front = nullptr;
  // (of the two decoder Perceivers of a `separate_perceiver` model only the first scans their common context: `scan_ctx`)
  call.guard = CtxGuard{m.ctx_max.f() + 3, 1.0f, 0.0f, F16_SAFE, false, scan_ctx};
  float* lat = resampler(m, s.L, call);
  const int n_a = two_term ? hg.n_pad : (int)hg.names.size() * s.PP, ld_a = round_up(n_a, 4);
  const float* hw = two_term ? (const float*)hg.ws.p : hg.w.f();
  const float* hb = two_term ? hg.bs.f() : hg.b.f();
  const int mode = two_term ? (2 | AURORA_F32_A_SPLIT | AURORA_F32_W_SPLIT) : -1;
  float* y_a = (float*)m.arena.take((size_t)B * Lp * C * ld_a * 4);
  if (hg.groups > 1)   // level c: rows (b L + l) C + c of `lat` -> the same rows of y_a, with that level's head
    s.L.linear(LinearOp(lat, (int64_t)C * D2, hw, D2, hb, y_a, (int64_t)C * ld_a, (int64_t)B * Lp, n_a, D2, AURORA_F32)
                   .f32_mode(mode).batched(C, D2, (int64_t)n_a * D2, ld_a, ld_a));
  else
    s.L.linear(LinearOp(lat, D2, hw, D2, hb, y_a, ld_a, (int64_t)B * Lp * C, n_a, D2, AURORA_F32).f32_mode(mode));
  std::vector<aurora_unpatch_var> ad;
  for (size_t hi = 0; hi < hg.names.size(); ++hi) {
    const int v = index_of(m.atmos_vars, hg.names[hi]);
    if (v < 0) continue;               // a `<v>_mod` head: consumed by its base variable
    if (s.io.out_atmos[v] == nullptr || s.io.atmos[v] == nullptr) continue;
    ad.push_back(atmos_unpatch(s, hg, hi, v));
  }
  in_launches_of_32(s, K_UNPATCHIFY, ad, [&](const aurora_unpatch_var* d, int n, int) {
    return aurora_hip_unpatchify(y_a, ld_a, d, n, B, C, s.Hp, s.Wp, s.P, s.L.stream);
  });
  m.arena.top = gmark;
}

// ---- level de-aggregation: the main Perceiver decodes every variable except those named in `separate_perceiver`, which
// get their own (decoder.py:232-248) ----
void decode_levels(Step& s, const float* x_cat) {
  Model& m = s.m;
  const int B = s.B, Cl = s.Cl, D2 = 2 * s.D;
  const int64_t Lp = s.Lp;
  const float* ctx = x_cat + (size_t)Lp * D2;
  if (B > 1) {   // latent levels 1.. of every batch element, made contiguous
    float* ctx_copy = (float*)m.arena.take((size_t)B * (Cl - 1) * Lp * D2 * 4);
    for (int b = 0; b < B; ++b)
      timed(m, s.L.stream, K_COPY2D, 0.0, [&] {
        return aurora_hip_copy2d(x_cat + ((size_t)b * Cl * Lp + Lp) * D2, D2, ctx_copy + (size_t)b * (Cl - 1) * Lp * D2, D2,
                                 (int64_t)(Cl - 1) * Lp, D2, AURORA_F32, s.L.stream);
      });
    ctx = ctx_copy;
  }
  if (!m.head_main.names.empty()) decode_group(s, m.head_main, m.dec_rs, m.dec_q.f(), m.dec_out_bound, true, ctx);
  if (m.has_alt && !m.head_alt.names.empty())   // (only the first Perceiver that runs scans their common context)
    decode_group(s, m.head_alt, m.dec_rs_alt, m.dec_q_alt.f(), m.dec_out_bound_alt, m.head_main.names.empty(), ctx);
}

}  // namespace

void run_step(Model& m, const StepIO& sio, void* stream) {
  const aurora_hip_step_io& io = *sio.io;
  const int new_step = io.rollout_step + 1;
  Step s{m, Launcher{m, stream}, io, sio.B, sio.T, m.P, m.D, m.Hp, m.Wp, m.Cl, m.n_levels, m.P * m.P, (int64_t)m.Hp * m.Wp,
         m.sharded(), m.band.rank, m.band.world,
         /*clamp_now=*/m.clamp_first ? new_step >= 1 : new_step > 1,   // aurora.py:368-388
         m.autocast, m.bb(), m.bbs()};
  Arena& A = m.arena;
  A.top = 0;
  const int B = s.B, D = s.D, n = m.n_stages;
  const int64_t L0 = (int64_t)s.Cl * s.Lp;
  // the four guard words of the step's operand-split decisions (0: encoder context when it is not part of the guarded
  // chain, 1: atmospheric / 2: surface patch-embedding inputs, 3: decoder context), cleared by ONE launch; their producers
  // fold the maxima in (patchify) or scan (absmax_fold)
  if (!m.dry) ok(aurora_hip_zero_words(m.ctx_max.f(), 4, stream));
  if (!m.dry)   // (what aurora_hip_guard_limits reports: of this step alone)
    for (int i = 0; i < 4; ++i) { m.guard_limit_min[i] = INFINITY; m.guard_launches[i] = 0; }

  // ================= encoder (encoder.py:198-366) =================
  float* xf = (float*)A.take((size_t)B * L0 * D * 4);                      // residual stream of stage 0 (fp32)
  void* xb = s.bf ? A.take((size_t)B * L0 * D * 2) : nullptr;              // bf16 shadow (GEMM operand)
  const size_t after_x = A.top;
  const float* xs1 = encode_surface(s);
  const float* lat = encode_levels(s);
  assemble(s, xs1, lat, xf, xb);
  A.top = after_x;   // every encoder temporary is dead

  // ================= backbone (swin3d.py:884-936) =================
  const AttnSet& aw = attn_weights(m, lora_key(m, io.rollout_step), stream);
  // x_cat (B*L0, 2*D0): decoder output | encoder stage-0 output -- allocated now so that it survives the stack
  float* x_cat = (float*)A.take((size_t)B * L0 * 2 * D * 4);
  std::vector<float*> skips;
  size_t bi = 0;
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < m.enc_depths[i]; ++k, ++bi) block(s, m.blocks[bi], aw.qkv[bi], aw.proj[bi], i, xf, xb, nullptr, 0);
    skips.push_back(xf);
    if (i < n - 1) merge_stage(s, i, xf, xb);
  }
  for (int i = 0; i < n; ++i) {
    const bool last_layer = i == n - 1;
    for (int k = 0; k < m.dec_depths[i]; ++k, ++bi)   // the last block of all writes the left half of x_cat
      block(s, m.blocks[bi], aw.qkv[bi], aw.proj[bi], n - 1 - i, xf, xb, last_layer && k == m.dec_depths[i] - 1 ? x_cat : nullptr, 2 * D);
    if (last_layer && m.dec_depths[i] == 0 && !m.dry) ok(aurora_hip_copy2d(xf, D, x_cat, 2 * D, (int64_t)B * L0, D, AURORA_F32, stream));
    if (i < n - 1) split_stage(s, i, skips, xf, xb);
  }
  timed(m, stream, K_COPY2D, 0.0, [&] { return aurora_hip_copy2d(skips[0], D, x_cat + D, 2 * D, (int64_t)B * L0, D, AURORA_F32, stream); });

  // ================= decoder (decoder.py:168-276) =================
  const size_t mark = A.top;
  decode_surface(s, x_cat);
  decode_levels(s, x_cat);
  A.top = mark;
}

}  // namespace aurora
