// The model handle of libaurora_hip.so: what depends on the parameters only -- aurora_hip_pack_weights and the packed-file
// format, the compute-dtype copies, LoRA merges and GEMM layouts of the weights, the bounds that feed the device-side range
// guards, and aurora_hip_finalize.  Host code only; every launch goes through the operator ABI of this same library.
#include "model.h"

namespace aurora {

constexpr int LORA_RANK = 8;

// ---- bounds for the range guards -------------------------------------------------------------------
float absmax(const std::vector<float>& h) {
  float mx = 0.f;
  for (float v : h) mx = std::max(mx, fabsf(v));
  return mx;
}
float absmax(const float* dev, size_t n) { return absmax(to_host(dev, n)); }
float max_row_l1(const std::vector<float>& h, int64_t rows, int64_t K, float floor) {
  float best = floor;
  for (int64_t r = 0; r < rows; ++r) {
    float sum = 0.f;
    for (int64_t k = 0; k < K; ++k) sum += fabsf(h[(size_t)r * K + k]);
    best = std::max(best, sum);
  }
  return best;
}

// ---- the fp16-pair form of a weight ----------------------------------------------------------------
// The linears refuse fp16-pair operands unless N % 128 == 0, K % 32 == 0 and K >= 96 (gemm.hip: check_call on `pre`, and
// `f32pp` of the plan after it).  `row_multiple` is the caller's rule for N: 128, or coarser where a site always was.
bool presplit_shape(int64_t rows, int64_t K, int row_multiple) { return rows % row_multiple == 0 && K % 32 == 0 && K >= 96; }
DevBuf presplit(const float* w, int64_t rows, int64_t K, int64_t ld, int row_multiple, int groups) {
  if (!presplit_shape(rows, K, row_multiple)) return DevBuf();
  DevBuf s((size_t)groups * rows * K * 4);
  ok(aurora_hip_split_f16(w, ld, s.p, K, groups * rows, (int)K, 64.0f, nullptr));
  hip_ok(hipDeviceSynchronize(), "split weights");
  return s;
}

namespace {

// A backbone weight in the compute dtype: the fp32 master itself (autocast off), the bf16 entry of a packed file, or a
// bf16 copy of the master made once.  `out_shape0` receives the leading dimension (hidden sizes are read off weights).
const void* compute_weight(Model& m, const std::string& name, void* stream, int64_t* out_shape0 = nullptr) {
  auto h = m.w16.find(name);
  if (h != m.w16.end()) {
    REQUIRE(m.autocast, "'%s' is stored in bf16 only: this packed file serves autocast (bf16 backbone) models", name.c_str());
    if (out_shape0) *out_shape0 = h->second.shape[0];
    return h->second.buf.p;
  }
  const Tensor& t = m.T_(name);
  if (out_shape0) *out_shape0 = t.shape[0];
  if (!m.autocast) return t.f();
  DevBuf b((size_t)t.numel * 2);
  ok(aurora_hip_convert(t.f(), b.p, t.numel, AURORA_F32, stream));
  m.keep.push_back(std::move(b));
  return m.keep.back().p;
}

Resampler pack_resampler(Model& m, const std::string& prefix, int depth, int heads) {
  Resampler r;
  for (int i = 0; i < depth; ++i) {
    const std::string p = prefix + ".layers." + std::to_string(i);
    Resampler::Layer l{};
    l.to_q = m.W(p + ".0.to_q.weight"); l.to_kv = m.W(p + ".0.to_kv.weight"); l.to_out = m.W(p + ".0.to_out.weight");
    l.fc1_w = m.W(p + ".1.net.0.weight"); l.fc1_b = m.W(p + ".1.net.0.bias");
    l.fc2_w = m.W(p + ".1.net.2.weight"); l.fc2_b = m.W(p + ".1.net.2.bias");
    l.ln1_w = m.W(p + ".2.weight"); l.ln1_b = m.W(p + ".2.bias");
    l.ln2_w = m.W(p + ".3.weight"); l.ln2_b = m.W(p + ".3.bias");
    if (m.has(p + ".0.ln_k.weight")) {
      l.ln_k_w = m.W(p + ".0.ln_k.weight"); l.ln_k_b = m.W(p + ".0.ln_k.bias");
      l.ln_q_w = m.W(p + ".0.ln_q.weight"); l.ln_q_b = m.W(p + ".0.ln_q.bias");
    }
    const Tensor& tkv = m.T_(p + ".0.to_kv.weight");
    l.inner = (int)m.T_(p + ".0.to_q.weight").shape[0];
    l.head_dim = l.inner / heads;
    l.hidden = (int)m.T_(p + ".1.net.0.weight").shape[0];
    l.dim = (int)m.T_(p + ".0.to_out.weight").shape[0];
    l.ctx_dim = (int)tkv.shape[1];
    // largest L1 row norm of the value projection: |v| <= v_l1 * max |context| (range guard of the fp16 operand split)
    const size_t n_v = (size_t)l.inner * l.ctx_dim;
    l.v_l1 = max_row_l1(to_host(tkv.f() + n_v, n_v), l.inner, l.ctx_dim, 1e-6f);
    // The two-term mode assumes |activation| < 65504 as well: only if every weight of the layer stays below the bound and
    // what a LayerNorm output can reach (sqrt(D) max|gain| + max|bias|) stays inside the range.
    const char* const linears[4] = {".0.to_kv.weight", ".0.to_out.weight", ".1.net.0.weight", ".1.net.2.weight"};
    float w_max = 0.f;
    for (const char* nm : linears) w_max = std::max(w_max, absmax(m.T_(p + nm)));
    const float ln_bound = absmax(m.T_(p + ".2.weight")) * sqrtf((float)l.dim) + absmax(m.T_(p + ".2.bias"));
    l.f16_mode = (w_max < PRESPLIT_W_MAX && ln_bound < F16_SAFE) ? bounded_mode() : -1;
    if (l.f16_mode == 2) {
      auto split = [&](const char* nm) -> const void* {
        const Tensor& t = m.T_(p + nm);
        // 256 rows where the kernel asks for 128: historical, kept
        DevBuf s = presplit(t.f(), t.shape[0], t.shape[1], t.shape[1], /*row_multiple=*/256);
        if (!s.p) return nullptr;
        r.own.push_back(std::move(s));
        return r.own.back().p;
      };
      l.to_kv_s = split(linears[0]); l.to_out_s = split(linears[1]); l.fc1_s = split(linears[2]); l.fc2_s = split(linears[3]);
    }
    r.layers.push_back(l);
  }
  return r;
}

// Fused decoder heads of a group of variables: [groups][n * P * P][2D] weights, V fastest inside a patch is handled by
// unpatchify's col0.  groups > 1: one head per pressure level (levelcond.py:36-69).
void build_heads(Model& m, HeadGroup& hg, const char* kind, const std::vector<std::string>& names, bool per_level) {
  const int PP = m.P * m.P, D2 = 2 * m.D;
  hg.names = names;
  hg.groups = per_level ? m.n_levels : 1;
  if (names.empty()) return;
  const size_t ldb = (size_t)round_up((int)names.size() * PP, 4);   // per-group bias rows padded: every group stays 16-byte aligned
  hg.w = DevBuf((size_t)hg.groups * names.size() * PP * D2 * 4);
  hg.b = DevBuf((size_t)hg.groups * ldb * 4);
  hip_ok(hipMemset(hg.b.p, 0, hg.b.bytes), "memset");
  for (int g = 0; g < hg.groups; ++g)
    for (size_t v = 0; v < names.size(); ++v) {
      std::string p = std::string("decoder.") + kind + "_heads." + names[v];
      if (per_level) p += ".layers." + level_to_str(m.levels[g]);
      const Tensor& wt = m.T_(p + ".weight");
      REQUIRE(wt.shape.size() == 2 && wt.shape[0] == PP && wt.shape[1] == D2, "bad head weight shape for %s", p.c_str());
      hip_ok(hipMemcpy(hg.w.f() + ((size_t)g * names.size() + v) * PP * D2, wt.f(), (size_t)PP * D2 * 4, hipMemcpyDeviceToDevice), "copy");
      hip_ok(hipMemcpy(hg.b.f() + (size_t)g * ldb + v * PP, m.W(p + ".bias"), (size_t)PP * 4, hipMemcpyDeviceToDevice), "copy");
    }
  // ---- the two-term form: N padded to whole 128-column tiles of the fp16-pair GEMM (zero rows cost MFMAs, not bytes of A) ----
  hg.n_pad = 0;
  hg.ws = DevBuf(); hg.bs = DevBuf();
  const int n = (int)names.size() * PP, n_pad = round_up(n, 128);   // the tile width of the 256 x 128 two-term kernel
  if (std::string(kind) != "atmos" || bounded_mode() != 2 || !presplit_shape(n_pad, D2, 128)) return;
  if (!(absmax(hg.w.f(), (size_t)hg.groups * n * D2) < PRESPLIT_W_MAX)) return;
  DevBuf padded((size_t)hg.groups * n_pad * D2 * 4);
  hip_ok(hipMemset(padded.p, 0, padded.bytes), "memset");
  hg.bs = DevBuf((size_t)hg.groups * n_pad * 4);
  hip_ok(hipMemset(hg.bs.p, 0, hg.bs.bytes), "memset");
  for (int g = 0; g < hg.groups; ++g) {
    hip_ok(hipMemcpy(padded.f() + (size_t)g * n_pad * D2, hg.w.f() + (size_t)g * n * D2, (size_t)n * D2 * 4, hipMemcpyDeviceToDevice), "copy");
    hip_ok(hipMemcpy(hg.bs.f() + (size_t)g * n_pad, hg.b.f() + (size_t)g * ldb, (size_t)n * 4, hipMemcpyDeviceToDevice), "copy");
  }
  // the kernel's own multiple, not 256: the head columns are few and every zero row costs MFMAs
  hg.ws = presplit(padded.f(), n_pad, D2, D2, /*row_multiple=*/128, hg.groups);
  hg.n_pad = n_pad;
}

}  // namespace

// Scores without a key projection (first layer of a Perceiver: perceiver.py:141-152 with the queries of perceiver.py:224-226 /
// decoder.py:225-231, which are model constants).  q_l . (W_k x) = (W_k^T q_l) . x, so `to_kv` becomes
//   [ W_v  |  one row W_k,h^T q_l,h / sqrt(head_dim) per (query l, head h)  |  zero rows up to a multiple of 256 ]
// -- Lq * heads rows instead of heads * head_dim: 48 instead of 512 in the encoder's level aggregation, 208 instead of 1,024 in
// the decoder's de-aggregation -- and a context row leaves that linear with its values and its SCALED SCORES against every
// query (perceiver_attention.hip: perceiver_attention_scores_kernel; perceiver_out.hip: perceiver_probs_kernel<.., true>).  The rows are
// summed in double on the host (64 terms each) and rounded once.  Not with a LayerNorm on the keys (`ln_k_q`), and only where
// the pre-split form exists iff to_kv's does (a context in the fp16-pair layout needs pre-split weights, step.hip).
void score_weights(Model& m, Resampler& r, const float* q0, int Lq, int heads) {
  r.vs_w = DevBuf();
  r.vs_ws = DevBuf();
  r.n_s = r.n_vs = r.vs_lq = 0;
  if (!m.score_weights || r.layers.empty() || q0 == nullptr) return;
  const auto& l = r.layers[0];
  if (l.ln_k_w != nullptr || l.head_dim * heads != l.inner || l.f16_mode < 0) return;
  const int inner = l.inner, hd = l.head_dim, K = l.ctx_dim, n_s = Lq * heads;
  const int n_vs = round_up(inner + n_s, 256);
  if (n_vs >= 2 * inner) return;   // nothing saved
  std::vector<float> wkv((size_t)2 * inner * K), q((size_t)Lq * inner), vs((size_t)n_vs * K, 0.f);
  hip_ok(hipMemcpy(wkv.data(), l.to_kv, wkv.size() * 4, hipMemcpyDeviceToHost), "download");
  hip_ok(hipMemcpy(q.data(), q0, q.size() * 4, hipMemcpyDeviceToHost), "download");
  std::copy(wkv.begin() + (size_t)inner * K, wkv.end(), vs.begin());   // the value half: rows inner .. 2 inner of to_kv
  const double scale = 1.0 / std::sqrt((double)hd);
  std::vector<double> acc((size_t)K);
  float s_max = 0.f;
  for (int lq = 0; lq < Lq; ++lq)
    for (int h = 0; h < heads; ++h) {
      std::fill(acc.begin(), acc.end(), 0.0);
      for (int d = 0; d < hd; ++d) {
        const double qd = q[(size_t)lq * inner + h * hd + d];
        const float* wr = wkv.data() + (size_t)(h * hd + d) * K;
        for (int c = 0; c < K; ++c) acc[c] += qd * wr[c];
      }
      float* dst = vs.data() + (size_t)(inner + lq * heads + h) * K;
      for (int c = 0; c < K; ++c) {
        dst[c] = (float)(acc[c] * scale);
        s_max = std::max(s_max, fabsf(dst[c]));
      }
    }
  if (!(s_max < PRESPLIT_W_MAX)) return;
  DevBuf w = to_device(vs), ws;
  // rows are padded to 256 above: the context stays as wide as a to_kv that pack_resampler's rule lets through
  if (l.to_kv_s != nullptr && l.f16_mode == 2) ws = presplit(w.f(), n_vs, K, K, /*row_multiple=*/256);
  if ((l.to_kv_s != nullptr) != (ws.p != nullptr)) return;
  r.vs_w = std::move(w); r.vs_ws = std::move(ws);
  r.n_s = n_s; r.n_vs = n_vs; r.vs_lq = Lq;
}

// LoRA-merged attention weights of one roll-out phase: W' = W + B A (rank 8, alpha / r = 1), one small GEMM per weight.
const AttnSet& attn_weights(Model& m, int key, void* stream) {
  auto it = m.attn_sets.find(key);
  if (it != m.attn_sets.end()) return it->second;
  AttnSet set;
  for (const Block& blk : m.blocks) {
    for (int which = 0; which < 2; ++which) {
      const std::string name = blk.prefix + (which == 0 ? ".attn.qkv" : ".attn.proj");
      if (key < 0 && m.w16.count(name + ".weight")) {   // packed bf16 file of a model without LoRA
        (which == 0 ? set.qkv : set.proj).push_back(compute_weight(m, name + ".weight", stream));
        continue;
      }
      const Tensor& wt = m.T_(name + ".weight");
      const int64_t out_f = wt.shape[0], in_f = wt.shape[1];
      const float* src = wt.f();
      DevBuf merged;
      if (key >= 0) {
        const std::string lp = blk.prefix + (which == 0 ? ".attn.lora_qkv.loras." : ".attn.lora_proj.loras.") + std::to_string(key);
        const Tensor& a = m.T_(lp + ".lora_A");   // (r, in)
        const Tensor& b = m.T_(lp + ".lora_B");   // (out, r)
        // operands zero-padded to one 32-wide fp32 K-tile: b_p (out, 32), a_t (in, 32) = A^T
        std::vector<float> ha((size_t)a.numel), hb((size_t)b.numel);
        hip_ok(hipMemcpy(ha.data(), a.f(), ha.size() * 4, hipMemcpyDeviceToHost), "download");
        hip_ok(hipMemcpy(hb.data(), b.f(), hb.size() * 4, hipMemcpyDeviceToHost), "download");
        std::vector<float> at((size_t)in_f * 32, 0.f), bp((size_t)out_f * 32, 0.f);
        for (int r_ = 0; r_ < LORA_RANK; ++r_)
          for (int64_t k = 0; k < in_f; ++k) at[(size_t)k * 32 + r_] = ha[(size_t)r_ * in_f + k];
        for (int64_t o = 0; o < out_f; ++o)
          for (int r_ = 0; r_ < LORA_RANK; ++r_) bp[(size_t)o * 32 + r_] = hb[(size_t)o * LORA_RANK + r_];
        DevBuf d_at = to_device(at), d_bp = to_device(bp);
        merged = DevBuf((size_t)out_f * in_f * 4);
        ok(aurora_hip_linear_ex(d_bp.p, 32, d_at.p, 32, nullptr, merged.p, in_f, nullptr, 0, src, in_f, out_f, (int)in_f, 32,
                                AURORA_F32, AURORA_ACT_NONE, -1, nullptr, 0.f, stream));
        hip_ok(hipStreamSynchronize(as_stream(stream)), "sync");   // d_at / d_bp die here
        src = merged.f();
      }
      const void* use = src;
      if (m.autocast) {
        DevBuf h((size_t)out_f * in_f * 2);
        ok(aurora_hip_convert(src, h.p, out_f * in_f, AURORA_F32, stream));
        hip_ok(hipStreamSynchronize(as_stream(stream)), "sync");
        use = h.p;
        set.own.push_back(std::move(h));
      } else if (key >= 0) {
        set.own.push_back(std::move(merged));
      }
      (which == 0 ? set.qkv : set.proj).push_back(use);
    }
  }
  // "all" mode: keep base + the three most recent sets
  while (m.attn_sets.size() > 3) {
    bool erased = false;
    for (auto jt = m.attn_sets.begin(); jt != m.attn_sets.end(); ++jt)
      if (jt->first != -1) { m.attn_sets.erase(jt); erased = true; break; }
    if (!erased) break;
  }
  return m.attn_sets.emplace(key, std::move(set)).first->second;
}

// ---- the encoder front composed: patch embedding folded into the level aggregation's context linears ----------------
// Upstream the atmospheric embedding x = A W_e^T + b_e + level_embed[c] (encoder.py:305-326) is read by the level aggregation
// alone (encoder.py:329), whose first operation on it is the bias-free `to_kv` (perceiver.py:117,142; `ln_k` comes behind the
// projection).  Nothing nonlinear stands between the two, so for level c
//   kv = A (W_ctx W_e[c])^T + W_ctx (b_e + level_embed[c])
// with W_ctx what the layer multiplies its context by: [W_v | score rows] of score_weights, or to_kv.  One GEMM of K = Kpad
// remains where a K = Kpad and a K = D one ran, and the embeddings (C B Lp rows of D) are neither written nor read.
//
// Worth it only where the composed linears do clearly less work than the two stages they replace: sum_i Kpad N_i against
// Kpad D + sum_i D N_i multiply-adds per context row.  The margin is a factor of two: the composed launch splits its fp32
// activation operand in the kernel (0.29 against 0.40 PFLOP/s for operands that arrive split), so at equal work
// it would be the slower one, and it has to stay bound by its output store as the stages it replaces are.  Patch size 4
// (Kpad 160, D 512, N 768) has 0.26 of the work and composes; patch size 10 (Kpad 1000) has 0.85 and keeps the two stages.
bool compose_front_rule(int Kpad, int D, const int* N, int n_layers) {
  if (Kpad <= 0 || D <= 0 || n_layers <= 0) return false;
  double composed = 0.0, staged = (double)Kpad * D;
  for (int i = 0; i < n_layers; ++i) {
    if (N[i] <= 0) return false;
    composed += (double)Kpad * N[i];
    staged += (double)D * N[i];
  }
  return 2.0 * composed <= staged;
}

namespace {

// Folds the embedding of `pk` into every layer of the encoder's level aggregation (all of them read the same context), or
// into none: a layer that cannot be composed keeps today's path whole.
void compose_front(Model& m, EmbedPack& pk) {
  const Resampler& rs = m.enc_rs;
  if (!m.compose_front || rs.layers.empty() || m.enc_bias.p == nullptr) return;
  const int D = m.D, C = m.n_levels, Kpad = pk.Kpad;
  std::vector<int> N;
  for (size_t i = 0; i < rs.layers.size(); ++i) {
    if (rs.layers[i].ctx_dim != D) return;
    N.push_back(i == 0 && rs.n_vs > 0 ? rs.n_vs : 2 * rs.layers[i].inner);
  }
  if (!compose_front_rule(Kpad, D, N.data(), (int)N.size())) return;
  const std::vector<float> we = to_host(pk.w.f(), (size_t)pk.groups * D * Kpad), eb = to_host(m.enc_bias.f(), (size_t)C * D);
  std::vector<ComposedCtx> out;
  for (size_t i = 0; i < rs.layers.size(); ++i) {
    const auto& ly = rs.layers[i];
    const bool scores = i == 0 && rs.n_vs > 0;
    const int n = N[i], v0 = scores ? 0 : ly.inner;   // value rows: the first `inner` of [v | scores], the second half of k | v
    const std::vector<float> wc = to_host(scores ? rs.vs_w.f() : ly.to_kv, (size_t)n * D);
    std::vector<float> w((size_t)pk.groups * n * Kpad), b((size_t)C * n);
    ok(aurora_hip_compose_weight(wc.data(), n, D, we.data(), Kpad, pk.groups, w.data()));
    ok(aurora_hip_compose_bias(wc.data(), n, D, eb.data(), C, b.data()));
    if (!(absmax(w) < PRESPLIT_W_MAX)) return;
    ComposedCtx cc;
    cc.N = n;
    cc.v_l1 = 1e-6f;
    for (int g = 0; g < pk.groups; ++g) {
      const auto first = w.begin() + ((size_t)g * n + v0) * Kpad;
      cc.v_l1 = max_row_l1(std::vector<float>(first, first + (size_t)ly.inner * Kpad), ly.inner, Kpad, cc.v_l1);
    }
    for (int c = 0; c < C; ++c)
      for (int r = 0; r < ly.inner; ++r) cc.vb_max = std::max(cc.vb_max, fabsf(b[(size_t)c * n + v0 + r]));
    cc.w = to_device(w);
    cc.bias = to_device(b);
    // in the fp16-pair form exactly where the stages it replaces are: the guarded chain is the same chain, one link shorter
    if (ly.f16_mode == 2 && pk.ws.p != nullptr && (scores ? rs.vs_ws.p : ly.to_kv_s) != nullptr)
      cc.ws = presplit(cc.w.f(), n, Kpad, Kpad, /*row_multiple=*/256, pk.groups);
    out.push_back(std::move(cc));
  }
  pk.composed = std::move(out);
}

}  // namespace

// (groups, D, Kpad) GEMM weight of a LevelPatchEmbed for the channels that are present and T history steps
// (patchembed.py:100-115): per-variable (D, 1, Tmax, P, P) weights cut to T and laid out (v, t, i, j) along K, zero-padded
// to a multiple of 32.  Level-conditioned models (levelcond.py:36-69) hold one such weight per pressure level.
const EmbedPack& embed_pack(Model& m, int kind, int T, const std::vector<char>& present) {
  const std::vector<Channel>& chans = kind == 0 ? m.surf_channels : m.atmos_channels;
  int64_t mask = 0, mask_hi = 0;
  REQUIRE(chans.size() <= 126, "more than 126 input channels");
  for (size_t i = 0; i < chans.size(); ++i)
    if (present[i]) (i < 63 ? mask : mask_hi) |= (int64_t)1 << (i % 63);
  const std::array<int64_t, 3> key{(int64_t)kind * 1024 + T, mask, mask_hi};
  auto it = m.embed_packs.find(key);
  if (it != m.embed_packs.end()) return it->second;
  EmbedPack pk;
  for (size_t i = 0; i < chans.size(); ++i)
    if (present[i]) pk.channels.push_back((int)i);
  REQUIRE(!pk.channels.empty(), "no %s variable given", kind == 0 ? "surface-level" : "atmospheric");
  const bool per_level = kind == 1 && !m.level_condition.empty();
  pk.groups = per_level ? m.n_levels : 1;
  const int V = (int)pk.channels.size(), PP = m.P * m.P;
  pk.K = V * T * PP;
  pk.Kpad = round_up(pk.K, 32);
  std::vector<float> host((size_t)pk.groups * m.D * pk.Kpad, 0.f);
  for (int g = 0; g < pk.groups; ++g) {
    const std::string prefix = kind == 0 ? "encoder.surf_token_embeds.weights."
                               : per_level ? "encoder.atmos_token_embeds.layers." + level_to_str(m.levels[g]) + ".weights."
                                           : "encoder.atmos_token_embeds.weights.";
    for (int v = 0; v < V; ++v) {
      const Tensor& t = m.T_(prefix + chans[pk.channels[v]].name);   // (D, 1, Tmax, P, P)
      REQUIRE(t.shape.size() == 5 && t.shape[0] == m.D && t.shape[2] >= T && t.shape[3] == m.P, "bad patch-embed weight shape");
      const int64_t Tmax = t.shape[2];
      const std::vector<float> wv = to_host(t);
      for (int d = 0; d < m.D; ++d)
        for (int tt = 0; tt < T; ++tt)
          memcpy(&host[((size_t)g * m.D + d) * pk.Kpad + ((size_t)v * T + tt) * PP], &wv[((size_t)d * Tmax + tt) * PP], PP * sizeof(float));
    }
  }
  pk.l1 = max_row_l1(host, (int64_t)pk.groups * m.D, pk.Kpad, 1e-6f);
  pk.w = to_device(host);
  // the fp16-pair form for the guarded two-term kernel (the raw, normalised inputs are bounded only by the guard); every
  // group is a GEMM of D rows, held to the 256 of the Perceiver weights: historical, kept
  if (bounded_mode() == 2 && absmax(host) < PRESPLIT_W_MAX)
    pk.ws = presplit(pk.w.f(), m.D, pk.Kpad, pk.Kpad, /*row_multiple=*/256, pk.groups);
  if (kind == 1) compose_front(m, pk);
  return m.embed_packs.emplace(key, std::move(pk)).first->second;
}

// Atmospheric heads of the main and the alternate decoder Perceiver (`separate_perceiver` + their `_mod`, decoder.py:232-248).
void build_atmos_heads(Model& m, bool per_level) {
  std::vector<std::string> sep = m.sep_perceiver, main_names, alt_names;
  if (!m.mod_heads.empty())
    for (const auto& v : m.sep_perceiver) sep.push_back(v + "_mod");
  for (const auto& n : m.atmos_heads) (contains(sep, n) ? alt_names : main_names).push_back(n);
  build_heads(m, m.head_main, "atmos", main_names, per_level);
  build_heads(m, m.head_alt, "atmos", alt_names, per_level);
}

// ---- the stages of aurora_hip_finalize -------------------------------------------------------------
namespace {

// Surface MLP behind the surface patch embedding: constants of its guarded two-term chain.
void surface_mlp_chain(Model& m) {
  const Tensor &t0 = m.T_("encoder.surf_mlp.net.0.weight"), &t2 = m.T_("encoder.surf_mlp.net.2.weight");
  const std::vector<float> w0 = to_host(t0), w2 = to_host(t2);
  const int64_t N0 = t0.shape[0], K0 = t0.shape[1];
  m.surf_l1_0 = max_row_l1(w0, N0, K0, 1e-6f);
  m.surf_b0 = absmax(m.T_("encoder.surf_mlp.net.0.bias"));
  m.surf_c = absmax(m.T_("encoder.surf_token_embeds.bias")) + absmax(m.T_("encoder.surf_level_encoding"));
  // both linears or neither (the chain hands fp16 pairs from one to the other); 256 rows as in pack_resampler: historical, kept
  m.surf_chain = bounded_mode() == 2 && absmax(w0) < PRESPLIT_W_MAX && absmax(w2) < PRESPLIT_W_MAX &&
                 presplit_shape(N0, K0, 256) && presplit_shape(K0, N0, 256);
  m.surf_w0_s = m.surf_chain ? presplit(t0.f(), N0, K0, K0, /*row_multiple=*/256) : DevBuf();
  m.surf_w2_s = m.surf_chain ? presplit(t2.f(), K0, N0, N0, /*row_multiple=*/256) : DevBuf();
}

// AdaLN modulation of every block: lead time -> time_mlp -> stacked modulation linears (film.py:38-49).
void modulation_table(Model& m, Launcher& L, const DevBuf& d_lead, std::vector<DevBuf>& scratch) {
  const int D = m.D;
  DevBuf t1((size_t)D * 4), silu_c((size_t)D * 4);
  L.linear(LinearOp(d_lead.p, D, m.W("backbone.time_mlp.0.weight"), D, m.W("backbone.time_mlp.0.bias"), t1.p, D, 1, D, D, AURORA_F32)
               .activation(AURORA_ACT_SILU));
  L.linear(LinearOp(t1.p, D, m.W("backbone.time_mlp.2.weight"), D, m.W("backbone.time_mlp.2.bias"), silu_c.p, D, 1, D, D, AURORA_F32)
               .activation(AURORA_ACT_SILU));   // SiLU(c): the only way c is ever used
  int64_t rows = 0;
  for (const Block& b : m.blocks) rows += 4 * b.dim;
  DevBuf w_all((size_t)rows * D * 4), b_all((size_t)rows * 4);
  int64_t off = 0;
  for (const Block& b : m.blocks)
    for (const char* nrm : {".norm1", ".norm2"}) {
      const std::string nm = b.prefix + nrm + ".ln_modulation.1";
      hip_ok(hipMemcpy(w_all.f() + off * D, m.W(nm + ".weight"), (size_t)2 * b.dim * D * 4, hipMemcpyDeviceToDevice), "copy");
      hip_ok(hipMemcpy(b_all.f() + off, m.W(nm + ".bias"), (size_t)2 * b.dim * 4, hipMemcpyDeviceToDevice), "copy");
      off += 2 * b.dim;
    }
  m.mod = DevBuf((size_t)rows * 4);
  L.linear(LinearOp(silu_c.p, D, w_all.p, D, b_all.f(), m.mod.p, rows, 1, (int)rows, D, AURORA_F32));
  for (DevBuf* b : {&t1, &silu_c, &w_all, &b_all}) scratch.push_back(std::move(*b));
}

// Every block's slices of the modulation table and its weights in the compute dtype; merge / split linears; base attention set.
void backbone_weights(Model& m, void* stream) {
  int64_t off = 0;
  for (Block& b : m.blocks) {   // chunk(2): shift first, then scale (film.py:48); scale_bias is 0 in every config
    b.shift1 = m.mod.f() + off; b.gain1 = m.mod.f() + off + b.dim; off += 2 * b.dim;
    b.shift2 = m.mod.f() + off; b.gain2 = m.mod.f() + off + b.dim; off += 2 * b.dim;
    int64_t hidden = 0;
    b.fc1_w = compute_weight(m, b.prefix + ".mlp.fc1.weight", stream, &hidden);
    b.hidden = (int)hidden;
    b.fc2_w = compute_weight(m, b.prefix + ".mlp.fc2.weight", stream);
    b.fc1_b = m.W(b.prefix + ".mlp.fc1.bias"); b.fc2_b = m.W(b.prefix + ".mlp.fc2.bias");
    b.qkv_b = m.W(b.prefix + ".attn.qkv.bias"); b.proj_b = m.W(b.prefix + ".attn.proj.bias");
  }
  for (int i = 0; i + 1 < m.n_stages; ++i) {
    const std::string p = "backbone.encoder_layers." + std::to_string(i) + ".downsample";
    m.merges.push_back({compute_weight(m, p + ".reduction.weight", stream), m.W(p + ".norm.weight"), m.W(p + ".norm.bias")});
    const std::string q = "backbone.decoder_layers." + std::to_string(i) + ".upsample";
    m.splits.push_back({compute_weight(m, q + ".lin1.weight", stream), compute_weight(m, q + ".lin2.weight", stream),
                        m.W(q + ".norm.weight"), m.W(q + ".norm.bias")});
  }
  attn_weights(m, -1, stream);
}

// Lead-time embedding, both Perceivers, the encoder's first queries (model constants) and the score rows made from them.
void perceivers(Model& m, Launcher& L, const DevBuf& d_lead) {
  const int D = m.D;
  m.lead_emb = DevBuf((size_t)D * 4);
  L.linear(LinearOp(d_lead.p, D, m.W("encoder.lead_time_embed.weight"), D, m.W("encoder.lead_time_embed.bias"), m.lead_emb.p, D, 1, D,
                    D, AURORA_F32));
  m.enc_rs = pack_resampler(m, "encoder.level_agg", m.enc_depth, m.perceiver_heads);
  m.dec_rs = pack_resampler(m, "decoder.level_decoder", m.dec_depth, m.perceiver_heads);
  const auto& l0 = m.enc_rs.layers[0];
  const int n_lat = m.Cl - 1;
  m.enc_q0 = DevBuf((size_t)n_lat * l0.inner * 4);
  L.linear(LinearOp(m.W("encoder.atmos_latents"), D, l0.to_q, D, nullptr, m.enc_q0.p, l0.inner, n_lat, l0.inner, D, AURORA_F32));
  if (l0.ln_q_w)
    L.layernorm(m.enc_q0.p, l0.inner, l0.ln_q_w, l0.ln_q_b, nullptr, 0, 0, m.enc_q0.f(), l0.inner, nullptr, 0, n_lat, l0.inner,
                1e-5f, AURORA_F32);
  hip_ok(hipStreamSynchronize(as_stream(L.stream)), "precompute sync");
  score_weights(m, m.enc_rs, m.enc_q0.f(), n_lat, m.perceiver_heads);
  // second decoder Perceiver for the variables of `separate_perceiver` (decoder.py:232-248)
  m.has_alt = !m.sep_perceiver.empty();
  if (m.has_alt) m.dec_rs_alt = pack_resampler(m, "decoder.level_decoder_alternate", m.dec_depth, m.perceiver_heads);
}

// Air pollution: Linear(2, 1) feature combiners of the positive variables (aurora.py:733-742).
void feature_combiners(Model& m) {
  for (int kind = 0; kind < 2; ++kind)
    for (Channel& ch : kind == 0 ? m.surf_channels : m.atmos_channels)
      if (ch.transform == 2) {
        const std::string p = std::string(kind == 0 ? "surf" : "atmos") + "_feature_combiner." + ch.name;
        const std::vector<float> wv = to_host(m.T_(p + ".weight")), bv = to_host(m.T_(p + ".bias"));
        REQUIRE(wv.size() == 2 && bv.size() == 1, "bad feature combiner shape for %s", p.c_str());
        ch.tw0 = wv[0]; ch.tw1 = wv[1]; ch.tb = bv[0];
      }
}

}  // namespace

}  // namespace aurora

using namespace aurora;

// out[g][n][k] = sum_d w_ctx[n][d] w_e[g][d][k], summed in double in the order of d and rounded once.  Host arithmetic.
extern "C" int aurora_hip_compose_weight(const float* w_ctx, int N, int D, const float* w_e, int K, int groups, float* out) {
  GUARDED({
    REQUIRE(w_ctx && w_e && out && N > 0 && D > 0 && K > 0 && groups > 0, "compose_weight: bad argument");
    std::vector<double> acc((size_t)K);
    for (int g = 0; g < groups; ++g)
      for (int n = 0; n < N; ++n) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int d = 0; d < D; ++d) {
          const double a = w_ctx[(size_t)n * D + d];
          const float* row = w_e + ((size_t)g * D + d) * K;
          for (int k = 0; k < K; ++k) acc[k] += a * row[k];
        }
        float* dst = out + ((size_t)g * N + n) * K;
        for (int k = 0; k < K; ++k) dst[k] = (float)acc[k];
      }
  })
}

// out[c][n] = sum_d w_ctx[n][d] bias[c][d], likewise.
extern "C" int aurora_hip_compose_bias(const float* w_ctx, int N, int D, const float* bias, int C, float* out) {
  GUARDED({
    REQUIRE(w_ctx && bias && out && N > 0 && D > 0 && C > 0, "compose_bias: bad argument");
    for (int c = 0; c < C; ++c)
      for (int n = 0; n < N; ++n) {
        double acc = 0.0;
        for (int d = 0; d < D; ++d) acc += (double)w_ctx[(size_t)n * D + d] * bias[(size_t)c * D + d];
        out[(size_t)c * N + n] = (float)acc;
      }
  })
}

extern "C" int aurora_hip_compose_front_rule(int Kpad, int D, const int32_t* N, int n_layers) {
  return compose_front_rule(Kpad, D, N, n_layers) ? 1 : 0;
}

extern "C" int aurora_hip_composed_value_bound(float v_l1, float embed_l1, float embed_bias_max, float composed_v_l1,
                                               float composed_vb_max, float out[6]) {
  GUARDED({
    REQUIRE(out && v_l1 > 0.f && embed_l1 > 0.f && composed_v_l1 > 0.f && embed_bias_max >= 0.f && composed_vb_max >= 0.f,
            "composed_value_bound: bad argument");
    const ValueBound staged{v_l1 * embed_l1, v_l1 * embed_bias_max}, folded = composed_value_bound(v_l1, embed_l1, embed_bias_max,
                                                                                              composed_v_l1, composed_vb_max);
    out[0] = staged.a; out[1] = staged.c; out[2] = (F16_SAFE / v_l1 - embed_bias_max) / embed_l1;
    out[3] = folded.a; out[4] = folded.c; out[5] = folded.word_limit();
  })
}

extern "C" int aurora_hip_front_composed(const aurora_hip_model* m) { return m != nullptr && m->front_composed ? 1 : 0; }

extern "C" int aurora_hip_pack_weights(aurora_hip_model* m, const char* name, const void* data, const int64_t* shape, int ndim,
                                       int dtype, int on_device) {
  GUARDED({
    REQUIRE(m && name && data && ndim >= 0 && ndim <= 8, "pack_weights: bad argument");
    REQUIRE(dtype == AURORA_F32, "pack_weights: parameters must be float32 (the engine keeps fp32 masters)");
    Tensor t;
    t.numel = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); t.numel *= shape[i]; }
    t.buf = DevBuf((size_t)t.numel * 4);
    hip_ok(hipMemcpy(t.buf.p, data, (size_t)t.numel * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice),
           "pack_weights copy");
    m->w[name] = std::move(t);
    m->finalized = false;
  })
}

// ---- packed weight files -----------------------------------------------------------------------------
// One self-describing binary that any host can read without pickle / torch:
//   "AURORAHIP1\0" | u32 n_entries | per entry: u32 name_len, name, u32 dtype (0 f32, 1 bf16), u32 ndim, i64 shape[ndim],
//   u64 n_bytes, raw little-endian data
// Saved by a FINALIZED handle: the large backbone matrices (MLP, merge / split, and the attention projections of models
// without LoRA) are written in bf16 when the handle runs the bf16 backbone -- exactly the bits the GEMMs consume --
// everything else as the fp32 master.  1.3 B parameters: 2.6 GB instead of 5 GB.
namespace {
const char PACK_MAGIC[] = "AURORAHIP1";

bool backbone_matrix(const Model& m, const std::string& name) {
  if (name.rfind("backbone.", 0) != 0 || name.size() < 7 || name.compare(name.size() - 7, 7, ".weight") != 0) return false;
  for (const char* tag : {".mlp.fc1.", ".mlp.fc2.", ".downsample.reduction.", ".upsample.lin1.", ".upsample.lin2."})
    if (name.find(tag) != std::string::npos) return true;
  if (!m.use_lora && (name.find(".attn.qkv.") != std::string::npos || name.find(".attn.proj.") != std::string::npos)) return true;
  return false;
}
}  // namespace

extern "C" int aurora_hip_save_packed(aurora_hip_model* mp, const char* path, void* stream) {
  GUARDED({
    REQUIRE(mp && path, "save_packed: null argument");
    Model& m = *mp;
    FILE* f = fopen(path, "wb");
    REQUIRE(f != nullptr, "save_packed: cannot open '%s' for writing", path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    auto put = [&](const void* p, size_t n) { REQUIRE(fwrite(p, 1, n, f) == n, "save_packed: short write"); };
    put(PACK_MAGIC, sizeof(PACK_MAGIC));
    const uint32_t n_entries = (uint32_t)(m.w.size() + m.w16.size());
    put(&n_entries, 4);
    std::vector<char> host;
    auto entry = [&](const std::string& name, const Tensor& t, uint32_t dtype, const void* dev, size_t bytes) {
      const uint32_t len = (uint32_t)name.size(), nd = (uint32_t)t.shape.size();
      put(&len, 4); put(name.data(), len); put(&dtype, 4); put(&nd, 4);
      for (int64_t d : t.shape) put(&d, 8);
      const uint64_t nb = bytes;
      put(&nb, 8);
      host.resize(bytes);
      hip_ok(hipMemcpy(host.data(), dev, bytes, hipMemcpyDeviceToHost), "save_packed download");
      put(host.data(), bytes);
    };
    for (const auto& kv : m.w) {
      if (m.autocast && backbone_matrix(m, kv.first)) {
        DevBuf h((size_t)kv.second.numel * 2);
        ok(aurora_hip_convert(kv.second.f(), h.p, kv.second.numel, AURORA_F32, stream));
        hip_ok(hipStreamSynchronize(as_stream(stream)), "save_packed");
        entry(kv.first, kv.second, AURORA_BF16, h.p, (size_t)kv.second.numel * 2);
      } else {
        entry(kv.first, kv.second, AURORA_F32, kv.second.f(), (size_t)kv.second.numel * 4);
      }
    }
    for (const auto& kv : m.w16) entry(kv.first, kv.second, AURORA_BF16, kv.second.buf.p, (size_t)kv.second.numel * 2);
  })
}

extern "C" int aurora_hip_load_packed(aurora_hip_model* mp, const char* path) {
  GUARDED({
    REQUIRE(mp && path, "load_packed: null argument");
    Model& m = *mp;
    FILE* f = fopen(path, "rb");
    REQUIRE(f != nullptr, "load_packed: cannot open '%s'", path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    auto get = [&](void* p, size_t n) { REQUIRE(fread(p, 1, n, f) == n, "load_packed: truncated file"); };
    char magic[sizeof(PACK_MAGIC)];
    get(magic, sizeof(magic));
    REQUIRE(memcmp(magic, PACK_MAGIC, sizeof(PACK_MAGIC)) == 0, "load_packed: '%s' is not a packed aurora_hip weight file", path);
    uint32_t n_entries = 0;
    get(&n_entries, 4);
    std::vector<char> host;
    for (uint32_t e = 0; e < n_entries; ++e) {
      uint32_t len = 0, dtype = 0, nd = 0;
      get(&len, 4);
      REQUIRE(len < 4096, "load_packed: corrupt entry");
      std::string name(len, '\0');
      get(&name[0], len);
      get(&dtype, 4); get(&nd, 4);
      REQUIRE(nd <= 8 && dtype <= 1, "load_packed: corrupt entry '%s'", name.c_str());
      Tensor t;
      t.numel = 1;
      for (uint32_t i = 0; i < nd; ++i) { int64_t d; get(&d, 8); t.shape.push_back(d); t.numel *= d; }
      uint64_t nb = 0;
      get(&nb, 8);
      REQUIRE(nb == (uint64_t)t.numel * (dtype == AURORA_F32 ? 4 : 2), "load_packed: size mismatch in '%s'", name.c_str());
      host.resize(nb);
      get(host.data(), nb);
      t.buf = DevBuf(nb);
      upload(t.buf.p, host.data(), nb);
      (dtype == AURORA_F32 ? m.w : m.w16)[name] = std::move(t);
    }
    m.finalized = false;
  })
}

extern "C" int aurora_hip_finalize(aurora_hip_model* mp, void* stream) {
  GUARDED({
    REQUIRE(mp != nullptr, "finalize: null model");
    Model& m = *mp;
    m.keep.clear(); m.attn_sets.clear(); m.embed_packs.clear(); m.merges.clear(); m.splits.clear();
    Launcher L{m, stream};
    surface_mlp_chain(m);
    std::vector<float> lead((size_t)m.D);
    const double hours = (double)(float)m.timestep_hours;
    fourier(LEAD_TIME, &hours, 1, m.D, lead.data());
    const DevBuf d_lead = to_device(lead);
    std::vector<DevBuf> scratch;   // operands of the stages' launches: freed after the last synchronisation
    modulation_table(m, L, d_lead, scratch);
    backbone_weights(m, stream);
    perceivers(m, L, d_lead);
    // decoder heads, fused over the variables of a group (level-conditioned atmospheric heads: per level set, at precompute)
    build_heads(m, m.head_surf, "surf", m.surf_heads, false);
    if (m.level_condition.empty()) build_atmos_heads(m, false);
    feature_combiners(m);
    hip_ok(hipStreamSynchronize(as_stream(stream)), "finalize sync");   // d_lead and the scratch die here
    m.finalized = true;
  })
}
