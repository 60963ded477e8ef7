// The model handle of libaurora_hip.so: creation and lifecycle.
//
// aurora_hip_create / _pack_weights / _finalize / _precompute / _set_time / _step / _destroy (include/aurora_hip.h) own
// everything the reference's `Aurora.forward` (aurora/model/aurora.py:265-392) needs besides the input fields: the
// configuration, the weights (fp32 masters + bf16 backbone copies, LoRA merged per roll-out phase), the tables that
// depend on parameters / grid / levels only (AdaLN modulation, Fourier position / scale / level encodings, window
// token tables, a latitude band's halo plans), the workspace, and the SEQUENCE of kernel launches of a step (step.hip) on
// a caller-supplied stream.  No torch, no Python: any host language that can call C can run Aurora on an MI355X through
// these functions; aurora_amd's own Python `Engine` is a thin binding of them.
//
// By lifetime: here what a configuration fixes (create, block and channel lists), band and staging setters, the step entry
// and profiling; model_weights.hip what depends on parameters only (weight packing, packed files, aurora_hip_finalize);
// model_grid.hip what depends on grid, levels or time (Fourier and window tables, aurora_hip_precompute, aurora_hip_set_time).
//
// Scope: every public model class -- Aurora, AuroraPretrained, AuroraSmallPretrained, Aurora12hPretrained, AuroraHighRes
// (any patch size / depths / history / LoRA mode, stabilised level aggregation, batch > 1), AuroraAirPollution and
// AuroraWave (level-conditioned embeddings / heads, dynamic and static inputs, feature combiners, difference prediction,
// second decoder Perceiver, NaN / density / angle channels) -- on one device or as one latitude band of a forecast
// sharded over several (aurora_hip_set_band).
// Host code only; every launch goes through the operator ABI of this same library.
#include "model.h"

namespace aurora {

hipEvent_t take_event(Model& m) {
  if (!m.event_pool.empty()) {
    hipEvent_t e = m.event_pool.back();
    m.event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  hip_ok(hipEventCreate(&e), "hipEventCreate");
  return e;
}

int bounded_mode() {
  static const int mode = getenv("AURORA_F32_GEMM") ? -1 : 2;
  return mode;
}

std::string level_to_str(double level) {
  const double value = round(level * 1000.0) / 1000.0;
  char buf[64];
  if (value == (double)(long long)value) snprintf(buf, sizeof buf, "%lld", (long long)value);
  else {
    snprintf(buf, sizeof buf, "%.3f", value);
    std::string t(buf);
    while (!t.empty() && t.back() == '0') t.pop_back();   // Python's str(float): shortest form of a 3-decimal value
    for (char& ch : t) if (ch == '.') ch = '_';
    return t;
  }
  return buf;
}

int lora_key(const Model& m, int step) {   // lora.py:105-129; -1 = no LoRA
  if (!m.use_lora || step >= m.lora_steps) return -1;
  if (m.lora_mode == 0) return 0;                       // single
  if (m.lora_mode == 1) return step == 0 ? -1 : 0;      // from_second
  return step;                                          // all
}

namespace {

const char* const DYNAMIC_NAMES[6] = {"tod_cos", "tod_sin", "dow_cos", "dow_sin", "doy_cos", "doy_sin"};   // encoder.py:246
void build_blocks(Model& m) {
  m.blocks.clear();
  for (int part = 0; part < 2; ++part)
    for (int i = 0; i < m.n_stages; ++i) {
      const int depth = part == 0 ? m.enc_depths[i] : m.dec_depths[i];
      const int stage = part == 0 ? i : m.n_stages - 1 - i;
      for (int j = 0; j < depth; ++j) {
        Block b{};
        b.prefix = std::string(part == 0 ? "backbone.encoder_layers." : "backbone.decoder_layers.") + std::to_string(i) +
                   ".blocks." + std::to_string(j);
        b.dim = m.stage_dim(stage);
        b.stage = stage;
        b.heads = part == 0 ? m.enc_heads[i] : m.dec_heads[i];
        b.shifted = j % 2 == 1;
        REQUIRE(b.dim == b.heads * 64, "the window-attention kernel is built for head_dim 64 (dim %d, %d heads)", b.dim,
                b.heads);
        m.blocks.push_back(b);
      }
    }
}

// Input channels of the two patch embeddings and the decoder's heads / outputs, from the variant keywords
// (encoder.py:226-303; aurora.py:733-742, 892-932; decoder.py:214-263).
void build_channels(Model& m) {
  m.surf_channels.clear(); m.atmos_channels.clear(); m.surf_heads.clear(); m.surf_out.clear(); m.atmos_heads.clear();
  if (m.variant == 2) {
    // ocean wave: the caller supplies the variables themselves; the model sees value (NaN -> 0) + density channels and
    // sin / cos of the directions -- the variables that stay, then the appended channels (aurora.py:892-912)
    std::vector<Channel> kept, appended;
    for (size_t i = 0; i < m.surf_inputs.size(); ++i) {
      const std::string& k = m.surf_inputs[i];
      const bool dens = contains(m.density_vars, k), ang = contains(m.angle_vars, k);
      if (!ang) kept.push_back({k, SRC_SURF, (int)i, dens ? 4 : 0});
      if (dens) appended.push_back({k + "_density", SRC_SURF, (int)i, 3});
      if (ang) {
        appended.push_back({k + "_sin", SRC_SURF, (int)i, 5});
        appended.push_back({k + "_cos", SRC_SURF, (int)i, 6});
      }
    }
    for (const auto& c : kept) { m.surf_channels.push_back(c); m.surf_out.push_back(c.name); }
    for (const auto& c : appended) m.surf_channels.push_back(c);
    for (const auto& c : m.surf_channels) m.surf_heads.push_back(c.name);
    for (const auto& a : m.angle_vars)   // predicted directions follow the variables that stayed (aurora.py:914-932)
      if (contains(m.surf_heads, a + "_sin") && !contains(m.surf_out, a)) m.surf_out.push_back(a);
    for (const auto& c : m.surf_channels)
      REQUIRE(contains(m.surf_vars, c.name), "ocean wave: channel '%s' is not among the model's surf_vars", c.name.c_str());
  } else {
    for (size_t i = 0; i < m.surf_inputs.size(); ++i) {
      const std::string& k = m.surf_inputs[i];
      const int tr = contains(m.pos_surf, k) ? (m.variant == 1 ? 2 : 1) : 0;   // clamp, or clamp + log feature combiner
      m.surf_channels.push_back({k, SRC_SURF, (int)i, tr});
      m.surf_heads.push_back(k);
      m.surf_out.push_back(k);
    }
    for (const auto& k : m.surf_inputs)
      if (contains(m.mod_heads, k)) m.surf_heads.push_back(k + "_mod");
  }
  for (size_t i = 0; i < m.static_vars.size(); ++i) m.surf_channels.push_back({m.static_vars[i], SRC_STATIC, (int)i, 0});
  if (m.dynamic_vars)
    for (int i = 0; i < 6; ++i) m.surf_channels.push_back({DYNAMIC_NAMES[i], SRC_DYN, i, 0});

  for (size_t i = 0; i < m.atmos_vars.size(); ++i) {
    const std::string& k = m.atmos_vars[i];
    const int tr = contains(m.pos_atmos, k) ? (m.variant == 1 ? 2 : 1) : 0;
    m.atmos_channels.push_back({k, SRC_ATMOS, (int)i, tr});
    m.atmos_heads.push_back(k);
  }
  for (const auto& k : m.atmos_vars)
    if (contains(m.mod_heads, k)) m.atmos_heads.push_back(k + "_mod");
  if (m.atmos_static_vars) {
    // static (and dynamic) variables at every level; prefixed when the dynamic ones are there (encoder.py:248-269)
    const std::string pre = m.dynamic_vars ? "static_" : "";
    for (size_t i = 0; i < m.static_vars.size(); ++i) m.atmos_channels.push_back({pre + m.static_vars[i], SRC_STATIC, (int)i, 0});
    if (m.dynamic_vars)
      for (int i = 0; i < 6; ++i) m.atmos_channels.push_back({pre + DYNAMIC_NAMES[i], SRC_DYN, i, 0});
  }
  if (m.index_bug) {
    // the slot of `static_z` is fed with `z`'s data (encoder.py:293-303, compat.py:156-159)
    int iz = -1, isz = -1;
    for (size_t i = 0; i < m.atmos_channels.size(); ++i) {
      if (m.atmos_channels[i].name == "z") iz = (int)i;
      if (m.atmos_channels[i].name == "static_z") isz = (int)i;
    }
    if (iz >= 0) {
      REQUIRE(isz >= 0, "'static_z' is not in list");
      Channel c = m.atmos_channels[iz];
      c.name = "static_z";
      m.atmos_channels[isz] = c;
    }
  }
}

}  // namespace

}  // namespace aurora

using namespace aurora;

// ---- C ABI ---------------------------------------------------------------------------------------
extern "C" int aurora_hip_create(const aurora_hip_config* c, aurora_hip_model** out) {
  GUARDED({
    REQUIRE(c != nullptr && out != nullptr, "create: null argument");
    REQUIRE(c->n_stages >= 1 && c->n_stages <= 4, "create: 1..4 backbone stages");
    REQUIRE(c->latent_levels > 1, "At least two latent levels are required.");
    REQUIRE(c->max_history > 0, "At least one history step is required.");
    REQUIRE(c->embed_dim % 32 == 0 && c->patch_size > 0, "create: bad embed_dim / patch_size");
    std::unique_ptr<aurora_hip_model> m(new aurora_hip_model());
    m->D = c->embed_dim; m->P = c->patch_size; m->Cl = c->latent_levels; m->perceiver_heads = c->num_heads;
    m->n_stages = c->n_stages;
    int se = 0, sd = 0;
    for (int i = 0; i < c->n_stages; ++i) {
      m->enc_depths[i] = c->encoder_depths[i]; m->dec_depths[i] = c->decoder_depths[i];
      m->enc_heads[i] = c->encoder_heads[i]; m->dec_heads[i] = c->decoder_heads[i];
      se += c->encoder_depths[i]; sd += c->decoder_depths[i];
    }
    REQUIRE(se == sd, "Encoder and decoder must have the same total depth.");
    for (int a = 0; a < 3; ++a) m->window[a] = c->window[a];
    REQUIRE(m->window[0] * m->window[1] * m->window[2] <= 144, "windows of more than 144 tokens are not supported");
    REQUIRE(m->Cl % m->window[0] == 0, "latent levels must be divisible by the window's level extent");
    m->enc_depth = c->enc_depth; m->dec_depth = c->dec_depth; m->max_history = c->max_history;
    m->ln_eps = c->perceiver_ln_eps; m->timestep_hours = c->timestep_hours;
    m->stabilise = c->stabilise_level_agg != 0; m->use_lora = c->use_lora != 0;
    m->lora_steps = c->lora_steps; m->lora_mode = c->lora_mode; m->autocast = c->autocast != 0;
    REQUIRE(m->lora_mode >= 0 && m->lora_mode <= 2, "create: lora_mode must be 0 (single), 1 (from_second) or 2 (all)");
    auto names = [](const char* const* p, int n, std::vector<std::string>& dst) {
      for (int i = 0; i < n; ++i) dst.push_back(p[i]);
    };
    names(c->surf_vars, c->n_surf, m->surf_vars);
    names(c->static_vars, c->n_static, m->static_vars);
    names(c->atmos_vars, c->n_atmos, m->atmos_vars);
    REQUIRE(!m->surf_vars.empty() && !m->atmos_vars.empty(), "create: variable lists must not be empty");
    // ---- variant keywords ----
    m->variant = c->variant;
    REQUIRE(m->variant >= 0 && m->variant <= 2, "create: variant must be 0 (base), 1 (air pollution) or 2 (ocean wave)");
    for (int i = 0; i < c->n_level_condition; ++i) m->level_condition.push_back(c->level_condition[i]);
    m->dynamic_vars = c->dynamic_vars != 0; m->atmos_static_vars = c->atmos_static_vars != 0;
    m->clamp_first = c->clamp_at_first_step != 0; m->index_bug = c->simulate_indexing_bug != 0;
    names(c->separate_perceiver, c->n_separate_perceiver, m->sep_perceiver);
    names(c->modulation_heads, c->n_modulation_heads, m->mod_heads);
    names(c->positive_surf_vars, c->n_positive_surf, m->pos_surf);
    names(c->positive_atmos_vars, c->n_positive_atmos, m->pos_atmos);
    names(c->surf_inputs, c->n_surf_inputs, m->surf_inputs);
    names(c->density_channel_surf_vars, c->n_density, m->density_vars);
    names(c->angle_surf_vars, c->n_angle, m->angle_vars);
    if (m->surf_inputs.empty()) m->surf_inputs = m->surf_vars;
    REQUIRE(m->variant == 2 || m->surf_inputs == m->surf_vars, "create: surf_inputs are for the ocean-wave variant");
    if (c->difference_history)
      for (int i = 0; i < c->n_modulation_heads; ++i)
        if (c->difference_history[i] >= 0) m->diff_index[m->mod_heads[i]] = c->difference_history[i];
    REQUIRE(m->static_vars.size() <= 60 && m->surf_inputs.size() <= 60 && m->atmos_vars.size() <= 60, "create: too many variables");
    build_blocks(*m);
    build_channels(*m);
    m->ctx_max = DevBuf(16);
    // how this handle runs its steps: fields of the configuration (0 = the library's default), never the environment
    const auto& tu = c->tuning;
    REQUIRE(tu.fuse_ln >= 0 && tu.fuse_ln <= 3, "create: tuning.fuse_ln = %d (0 default, 1 never, 2 by the fill rule, 3 always)", tu.fuse_ln);
    auto sw = [](int32_t v, bool dflt, const char* what) {
      REQUIRE(v >= 0 && v <= 2, "create: tuning.%s = %d (0 default, 1 off, 2 on)", what, v);
      return v == 0 ? dflt : v == 2;
    };
    m->fuse_ln = tu.fuse_ln == 0 ? 1 : tu.fuse_ln - 1;
    m->split_attention = sw(tu.band_split_attention, false, "band_split_attention");
    m->qkv_planes = sw(tu.qkv_planes, true, "qkv_planes");
    m->split_k = sw(tu.split_k, true, "split_k");
    m->reassoc_out = sw(tu.perceiver_reassoc, true, "perceiver_reassoc");
    m->score_weights = sw(tu.score_weights, true, "score_weights");
    m->compose_front = sw(tu.compose_front, true, "compose_front");
    m->tickets = DevBuf(SPLIT_TICKETS * sizeof(int32_t));
    hip_ok(hipMemset(m->tickets.p, 0, SPLIT_TICKETS * sizeof(int32_t)), "hipMemset");
    *out = m.release();
  })
}

extern "C" void aurora_hip_destroy(aurora_hip_model* m) { delete m; }

extern "C" int aurora_hip_set_band(aurora_hip_model* mp, const aurora_hip_band* band) {
  GUARDED({
    REQUIRE(mp != nullptr, "set_band: null model");
    Model& m = *mp;
    if (band == nullptr || band->world <= 1) {
      m.band = aurora_hip_band{0, 1, nullptr, nullptr, nullptr};
    } else {
      REQUIRE(band->rank >= 0 && band->rank < band->world, "set_band: rank %d of %d", band->rank, band->world);
      REQUIRE(band->post && band->wait, "set_band: the halo transport callbacks are required");
      m.band = *band;
    }
    m.have_grid = false;   // the grid tables are per band: precompute again
    m.plans.clear(); m.rows.clear();
    m.stage_send = m.stage_recv = nullptr;
    m.staging_bytes = m.staging_need = 0;
  })
}

extern "C" int aurora_hip_band_rows(const aurora_hip_model* m, int32_t* row0, int32_t* row1) {
  GUARDED({
    REQUIRE(m && row0 && row1 && m->have_grid, "band_rows: precompute the grid first");
    const int h0 = m->sharded() ? m->rows[0][m->band.rank][0] : 0;
    *row0 = h0 * m->P;
    *row1 = (h0 + m->Hp) * m->P;
  })
}

extern "C" int64_t aurora_hip_band_staging_bytes(const aurora_hip_model* m) { return m ? m->staging_need : 0; }

extern "C" int aurora_hip_set_band_staging(aurora_hip_model* m, void* send, void* recv, int64_t staging_bytes) {
  GUARDED({
    REQUIRE(m != nullptr, "set_band_staging: null model");
    REQUIRE(staging_bytes >= m->staging_need, "set_band_staging: %lld bytes per buffer, %lld needed", (long long)staging_bytes,
            (long long)m->staging_need);
    REQUIRE(m->staging_need == 0 || (send && recv && (uintptr_t)send % 16 == 0 && (uintptr_t)recv % 16 == 0),
            "set_band_staging: two 16-byte aligned device buffers are required");
    m->stage_send = send;
    m->stage_recv = recv;
    m->staging_bytes = staging_bytes;
  })
}

extern "C" int aurora_hip_output_vars(const aurora_hip_model* m, const char** names, int capacity) {
  if (!m) return 0;
  if (names)
    for (int i = 0; i < capacity && i < (int)m->surf_out.size(); ++i) names[i] = m->surf_out[i].c_str();
  return (int)m->surf_out.size();
}

extern "C" int aurora_hip_step(aurora_hip_model* mp, const aurora_hip_step_io* io, void* stream) {
  GUARDED({
    REQUIRE(mp && io, "step: null argument");
    Model& m = *mp;
    REQUIRE(m.finalized && m.have_grid, "step: finalize the weights and precompute the grid first");
    REQUIRE(io->B >= 1 && io->T >= 1, "step: empty batch");
    REQUIRE(io->T <= m.max_history, "%d > %d.", io->T, m.max_history);
    REQUIRE(m.abs_B >= io->B, "step: call aurora_hip_set_time for this batch first");
    REQUIRE(io->surf && io->atmos && io->out_surf && io->out_atmos && (m.static_vars.empty() || io->stat), "step: null field list");
    if (m.sharded()) {
      REQUIRE(io->B == 1, "latitude-band sharding runs one forecast (batch size 1) across the ranks");
      REQUIRE(m.staging_need == 0 || m.staging_bytes >= m.staging_need, "step: hand over the band's staging buffers first "
              "(aurora_hip_set_band_staging, %lld bytes each)", (long long)m.staging_need);
    }
    StepIO s{io, io->B, io->T};
    // LoRA sets are merged outside the dry run (they allocate and launch)
    attn_weights(m, lora_key(m, io->rollout_step), stream);
    m.dry = true;
    m.arena.peak = 0;
    try { run_step(m, s, stream); } catch (...) { m.dry = false; throw; }
    m.dry = false;
    if (m.arena.peak > m.arena.cap) {
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(as_stream(stream), &cap);
      REQUIRE(cap == hipStreamCaptureStatusNone, "step: the workspace must grow; run one step outside graph capture first");
      hip_ok(hipDeviceSynchronize(), "sync before growing the workspace");
      if (m.arena.base) (void)hipFree(m.arena.base);
      m.arena.base = nullptr;
      m.arena.cap = 0;
      void* p = nullptr;
      hip_ok(hipMalloc(&p, m.arena.peak), "workspace allocation");
      m.arena.base = (char*)p;
      m.arena.cap = m.arena.peak;
      m.generation += 1;
    }
    // split-K tickets must be zero when a launch starts (gemm.hip).  Every launch leaves them zero, but a launch that was
    // aborted on the DEVICE (a fault, a reset) returns normally to the host and may have left counts behind: a sharded step --
    // the only kind that splits along K -- clears them first, whatever happened before (one 16 KiB memset node; a captured
    // graph replays it too).
    if (m.sharded() && m.split_k)
      hip_ok(hipMemsetAsync(m.tickets.p, 0, SPLIT_TICKETS * sizeof(int32_t), as_stream(stream)), "zeroing the split-K tickets");
    run_step(m, s, stream);
  })
}

namespace {
const char* const KIND_NAMES[K_COUNT] = {"linear_bf16", "linear_f32", "window_attention_bf16", "layernorm", "merge_ln",
                                         "split_ln", "patchify", "perceiver_attention", "assemble_tokens", "unpatchify",
                                         "copy2d", "absmax", "linear_layernorm_bf16", "gather_rows", "perceiver_out"};
}

extern "C" int aurora_hip_profile_begin(aurora_hip_model* m, uint32_t kind_mask) {
  GUARDED({
    REQUIRE(m != nullptr, "profile_begin: null model");
    for (auto& t : m->timed) { m->event_pool.push_back(t.e0); m->event_pool.push_back(t.e1); }
    m->timed.clear();
    m->profile_mask = kind_mask;
  })
}

extern "C" int aurora_hip_profile_end(aurora_hip_model* m, aurora_hip_profile_entry* out, int capacity, int* n_out) {
  GUARDED({
    REQUIRE(m && out && n_out && capacity >= K_COUNT, "profile_end: need room for %d entries", (int)K_COUNT);
    m->profile_mask = 0;
    hip_ok(hipDeviceSynchronize(), "profile_end");
    for (int k = 0; k < K_COUNT; ++k) out[k] = aurora_hip_profile_entry{KIND_NAMES[k], 0, 0.0, 0.0};
    for (auto& t : m->timed) {
      float ms = 0.f;
      hip_ok(hipEventElapsedTime(&ms, t.e0, t.e1), "hipEventElapsedTime");
      out[t.kind].launches += 1;
      out[t.kind].ms += ms;
      out[t.kind].work += t.work;
      m->event_pool.push_back(t.e0);
      m->event_pool.push_back(t.e1);
    }
    m->timed.clear();
    *n_out = K_COUNT;
  })
}

extern "C" int aurora_hip_profile_end_list(aurora_hip_model* m, aurora_hip_profile_entry* out, int capacity, int* n_out) {
  GUARDED({
    REQUIRE(m && n_out && (out || capacity == 0), "profile_end_list: bad arguments");
    m->profile_mask = 0;
    hip_ok(hipDeviceSynchronize(), "profile_end_list");
    *n_out = (int)m->timed.size();
    if (capacity < *n_out) return AURORA_OK;   // (query: the launches stay recorded)
    int i = 0;
    for (auto& t : m->timed) {
      float ms = 0.f;
      hip_ok(hipEventElapsedTime(&ms, t.e0, t.e1), "hipEventElapsedTime");
      out[i++] = aurora_hip_profile_entry{KIND_NAMES[t.kind], 1, ms, t.work};
      m->event_pool.push_back(t.e0);
      m->event_pool.push_back(t.e1);
    }
    m->timed.clear();
  })
}

extern "C" int64_t aurora_hip_generation(const aurora_hip_model* m) { return m ? m->generation : 0; }

extern "C" int aurora_hip_abi_sizes(int32_t* out, int capacity) {
  const int32_t sizes[] = {(int32_t)sizeof(aurora_hip_config), (int32_t)sizeof(aurora_hip_grid), (int32_t)sizeof(aurora_hip_step_io),
                           (int32_t)sizeof(aurora_hip_band), (int32_t)sizeof(aurora_hip_halo_msg), (int32_t)sizeof(aurora_hip_plan_info),
                           (int32_t)sizeof(aurora_patch_var), (int32_t)sizeof(aurora_unpatch_var), (int32_t)sizeof(aurora_hip_profile_entry)};
  const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
  for (int i = 0; i < n && i < capacity; ++i) out[i] = sizes[i];
  return n;
}

extern "C" int aurora_hip_guard_limits(const aurora_hip_model* m, float out[8]) {
  GUARDED({
    REQUIRE(m && out, "guard_limits: bad arguments");
    for (int i = 0; i < 4; ++i) {
      out[i] = m->guard_limit_min[i];
      out[4 + i] = (float)m->guard_launches[i];
    }
  })
}

extern "C" int64_t aurora_hip_workspace_bytes(const aurora_hip_model* m) { return m ? (int64_t)m->arena.cap : 0; }

extern "C" int aurora_hip_guard_words(const aurora_hip_model* m, float out[4], void* stream) {
  GUARDED({
    REQUIRE(m && out && m->ctx_max.p, "guard_words: bad arguments");
    static_assert(AURORA_F16_SAFE_RANGE == F16_SAFE, "the header's constant is the step's");
    hip_ok(hipMemcpyAsync(out, m->ctx_max.p, 4 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream), "guard_words");
    hip_ok(hipStreamSynchronize((hipStream_t)stream), "guard_words");
  })
}
