// Replays, on the host, the order in which the stages of `resampler` (aurora_amd/csrc/step.hip: project_context, project_queries,
// attend_reassociated / attend_plain, resampler_mlp, over the pointers `resampler_layer` sets) use the regions that `layer_space`
// (aurora_amd/csrc/resampler_space.h) lays out, over every level count, both Perceivers' widths and every switch, and checks
// launch by launch that nothing a launch writes overlaps what the same launch reads or what is still live, and that every
// range lies inside its region.  Prints one line per violating tuple; exit status 1 if there was one.
//
//   resampler_space_check dim,inner,heads,hidden[,enc|dec] ...      (one argument per Perceiver; tests/test_resampler_space.py)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "resampler_space.h"

using aurora::LayerShape;
using aurora::LayerSpace;

namespace {

enum Region { Y, L, S };
struct Range { Region region; size_t lo, hi; const char* name; };

bool overlap(const Range& a, const Range& b) { return a.region == b.region && a.lo < b.hi && b.lo < a.hi && a.lo < a.hi && b.lo < b.hi; }

struct Widths { int dim, inner, heads, hidden; bool encoder; };

struct Check {
  const LayerShape& sh;
  const LayerSpace& sp;
  const char* side;
  int failures = 0;

  void fail(const char* stage, const char* what, const Range* a = nullptr, const Range* b = nullptr) {
    ++failures;
    std::printf("VIOLATION %s layer=%zu dim=%d inner=%d heads=%d Lq=%d Lk=%d n_vs=%d reassoc_out=%d f16_mode=%d ln_k=%d B=%d cols=%lld"
                " | scores=%d reassoc=%d kv_ld=%d unit=%zu kv_bytes=%zu p_off=%zu s_bytes=%zu | %s: %s",
                side, sh.layer, sh.dim, sh.inner, sh.heads, sh.Lq, sh.Lk, sh.n_vs, (int)sh.reassoc_out, sh.f16_mode, (int)sh.ln_k, sh.B,
                (long long)sh.cols, (int)sp.scores, (int)sp.reassoc, sp.kv_ld, sp.unit, sp.kv_bytes, sp.p_off, sp.s_bytes, stage, what);
    if (a) std::printf(" %s %c[%zu, %zu)", a->name, "YLS"[a->region], a->lo, a->hi);
    if (b) std::printf(" over %s %c[%zu, %zu)", b->name, "YLS"[b->region], b->lo, b->hi);
    std::printf("\n");
  }
  void inside(const char* stage, const Range& r) {
    const size_t size = r.region == S ? sp.s_bytes : sp.unit;
    if (r.hi > size || r.lo > r.hi) fail(stage, "outside its region:", &r);
    if (r.lo % 16 != 0) fail(stage, "not 16-byte aligned:", &r);   // every kernel here takes float4 / fp16-pair rows
  }
  // One launch: `writes` against what it reads and what has to survive it.
  void launch(const char* stage, const std::vector<Range>& reads, const std::vector<Range>& live, const std::vector<Range>& writes) {
    for (const Range& r : reads) inside(stage, r);
    for (const Range& w : writes) {
      inside(stage, w);
      for (const Range& r : reads)
        if (overlap(w, r)) fail(stage, "writes what it reads:", &w, &r);
      for (const Range& l : live)
        if (overlap(w, l)) fail(stage, "writes what is still live:", &w, &l);
    }
    for (size_t a = 0; a < writes.size(); ++a)
      for (size_t b = a + 1; b < writes.size(); ++b)
        if (overlap(writes[a], writes[b])) fail(stage, "two results of one launch overlap:", &writes[a], &writes[b]);
  }
};

int replay(const LayerShape& sh, const char* side) {
  const LayerSpace sp = aurora::layer_space(sh);
  Check c{sh, sp, side};
  const int64_t n_cols = (int64_t)sh.B * sh.cols, n_rows = n_cols * sh.Lq;
  const size_t att_bytes = (size_t)n_rows * sh.inner * 4;
  const Range kv{S, 0, sp.kv_bytes, "k|v"};
  const Range q{S, aurora::round256(sp.kv_bytes), aurora::round256(sp.kv_bytes) + sp.q_bytes, "q"};
  const Range att = sp.att_in_y ? Range{Y, 0, att_bytes, "att"} : Range{S, sp.att_off, sp.att_off + att_bytes, "att"};
  const Range P{S, sp.p_off, sp.p_off + sp.p_bytes, "P"};
  const Range Vp{Y, 0, (size_t)n_cols * sh.Lk * sh.inner * 4, "Vp"};
  const Range o{S, 0, sp.unit, "o"};
  const Range lat1{L, 0, sp.unit, "L"};
  std::vector<Range> qs;
  if (sh.layer > 0) qs.push_back(q);
  std::vector<Range> kvq = qs;
  kvq.push_back(kv);

  c.launch("1 to_kv", {}, {}, {kv});                       // project_context (the key LayerNorm, norm_keys, works in place)
  if (sh.layer > 0) c.launch("2 to_q", {}, {kv}, {q});
  if (sp.reassoc) {
    c.launch("3 probs", kvq, {}, {P, Vp});
    c.launch("4 perceiver_out", {P, Vp}, {}, {o});
    // the plain pair behind it runs only where the two above did not (one device word decides): k | v is intact then
    c.launch("3' attention_unless", kvq, {}, {att});
    c.launch("4' to_out", {att}, {}, {o});
  } else {
    c.launch("3 attention", kvq, {}, {att});
    c.launch("4 to_out", {att}, {}, {o});
  }
  c.launch("5 layernorm 1", {o}, {}, {lat1});
  // 6 / 7: fc1 -> fc2 in row chunks through `hid`
  if (sp.chunk_rows < 1) c.fail("6 mlp", "chunk_rows < 1");
  else {
    if (sp.chunk_rows < n_rows && sp.chunk_rows % 256 != 0) c.fail("6 mlp", "a chunk that is not whole row tiles");
    if (sp.chunk_rows > n_rows) c.fail("6 mlp", "a chunk longer than the rows");
    int64_t done = 0;
    for (int64_t r0 = 0; r0 < n_rows; r0 += sp.chunk_rows) {
      const int64_t nr = std::min<int64_t>(sp.chunk_rows, n_rows - r0);
      const Range hid{S, 0, (size_t)nr * sp.hid_row, "hid"};
      const Range l_rows{L, (size_t)r0 * sh.dim * 4, (size_t)(r0 + nr) * sh.dim * 4, "L rows"};
      const Range y_rows{Y, (size_t)r0 * sh.dim * 4, (size_t)(r0 + nr) * sh.dim * 4, "Y rows"};
      c.launch("6 fc1", {l_rows}, {lat1}, {hid});
      c.launch("7 fc2", {hid}, {lat1}, {y_rows});
      done += nr;
      if (c.failures) break;
    }
    if (!c.failures && done != n_rows) c.fail("7 fc2", "the chunks do not cover the rows");
  }
  // the flags the launches above were chosen by
  if (sp.reassoc && !(sh.reassoc_out && sh.layer == 0 && sh.out_supported && sh.f16_mode == 2 && sh.to_out_s)) c.fail("flags", "re-associated where it is not eligible");
  if (sp.scores && !(sh.layer == 0 && sh.n_vs > 0 && sh.vs_lq == sh.Lq && !sh.ln_k)) c.fail("flags", "scores where there are none");
  if (sp.kv_ld != (sp.scores ? sh.n_vs : 2 * sh.inner)) c.fail("flags", "kv_ld");
  return c.failures;
}

// aurora_hip_perceiver_out_supported (csrc/perceiver_out.hip), which this program cannot link: the kernels exist for these shapes
bool out_supported(int Lq, int Lk, int heads, int head_dim, int N) {
  return (Lq == 3 || Lq == 4 || Lq == 13) && Lk == 3 && head_dim == 64 && heads >= 2 && heads % 2 == 0 && N > 0 && N % 128 == 0;
}

int round_up(int x, int m) { return (x + m - 1) / m * m; }

}  // namespace

int main(int argc, char** argv) {
  std::vector<Widths> widths;
  for (int a = 1; a < argc; ++a) {
    Widths w{};
    char side[8] = "";
    if (std::sscanf(argv[a], "%d,%d,%d,%d,%7s", &w.dim, &w.inner, &w.heads, &w.hidden, side) != 5 ||
        (std::strcmp(side, "enc") != 0 && std::strcmp(side, "dec") != 0) || w.dim <= 0 || w.inner <= 0 || w.heads <= 0 ||
        w.inner % w.heads != 0 || w.hidden <= 0) {
      std::fprintf(stderr, "usage: resampler_space_check dim,inner,heads,hidden,enc|dec ...\n");
      return 2;
    }
    w.encoder = std::strcmp(side, "enc") == 0;
    widths.push_back(w);
  }
  if (widths.empty()) {
    std::fprintf(stderr, "usage: resampler_space_check dim,inner,heads,hidden,enc|dec ...\n");
    return 2;
  }
  const int64_t col_counts[] = {1, 7, 32, 4050, 7200};
  long long tuples = 0, reassoc = 0, scores = 0, chunked = 0, att_in_s = 0;
  int failures = 0;
  for (const Widths& w : widths)
    for (int n = 1; n <= 13; ++n) {
      // decoder: Lq = the levels, three latent keys per column; encoder: three latent queries, Lk = the levels
      const int Lq = w.encoder ? 3 : n, Lk = w.encoder ? n : 3;
      const int head_dim = w.inner / w.heads;
      const int n_vs_on = round_up(w.inner + Lq * w.heads, 256) < 2 * w.inner ? round_up(w.inner + Lq * w.heads, 256) : 0;
      for (int score_weights = 0; score_weights < 2; ++score_weights)
        for (int reassoc_out = 0; reassoc_out < 2; ++reassoc_out)
          for (int presplit = 0; presplit < 2; ++presplit)       // f16_mode 2 with every pre-split weight, or -1 with none
            for (int ln_k = 0; ln_k < (w.encoder ? 2 : 1); ++ln_k)   // (`stabilise_level_agg`: the encoder's only)
              for (size_t layer = 0; layer < 2; ++layer)
                for (int64_t cols : col_counts)
                  for (int B = 1; B <= 2; ++B) {
                    LayerShape sh{};
                    sh.layer = layer;
                    sh.dim = w.dim; sh.inner = w.inner; sh.hidden = w.hidden; sh.head_dim = head_dim; sh.heads = w.heads;
                    // (score_weights packs nothing behind a key LayerNorm or without a usable mode: model_weights.hip)
                    sh.n_vs = score_weights && !ln_k ? n_vs_on : 0;
                    sh.vs_lq = sh.n_vs ? Lq : 0;
                    sh.ln_k = ln_k && layer == 0;
                    sh.to_out_s = sh.fc1_s = sh.fc2_s = presplit != 0;
                    sh.f16_mode = presplit ? 2 : -1;
                    sh.reassoc_out = reassoc_out != 0;
                    sh.out_supported = out_supported(Lq, Lk, w.heads, head_dim, w.dim);
                    sh.B = B; sh.cols = cols; sh.ctx_rows = (int64_t)B * cols * Lk; sh.Lq = Lq; sh.Lk = Lk;
                    failures += replay(sh, w.encoder ? "encoder" : "decoder");
                    const LayerSpace sp = aurora::layer_space(sh);
                    ++tuples; reassoc += sp.reassoc; scores += sp.scores; att_in_s += !sp.att_in_y;
                    chunked += sp.chunk_rows < (int64_t)B * cols * Lq;
                  }
    }
  std::printf("%lld tuples (%lld re-associated, %lld with scores, %lld with a chunked MLP, %lld with att in S): %d violations\n", tuples,
              reassoc, scores, chunked, att_in_s, failures);
  return failures ? 1 : 0;
}
