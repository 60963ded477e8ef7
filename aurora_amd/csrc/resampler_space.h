// Workspace layout of one resampler layer (step.hip:resampler_layer takes it from the arena; the stages of `resampler` use
// it in the order tests/resampler_space_check.cpp replays).  Plain values in, byte offsets out: nothing here knows
// HIP or the model, so that a host program can replay the layout without a device (tests/resampler_space_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace aurora {

constexpr size_t round256(size_t x) { return (x + 255) & ~size_t(255); }

// What the layout depends on: the widths of layer `layer` of a resampler, which of its optional weights exist, the
// resampler's score weights (model_weights.hip:score_weights), the model's switches and the shape of the call.
struct LayerShape {
  size_t layer;                              // index of the layer in its resampler
  int dim, inner, hidden, head_dim, heads;
  int n_vs, vs_lq;                           // of the resampler: row width of [v | scores] and the Lq it was packed for (0: none)
  bool ln_k, to_out_s, fc1_s, fc2_s;         // LayerNorm on the keys; pre-split (fp16-pair) weights of to_out / fc1 / fc2
  int f16_mode;
  bool reassoc_out;                          // the model's switch (AURORA_PERCEIVER_REASSOC)
  bool out_supported;                        // aurora_hip_perceiver_out_supported(Lq, Lk, heads, head_dim, dim)
  int B;
  int64_t cols, ctx_rows;
  int Lq, Lk;
};

// Workspace of a resampler layer: three regions instead of one buffer per intermediate (the decoder's intermediates are
// 3.5 GB each at 0.25 degree) --
//   Y  the layer's result (it outlives the rest; stack order); until fc2 writes it, it holds the attention output
//   L  the MLP's input / residual (LayerNorm 1 output): fp32 values, or their fp16 pairs
//   S  scratch: k | v (and q), then to_out's result, then the MLP's hidden layer, each dead before the next is written;
//      the MLP runs in row chunks so that a chunk's hidden layer fits
// Y and L are `unit` bytes each, S is `s_bytes`; the offsets are into S.
struct LayerSpace {
  size_t unit, kv_bytes, q_bytes, att_off, p_off, p_bytes, s_bytes, hid_row;
  int kv_ld;
  int64_t chunk_rows;
  bool scores, att_in_y, att_pairs, reassoc, pairs;
};
inline LayerSpace layer_space(const LayerShape& ly) {
  const int inner = ly.inner, Dd = ly.dim, Lq = ly.Lq, Lk = ly.Lk;
  const size_t i = ly.layer;
  const int64_t n_cols = (int64_t)ly.B * ly.cols, n_rows = n_cols * Lq;
  LayerSpace s{};
  s.unit = (size_t)n_rows * Dd * 4;
  // First layer, queries known at pack time: the context rows leave `to_kv` as [v | scores with every query] -- no keys
  // (model_weights.hip:score_weights); else k | v.
  s.scores = i == 0 && ly.n_vs > 0 && ly.vs_lq == Lq && !ly.ln_k;
  s.kv_ld = s.scores ? ly.n_vs : 2 * inner;
  s.kv_bytes = (size_t)ly.ctx_rows * s.kv_ld * 4;
  s.q_bytes = i > 0 ? (size_t)n_rows * inner * 4 : 0;
  const size_t att_bytes = (size_t)n_rows * inner * 4;
  s.att_in_y = att_bytes <= s.unit;   // (inner == dim in every published model; else behind everything it coexists with)
  const size_t kvq_bytes = round256(s.kv_bytes) + round256(s.q_bytes);
  s.att_off = round256(std::max(s.unit, kvq_bytes));
  s.hid_row = (size_t)ly.hidden * 4;
  const size_t hid_min = (size_t)std::min<int64_t>(n_rows, 256) * s.hid_row;   // at least one row tile of the hidden layer
  // The decoder's de-aggregation (first layer: queries shared by all columns, three keys per column) runs RE-ASSOCIATED
  // (perceiver_out.hip): to_out of the three value rows per column and head, then the Lq x 3 convex combinations per head
  // in registers -- the attention output and its Lq-row `to_out` GEMM do not exist.  Its inputs: the softmax weights P
  // (behind to_out's result AND behind k | v, which the launch that writes P is still reading, in the scratch region) and
  // the value rows as fp16 pairs (in the result region, until fc2 writes there).  Two fp16 terms: decided on the device by
  // the guard of the linear it replaces.
  s.att_pairs = ly.to_out_s && inner % 32 == 0;
  s.reassoc = ly.reassoc_out && i == 0 && s.att_pairs && s.att_in_y && ly.f16_mode == 2 &&
              (size_t)n_cols * Lk * inner * 4 <= s.unit && ly.out_supported;
  // (k | v is wider than to_out's result where 3 kv_ld > Lq dim: 3 or 4 levels at the published widths)
  s.p_off = round256(std::max(s.unit, s.kv_bytes));
  s.p_bytes = s.reassoc ? (size_t)n_cols * ly.heads * 64 * 4 : 0;
  s.s_bytes = std::max(std::max(s.att_in_y ? std::max(s.unit, kvq_bytes) : s.att_off + att_bytes, hid_min),
                       s.reassoc ? s.p_off + s.p_bytes : (size_t)0);
  // The MLP in the fp16-pair layout end to end: the LayerNorm writes its result already split (and ONLY split), fc1
  // reads that and writes its GELU'd result split, fc2 reads that -- neither GEMM splits anything -- and the LayerNorm
  // behind the MLP takes the split array as its residual.
  s.pairs = ly.fc1_s && ly.fc2_s && Dd % 32 == 0;
  s.chunk_rows = std::min<int64_t>(n_rows, (int64_t)(s.s_bytes / s.hid_row));
  if (s.chunk_rows < n_rows) s.chunk_rows = s.chunk_rows / 256 * 256;   // whole row tiles per chunk (>= 256 rows fit: hid_min)
  return s;
}

}  // namespace aurora
