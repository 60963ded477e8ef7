// The tiny (3 x 13 / 13 x 3) per-column cross attentions of the Perceiver resamplers (HBM-bound), from keys or from
// pre-multiplied scores.  Lane layout and the sum across a group: perceiver.h; the re-associated decoder path:
// perceiver_out.hip.
#include <math.h>

#include <type_traits>

#include "perceiver.h"

namespace aurora {
namespace {

struct PercArgs {
  const void* q; int64_t q_col_stride; const void* kv; void* out;
  int B; int64_t cols_per_b, kv_bstride, kv_lstride; int Lq, Lk, heads;
  const float* pair_guard; float pair_limit;   // fp32 results leave as fp16 pairs iff *pair_guard < pair_limit (else fp32)
  const float* skip_guard; float skip_limit;   // the launch retires at once iff *skip_guard < skip_limit (null: never)
};

// QC: queries taken together, so that a column's keys / values are read once per chunk of QC queries, not once per query.
// Chosen from Lq at launch (perceiver_chunk below): 3 for the encoder's three latent queries (a chunk of 4 computed a fourth,
// discarded, query: a third more arithmetic), 7 for the decoder's thirteen level queries (7 + 6: two passes over the three keys
// instead of four, and 14 slots for 13 queries instead of 16), 4 otherwise.
// FEWK: at most four keys (the decoder's three latent levels): the column's keys and values are read ONCE, into
// registers, for all query chunks, and a query's softmax is taken over its (<= 4) scores at once -- one exponential per
// score and no running-maximum rescaling of the output (the online form: two exponentials and a rescale per key).
template <typename T, int HDIM, int QC, bool FEWK = false>
__global__ __launch_bounds__(256) void perceiver_attention_kernel(const PercArgs p) {
  constexpr int LPG = HDIM / 4;   // lanes per (column, head)
  if (p.skip_guard != nullptr && *p.skip_guard < p.skip_limit) return;   // (uniform) the re-associated pair does the work
  const int inner = p.heads * HDIM;
  // (the decomposition of perceiver.h)
  const int64_t n_cols = (int64_t)p.B * p.cols_per_b;
  const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LPG;
  const int d0 = (int)(threadIdx.x % LPG) * 4;
  if (grp >= n_cols * p.heads) return;   // (whole groups leave together)
  const int h = (int)(grp % p.heads);
  const int64_t col = grp / p.heads;
  const int b = (int)(col / p.cols_per_b);
  const int64_t l = col - (int64_t)b * p.cols_per_b;
  const float scale = rsqrtf((float)HDIM);
  const bool pairs = std::is_same<T, float>::value && p.pair_guard != nullptr && *p.pair_guard < p.pair_limit;   // (uniform)
  const T* kv0 = reinterpret_cast<const T*>(p.kv) + (b * p.kv_bstride + l) * (2 * (int64_t)inner) + h * HDIM + d0;
  const int64_t kv_step = p.kv_lstride * (2 * (int64_t)inner);
  float kk[FEWK ? 4 : 1][4], vv[FEWK ? 4 : 1][4];
  if constexpr (FEWK) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const T* kp = kv0 + (j < p.Lk ? j : 0) * kv_step;   // (a slot past Lk repeats key 0; its weight is zero)
      load4(kp, kk[j]);
      load4(kp + inner, vv[j]);
    }
  }
  for (int i0 = 0; i0 < p.Lq; i0 += QC) {
    float qv[QC][4], o[QC][4], mx[QC], sum[QC];
#pragma unroll
    for (int c = 0; c < QC; ++c) {
      const int i = i0 + c < p.Lq ? i0 + c : p.Lq - 1;   // (a padded slot repeats the last query; not stored)
      load4(reinterpret_cast<const T*>(p.q) + (col * p.q_col_stride + i) * inner + h * HDIM + d0, qv[c]);
      o[c][0] = o[c][1] = o[c][2] = o[c][3] = 0.f;
      mx[c] = -INFINITY;
      sum[c] = 0.f;
    }
    if constexpr (FEWK) {
#pragma unroll
      for (int c = 0; c < QC; ++c) {
        float sc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = fmaf(qv[c][0], kk[j][0], fmaf(qv[c][1], kk[j][1], fmaf(qv[c][2], kk[j][2], qv[c][3] * kk[j][3])));
          sc[j] = j < p.Lk ? group_sum<LPG>(d) * scale : -INFINITY;
        }
        const float m = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = __expf(sc[j] - m);   // (exp(-inf) = 0 for the slots past Lk)
        sum[c] = (e[0] + e[1]) + (e[2] + e[3]);
#pragma unroll
        for (int d = 0; d < 4; ++d) o[c][d] = fmaf(e[0], vv[0][d], fmaf(e[1], vv[1][d], fmaf(e[2], vv[2][d], e[3] * vv[3][d])));
      }
    }
#pragma unroll 4   // (several keys' loads in flight; the online-softmax chain only orders the arithmetic)
    for (int j = 0; j < (FEWK ? 0 : p.Lk); ++j) {
      const T* kp = kv0 + j * kv_step;
      float k4[4], v4[4];
      load4(kp, k4);
      load4(kp + inner, v4);
#pragma unroll
      for (int c = 0; c < QC; ++c) {
        float sc = fmaf(qv[c][0], k4[0], fmaf(qv[c][1], k4[1], fmaf(qv[c][2], k4[2], qv[c][3] * k4[3])));
        sc = group_sum<LPG>(sc) * scale;
        const float nm = fmaxf(mx[c], sc);
        // (__expf = v_exp_f32 of the scaled argument: 2 instructions against expf's ~10; its argument error, 6e-8 |x|,
        // only matters for terms that are themselves ~e^-|x|)
        const float corr = __expf(mx[c] - nm), e = __expf(sc - nm);
        mx[c] = nm;
        sum[c] = sum[c] * corr + e;
#pragma unroll
        for (int d = 0; d < 4; ++d) o[c][d] = fmaf(e, v4[d], o[c][d] * corr);
      }
    }
#pragma unroll
    for (int c = 0; c < QC; ++c) {
      if (i0 + c < p.Lq) {
        const float inv = 1.0f / sum[c];
        const float r4[4] = {o[c][0] * inv, o[c][1] * inv, o[c][2] * inv, o[c][3] * inv};
        if (pairs) {
          // the fp16-pair layout of the two-term GEMM that reads this next (to_out): lanes 2i, 2i+1 hold 8 consecutive
          // features between them and trade halves, the even lane stores the eight high halves, the odd one the remainders
          uint32_t h0, h1, l0, l1;
          split_pair_f16(r4[0], r4[1], h0, l0);
          split_pair_f16(r4[2], r4[3], h1, l1);
          const bool odd = (threadIdx.x & 1) != 0;
          auto swap1 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, true); };
          const uint32_t s0 = swap1(odd ? h0 : l0), s1 = swap1(odd ? h1 : l1);
          const int f8 = (h * HDIM + d0) & ~7;
          char* d = reinterpret_cast<char*>(p.out) + ((col * p.Lq + i0 + c) * inner + (f8 & ~31)) * 4 + (f8 & 31) * 2 + (odd ? 64 : 0);
          *reinterpret_cast<u32x4*>(d) = odd ? u32x4{s0, s1, l0, l1} : u32x4{h0, h1, s0, s1};
        } else {
          store4(reinterpret_cast<T*>(p.out) + (col * p.Lq + i0 + c) * inner + h * HDIM + d0, r4);
        }
      }
    }
  }
}

// The same attention from PRE-MULTIPLIED scores (first Perceiver layer: its queries are model constants, so
//   q_l . (W_k x_j) = (W_k^T q_l) . x_j
// and the key half of to_kv shrinks from `inner` columns to Lq * heads -- the rows W_k^T q_l / sqrt(head_dim) are made when the
// weights are packed, model_weights.hip:score_weights).  A context row of `vs` holds [v (inner) | ... scores at s_off: (query l, head h)
// at l * heads + h].  Lane layout as above; a group's scores are the same address in all its lanes (one broadcast load), the
// softmax needs no cross-lane traffic at all: two passes over a query's Lk scores (maximum, then exponentials), one over
// the values.  QC queries share a pass over the column's values.
struct PercScoreArgs {
  const float* vs; int64_t ld; int s_off; void* out;
  int B; int64_t cols_per_b, kv_bstride, kv_lstride; int Lq, Lk, heads;
  const float* pair_guard; float pair_limit;
  const float* skip_guard; float skip_limit;
};

template <int HDIM, int QC>
__global__ __launch_bounds__(256) void perceiver_attention_scores_kernel(const PercScoreArgs p) {
  constexpr int LPG = HDIM / 4;
  if (p.skip_guard != nullptr && *p.skip_guard < p.skip_limit) return;   // (uniform)
  const int inner = p.heads * HDIM;
  // (the decomposition of perceiver.h)
  const int64_t n_cols = (int64_t)p.B * p.cols_per_b;
  const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LPG;
  const int d0 = (int)(threadIdx.x % LPG) * 4;
  if (grp >= n_cols * p.heads) return;   // (whole groups leave together)
  const int h = (int)(grp % p.heads);
  const int64_t col = grp / p.heads;
  const int b = (int)(col / p.cols_per_b);
  const int64_t l = col - (int64_t)b * p.cols_per_b;
  const bool pairs = p.pair_guard != nullptr && *p.pair_guard < p.pair_limit;   // (uniform)
  const float* row0 = p.vs + (b * p.kv_bstride + l) * p.ld;
  const int64_t step = p.kv_lstride * p.ld;
  for (int i0 = 0; i0 < p.Lq; i0 += QC) {
    const float* sc[QC];
    float mx[QC], sum[QC], o[QC][4];
#pragma unroll
    for (int c = 0; c < QC; ++c) {
      const int i = i0 + c < p.Lq ? i0 + c : p.Lq - 1;   // (a padded slot repeats the last query; not stored)
      sc[c] = row0 + p.s_off + i * p.heads + h;
      mx[c] = -INFINITY;
      sum[c] = 0.f;
      o[c][0] = o[c][1] = o[c][2] = o[c][3] = 0.f;
    }
#pragma unroll 4
    for (int j = 0; j < p.Lk; ++j)
#pragma unroll
      for (int c = 0; c < QC; ++c) mx[c] = fmaxf(mx[c], sc[c][j * step]);
#pragma unroll 4
    for (int j = 0; j < p.Lk; ++j) {
      float v4[4];
      load4(row0 + j * step + h * HDIM + d0, v4);
#pragma unroll
      for (int c = 0; c < QC; ++c) {
        const float e = __expf(sc[c][j * step] - mx[c]);
        sum[c] += e;
#pragma unroll
        for (int d = 0; d < 4; ++d) o[c][d] = fmaf(e, v4[d], o[c][d]);
      }
    }
#pragma unroll
    for (int c = 0; c < QC; ++c) {
      if (i0 + c < p.Lq) {
        const float inv = 1.0f / sum[c];
        const float r4[4] = {o[c][0] * inv, o[c][1] * inv, o[c][2] * inv, o[c][3] * inv};
        if (pairs) {   // the fp16-pair layout, as perceiver_attention_kernel writes it
          uint32_t h0, h1, l0, l1;
          split_pair_f16(r4[0], r4[1], h0, l0);
          split_pair_f16(r4[2], r4[3], h1, l1);
          const bool odd = (threadIdx.x & 1) != 0;
          auto swap1 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, true); };
          const uint32_t s0 = swap1(odd ? h0 : l0), s1 = swap1(odd ? h1 : l1);
          const int f8 = (h * HDIM + d0) & ~7;
          char* d = reinterpret_cast<char*>(p.out) + ((col * p.Lq + i0 + c) * inner + (f8 & ~31)) * 4 + (f8 & 31) * 2 + (odd ? 64 : 0);
          *reinterpret_cast<u32x4*>(d) = odd ? u32x4{s0, s1, l0, l1} : u32x4{h0, h1, s0, s1};
        } else {
          store4(reinterpret_cast<float*>(p.out) + (col * p.Lq + i0 + c) * inner + h * HDIM + d0, r4);
        }
      }
    }
  }
}

// The query chunk (the QC of the kernels above) and whether the few-keys form runs, from the shape.
struct PercChunk { int qc; bool few_keys; };

constexpr PercChunk perceiver_chunk(int Lq, int Lk, int head_dim, bool from_scores) {
  if (Lq % 3 == 0 && Lq <= 6) return {3, false};
  // (from keys, chunks of 7 only up to head_dim 64)
  if (Lq > 8 && (from_scores || head_dim <= 64)) return {7, !from_scores && Lk <= 4};
  return {4, false};
}

constexpr bool chunk_is(PercChunk c, int qc, bool few_keys = false) { return c.qc == qc && c.few_keys == few_keys; }
// the shapes of the model (the encoder's 3 latent queries, the decoder's 13 levels over 3 latents) and head_dim 128
static_assert(chunk_is(perceiver_chunk(3, 13, 32, false), 3) && chunk_is(perceiver_chunk(3, 13, 32, true), 3), "Lq = 3");
static_assert(chunk_is(perceiver_chunk(6, 13, 64, false), 3) && chunk_is(perceiver_chunk(6, 13, 64, true), 3), "Lq = 6");
static_assert(chunk_is(perceiver_chunk(13, 3, 64, false), 7, true), "the decoder: few keys");
static_assert(chunk_is(perceiver_chunk(13, 5, 64, false), 7) && chunk_is(perceiver_chunk(13, 3, 64, true), 7), "Lq = 13");
static_assert(chunk_is(perceiver_chunk(13, 3, 128, false), 4) && chunk_is(perceiver_chunk(13, 3, 128, true), 7), "head_dim 128");
// the boundaries
static_assert(chunk_is(perceiver_chunk(4, 3, 64, false), 4) && chunk_is(perceiver_chunk(8, 3, 64, false), 4) &&
                  chunk_is(perceiver_chunk(9, 3, 64, false), 7, true) && chunk_is(perceiver_chunk(9, 5, 64, false), 7),
              "Lq = 4, 8, 9");
static_assert(chunk_is(perceiver_chunk(4, 3, 64, true), 4) && chunk_is(perceiver_chunk(8, 3, 64, true), 4) &&
                  chunk_is(perceiver_chunk(9, 3, 64, true), 7) && chunk_is(perceiver_chunk(9, 4, 64, false), 7, true),
              "Lq = 4, 8, 9 from scores; Lk = 4");

// f(head_dim as a constant) for the head sizes the kernels are built for; false for any other
template <typename F>
bool for_head_dim(int head_dim, F&& f) {
  switch (head_dim) {
    case 16: f(std::integral_constant<int, 16>{}); return true;
    case 32: f(std::integral_constant<int, 32>{}); return true;
    case 64: f(std::integral_constant<int, 64>{}); return true;
    case 128: f(std::integral_constant<int, 128>{}); return true;
    default: return false;
  }
}

// (every chunk is built for every head size, also those perceiver_chunk never picks there)
template <typename T, int HDIM>
void launch_keys(PercChunk c, dim3 grid, void* stream, const PercArgs& p) {
  const dim3 block(256);
  if (c.qc == 3) hipLaunchKernelGGL((perceiver_attention_kernel<T, HDIM, 3>), grid, block, 0, as_stream(stream), p);
  else if (c.qc == 7 && c.few_keys) hipLaunchKernelGGL((perceiver_attention_kernel<T, HDIM, 7, true>), grid, block, 0, as_stream(stream), p);
  else if (c.qc == 7) hipLaunchKernelGGL((perceiver_attention_kernel<T, HDIM, 7>), grid, block, 0, as_stream(stream), p);
  else hipLaunchKernelGGL((perceiver_attention_kernel<T, HDIM, 4>), grid, block, 0, as_stream(stream), p);
}

template <int HDIM>
void launch_scores(PercChunk c, dim3 grid, void* stream, const PercScoreArgs& p) {
  const dim3 block(256);
  if (c.qc == 3) hipLaunchKernelGGL((perceiver_attention_scores_kernel<HDIM, 3>), grid, block, 0, as_stream(stream), p);
  else if (c.qc == 7) hipLaunchKernelGGL((perceiver_attention_scores_kernel<HDIM, 7>), grid, block, 0, as_stream(stream), p);
  else hipLaunchKernelGGL((perceiver_attention_scores_kernel<HDIM, 4>), grid, block, 0, as_stream(stream), p);
}

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_perceiver_attention(const void* q, int64_t q_col_stride, const void* kv, void* out,
                                              int B, int64_t cols_per_b, int64_t kv_bstride, int64_t kv_lstride,
                                              int Lq, int Lk, int heads, int head_dim, int dtype, void* stream) {
  return aurora_hip_perceiver_attention_ex(q, q_col_stride, kv, out, B, cols_per_b, kv_bstride, kv_lstride, Lq, Lk, heads,
                                           head_dim, dtype, nullptr, 0.f, stream);
}

extern "C" int aurora_hip_perceiver_attention_ex(const void* q, int64_t q_col_stride, const void* kv, void* out,
                                                 int B, int64_t cols_per_b, int64_t kv_bstride, int64_t kv_lstride,
                                                 int Lq, int Lk, int heads, int head_dim, int dtype,
                                                 const float* pair_guard, float pair_limit, void* stream) {
  return aurora_hip_perceiver_attention_unless(q, q_col_stride, kv, out, B, cols_per_b, kv_bstride, kv_lstride, Lq, Lk, heads,
                                               head_dim, dtype, pair_guard, pair_limit, nullptr, 0.f, stream);
}

extern "C" int aurora_hip_perceiver_attention_unless(const void* q, int64_t q_col_stride, const void* kv, void* out,
                                                     int B, int64_t cols_per_b, int64_t kv_bstride, int64_t kv_lstride,
                                                     int Lq, int Lk, int heads, int head_dim, int dtype,
                                                     const float* pair_guard, float pair_limit, const float* skip_guard,
                                                     float skip_limit, void* stream) {
  AURORA_CHECK_ARG(dtype == AURORA_F32 || dtype == AURORA_BF16, "perceiver_attention: bad dtype");
  AURORA_CHECK_ARG(Lq > 0 && Lk > 0 && heads > 0 && B > 0 && cols_per_b > 0, "perceiver_attention: empty problem");
  AURORA_CHECK_ARG(pair_guard == nullptr || (dtype == AURORA_F32 && (heads * head_dim) % 32 == 0 && head_dim % 8 == 0),
                   "perceiver_attention: fp16-pair output needs fp32 and heads * head_dim %% 32 == 0");
  PercArgs p{q, q_col_stride, kv, out, B, cols_per_b, kv_bstride, kv_lstride, Lq, Lk, heads, pair_guard, pair_limit, skip_guard,
             skip_limit};
  const int64_t items = (int64_t)B * cols_per_b * heads * (head_dim / 4);   // one lane per 4 features of a head
  const dim3 grid(blocks_for(items, 256));
  const PercChunk chunk = perceiver_chunk(Lq, Lk, head_dim, false);
  const bool built = for_head_dim(head_dim, [&](auto HD) {
    if (dtype == AURORA_F32) launch_keys<float, decltype(HD)::value>(chunk, grid, stream, p);
    else launch_keys<bf16_t, decltype(HD)::value>(chunk, grid, stream, p);
  });
  AURORA_CHECK_ARG(built, "perceiver_attention: head_dim %d not in {16,32,64,128}", head_dim);
  return check_launch("perceiver_attention");
}

extern "C" int aurora_hip_perceiver_attention_scores(const float* vs, int64_t ld_vs, int s_off, void* out, int B,
                                                     int64_t cols_per_b, int64_t kv_bstride, int64_t kv_lstride, int Lq, int Lk,
                                                     int heads, int head_dim, const float* pair_guard, float pair_limit,
                                                     const float* skip_guard, float skip_limit, void* stream) {
  AURORA_CHECK_ARG(vs && out && Lq > 0 && Lk > 0 && heads > 0 && B > 0 && cols_per_b > 0, "perceiver_attention_scores: empty problem");
  if (const int rc = check_scores_row("perceiver_attention_scores", vs, ld_vs, s_off, Lq, heads, head_dim)) return rc;
  AURORA_CHECK_ARG(pair_guard == nullptr || ((heads * head_dim) % 32 == 0 && head_dim % 8 == 0),
                   "perceiver_attention_scores: fp16-pair output needs heads * head_dim %% 32 == 0");
  PercScoreArgs p{vs, ld_vs, s_off, out, B, cols_per_b, kv_bstride, kv_lstride, Lq, Lk, heads, pair_guard, pair_limit, skip_guard,
                  skip_limit};
  const int64_t items = (int64_t)B * cols_per_b * heads * (head_dim / 4);
  const dim3 grid(blocks_for(items, 256));
  const PercChunk chunk = perceiver_chunk(Lq, Lk, head_dim, true);
  const bool built = for_head_dim(head_dim, [&](auto HD) { launch_scores<decltype(HD)::value>(chunk, grid, stream, p); });
  AURORA_CHECK_ARG(built, "perceiver_attention_scores: head_dim %d not in {16,32,64,128}", head_dim);
  return check_launch("perceiver_attention_scores");
}
