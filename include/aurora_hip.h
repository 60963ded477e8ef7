/*
 * aurora_hip.h -- C ABI of libaurora_hip.so, the MI355X (gfx950) compute library behind
 * aurora_amd.Aurora.forward / rollout.
 *
 * The reference (microsoft/aurora) has no FFI: its operator boundary is the torch.nn.Module
 * call interface.  Every entry point below therefore replaces one
 * torch-level operator group of the reference's hot path and cites it.  All pointers are raw
 * DEVICE pointers (hipMalloc'ed / torch-allocated), `stream` is a hipStream_t passed as void*,
 * sizes are element counts unless stated, strides ("ld*") are in elements.  No torch types.
 * Every function only enqueues work on `stream` and returns 0 on success or a negative
 * AURORA_E_* code; aurora_hip_last_error() describes the last failure of the calling thread.
 *
 * dtype codes: AURORA_F32 = 0 (float), AURORA_BF16 = 1 (bfloat16, raw uint16 storage), AURORA_F64 = 2 (double; regrid
 * sources only).
 */
#ifndef AURORA_HIP_H
#define AURORA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AURORA_F32 0
#define AURORA_BF16 1
#define AURORA_F64 2

#define AURORA_OK 0
#define AURORA_E_ARG (-1)     /* invalid argument (shape / alignment / dtype) */
#define AURORA_E_LAUNCH (-2)  /* HIP launch error */

#define AURORA_ACT_NONE 0
#define AURORA_ACT_GELU 1 /* exact erf GELU (torch.nn.GELU default) */
#define AURORA_ACT_SILU 2 /* x * sigmoid(x) (time_mlp / AdaLN modulation, swin3d.py:805-809, film.py:28) */

const char* aurora_hip_last_error(void);
int aurora_hip_version(void);

/* ---- dense linear layers ------------------------------------------------------------------
 * C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) (+ residual[M,N]);  W is nn.Linear's (out,in)
 * row-major weight.  A, W, C share `dtype`; accumulation is fp32 on the MFMA units
 * (v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x4_f32).  bias and residual are fp32 (nullable).
 * C2 (nullable) receives a second copy of the result in the OTHER dtype (fp32 <-> bf16).
 * ldr == 0 broadcasts one residual row to every output row.
 * Constraints: K * sizeof(dtype) % 128 == 0 (zero-pad K otherwise); lda/ldw multiples of
 * 16 bytes; operand pointers 16-byte aligned.  Outputs whose rows are not 16-byte aligned take
 * a scalar store path.
 * Replaces F.linear call sites: swin3d.py:59-66,153,169,554,609-612, perceiver.py:79-88,
 * 141-152, encoder.py:318-363, decoder.py:214-263, film.py:48, patchembed.py:112 (as GEMM
 * over unfolded patches).
 */
int aurora_hip_linear(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                      void* C, int64_t ldc, void* C2, int64_t ldc2,
                      const float* residual, int64_t ldr,
                      int64_t M, int N, int K, int dtype, int act, void* stream);

/* aurora_hip_linear with the fp32 numerics chosen PER CALL (the library keeps no mutable state):
 * f32_gemm says how a large fp32 linear (N % 256 == 0) is multiplied; -1 takes the process default.
 *   1 (default): every fp32 operand is split exactly into three bf16 terms and six bf16 MFMAs per K-slab
 *      reproduce the fp32 product to ~1e-7 relative (fp32-grade, no range restriction, 16/6 of the fp32 MFMA rate).
 *   2: two fp16 terms (round-to-nearest: a_h + a_l = a to 2^-24 |a|), three fp16 MFMAs, the weight operand scaled
 *      by 2^6 and the result scaled back exactly.  Same accuracy, but inside fp16's range only: activations must
 *      satisfy |x| < 65504 (|x| < 0.25 carries an absolute error of up to 3e-8), weights |w| < 1000.  Meant for
 *      linears whose input is bounded by construction (a LayerNorm output, the GELU of a linear of one), whatever
 *      the model inputs are.  With `guard` != NULL the decision is taken on the device, per launch: the two-term
 *      split runs only if *guard < guard_limit, else the three-term bf16 split -- the caller leaves max |activation|
 *      (or an upper bound of it, scaled into guard_limit) there, e.g. with aurora_hip_absmax, without any host
 *      synchronisation.
 *   0: native v_mfma_f32_16x16x4_f32 FMA chains (bitwise an fp32 FMA chain; erff in the GELU epilogue).
 * The environment variable AURORA_F32_GEMM=native|bf16|f16 sets the process default, which
 * aurora_hip_default_f32_gemm() reports.  The reference's counterpart is the fp32 F.linear outside autocast
 * (encoder.py / decoder.py, aurora.py:322-349). */
int aurora_hip_linear_ex(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                         void* C, int64_t ldc, void* C2, int64_t ldc2,
                         const float* residual, int64_t ldr,
                         int64_t M, int N, int K, int dtype, int act,
                         int f32_gemm, const float* guard, float guard_limit, void* stream);
int aurora_hip_default_f32_gemm(void);
/* `batch` independent problems of the same shape in ONE launch (strided batch): problem g reads A + g * stride_a,
 * W + g * stride_w, bias + g * stride_bias and writes C + g * stride_c (strides in elements; every problem stays 16-byte
 * aligned; stride 0 shares an operand).  Same kernels, modes and constraints as aurora_hip_linear_ex, no second output /
 * residual.  Replaces the reference's per-level Python loops: LevelConditioned patch embeddings and heads
 * (levelcond.py:36-69: one weight per pressure level) and the per-level bias of the atmospheric patch embedding
 * (encoder.py:318-330). */
int aurora_hip_linear_batched(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C, int64_t ldc,
                              int64_t M, int N, int K, int dtype, int act, int f32_gemm, const float* guard,
                              float guard_limit, int batch, int64_t stride_a, int64_t stride_w, int64_t stride_bias,
                              int64_t stride_c, void* stream);

/* Which kernel the calls above would launch, without launching anything: the argument checks and the dispatch decision of
 * the launch path itself, run on a description of the call.  Host arithmetic only; with cus > 0 no device is needed.
 *   f32_gemm                  : as aurora_hip_linear_ex, AURORA_F32_*_SPLIT bits included; has_guard: a guard word is given.
 *   ldc / c_addr              : leading dimension and address of C -- of the address only its value modulo 16 is read (a
 *                               real address, or 16 + a byte offset); likewise ldc2 / c2_addr and ldr / residual_addr,
 *                               address 0 = no second output / no residual.
 *   workspace_bytes, n_tickets, split : the scratch of aurora_hip_linear_ws; workspace_bytes < 0 = a call without scratch.
 *   plane_stride, plane_heads : aurora_hip_linear_planes (0, 0 otherwise).
 *   cus                       : compute units of the device to plan for; 0 = the current device's.
 * plan_out[0..5]: kernel (AURORA_PLAN_*), 1 if a guarded two-term launch is followed by its three-term twin, tile rows,
 * tile columns, K slices (0 or 1: none), and whether the kernels would use their 16-byte stores (all of C, C2 and the
 * residual 16-byte aligned row by row).  Returns what the call itself would return for bad arguments. */
#define AURORA_PLAN_F32_THREE 0
#define AURORA_PLAN_F32_TWO 1
#define AURORA_PLAN_F32_PP 2
#define AURORA_PLAN_F32_PP_W 3
#define AURORA_PLAN_F32_PP_AW 4
#define AURORA_PLAN_F32_PP_W_TALL 5
#define AURORA_PLAN_F32_PP_AW_TALL 6
#define AURORA_PLAN_TILE128 7
#define AURORA_PLAN_RING 8
#define AURORA_PLAN_RING_MID 9
#define AURORA_PLAN_PP 10
#define AURORA_PLAN_PP_SPLITK 11
#define AURORA_PLAN_A4 12
int aurora_hip_linear_plan(int64_t M, int N, int K, int dtype, int f32_gemm, int has_guard, int batch, int64_t ldc,
                           int64_t c_addr, int64_t ldc2, int64_t c2_addr, int64_t ldr, int64_t residual_addr,
                           int64_t workspace_bytes, int n_tickets, int split, int64_t plane_stride, int plane_heads,
                           int cus, int32_t* plan_out);

/* aurora_hip_linear for callers that can lend scratch memory: a bf16 linear with few 256 x 256 tiles and a long K (the
 * per-rank shapes of a latitude band at the coarse backbone stages, swin3d.py:59-66,153,169 at M = 2,160: 72 tiles on
 * 256 CUs, K = 8192) is then split along K inside ONE launch -- every tile's K range is cut into `split` slices, one
 * workgroup each; slices publish their fp32 accumulators to `workspace` and take a ticket of their tile, and whoever
 * draws a tile's last ticket adds the slices up in slice order and runs the epilogue.  No workgroup waits for another
 * (nothing depends on dispatch order), the result does not depend on arrival order; it differs from the un-split
 * product by the rounding of split - 1 fp32 additions per element.
 *   aurora_hip_linear_workspace: bytes of scratch the library would like for this shape (0: it would not split).
 *   workspace, workspace_bytes : 16-byte aligned scratch, contents irrelevant; too small / NULL = no split.
 *   tickets, n_tickets         : int32 words, ZERO on entry and left zero (one per tile); fewer than tiles = no split.
 *                                NOT validated: a count left behind by a launch that never finished (a device fault, a
 *                                torn-down graph) means no workgroup of that tile ever draws its last ticket -- the tile's
 *                                output rows are never written, silently.  A device-side abort returns normally to the
 *                                host, so "after a failed launch" cannot be told: re-zero the words (hipMemsetAsync) ahead
 *                                of a batch of launches -- the model handle does so at the start of EVERY sharded step.
 *                                Two launches that may run at the same time need their own ticket words.
 *   split                      : 0 lets the library choose, 1 forbids, > 1 asks for that many slices.
 * fp32 problems and shapes that would not split run exactly as aurora_hip_linear. */
int64_t aurora_hip_linear_workspace(int64_t M, int N, int K, int dtype);
int aurora_hip_linear_ws(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C, int64_t ldc,
                         void* C2, int64_t ldc2, const float* residual, int64_t ldr, int64_t M, int N, int K, int dtype,
                         int act, void* workspace, int64_t workspace_bytes, int32_t* tickets, int n_tickets, int split,
                         void* stream);

/* The qkv linear of a Swin block (swin3d.py:153) with its result in HEAD PLANES instead of rows: the 64-column blocks of
 * C = A W^T + bias are q, k, v of the attention heads (block sel * heads + h, swin3d.py:154-156 reshapes exactly these);
 * head h owns a plane of [M rows][q | k | v = 192 elements] bf16, `plane_stride` elements (>= 192 M, a multiple of 8)
 * behind the previous head's.  The window attention gathers q, k and v of one (token, head) at a time: in a plane that is
 * 384 contiguous bytes, and a window's runs of consecutive tokens are contiguous runs of DRAM; in rows of 3 D elements
 * they are three 128-byte pieces D * 2 bytes apart, every token 3 D * 2 bytes further (aurora_hip_window_attention_planes
 * reads this layout).  N = 64 heads x 3, or x 2 / x 1 with C moved 64 / 128 elements into the row (k | v of halo rows).
 * bf16 only; same arithmetic and bits as aurora_hip_linear. */
int aurora_hip_linear_planes(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C,
                             int64_t plane_stride, int heads, int64_t M, int N, int K, int dtype, void* stream);

/* Mode 2 with operands that are ALREADY split (flags OR-ed into f32_gemm = 2): the split is the same arithmetic wherever
 * it happens, so results are bit-identical to plain mode 2, but a GEMM whose operands arrive split spends no VALU work
 * on them -- the two-term kernel goes from 0.29 to 0.40 PFLOP/s fp32-equivalent when both do.
 * The fp16-pair layout of a row of K fp32 values (K % 32 == 0) occupies the same K * 4 bytes: per group of 32 features
 * 128 bytes, first the 32 fp16 high halves h = fp16(x), then the 32 fp16 remainders l = fp16(x - h); strides stay in
 * 4-byte units.  aurora_hip_split_f16 produces it (weights: scale = 64, the 2^6 of mode 2), aurora_hip_layernorm_split
 * and a linear with AURORA_F32_C_SPLIT write it directly.
 *   AURORA_F32_W_SPLIT: W is in the pair layout, scaled by 64.  With a guard the launch runs iff *guard < guard_limit
 *     and has NO fallback of its own: pair it with an f32_gemm = 1 call on the fp32 weights carrying the same guard
 *     (mode 1 with a guard runs iff the guard FAILS).
 *   AURORA_F32_A_SPLIT: A is in the pair layout (unscaled); needs AURORA_F32_W_SPLIT.  With a guard it is for a buffer whose
 *     FORMAT was decided by that same guard and limit on the device: written as pairs by a guarded two-term producer
 *     (AURORA_F32_C_SPLIT) iff the guard holds, as fp32 by its mode-1 twin otherwise -- consumer and producer switch together.
 *   AURORA_F32_C_SPLIT: C is written in the pair layout (after bias / activation / residual); ldc % 32 == 0, no C2.
 * Shapes: N % 256 == 0, K % 32 == 0, K >= 96. */
#define AURORA_F32_A_SPLIT 4
#define AURORA_F32_W_SPLIT 8
#define AURORA_F32_C_SPLIT 16
int aurora_hip_split_f16(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int K,
                         float scale, void* stream);

/* out[0] = max |x[i]| over n contiguous fp32 values (x 16-byte aligned); NaNs are ignored.
 * aurora_hip_absmax_fold: out[0] = max(out[0], max |x[i]|) -- no zeroing, so that several producers can share one word;
 * aurora_hip_zero_words clears n <= 64 such words with one tiny launch (a step clears all of its guard words at once:
 * a 4-byte hipMemsetAsync in front of every absmax cost a latitude band ~90 us each). */
int aurora_hip_absmax(const float* x, int64_t n, float* out, void* stream);
int aurora_hip_absmax_fold(const float* x, int64_t n, float* out, void* stream);
int aurora_hip_zero_words(float* words, int n, void* stream);

/* ---- 3D shifted-window attention core ------------------------------------------------------
 * For every window w and head h: O = softmax(Q K^T / sqrt(hd) + mask) V over the window's
 * `win_tokens` (<= 144) tokens.  qkv: [B][L][3*D] with columns q | k | v, each head-major
 * (swin3d.py:153-155).  The roll / pad / window-partition / reverse / crop / un-roll index
 * permutations of swin3d.py:471-505 are folded into `tok` (int32 [n_windows][win_tokens],
 * token index inside one batch element or -1 for a zero-padded position; padded positions
 * carry q = k = v = qkv_bias, exactly as Linear(0) does in the reference).  `grp`
 * (uint8 [n_windows][win_tokens], nullable) holds the communication-group labels of
 * compute_3d_shifted_window_mask (swin3d.py:303-360): score += -100 where labels differ.
 * Output O: [B][L][D], token order, padded positions are not written.  head_dim must be 64.
 * Replaces WindowAttention.forward's SDPA (swin3d.py:154-168) + swin3d.py:177-285,471-505.
 * Latitude-band sharding: a rank passes qkv = [owned rows | halo rows received from its
 * neighbours] (L rows) and L_out = number of owned rows; outputs are written for tokens < L_out
 * only (out has L_out rows per batch element).  Un-sharded callers pass L_out = L.
 */
int aurora_hip_window_attention(const void* qkv, const float* qkv_bias, void* out,
                                const int32_t* tok, const uint8_t* grp,
                                int B, int64_t L, int64_t L_out, int D, int heads, int n_windows,
                                int win_tokens, int dtype, void* stream);
/* The same with q | k | v in head planes (aurora_hip_linear_planes): head h owns [B * L rows][q | k | v = 192 elements]
 * bf16, planes `plane_stride` elements apart (>= 192 B L); row b * L + t is token t of batch element b.
 * plane_stride = 0: the row layout above.  Same results, bit for bit. */
int aurora_hip_window_attention_planes(const void* qkv, int64_t plane_stride, const float* qkv_bias, void* out,
                                       const int32_t* tok, const uint8_t* grp,
                                       int B, int64_t L, int64_t L_out, int D, int heads, int n_windows,
                                       int win_tokens, int dtype, void* stream);

/* ---- (adaptive) layer norm with residual --------------------------------------------------
 * out[r,:] = res[r % res_mod? ,:] + LN(y[r,:]) * gain[:] + shift[:]   (res nullable)
 * y: [M][D] of `dtype` with row stride ldy; statistics in fp32, eps as given.
 * gain/shift: fp32 [D] (AdaLN: scale_bias + scale, shift -- film.py:48-49; affine LN: weight,
 * bias).  res: fp32, row stride ldr; row index is r, or r % res_mod when res_mod > 0
 * (Perceiver latents broadcast over grid columns, perceiver.py:224-232).
 * out_f32 (nullable, stride ldo) and out_t (nullable, `dtype`, stride ldt) receive the result.
 * Replaces swin3d.py:507-508, perceiver.py:224-232, encoder.py:320, perceiver.py:144-147.
 */
int aurora_hip_layernorm(const void* y, int64_t ldy, const float* gain, const float* shift,
                         const float* res, int64_t ldr, int64_t res_mod,
                         float* out_f32, int64_t ldo, void* out_t, int64_t ldt,
                         int64_t M, int D, float eps, int dtype, void* stream);
/* bf16 linear + (adaptive) LayerNorm + residual in ONE launch, for N = D = 512 (stage 0 of the backbone):
 *     x_out = x_in + LN(A W^T + bias) * gain + shift,     x_bf16 = bf16(x_out)   (nullable)
 * i.e. `x = shortcut + norm1(proj(attn), c)` and `x = x + norm2(mlp(x), c)` of a Swin block (swin3d.py:507-508,
 * film.py:38-49) without writing the linear's result to memory.  A, W bf16 (K contiguous, K % 32 == 0, K >= 96); the
 * linear's result is rounded to bf16 before the statistics, as the reference's autocast linear is; fp32 statistics
 * (two passes), fp32 residual stream; x_out may alias x_in.  One workgroup owns 128 whole rows. */
int aurora_hip_linear_layernorm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                                const float* gain, const float* shift,
                                const float* x_in, int64_t ldx, float* x_out, int64_t ldo,
                                void* x_bf16, int64_t ldb, int64_t M, int N, int K, float eps, void* stream);

/* The same for fp32 rows, with the fp16-pair layout of the two-term GEMMs (see AURORA_F32_A_SPLIT) on either side: the
 * LayerNorm in front of a Perceiver MLP hands its result to fc1 already split (out_split; out_f32 may then be NULL),
 * and the LayerNorm behind the MLP takes that same array as its residual (res_is_split = 1: the residual value is
 * high half + remainder, equal to the fp32 value to 2^-23 relative) -- the fp32 copy is never written.
 * D % 32 == 0; pair-layout strides % 32 == 0 (4-byte units).  Either output may be NULL, not both. */
int aurora_hip_layernorm_split(const float* y, int64_t ldy, const float* gain, const float* shift,
                               const void* res, int64_t ldr, int64_t res_mod, int res_is_split,
                               float* out_f32, int64_t ldo, void* out_split, int64_t ld_split,
                               int64_t M, int D, float eps, void* stream);

/* ---- patch merging: 2x2 gather + LayerNorm(4D) -------------------------------------------
 * x: fp32 residual stream [B][C][H][W][D] -> out `dtype` [B][C][H2][W2][4D], H2 = ceil(H/2),
 * features ordered (h, w, D), zero padding at the bottom/right (swin3d.py:526-553).
 * The following Linear(4D, 2D) is an aurora_hip_linear call.
 */
int aurora_hip_merge_ln(const float* x, const float* ln_w, const float* ln_b, void* out,
                        int B, int C, int H, int W, int D, float eps, int dtype, void* stream);

/* ---- patch splitting: pixel shuffle + crop + LayerNorm(D/2) ------------------------------
 * y: `dtype` [B][C][H][W][2D'] with 2D' = 4*Dq (output of lin1) -> out `dtype`
 * [B][C][2H-crop_h][2W-crop_w][Dq]  (swin3d.py:574-611).
 */
int aurora_hip_split_ln(const void* y, const float* ln_w, const float* ln_b, void* out,
                        int B, int C, int H, int W, int Dq, int crop_h, int crop_w, float eps,
                        int dtype, void* stream);

/* ---- patch embedding front end: normalise + unfold ----------------------------------------
 * Builds the GEMM operand of LevelPatchEmbed (patchembed.py:100-115):
 * out[((c*B + b)*Hp + hp)*Wp + wp][k_offset + (v*T + t)*P*P + i*P + j] =
 *     f_v( (src_v[b,t,c,hp*P+i,wp*P+j] - loc_v[c]) * inv_scale_v[c] )
 * rows are ordered (level, batch, patch) so that one level's rows are contiguous (per-level
 * weights / biases are then plain row ranges).  The Batch.normalise affine map
 * (batch.py:94-116) is fused in.  Columns [K_total, Kpad) are zero-filled by the call whose
 * variables end at K_total.  `desc` is a HOST array of n_vars (<= 32) descriptors; their
 * `src`, `loc`, `inv_scale` members are device pointers.  Strides are in elements and may be
 * 0 (static variables broadcast over batch/history/level; constant planes).
 * transform codes: 0 none, 1 clamp(min=0) (aurora.py:301-317), 2 clamp + air-pollution
 * feature combiner (aurora.py:733-742) with Linear(2,1) weights tw0, tw1 and bias tb;
 * ocean-wave channels (aurora.py:892-912, NaN = missing): 3 density = !isnan, 4 value with
 * NaN -> 0, 5 sin(deg2rad(x)) and 6 cos(deg2rad(x)), both with NaN -> 0.
 */
typedef struct aurora_patch_var {
  const float* src;       /* device: first element of the variable                           */
  int64_t stride_b;       /* element strides: batch, history step, level, latitude, longitude */
  int64_t stride_t;
  int64_t stride_c;
  int64_t stride_h;
  int64_t stride_w;
  const float* loc;       /* device [n_lvl] location                                          */
  const float* inv_scale; /* device [n_lvl] 1/scale                                           */
  int32_t transform;
  float tw0, tw1, tb;
} aurora_patch_var;

int aurora_hip_patchify(const aurora_patch_var* desc, int n_vars, void* out, int64_t Kpad,
                        int k_offset, int K_total, int B, int T, int n_lvl, int Hp, int Wp, int P,
                        int dtype, void* stream);
/* The same, and max |value written| is folded into *absmax (nullable; not zeroed here: aurora_hip_zero_words) -- the
 * guard word of the operand-split decision of the linears that read `out` (aurora_hip_linear_ex), at no extra pass. */
int aurora_hip_patchify_absmax(const aurora_patch_var* desc, int n_vars, void* out, int64_t Kpad,
                               int k_offset, int K_total, int B, int T, int n_lvl, int Hp, int Wp, int P,
                               int dtype, float* absmax, void* stream);

/* ---- small-set cross attention of the Perceiver resamplers ---------------------------------
 * Per grid column col in [0, n_cols) and head: softmax(q k^T / sqrt(hd)) v over Lk keys.
 * q: fp32/bf16 [Lq][inner] shared by all columns when q_col_stride == 0, else rows
 * (col*Lq + i).  kv: key j of column (b, l) is one row, columns k | v
 * (2*inner), row index b*kv_bstride + j*kv_lstride + l.  out rows (col*Lq + i), [inner].  Replaces perceiver.py:141-152 as used by
 * encoder.py:184-196 (Lq=3, Lk=levels) and decoder.py:156-166 (Lq=levels, Lk=3).
 */
int aurora_hip_perceiver_attention(const void* q, int64_t q_col_stride, const void* kv, void* out,
                                   int B, int64_t cols_per_b, int64_t kv_bstride, int64_t kv_lstride,
                                   int Lq, int Lk, int heads, int head_dim, int dtype, void* stream);
/* The same with a device-side choice of the OUTPUT format (fp32 only): the rows are written as fp16 pairs (see
 * AURORA_F32_A_SPLIT) iff *pair_guard < pair_limit, as fp32 otherwise -- the guard and limit of the guarded two-term
 * linear that reads them next (to_out), so that producer, consumer and its three-term twin switch together. */
int aurora_hip_perceiver_attention_ex(const void* q, int64_t q_col_stride, const void* kv, void* out,
                                      int B, int64_t cols_per_b, int64_t kv_bstride, int64_t kv_lstride,
                                      int Lq, int Lk, int heads, int head_dim, int dtype,
                                      const float* pair_guard, float pair_limit, void* stream);
/* The same as one half of a device-side choice between this kernel and the re-associated pair below: the launch retires
 * at once iff *skip_guard < skip_limit (null: never). */
int aurora_hip_perceiver_attention_unless(const void* q, int64_t q_col_stride, const void* kv, void* out,
                                          int B, int64_t cols_per_b, int64_t kv_bstride, int64_t kv_lstride,
                                          int Lq, int Lk, int heads, int head_dim, int dtype,
                                          const float* pair_guard, float pair_limit, const float* skip_guard,
                                          float skip_limit, void* stream);

/* ---- the decoder's level de-aggregation, re-associated (perceiver.py:141-152 + its `to_out`, decoder.py:156-166, 225-231)
 * With queries shared by all columns (q_col_stride == 0) and Lk = 3 keys per column,
 *     to_out(concat_h sum_j p[l,h,j] v[j,h,:]) = sum_h sum_j p[l,h,j] (W_out[:, h-th 64 columns] v[j,h,:]):
 * the three values of a column are projected per head (Lk rows per column instead of Lq) and combined with the softmax
 * weights in registers; the attention output is never written.  fp32-grade: two fp16 terms per operand (the values must be
 * inside fp16's range: the caller's guard), fp32 weights p, fp32 accumulation.
 *   _probs: P[col][head][l][2] = (p_0, p_1) of p = softmax_j(q_l . k_j / 8) for l = 0, their differences to level 0 for
 *           l > 0 (fp32, 64 floats per (col, head), zero-padded; p_2 = 1 - p_0 - p_1) and Vp[col * 3 + j][inner] = (v_0 - v_2, v_1 - v_2, v_2)[j] in the fp16-pair layout
 *           (AURORA_F32_A_SPLIT); q, kv as aurora_hip_perceiver_attention.
 *   _out:   out[col * Lq + l][0..N) = sum_h W_h (Vp_2 + p_0 Vp_0 + p_1 Vp_1)[col, h] + bias, W_h = W_pairs[:, 64 h .. 64 h + 63];
 *           W_pairs: [N][ldw] pre-split weights scaled by 2^6 (aurora_hip_split_f16 with scale 64).
 * Both retire at once unless *guard < guard_limit (null: always run).  Built for Lq in {3, 4, 13},
 * Lk = 3, head_dim 64, an even number of heads, N % 128 == 0: aurora_hip_perceiver_out_supported says whether a shape is. */
int aurora_hip_perceiver_out_supported(int Lq, int Lk, int heads, int head_dim, int N);
int aurora_hip_perceiver_probs(const float* q, const float* kv, float* P, void* Vp, int B, int64_t cols_per_b,
                               int64_t kv_bstride, int64_t kv_lstride, int Lq, int Lk, int heads, int head_dim,
                               const float* guard, float guard_limit, void* stream);
/* The same two from PRE-MULTIPLIED scores.  The queries of a first Perceiver layer are model constants, so
 * q_l . (W_k x_j) = (W_k^T q_l) . x_j: the key half of `to_kv` (perceiver.py:141-143) shrinks from heads * head_dim columns to
 * Lq * heads rows made at pack time (scaled by 1 / sqrt(head_dim)).  A context row of `vs` (ld_vs floats apart, row index as kv
 * above) holds [v (heads * head_dim) | ... | score of (query l, head h) at s_off + l * heads + h].  fp32 only.
 * _attention_scores: out / pair_guard / skip_guard as aurora_hip_perceiver_attention_unless.
 * _probs_scores: P / Vp / guard as aurora_hip_perceiver_probs. */
int aurora_hip_perceiver_attention_scores(const float* vs, int64_t ld_vs, int s_off, void* out, int B, int64_t cols_per_b,
                                          int64_t kv_bstride, int64_t kv_lstride, int Lq, int Lk, int heads, int head_dim,
                                          const float* pair_guard, float pair_limit, const float* skip_guard, float skip_limit,
                                          void* stream);
int aurora_hip_perceiver_probs_scores(const float* vs, int64_t ld_vs, int s_off, float* P, void* Vp, int B, int64_t cols_per_b,
                                      int64_t kv_bstride, int64_t kv_lstride, int Lq, int Lk, int heads, int head_dim,
                                      const float* guard, float guard_limit, void* stream);
int aurora_hip_perceiver_out(const void* Vp, const void* W_pairs, int64_t ldw, const float* P, const float* bias,
                             float* out, int64_t ldo, int64_t n_cols, int Lq, int Lk, int heads, int head_dim, int N,
                             const float* guard, float guard_limit, void* stream);

/* ---- token assembly at the encoder output -------------------------------------------------
 * x[b][c][l][:] = (c == 0 ? surf[b][l][:] : agg[(b*L + l)*(Cl-1) + c-1][:])
 *                 + pos_scale[l][:] + time_emb[b][:]
 * (encoder.py:332-363).  Writes the fp32 stream and, if out_t != NULL, a `dtype` copy.
 */
int aurora_hip_assemble_tokens(const float* surf, const float* agg, const float* pos_scale,
                               const float* time_emb, float* out_f32, void* out_t,
                               int B, int Cl, int64_t L, int D, int dtype, void* stream);

/* ---- decoder back end: unpatchify + post-decoder hooks + clamp + unnormalise ----------------
 * y: fp32 [(b*L + l)*n_lvl + c][ldy] head outputs (decoder.py:214-263, util.py:18-41); variable
 * v, level c, in-patch pixel (i, j) sits in column col0 + c*lvl_stride + i*P + j (lvl_stride != 0
 * for level-conditioned heads).  Writes dst_v[b][c][hp*P+i][wp*P+j] = g(z) * scale_v[c] + loc_v[c]
 * with Batch.unnormalise (batch.py:118-140) fused, where
 *   z = y                                         plain variables
 *   z = y + (1 + y_mod) * (prev - loc) * inv      difference prediction (aurora.py:761-779),
 *                                                 y_mod at mod_col0 (>= 0), prev the raw previous
 *                                                 state of the same variable
 *   then z = min(z, 1) on the levels in clamp_max1_levels (bit c; SO2 fix aurora.py:781-794)
 *   then g = clamp(min=0) if clamp_min0 (aurora.py:368-388);
 *   ocean-wave post hook (aurora.py:914-932): angle_col0 >= 0 makes col0 / angle_col0 the sin / cos
 *   heads of a direction, z = rad2deg(atan2(sin, cos)) mod 360; dens_col0 >= 0 keeps z only where
 *   mask[h][w] > mask_thresh (water) and the density head is >= 0 (sigmoid >= 0.5), else NaN.
 * `desc`: HOST array of n_vars (<= 32) descriptors with device pointers inside.
 */
typedef struct aurora_unpatch_var {
  float* dst;             /* [B][n_lvl][H][W] contiguous                                      */
  const float* loc;       /* device [n_lvl]                                                   */
  const float* scale;     /* device [n_lvl]                                                   */
  int32_t clamp_min0;
  int32_t col0;
  int32_t lvl_stride;
  int32_t mod_col0;       /* -1: no modulation head                                           */
  const float* prev;      /* device, raw units: prev[b*prev_sb + c*prev_sc + h*prev_sh + w]   */
  int64_t prev_sb, prev_sc, prev_sh;
  const float* inv_scale; /* device [n_lvl] 1/scale (only read when mod_col0 >= 0)            */
  uint32_t clamp_max1_levels;
  int32_t angle_col0;     /* -1: not a direction                                              */
  int32_t dens_col0;      /* -1: no density channel                                           */
  const float* mask;      /* device, raw water-body mask plane (H, W), row stride mask_sh     */
  int64_t mask_sh;
  float mask_thresh;      /* raw-units threshold equivalent to "normalised value > 0"         */
} aurora_unpatch_var;

int aurora_hip_unpatchify(const float* y, int64_t ldy, const aurora_unpatch_var* desc, int n_vars,
                          int B, int n_lvl, int Hp, int Wp, int P, void* stream);

/* ---- utility ------------------------------------------------------------------------------ */
/* dst[r, 0:cols] = src[r, 0:cols] for r < rows (row strides in elements of `dtype`). */
int aurora_hip_copy2d(const void* src, int64_t lds_, void* dst, int64_t ldd, int64_t rows,
                      int64_t cols, int dtype, void* stream);
/* dst row r = src row idx[r] (r < n_rows), rows of row_bytes bytes (multiple of 16), pitches in bytes.
 * Packs the halo rows a latitude band sends to a neighbour (new: the reference is single-device). */
int aurora_hip_gather_rows(const void* src, int64_t src_pitch_bytes, const int32_t* idx, void* dst,
                           int64_t dst_pitch_bytes, int64_t n_rows, int64_t row_bytes, void* stream);
/* dst (other dtype) = convert(src): n elements, fp32 -> bf16 (round-nearest-even) or back. */
int aurora_hip_convert(const void* src, void* dst, int64_t n, int src_dtype, void* stream);

/* =============================================================================================
 * Model handle: ONE FORECAST STEP behind the C ABI.
 *
 * Replaces `Aurora.forward` (aurora/model/aurora.py:265-392) = Perceiver3DEncoder.forward (encoder.py:198-366) +
 * Swin3DTransformerBackbone.forward (swin3d.py:884-936) + Perceiver3DDecoder.forward (decoder.py:168-276) with the
 * normalisation of Batch.normalise / unnormalise (batch.py:94-140) fused in, for EVERY public model class: Aurora,
 * AuroraPretrained, AuroraSmallPretrained, Aurora12hPretrained, AuroraHighRes, and the variants AuroraAirPollution
 * (level-conditioned embeddings / heads levelcond.py:36-69, dynamic and static inputs encoder.py:226-303, feature combiners
 * and difference prediction aurora.py:726-796, second decoder Perceiver decoder.py:232-248) and AuroraWave (density / angle
 * channels and their inverse, aurora.py:854-932).  A forecast can run on one device or as one latitude band of a
 * sharded forecast (aurora_hip_set_band below).  Call order:
 *
 *   aurora_hip_create(&config, &model)
 *   aurora_hip_pack_weights(model, name, data, shape, ndim, AURORA_F32, on_device)   for every state_dict entry, after the
 *                                       checkpoint adapters (compat.py) -- names and shapes are the reference's schema
 *   aurora_hip_finalize(model, stream)          bf16 backbone copies, AdaLN modulation, fused heads, base weight set
 *   aurora_hip_precompute(model, &grid, stream) per grid / level set: Fourier tables, window tables, statistics
 *   per step:  aurora_hip_set_time(model, hours, B, stream);  aurora_hip_step(model, &io, stream)
 *   aurora_hip_destroy(model)
 *
 * Everything is enqueued on `stream`; a step performs no host synchronisation and may be captured into a hipGraph once
 * one step has run eagerly (the workspace grows on the first step; aurora_hip_set_time stays outside the capture; replay only
 * while aurora_hip_generation() is unchanged).
 * One in-flight step per handle (the reference's own threading contract, foundry/server/mlflow_wrapper.py:121).
 * The library keeps no state outside the handles.
 */
typedef struct aurora_hip_model aurora_hip_model;

typedef struct aurora_hip_config {   /* Aurora.__init__ keywords, aurora/model/aurora.py:55-95 */
  int32_t embed_dim, patch_size, latent_levels, num_heads;   /* num_heads: heads of the Perceivers */
  int32_t n_stages;                                          /* len(encoder_depths), <= 4 */
  int32_t encoder_depths[4], encoder_heads[4], decoder_depths[4], decoder_heads[4];
  int32_t window[3];
  int32_t enc_depth, dec_depth;
  float perceiver_ln_eps;
  int32_t max_history;
  double timestep_hours;
  int32_t stabilise_level_agg, use_lora, lora_steps, lora_mode;   /* lora_mode: 0 single, 1 from_second, 2 all */
  int32_t autocast;                                          /* 1: bf16 backbone (aurora.py:327-343) */
  int32_t n_surf, n_static, n_atmos;
  const char* const* surf_vars;                              /* fixes the order of every per-variable array below */
  const char* const* static_vars;
  const char* const* atmos_vars;
  /* ---- variant keywords (aurora.py:86-95); zero-initialised = the ERA5 model family -------------------------------
   * variant: 0 base; 1 air pollution: positive variables go through the clamp + log feature combiner
   * (`{surf,atmos}_feature_combiner.<var>` weights, aurora.py:733-742), variables in `modulation_heads` with an entry in
   * difference_history predict a difference to that history state (aurora.py:761-779), SO2 is capped at the levels
   * >= 850 hPa when LoRA is on (aurora.py:781-794); 2 ocean wave: `surf_vars` are the model's channels (`<v>_sin`,
   * `<v>_cos`, `<v>_density`, ...), `surf_inputs` the variables the caller supplies after AuroraWave's
   * batch_transform_hook; density / sin / cos channels are derived on the fly and inverted after the decoder
   * (aurora.py:892-932; the water-body mask is the static variable "wmb"). */
  int32_t variant;
  int32_t n_level_condition;                                 /* levels with their own patch embedding / heads (levelcond.py) */
  const double* level_condition;
  int32_t dynamic_vars, atmos_static_vars, clamp_at_first_step, simulate_indexing_bug;
  int32_t n_separate_perceiver;  const char* const* separate_perceiver;
  int32_t n_modulation_heads;    const char* const* modulation_heads;
  const int32_t* difference_history;                         /* [n_modulation_heads] history index, -1: no difference */
  int32_t n_positive_surf;       const char* const* positive_surf_vars;
  int32_t n_positive_atmos;      const char* const* positive_atmos_vars;
  int32_t n_surf_inputs;         const char* const* surf_inputs;              /* wave only; 0: = surf_vars */
  int32_t n_density;             const char* const* density_channel_surf_vars;
  int32_t n_angle;               const char* const* angle_surf_vars;
  /* ---- how THIS handle runs its steps (results are the same bits or within the documented bounds either way); all zero =
   * the library's defaults.  Read when the handle is created and kept in it: nothing reads the environment, and two handles
   * of one process may differ.  (The Python front end fills these from the AURORA_* environment variables of INTEGRATION.md,
   * once, when it creates a handle.)  Switches: 0 default, 1 off, 2 on. */
  struct aurora_hip_tuning {
    int32_t fuse_ln;               /* D = 512 linear + AdaLN in one launch: 0 default (= 2), 1 never, 2 when its row tiles fill the chip, 3 always */
    int32_t band_split_attention;  /* a latitude band's interior windows as a launch of their own in front of the halo wait (default off) */
    int32_t qkv_planes;            /* bf16 blocks: q | k | v in head planes (default on; off: token rows -- same bits) */
    int32_t split_k;               /* few-tile / long-K bf16 linears split along K (default on; off: a band's bf16 arithmetic is the
                                      un-sharded step's bit for bit whatever the CU count) */
    int32_t perceiver_reassoc;     /* decoder de-aggregation re-associated (aurora_hip_perceiver_out; default on) */
    int32_t score_weights;         /* first Perceiver layers: to_kv's key half replaced by the Lq * heads rows W_k^T q_l (the queries
                                      are model constants), attention from those scores (default on; off: k | v, then q . k) */
    int32_t compose_front;         /* encoder front: the atmospheric patch embedding folded into the level aggregation's context
                                      linears where that halves their work or better (aurora_hip_compose_front_rule; default on;
                                      off: embedding, then to_kv -- the same map, other rounding points) */
    int32_t reserved[1];
  } tuning;
} aurora_hip_config;

typedef struct aurora_hip_grid {     /* HOST pointers */
  int32_t n_lat, n_lon;              /* of the data; one surplus latitude row (n_lat % patch == 1) is dropped, batch.py:142-168 */
  const double* lat;                 /* [n_lat] degrees, decreasing */
  const double* lon;                 /* [n_lon] degrees */
  int32_t n_levels;
  const double* levels;              /* [n_levels] hPa */
  int32_t levels_float32;            /* 1: the levels pass through float32 (a tuple containing a float upstream) */
  const double* surf_loc;            /* normalisation statistics (aurora/normalisation.py): [n_surf] */
  const double* surf_scale;
  const double* static_loc;          /* [n_static] */
  const double* static_scale;
  const double* atmos_loc;           /* [n_atmos][n_levels] */
  const double* atmos_scale;
  /* Optional (both or neither): the Fourier position / scale features of the patch grid, [L][embed_dim] each, L = patches
   * per level.  The reference derives them from lat / lon in float32 torch kernels whose last-ulp behaviour the expansion
   * amplifies (wavelengths down to 1e-4 km); a caller that must reproduce a particular host's numbers bit for bit
   * supplies them, otherwise they are computed here (float32 geometry as upstream, fp64 trigonometry). */
  const float* pos_encoding;
  const float* scale_encoding;
} aurora_hip_grid;

typedef struct aurora_hip_step_io {  /* DEVICE pointers; variable order = the config's (surf: surf_inputs for the wave variant) */
  int32_t B, T;                      /* batch size, history states given (<= max_history) */
  const float* const* surf;          /* [n_surf]   each (B, T, n_lat, n_lon) with element strides surf_strides; NULL entry = absent */
  int64_t surf_strides[4];
  const float* const* stat;          /* [n_static] each (n_lat, n_lon) with element strides static_strides; NULL entry = absent */
  int64_t static_strides[2];
  const float* const* atmos;         /* [n_atmos]  each (B, T, n_levels, n_lat, n_lon) with element strides atmos_strides; NULL = absent */
  int64_t atmos_strides[5];
  float* const* out_surf;            /* [n_out_surf] each (B, H', n_lon) contiguous, H' = n_lat - n_lat % patch; n_out_surf and the
                                        order are aurora_hip_output_vars' (= the surface inputs, except for the wave variant) */
  float* const* out_atmos;           /* [n_atmos]  each (B, n_levels, H', n_lon) contiguous */
  int32_t rollout_step;              /* Metadata.rollout_step of the input: selects the LoRA weight set (lora.py:105-129) and
                                        whether positive variables are clamped (aurora.py:368-388) */
} aurora_hip_step_io;
/* A band of a sharded forecast (aurora_hip_set_band) passes and receives ITS latitude rows only: n_lat above is then the
 * band's row count, aurora_hip_band_rows tells which rows of the full grid those are. */

int aurora_hip_create(const aurora_hip_config* config, aurora_hip_model** out);
void aurora_hip_destroy(aurora_hip_model* model);
/* One state_dict entry (float32; `data` on the host, or on the device if on_device != 0).  The handle keeps its own copy. */
int aurora_hip_pack_weights(aurora_hip_model* model, const char* name, const void* data, const int64_t* shape, int ndim,
                            int dtype, int on_device);
int aurora_hip_finalize(aurora_hip_model* model, void* stream);
/* Packed weight files: a self-describing binary ("AURORAHIP1", entries of name / dtype / shape / raw data) that replaces
 * the pickled `.ckpt` + adapters (aurora.py:432-456, compat.py) for hosts without Python.  _save_packed writes what a
 * finalized handle holds -- the large backbone matrices in bf16 when the handle runs the bf16 backbone (the bits the
 * GEMMs consume: 2.6 GB instead of 5 GB for the 1.3 B model), the rest as fp32 -- and _load_packed fills a freshly created
 * handle from such a file instead of aurora_hip_pack_weights calls (then _finalize as usual).  bf16-only files serve
 * autocast handles; LoRA models keep fp32 attention projections (the merge W + BA is done in fp32). */
int aurora_hip_save_packed(aurora_hip_model* model, const char* path, void* stream);
int aurora_hip_load_packed(aurora_hip_model* model, const char* path);
int aurora_hip_precompute(aurora_hip_model* model, const aurora_hip_grid* grid, void* stream);
/* The position / scale tables aurora_hip_precompute derives from lat / lon when the grid carries no tables of its own
 * (posencoding.py:61-192; HOST pointers in and out, no device work): pos_out and scale_out are
 * [(n_lat / patch) * (n_lon / patch)][embed_dim] floats; a surplus latitude row is ignored.  Float32 geometry as upstream,
 * fp64 trigonometry -- equal to the reference's torch tables except where its float32 sin / sqrt differ in the last ulp,
 * which the shortest wavelengths amplify (tests/test_encodings.py states the bound per wavelength). */
int aurora_hip_pos_scale_encoding(const double* lat, const double* lon, int n_lat, int n_lon, int patch_size,
                                  int embed_dim, float* pos_out, float* scale_out);
/* Absolute times of the batch elements in hours since the Unix epoch (encoder.py:359-363), host pointer. */
int aurora_hip_set_time(aurora_hip_model* model, const double* time_hours, int B, void* stream);
int aurora_hip_step(aurora_hip_model* model, const aurora_hip_step_io* io, void* stream);
int64_t aurora_hip_workspace_bytes(const aurora_hip_model* model);
/* Which fp32 path did the last step take?  The large fp32 linears of encoder and decoder pick their operand split on the
 * DEVICE, from guard words the step leaves behind (aurora_hip_linear_ex): out[0] max |encoder context| (only when the encoder
 * is not part of the guarded chain, else 0), out[1] / out[2] max |normalised atmospheric / surface input| (folded in by
 * patchify), out[3] max |decoder context|.  A word below AURORA_F16_SAFE_RANGE (after the layer's own scaling, see
 * DESIGN.md 3) means two fp16 terms, above it three bf16 terms -- same accuracy, different speed.  Synchronises `stream`. */
#define AURORA_F16_SAFE_RANGE 16384.0f
int aurora_hip_guard_words(const aurora_hip_model* model, float out[4], void* stream);
/* What were those words compared against?  Every guarded launch of a step runs its two-term form iff word < limit, with a
 * limit the handle derives from its weights (L1 row norms and bias maxima of the linears between the measured quantity and the
 * launch's activation operand).  Of the handle's last step: out[i], i = 0..3, the SMALLEST limit any launch compared word i
 * against (+inf if none did), out[4 + i] the number of launches that carried word i (a guarded pair counts twice).  word i <
 * out[i] <=> every guarded launch on word i took two fp16 terms.  Host bookkeeping: no device work, no synchronisation. */
int aurora_hip_guard_limits(const aurora_hip_model* model, float out[8]);
/* ---- the encoder front composed: the atmospheric patch embedding is linear and read by the level aggregation's
 * bias-free context linears alone, so kv = A (W_ctx W_e[c])^T + W_ctx (b_e + level_embed[c]) -- one GEMM of K = Kpad where
 * one of K = Kpad and one of K = D ran.  The pieces, as pure host functions (HOST pointers, no device work), so that the
 * composition, the rule and the guard limits can be checked without a device:
 *   _compose_weight      out[g][n][k] = sum_d w_ctx[n][d] w_e[g][d][k] (w_ctx (N, D), w_e (groups, D, K)), summed in double, rounded once
 *   _compose_bias        out[c][n]    = sum_d w_ctx[n][d] bias[c][d]   (bias (C, D)), likewise
 *   _compose_front_rule  1 iff 2 sum_i Kpad N[i] <= Kpad D + sum_i D N[i]: the composed linears do at most half the multiply-adds
 *                        of the stages they replace (patch size 4: 0.26, composed; patch size 10: 0.85, not)
 *   _composed_value_bound  |v| <= a w + c for the attention's value rows, w = max |normalised input|: out[0..2] = a, c and the
 *                        limit on w from the two stages (a = v_l1 embed_l1, c = v_l1 embed_bias_max), out[3..5] the same from the
 *                        composed value rows' own L1 norm and bias maximum -- a and c never above the stages', so the limit on w
 *                        never below
 *   _front_composed      1 iff the handle's last step ran its encoder front composed */
int aurora_hip_compose_weight(const float* w_ctx, int N, int D, const float* w_e, int K, int groups, float* out);
int aurora_hip_compose_bias(const float* w_ctx, int N, int D, const float* bias, int C, float* out);
int aurora_hip_compose_front_rule(int Kpad, int D, const int32_t* N, int n_layers);
int aurora_hip_composed_value_bound(float v_l1, float embed_l1, float embed_bias_max, float composed_v_l1,
                                    float composed_vb_max, float out[6]);
int aurora_hip_front_composed(const aurora_hip_model* model);
/* Counts the re-allocations of device memory that enqueued work points at: the workspace (it grows with the first step of
 * a larger batch / history / grid), the time buffers (a larger batch), the grid tables (aurora_hip_precompute).  A hipGraph
 * captured from aurora_hip_step is valid for as long as this number does not change. */
int64_t aurora_hip_generation(const aurora_hip_model* model);
/* sizeof() of the structs of this header as the library was compiled, in the order aurora_hip_config, aurora_hip_grid,
 * aurora_hip_step_io, aurora_hip_band, aurora_hip_halo_msg, aurora_hip_plan_info, aurora_patch_var, aurora_unpatch_var,
 * aurora_hip_profile_entry: a binding in another language checks its own struct declarations against them.  Returns the
 * number of entries. */
int aurora_hip_abi_sizes(int32_t* out, int capacity);
/* Names of the surface variables a step predicts, in the order of aurora_hip_step_io.out_surf (ocean wave: the non-angle
 * variables, then the directions, aurora.py:914-932; otherwise the surface inputs).  Returns the count; `names` may be NULL. */
int aurora_hip_output_vars(const aurora_hip_model* model, const char** names, int capacity);
/* aurora_hip_set_time with the calendar fields the dynamic variables of the air-pollution model are made of
 * (encoder.py:226-246): calendar[b] = {hour of day, weekday (Monday = 0), day of month}; NULL derives them from the time
 * stamp as UTC. */
int aurora_hip_set_time_ex(aurora_hip_model* model, const double* time_hours, const int32_t* calendar, int B, void* stream);

/* ---- one forecast across several devices: latitude bands + halo exchange (the reference is
 * single-device) ---------------------------------------------------------------------------------------------------------
 * Every rank owns a contiguous band of latitude rows at every backbone stage (boundaries on the coarsest stage, doubled
 * per finer stage, so patch merges / splits stay local; on window rows of the finer stages when that is balanced, else the
 * most balanced split whose windows stay within two neighbouring ranks -- a rank exchanges with rank - 1 and rank + 1 only,
 * aurora_hip_precompute fails if no such split exists).  Everything except window attention is local to a token, a 2 x 2
 * block or a grid column.  A shifted-window block needs k | v of the neighbouring band's first / last rows: the handle
 * gathers those rows of the block's INPUT into `send` staging buffers (half the bytes of k | v, and available before the
 * qkv GEMM), calls `post` (start sending / receiving; asynchronous to `stream`), runs its own qkv GEMM and the windows that
 * need no halo row, calls `wait` (make `stream` wait for the messages), projects the received rows to k | v itself and
 * attends the boundary windows.  The TRANSPORT is the host's: RCCL point-to-point (torch.distributed / ncclSend /
 * ncclRecv) in production, anything else in tests -- the library does not link a communication library.
 * Message buffers are the two staging buffers the host hands over (its own allocations, so that its transport can address
 * them): one that the handle fills with what is sent, one that receives; at least aurora_hip_band_staging_bytes() each
 * (valid after aurora_hip_precompute).  A message is a byte range of one of them: what goes to / comes from the previous
 * rank first, the next rank's behind it -- so one gather launch packs both and one GEMM projects both.
 * Call order: create, pack, finalize, aurora_hip_set_band, aurora_hip_precompute with the FULL grid, aurora_hip_band_rows,
 * aurora_hip_set_band_staging, then steps on the band's rows. */
typedef struct aurora_hip_halo_msg {
  int32_t peer;       /* rank */
  int32_t reserved;
  int64_t offset;     /* byte offset into the send (for a send) or the receive (for a receive) staging buffer */
  int64_t bytes;
} aurora_hip_halo_msg;
typedef int (*aurora_hip_halo_post_fn)(void* user, const aurora_hip_halo_msg* sends, int32_t n_sends,
                                       const aurora_hip_halo_msg* recvs, int32_t n_recvs, void* stream);
typedef int (*aurora_hip_halo_wait_fn)(void* user, void* stream);
typedef struct aurora_hip_band {
  int32_t rank, world;
  aurora_hip_halo_post_fn post;
  aurora_hip_halo_wait_fn wait;
  void* user;
} aurora_hip_band;
int aurora_hip_set_band(aurora_hip_model* model, const aurora_hip_band* band);   /* world <= 1: un-sharded again */
/* Data rows [row0, row1) of the full (cropped) latitude axis that this rank owns. */
int aurora_hip_band_rows(const aurora_hip_model* model, int32_t* row0, int32_t* row1);
int64_t aurora_hip_band_staging_bytes(const aurora_hip_model* model);
int aurora_hip_set_band_staging(aurora_hip_model* model, void* send, void* recv, int64_t staging_bytes);
/* The partition and the attention plans themselves, as pure host functions (no model, no device work): what the handle
 * uses internally, exposed for hosts that place data themselves and for tests (tests/test_partition.py compares them with
 * numpy plans that are replayed against global attention).
 * aurora_hip_band_partition: owned token rows [h0, h1) of `rank` at backbone stage `stage` (0 = finest) of an
 * `n_stages`-stage U-net over a token grid res0 = (levels, latitude rows, longitude columns).
 * aurora_hip_band_plan: the plan of one block flavour at one stage: `res` the stage's token grid, rows[2 r], rows[2 r + 1]
 * the owned rows of rank r there.  Fills `info`; the arrays may be NULL (query sizes first): tok / grp
 * [n_windows][win_tokens] (index into [owned rows | halo rows], -1 = padding or a position no owned query can see; grp is
 * left untouched when has_groups == 0), send_idx_prev / _next: local indices of the owned rows sent to rank - 1 / + 1,
 * in the receiver's halo order. */
typedef struct aurora_hip_plan_info {
  int32_t n_windows, win_tokens, n_own, n_halo, n_interior;   /* the first n_interior windows touch no halo row */
  int32_t recv_offset[2], recv_count[2], send_count[2];       /* [0] previous rank, [1] next rank; offsets into the halo rows */
  int32_t has_groups;
} aurora_hip_plan_info;
int aurora_hip_band_partition(int n_stages, const int32_t res0[3], const int32_t window[3], int world, int rank, int stage,
                              int32_t* h0, int32_t* h1);
int aurora_hip_band_plan(const int32_t res[3], const int32_t window[3], int shifted, int world, int rank,
                         const int32_t* rows, aurora_hip_plan_info* info, int32_t* tok, uint8_t* grp,
                         int32_t* send_idx_prev, int32_t* send_idx_next);

/* Per-launch timing of the handle's own kernels: between _begin and _end every launch of a kernel kind whose bit is set
 * in kind_mask (bit i = entry i of the table _end returns: linear_bf16, linear_f32, window_attention_bf16, layernorm,
 * merge_ln, split_ln, patchify, perceiver_attention, assemble_tokens, unpatchify, copy2d, absmax, linear_layernorm_bf16,
 * gather_rows, perceiver_out) is bracketed by a HIP event pair on the launch stream.  _end synchronises the device and
 * fills `out` (capacity >= 15): launches, summed
 * milliseconds and summed algorithmic work (FLOPs for the linears, bytes for the window attention) per kind.  This is
 * what bench.py's `roofline` is computed from.  An event pair keeps a launch from overlapping its neighbours. */
typedef struct aurora_hip_profile_entry {
  const char* kernel;
  int64_t launches;
  double ms;
  double work;
} aurora_hip_profile_entry;
int aurora_hip_profile_begin(aurora_hip_model* model, uint32_t kind_mask);
int aurora_hip_profile_end(aurora_hip_model* model, aurora_hip_profile_entry* out, int capacity, int* n_out);
/* The same, one entry per LAUNCH in launch order (launches = 1; `work` tells the shapes of a kind apart).  With capacity
 * smaller than the number of recorded launches only *n_out is set and the recording is kept: query first, then fetch. */
int aurora_hip_profile_end_list(aurora_hip_model* model, aurora_hip_profile_entry* out, int capacity, int* n_out);

/* ---- regridding a batch on the device (Batch.regrid of a GPU-resident batch; the reference's Batch.regrid / interpolate,
 * batch.py:192-222, 299-362) ------------------------------------------------------------------------------------------------
 * Bilinear interpolation from a (lat, lon) grid to another, periodic in longitude, exactly as the host path computes it
 * (scipy.interpolate.RegularGridInterpolator(method="linear", bounds_error=False, fill_value=None) on the grid
 * (lat, [lon[n-1] - 360, lon..., lon[0] + 360]) in fp64, rounded to fp32): on each axis, sorted ascending, a target takes
 * the interval of the largest node <= it, clamped to the first / last interval (so a target on the last node takes the
 * last interval and targets outside the axis extrapolate linearly), and the weight t = (x - x[i]) / (x[i+1] - x[i]); all
 * four corners are summed even where a weight is zero, so a NaN there gives NaN.
 * aurora_hip_regrid_plan: the interpolation tables, pure host arithmetic (no device work).  lat: n_lat >= 2 finite,
 * strictly increasing or decreasing values; lon: n_lon >= 2 finite, strictly increasing values spanning less than 360
 * degrees; targets finite.  Writes rows[2 k], rows[2 k + 1] (source rows) and row_w[k] (weight of the second) for every
 * target latitude k, cols[2 k], cols[2 k + 1] (source columns, wrapped) and col_w[k] for every target longitude k.
 * aurora_hip_regrid: dst[p][r][c] = the interpolation of src[p] (n_lat x n_lon, row-major, AURORA_F32 or AURORA_F64) for
 * every plane p < n_planes, output row r < n_rows_out and column c < n_cols_out, in ONE launch.  src_planes / dst_planes
 * are DEVICE arrays of n_planes plane pointers (4-byte aligned fp32 output planes of n_rows_out x n_cols_out; no other
 * alignment needed); the four tables are device copies of the plan's.  Passing rows + 2 r0, row_w + r0 with
 * n_rows_out = r1 - r0 regrids output rows [r0, r1) only.  Table indices are clamped into the source plane.  No host
 * synchronisation, no workspace: capturable in a hipGraph. */
int aurora_hip_regrid_plan(const double* lat, int n_lat, const double* lon, int n_lon, const double* lat_new, int n_lat_new,
                           const double* lon_new, int n_lon_new, int32_t* rows, double* row_w, int32_t* cols,
                           double* col_w);
int aurora_hip_regrid(const void* const* src_planes, int src_dtype, float* const* dst_planes, int n_planes, int n_lat,
                      int n_lon, const int32_t* rows, const double* row_w, int n_rows_out, const int32_t* cols,
                      const double* col_w, int n_cols_out, void* stream);

/* ---- conservative (area-weighted) regridding of a batch on the device (aurora_amd.conservative_regrid; not in the
 * reference) ----------------------------------------------------------------------------------------------------------------
 * First-order conservative remapping from a (lat, lon) grid to another: a target cell takes the mean of the source cells
 * it overlaps, weighted by the overlap (sin(lat) x degrees of longitude), over the source values that are finite.
 * aurora_amd/conservative.py states the cell model and builds the tables; a C host fills them itself as follows.
 *
 * Tables, all in DEVICE memory.  For the rows (i < n_rows_out) and, alike, for the columns (j < n_cols_out):
 *   first    int32 [n][2]  first[i][0]: source index of the first tap of target cell i; first[i][1]: index of its first
 *                          weight in w (>= 0).  Tap t < count[i] reads source row first[i][0] + t (clamped into
 *                          [0, n_lat - 1]) or source column (first[j][0] + t) mod n_lon (first[j][0] clamped into
 *                          [0, 3 n_lon - 1]: a full-circle source stores n_lon + k for column k, so that a cell that
 *                          straddles the seam starts at n_lon - 1 or below and runs eastward), with weight
 *                          w[first[.][1] + t].  Along the columns neither first[j][0] nor first[j][0] + count[j] may
 *                          decrease (a cell without taps takes the end of its western neighbours): the kernel takes the
 *                          span of source columns of a tile of target columns from the tile's first and last cell.
 *   count    int32 [n]     taps of the cell, 0 .. 64 (clamped); 0: the cell is NaN.
 *   w        fp64 [...]    the overlaps, cell after cell, every one > 0; first[.][1] + count must stay inside it.
 *   measure  fp64 [n]      A_i / B_j: the full measure of the target cell (sin(lat) difference / degrees).
 * Arithmetic: fp64, each operation rounded on its own (no fused multiply-add).  For target row i and every source
 * column c, over the row taps (a, r) in order from cn = cd = 0: where x[r][c] is finite, cn += a * x[r][c] and cd += a.
 * For target column j, over the column taps (b, c) in order from n = d = 0: n += b * cn[c], d += b * cd[c].
 * dst[p][i][j] = (float)(n / d) where d > 0 and d >= min_valid * (A_i * B_j), and NaN otherwise.
 *
 * src_planes / dst_planes: DEVICE arrays of n_planes plane pointers: sources n_lat x n_lon row-major, AURORA_F32 or
 * AURORA_F64, element-aligned (16-byte aligned planes with n_lon % 4 == 0 are read 16 bytes at a time; the result is the
 * same bits either way); destinations fp32 n_rows_out x n_cols_out, 4-byte aligned, not overlapping any source.  ONE
 * launch over every plane; a plane's result does not depend on the other planes.  min_valid in (0, 1].  Null pointers,
 * sizes < 1, another dtype and a min_valid outside (0, 1] are AURORA_E_ARG before anything is launched.  Every source
 * index is clamped or wrapped into the plane whatever the tables hold.  No workspace, no atomics, nothing read back, no
 * host synchronisation: capturable in a hipGraph. */
int aurora_hip_conservative_regrid(const void* const* src_planes, int src_dtype, float* const* dst_planes, int n_planes,
                                   int n_lat, int n_lon, int n_rows_out, int n_cols_out, const int32_t* row_first,
                                   const int32_t* row_count, const double* row_w, const double* row_measure,
                                   const int32_t* col_first, const int32_t* col_count, const double* col_w,
                                   const double* col_measure, double min_valid, void* stream);

/* ---- scoring a forecast against truth on the device (aurora_amd.scores: latitude-weighted RMSE / bias / MAE and the
 * anomaly correlation; not in the reference) -------------------------------------------------------------------------------
 * A plane is one variable, level and batch element: n_lat x n_lon fp32, row-major.  For every plane k < n_planes the
 * prediction p, the truth t and, unless clim_planes is NULL, the climatology c are read once and reduced to eight fp64 sums
 * sums[8 k + slot] over the VALID points of the plane, with the weight w = row_w[i] of the point's row i:
 *   slot 0  1                          (the count of valid points, exact)
 *   slot 1  w                          (the normaliser)
 *   slot 2  w d,  d = p - t            (bias      = S2 / S1)
 *   slot 3  w d^2                      (RMSE      = sqrt(S3 / S1))
 *   slot 4  w |d|                      (MAE       = S4 / S1)
 *   slot 5  w p' t',  p' = p - c, t' = t - c      (ACC = S5 / sqrt(S6 S7))
 *   slot 6  w p'^2
 *   slot 7  w t'^2
 * Slots 5-7 are 0 without a climatology.  A point is valid where every input that is present (p, t and, if given, c) is
 * finite; a plane without a valid point gives count 0 and all sums 0.  Differences and products are formed in fp64 from the
 * fp32 inputs and accumulated in fp64.
 * Determinism: the reduction tree is fixed (lane -> wavefront -> workgroup -> one partial per plane and row chunk in
 * `workspace` -> partials added in chunk order by a second launch; no floating-point atomics), and the row chunks of a plane
 * depend on n_lat and n_lon only.  The eight sums of a plane are therefore repeatable bit for bit and depend on the plane's
 * own values, row_w, n_lat and n_lon alone: not on n_planes, on the other planes of the call, or on pointer alignment.
 * pred_planes / truth_planes / clim_planes are DEVICE arrays of n_planes plane pointers (4-byte aligned; 16-byte loads are
 * used where a plane's pointers and n_lon allow); row_w: n_lat device doubles; sums: n_planes x 8 device doubles; workspace:
 * aurora_hip_scores_workspace_bytes(n_planes, n_lat, n_lon) device bytes, 8-byte aligned, no initialisation needed (0 bytes
 * for a non-positive argument).  n_planes = 0 is a no-op.  The inputs are not modified.  Two launches, no host
 * synchronisation, no allocation: capturable in a hipGraph. */
size_t aurora_hip_scores_workspace_bytes(int n_planes, int n_lat, int n_lon);
int aurora_hip_scores(const float* const* pred_planes, const float* const* truth_planes, const float* const* clim_planes,
                      int n_planes, int n_lat, int n_lon, const double* row_w, double* sums, void* workspace, void* stream);

/* ---- scoring an ENSEMBLE against truth on the device (aurora_amd.ensemble_scores: CRPS, ensemble-mean RMSE / bias / MAE,
 * spread, rank histogram; not in the reference) ----------------------------------------------------------------------------
 * Planes as above.  For every plane k < n_planes the M = n_members member planes x_1 .. x_M and the truth plane y are read once.
 * A point is VALID where y and all M members are finite.  Everything is formed in fp64 from the differences to truth,
 * d_m = (double)x_m - (double)y (never from the raw values), per valid point, with the weight w = row_w[i] of the point's row:
 *   per point                                                                    sums[8 k + slot] = sum over valid points of
 *   slot 0                                                                       1   (the count, exact)
 *   slot 1                                                                       w
 *   slot 2  e = (sum_m d_m) / M, members added in member order                   w e     (bias = S2 / S1)
 *   slot 3                                                                       w e^2   (RMSE of the ensemble mean = sqrt(S3 / S1))
 *   slot 4                                                                       w |e|   (MAE of the ensemble mean = S4 / S1)
 *   slot 5  a = (sum_m |d_m|) / M                                                w a
 *   slot 6  g = (1 / M^2) sum_i sum_j |d_i - d_j|
 *             = (2 / M^2) sum_k (2 k - M - 1) d_(k),  d_(1) <= ... <= d_(M)      w g
 *   slot 7  v = sum_m (d_m - e)^2 / (M - 1)                                      w v
 * so that CRPS = (S5 - S6 / 2) / S1, fair CRPS = (S5 - (S6 / 2) M / (M - 1)) / S1, spread = sqrt(S7 / S1) and
 * spread / skill = sqrt((M + 1) / M) spread / RMSE.  (The kernel takes g in the sorted form and multiplies by 1 / M, 2 / M^2
 * and 1 / (M - 1) rounded to fp64; a, g and the counts are formed from the sorted members and do not depend on their order.)
 * hist[(M + 2) k + b] for b <= M is the rank histogram: the number of valid points with exactly b members BELOW the truth
 * (x_m < y, compared as fp32, unweighted); hist[(M + 2) k + M + 1] is the number of valid points with some x_m == y (ties:
 * where a bounded variable sits on its bound the low bins mean little).  All counts are exact; the bins add up to slot 0.
 * A plane without a valid point gives zeros throughout.
 * Determinism as above: a fixed tree (lane -> wavefront -> workgroup -> one partial per plane and row chunk in `workspace`
 * -> partials added in chunk order by a second launch), no atomics; the row chunks of a plane depend on n_lat, n_lon and the
 * member-count bucket (4, 8, 16, 32, 64: the smallest that holds M) only, so the results of a plane are repeatable bit for
 * bit and depend on its own values, row_w, M, n_lat and n_lon alone.
 * member_planes: DEVICE array of n_members x n_planes plane pointers, member-major (member m, plane k at [m n_planes + k]);
 * truth_planes: n_planes pointers (all 4-byte aligned; 16-byte loads are used for M <= 16 where every pointer of a plane and
 * n_lon allow).  2 <= n_members <= 64.  row_w: n_lat device doubles; sums: n_planes x 8 device doubles; hist: n_planes x
 * (n_members + 2) device int64; workspace: what the _workspace_bytes function returns for the same sizes, 8-byte aligned, no
 * initialisation needed (0 bytes for an argument out of range).  n_planes = 0 is a no-op.  The inputs are not modified.  Two
 * launches, no host synchronisation, no allocation: capturable in a hipGraph. */
size_t aurora_hip_ensemble_scores_workspace_bytes(int n_members, int n_planes, int n_lat, int n_lon);
int aurora_hip_ensemble_scores(const float* const* member_planes, const float* const* truth_planes, int n_members, int n_planes,
                               int n_lat, int n_lon, const double* row_w, double* sums, int64_t* hist, void* workspace,
                               void* stream);

/* ---- quantile maps of an ENSEMBLE and the truth's rank map on the device (aurora_amd.ensemble_quantiles: the median, the
 * 10 % and 90 % maps, where the truth fell outside the ensemble; not in the reference) --------------------------------------
 * Planes and plane-pointer arrays as for aurora_hip_ensemble_scores; M = n_members, 2 <= M <= 64.  Per point of plane k:
 *   validity  the point is VALID where all M members are finite; at an invalid point every quantile is NaN.
 *   order     the M fp32 values are put in ascending order x_(0) <= ... <= x_(M-1) of the integer key
 *             bits ^ ((bits >> 31) & 0x7fffffff): the order of the floats, with -0 below +0.
 *   index     for each q[i], 1 <= n_q <= 8 finite values in [0, 1], any order, repeats allowed: h = (M - 1) q[i] in fp64,
 *             j = min(floor(h), M - 1), g = h - j, hi = min(j + 1, M - 1).  The LIBRARY forms (j, g) from the HOST array q
 *             and passes them to the kernel by value; nothing is uploaded.
 *   value     quantiles[((k n_q + i) n_lat + row) n_lon + col] = (float)(a + g (b - a)), a = (double)x_(j), b = (double)x_(hi):
 *             the subtraction, the product and the sum are each rounded to fp64 on their own (no fused multiply-add), and
 *             the result is rounded to fp32 once.  With g = 0 that is x_(j): q = 0 gives the minimum, q = 1 the maximum.
 *   rank      with truth_planes: rank[(k n_lat + row) n_lon + col] = #{m : x_m < y}, the values compared as they are stored
 *             (the rule of the rank histogram of aurora_hip_ensemble_scores); -1 where y or any member is not finite.  The
 *             quantiles do not depend on the truth.
 * truth_planes and rank are both given or both NULL.  quantiles: n_planes x n_q x n_lat x n_lon device floats, 4-byte
 * aligned; rank: n_planes x n_lat x n_lon device int8.  16-byte loads and stores are used for M <= 16 where every member
 * pointer, the truth pointer, the plane's output pointers and n_lon allow; the same bits are written either way.  The outputs
 * must not overlap the inputs, which are not modified.  n_planes = 0 is a no-op.  ONE launch: no workspace, no atomics, no
 * reduction across threads, no host synchronisation, no allocation: capturable in a hipGraph.  A plane's maps depend on its
 * own values, M and q alone, not on the order of the members and not on the other planes of the call. */
int aurora_hip_ensemble_quantiles(const float* const* member_planes, const float* const* truth_planes, int n_members,
                                  int n_planes, int n_lat, int n_lon, const double* q, int n_q, float* quantiles, int8_t* rank,
                                  void* stream);

/* ---- zonal power spectra of a forecast on the device (aurora_amd.spectra; not in the reference) ---------------------------
 * Planes as above, N = n_lon, K = N / 2 + 1 wavenumbers.  For row i of a plane
 *   X_i[k] = sum_n x_i[n] exp(-2 pi i k n / N),  k = 0 .. K-1,        P_i[k] = c_k |X_i[k]|^2 / N^2,
 * with c_0 = 1, c_{N/2} = 1 for an even N and c_k = 2 otherwise, so that sum_k P_i[k] = mean_n x_i[n]^2.  A row is VALID when
 * all N values of every input present (pred and, unless truth_planes is NULL, truth) are finite; validity is decided from the
 * inputs.  band_w is n_bands x n_lat device doubles: the weight w_i of row i in band b, 0 where the row is outside the band
 * (a row belongs to band b exactly where band_w[b n_lat + i] > 0).  For every plane, field and band
 *   power[((plane F + f) n_bands + b) K + k] = sum_{i valid, i in b} w_i P_i[k] / sum_{i valid, i in b} w_i,
 *   rows[plane n_bands + b]                  = the number of valid rows in band b;  a band without one gives NaN and 0.
 * F = 1 without a truth (f = 0: pred); F = 3 with one (f = 0 pred, 1 truth, 2 the error pred - truth, formed in fp64 as
 * X_pred - X_truth).  Everything is fp64: the fp32 values are converted exactly, folded (x[n] +- x[N - n], one rounding per
 * pair) and multiplied on the fp64 matrix pipe (v_mfma_f64_16x16x4_f64) against cosines and sines taken from `twiddle`,
 * accumulating over longitude in ascending order.  twiddle: 2 N device doubles, twiddle[2 m] = cos(2 pi m / N),
 * twiddle[2 m + 1] = sin(2 pi m / N), m = 0 .. N-1, computed by the caller in fp64.
 * Determinism: a fixed tree (MFMA accumulator over longitude -> the rows of a 16-row tile in a fixed order -> one partial per
 * plane and chunk of 32 grid rows in `workspace`, filled tile by tile by the lane that owns the value -> partials added in
 * chunk order by a second launch; no floating-point atomics).  A plane's spectrum is repeatable bit for bit and depends on its
 * own values, band_w, n_lat, n_lon and the presence of a truth alone: not on n_planes, on the other planes of the call, or on
 * pointer alignment (4-byte aligned plane pointers; every load of a plane is a 4-byte load).
 * 2 <= n_lon <= 4096, 1 <= n_bands <= 8.  workspace: the only temporary,
 *   n_planes x ceil(n_lat / 32) x (F n_bands K + 2 n_bands) doubles = aurora_hip_spectra_workspace_bytes(...) bytes
 * (0 for an argument out of range), 8-byte aligned, no initialisation needed; workspace_bytes is what the caller lends and is
 * checked.  n_planes = 0 is a no-op.  The inputs are not modified.  Two launches, no host synchronisation, no allocation, no
 * environment variable: capturable in a hipGraph. */
size_t aurora_hip_spectra_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_bands, int has_truth);
int aurora_hip_spectra(const float* const* pred_planes, const float* const* truth_planes, int n_planes, int n_lat, int n_lon,
                       int n_bands, const double* band_w, const double* twiddle, double* power, int64_t* rows, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- spherical-harmonic power spectra on the device (aurora_amd.sphere_spectra; not in the reference) --------------------
 * Planes as above on a full circle of N = n_lon equally spaced longitudes and H = n_lat >= 2 strictly monotonic latitudes.
 * THE RULE of aurora_amd/sphere_spectra.py, for the device:
 *   TABLE      `table` holds A[m][l][i] = 0.5 w_i Pbar_l^m(sin lat_i) for 0 <= m <= l <= lmax, 0 <= i < H as device doubles,
 *              packed triangularly at (m (lmax + 1) - m (m - 1) / 2 + (l - m)) H + i; w the interpolatory quadrature weights of
 *              the latitude nodes, Pbar the 4 pi-normalised associated Legendre functions, both formed by the caller in fp64.
 *   LMAX       0 <= lmax <= min((H - 1) / 2, (N - 1) / 2): the quadrature is exact for every product of two basis functions
 *              up to that degree and no further.  A table above 1 GiB is refused; the message names the largest lmax that fits.
 *   TRANSFORM  F_m(i) = (1/N) sum_n x_i[n] exp(-2 pi i m n / N), m = 0 .. lmax, the fp32 values converted to fp64 exactly
 *              (folded against `twiddle` as in aurora_hip_spectra);  a_lm = sum_i A[m][l][i] F_m(i);
 *              S_l = sum_{m = 0 .. l} c_m |a_lm|^2, c_0 = 1 and c_m = 2 otherwise, m ascending.
 *   TRUTH      unless truth_planes is NULL, the same S from a^truth and from a^pred - a^truth: F = 3 fields (pred, truth,
 *              error), else F = 1.    power[(plane F + f) (lmax + 1) + l] = S_l.
 *   VALIDITY   a plane is valid where every value of every input given is finite; an invalid plane gives NaN in every field
 *              and valid[plane] = 0 (else 1).  Exception: a pole row -- row 0 where pole_rows & 1, row H - 1 where
 *              pole_rows & 2 -- that holds a non-finite value in any input enters as zeros in every input and is counted in
 *              pole_rows_dropped[plane]; its weight is not redistributed.
 * Three launches: the zonal stage writes F to the workspace as (re, im) in the order [plane][field][m][i]; the Legendre stage
 * is a triangular batch of GEMMs on v_mfma_f64_16x16x4_f64 (rows: 16 degrees, K: latitude in steps of 4, columns: planes) that
 * adds c_m |a_lm|^2 in registers over segments of 16 consecutive m and writes one partial per segment (only the segments that
 * reach a tile's degrees are launched); the finish adds the segments a degree has, l / 16 + 1 of them, in m order.  No floating-point atomics; the tree depends on (H, N, lmax, the presence of a truth) alone; a plane's
 * result is repeatable bit for bit and does not depend on the other planes of the call or on pointer alignment (every load of
 * a plane is a 4-byte load).  workspace: 16-byte aligned, no initialisation needed,
 *   n_planes x (1 or 2) x 16 (lmax + 1) H bytes of F, then n_planes x F x ceil((lmax + 1) / 16) x (lmax + 1) doubles of
 *   partials, then n_planes x ceil(H / 32) x 2 int32 flags, rounded up to 16 = aurora_hip_sphere_spectra_workspace_bytes(...)
 * (0 for an argument out of range).  n_planes = 0 is a no-op.  The inputs are not modified.  No host synchronisation, no
 * allocation, no environment variable: capturable in a hipGraph. */
size_t aurora_hip_sphere_spectra_workspace_bytes(int n_planes, int n_lat, int n_lon, int lmax, int has_truth);
int aurora_hip_sphere_spectra(const float* const* pred_planes, const float* const* truth_planes, int n_planes, int n_lat,
                              int n_lon, int lmax, int pole_rows, const double* table, const double* twiddle, double* power,
                              uint8_t* valid, int32_t* pole_rows_dropped, void* workspace, size_t workspace_bytes, void* stream);

/* ---- spherical-harmonic analysis and synthesis on the device (aurora_amd.sphere_transform; not in the reference) ----------
 * The grid, `table` (the ANALYSIS table A), LMAX, `twiddle`, `pole_rows` and VALIDITY of aurora_hip_sphere_spectra, without a
 * truth.  THE RULE of aurora_amd/sphere_transform.py, for the device:
 *   ANALYSIS   F_m(i) as above; a_lm = sum_i A[m][l][i] F_m(i), rows ascending.  coeff holds n_planes x (lmax + 1) x (lmax + 1)
 *              pairs (re, im) of doubles, coeff[2 ((plane (lmax + 1) + m) (lmax + 1) + l)]: m first, then l.  The call writes
 *              EVERY element: 0 where l < m, NaN in both parts for an invalid plane (valid[plane] = 0); a dropped pole row
 *              enters as zeros and is counted.  The buffer needs no clearing.
 *   SYNTHESIS TABLE  `table` of aurora_hip_sphere_synthesis holds P[m][l][i] = Pbar_l^m(sin lat_i), the basis WITHOUT the
 *              quadrature weights, packed exactly like A (same offset formula, same size, same 1 GiB cap).
 *   INVERSE LEGENDRE  G_m(i) = sum_{l = m .. lmax} b_lm P[m][l][i], l ascending in steps of 4 in the fp64 accumulator of
 *              v_mfma_f64_16x16x4_f64; a step beyond lmax multiplies zeros.  Elements of coeff with l < m are not read.
 *   INVERSE ZONAL  y_i[n] = sum_{m = 0 .. lmax} c_m (Re G_m(i) cos(2 pi m n / N) - Im G_m(i) sin(2 pi m n / N)), c_0 = 1 and
 *              c_m = 2 otherwise, m ascending, FOLDED: for 0 <= n <= N/2, E = sum c_m Re G cos and O = sum c_m Im G sin against
 *              `twiddle` at (m n) mod N; out[n] = (float)(E - O) and, for 0 < n < N/2, out[N - n] = (float)(E + O): one
 *              rounding to fp32.  out: n_planes contiguous planes of n_lat x n_lon floats, 4-byte aligned.
 *   INVALID    valid may be NULL (every plane is synthesised); a plane with valid[plane] = 0 is NaN at every point.  A
 *              dropped pole row is synthesised like any other row.
 * Two launches each.  Analysis: the zonal stage of aurora_hip_sphere_spectra, then the Legendre stage with one wavefront per
 * (16 degrees, 16 consecutive m, 16 planes), every such pair launched, which stores its accumulators.  Synthesis: the inverse
 * Legendre stage with one wavefront per (16 latitudes, one m, 16 planes), which writes G as (re, im) in the order [plane][m][i],
 * then the folded inverse tile per 16 grid rows, the columns n = 0 .. N/2 in passes of 768, stored 4 bytes at a time.  No
 * floating-point atomics; a plane's result is repeatable bit for bit and does not depend on the other planes of the call or
 * on pointer alignment.  Every table, coefficient and workspace index is clamped into its array.  workspace: 16-byte aligned, no
 * initialisation needed: n_planes x 16 (lmax + 1) H bytes of F, then n_planes x ceil(H / 32) x 2 int32 flags, rounded up to 16
 * = aurora_hip_sphere_analysis_workspace_bytes(...); n_planes x 16 (lmax + 1) H bytes of G
 * = aurora_hip_sphere_synthesis_workspace_bytes(...) (0 for an argument out of range).  n_planes = 0 is a no-op.  The inputs
 * are not modified.  No host synchronisation, no allocation, no environment variable: capturable in a hipGraph. */
size_t aurora_hip_sphere_analysis_workspace_bytes(int n_planes, int n_lat, int n_lon, int lmax);
int aurora_hip_sphere_analysis(const float* const* planes, int n_planes, int n_lat, int n_lon, int lmax, int pole_rows,
                               const double* table, const double* twiddle, double* coeff, uint8_t* valid,
                               int32_t* pole_rows_dropped, void* workspace, size_t workspace_bytes, void* stream);
size_t aurora_hip_sphere_synthesis_workspace_bytes(int n_planes, int n_lat, int n_lon, int lmax);
int aurora_hip_sphere_synthesis(const double* coeff, const uint8_t* valid, int n_planes, int n_lat, int n_lon, int lmax,
                                const double* table, const double* twiddle, float* out, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ---- events: contingency tables and the Fractions Skill Score on the device (aurora_amd.event_scores; not in the reference)
 * Planes as above.  A point (i, j) is VALID where pred and truth are both finite.  For plane k, threshold
 * thr = thresholds[k T + t] (fp32, compared in fp32) and the odd window size n = scales[s] = 2 h + 1:
 *   f(i,j) = valid && pred >= thr,   o(i,j) = valid && truth >= thr     (both <= with below != 0; a NaN threshold: no event)
 *   cf(i,j) = sum_{|di| <= h, |dj| <= h} f(i + di, (j + dj) mod n_lon),  co likewise:
 * periodic in longitude, rows outside [0, n_lat) and invalid points count 0.  Summed over the VALID centre columns j of row i:
 *   rowsums[(((k T + t) S + s) n_lat + i) 3 + 0] = sum_j (cf - co)^2
 *   rowsums[(((k T + t) S + s) n_lat + i) 3 + 1] = sum_j cf^2
 *   rowsums[(((k T + t) S + s) n_lat + i) 3 + 2] = sum_j co^2
 *   valid[k n_lat + i]                           = the number of valid points of row i.
 * At n = 1 these are the contingency table of the row: hits = (Bf + Bo - A) / 2, false alarms = Bf - hits, misses = Bo - hits.
 * Everything is an integer and exact (an entry < 4096 x 63^4 < 2^36): the result does not depend on the order of additions,
 * is repeatable bit for bit, and a plane's numbers depend on its own values and thresholds alone -- not on n_planes, on the
 * other planes, or on pointer alignment (4-byte aligned plane pointers; every load of a plane is a 4-byte load).
 * thresholds: n_planes x T DEVICE floats; scales: S HOST int32, odd, ascending, distinct, scales[0] == 1, each <= 63 and
 * <= n_lon.  1 <= T <= 8, 1 <= S <= 8, 1 <= n_lon <= 4096.  rowsums: n_planes x T x S x n_lat x 3 device int64; valid:
 * n_planes x n_lat device int64; both 8-byte aligned, no initialisation needed.
 * The call needs NO workspace: aurora_hip_event_scores_workspace_bytes returns 0 for every argument, `workspace` may be NULL
 * and workspace_bytes 0 (the tables are cleared by a first small launch and filled by 64-bit integer vector atomics).  Arguments are
 * checked before anything is enqueued (AURORA_E_ARG and aurora_hip_last_error()).  n_planes = 0 is a no-op.  The inputs are not
 * modified.  Two launches, no host synchronisation, no allocation, no environment variable: capturable in a
 * hipGraph. */
size_t aurora_hip_event_scores_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_thresholds, int n_scales);
int aurora_hip_event_scores(const float* const* pred_planes, const float* const* truth_planes, int n_planes, int n_lat,
                            int n_lon, const float* thresholds, int n_thresholds, const int32_t* scales, int n_scales, int below,
                            int64_t* rowsums, int64_t* valid, void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-point statistics over a sequence of planes on the device (aurora_amd.FieldStats; not in the reference) -----------
 * The scorers above reduce a plane over space; this one reduces over SAMPLES (roll-out steps, ensemble members, forecast -
 * truth pairs) and keeps the map.  A plane is n_points = n_lat x n_lon fp32 values; a call brings n_samples (1..64) samples
 * of each of n_planes planes and applies them, in sample order, to a state the caller owns.
 * Sample value of a point, with x the value in sample_planes:
 *   second operand b given:  x <- fp32(sqrt((double)x^2 + (double)b^2))          (a wind speed from its components)
 *   v = (double)x - (double)r with a reference r, else v = (double)x;   w = fp32(v)  (= v exactly without a reference)
 * A sample whose x, b or r (or derived x) is not finite is SKIPPED at that point: nothing of the point's state changes.
 * State: arrays [plane][point], contiguous; valid when zero-filled (n = 0 makes origin, vmin, vmax, argmin, argmax unset):
 *   n        int32   valid samples so far
 *   origin   fp32    w of the first valid sample
 *   s1, s2   fp64    sum d and sum d^2 with d = v - (double)origin: SHIFTED sums (differences, never raw values), so that
 *                    mean = origin + s1 / n, var = (s2 - s1^2 / n) / (n - ddof), mean square = (s2 + 2 origin s1 + n origin^2) / n
 *   vmin, vmax       fp32   minimum and maximum of w
 *   argmin, argmax   int32  global index of the FIRST sample that reached the minimum / maximum
 *   exceed, run, longest   int32 [plane][t][point], t < T: with the event w >= thresholds[plane T + t] (<= with below != 0; a
 *                    NaN threshold: no event) the number of events, the current run of consecutive events and the longest
 *                    run.  A skipped sample neither extends nor breaks a run.
 * The global index of the call's first sample is read from *sample_index (a DEVICE int64) by the main launch; a second,
 * one-thread launch then adds n_samples to it.  No host counter: a captured call replays with the right indices.  Indices
 * are kept as int32.
 * sample_planes: DEVICE array of n_samples x n_planes plane pointers, sample-major (sample s, plane k at [s n_planes + k]);
 * ref_planes: n_planes pointers or NULL; second_planes: n_samples x n_planes pointers or NULL; a NULL entry of either means
 * "none for this plane".  All plane pointers 4-byte aligned; 16-byte loads and stores are used for a plane where
 * n_points % 4 == 0 and every pointer involved is 16-byte aligned (the same elements either way).  thresholds: n_planes x T
 * device floats, 0 <= T <= 8 (T = 0: thresholds, exceed, run, longest may be NULL).  s1, s2, sample_index 8-byte aligned.
 * Determinism: nothing is reduced across threads.  A point's state depends on its own samples in their order alone: not on
 * n_planes, on the other planes, on pointer alignment, or on how the samples are grouped into calls (one call with S samples
 * leaves the bits that S calls with one sample leave).
 * One main launch over all planes and samples (a point's state is read once and written once: 4 n_samples + 2 (36 + 12 T)
 * bytes per point) and the one-thread launch.  Arguments are checked before anything is enqueued (AURORA_E_ARG and
 * aurora_hip_last_error()).  n_planes = 0 is a no-op.  The inputs are not modified.  No workspace, no atomics, no host
 * synchronisation, no allocation, no environment variable: capturable in a hipGraph. */
int aurora_hip_field_stats_update(const float* const* sample_planes, const float* const* ref_planes,
                                  const float* const* second_planes, int n_samples, int n_planes, int64_t n_points,
                                  const float* thresholds, int n_thresholds, int below, int64_t* sample_index, int32_t* n,
                                  float* origin, double* s1, double* s2, float* vmin, float* vmax, int32_t* argmin,
                                  int32_t* argmax, int32_t* exceed, int32_t* run, int32_t* longest, void* stream);

/* ---- event probabilities of an ENSEMBLE on the device (aurora_amd.probability_scores: Brier score and its decomposition,
 * reliability diagram, ROC; not in the reference) ----------------------------------------------------------------------------
 * Planes, members and thresholds as above: for every plane p < n_planes the M = n_members member planes x_1 .. x_M and the
 * truth plane y are read once.  A point is VALID where y and all M members are finite.  For the threshold
 * thr = thresholds[p T + t] (fp32, compared in fp32), over the valid points:
 *   k(i,j) = #{m : x_m >= thr} in 0..M,    o(i,j) = [y >= thr]       (both <= with below != 0; a NaN threshold: k = 0, o = 0)
 *   rows[(((p n_lat + i) T + t) 2 + o) (M + 1) + k] = the number of valid points of row i with that (o, k)
 * -- the whole output.  The ensemble's forecast probability of the event at a point is k / M, so with row weights w_i and
 * W[o][k] = sum_i w_i rows[i][t][o][k], n_k = W[0][k] + W[1][k], N = sum_k n_k, p_k = k / M, the caller forms
 *   Brier score = sum_k (W[1][k] (1 - p_k)^2 + W[0][k] p_k^2) / N,   base rate obar = sum_k W[1][k] / N,
 *   observed frequency obar_k = W[1][k] / n_k,   reliability = sum_k n_k (p_k - obar_k)^2 / N,
 *   resolution = sum_k n_k (obar_k - obar)^2 / N,   uncertainty = obar (1 - obar)     (Brier = reliability - resolution +
 *   uncertainty exactly: the forecast takes M + 1 values only),   and the ROC points of "warn when k >= c":
 *   hit rate = sum_{k >= c} W[1][k] / sum_k W[1][k],  false alarm rate likewise from W[0]    (aurora_amd/probability.py).
 * Every number is an exact integer (an entry <= n_lon < 2^31), so the table does not depend on any order of addition and is
 * repeatable bit for bit; a plane's table depends on its own values and thresholds alone -- not on n_planes, on the other
 * planes, or on pointer alignment -- and the order of the members does not matter.  The bins of a (row, t) add up to the
 * row's valid points; a row or plane without a valid point gives zeros.
 * member_planes: DEVICE array of n_members x n_planes plane pointers, member-major (member m, plane p at [m n_planes + p]);
 * truth_planes: n_planes pointers (all 4-byte aligned; 16-byte loads are used for a plane where every pointer of it is 16-byte
 * aligned and n_lon % 4 == 0: the same elements either way).  thresholds: n_planes x T DEVICE floats.  2 <= n_members <= 64,
 * 1 <= T <= 8, n_lat >= 1, 1 <= n_lon < 2^31.  rows: n_planes x n_lat x T x 2 x (M + 1) device int32, 4-byte aligned, no
 * initialisation needed: every entry is written, with plain stores, by the wavefront that owns the row (no global atomics,
 * no clearing launch).  There is no workspace and no plane-sized temporary.  Arguments are checked before anything is enqueued
 * (AURORA_E_ARG and aurora_hip_last_error()).  n_planes = 0 is a no-op.  The inputs are not modified.  One launch; the call
 * allocates nothing, does not wait for the device and reads no environment variable: capturable in a hipGraph. */
int aurora_hip_probability_scores(const float* const* member_planes, const float* const* truth_planes, int n_members,
                                  int n_planes, int n_lat, int n_lon, const float* thresholds, int n_thresholds, int below,
                                  int32_t* rows, void* stream);

/* ---- conditional scores on the device (aurora_amd.conditional_scores: error by truth bin, thresholded RMSE of the tails; not
 * in the reference) -----------------------------------------------------------------------------------------------------------
 * Planes as above.  For every plane k < n_planes the prediction p, the truth t and, unless its array is NULL, a centre map c and
 * a scale map s are read once.  With v the binned field (t, or p with by_pred != 0) and e_j = edges[k n_edges + j] (fp32):
 *   a   = (double)v - (double)c                      (one fp64 subtraction; c = 0 without centre_planes)
 *   bin = #{ j < n_edges : a >= (double)e_j * (double)s }   (one fp64 product per edge, alone on its side of the comparison;
 *                                                     s = 1 without scale_planes; a NaN edge is never passed)
 * so a plane has n_edges + 1 bins, and with ascending edges bin b holds the points between edge b - 1 and edge b.  A point is
 * VALID where p and t are finite, every map that is present is finite, and s >= 0 (s = 0 is legal: the products are +-0 and
 * the point falls by the sign of a).  Over the valid points of bin b, with w = row_w[i] of the point's row i and d = p - t:
 *   sums[(k (n_edges + 1) + b) 5 + slot]:  slot 0  1 (the count, exact)   slot 1  w   slot 2  w d   slot 3  w d^2   slot 4  w |d|
 * -- the first five slots of aurora_hip_scores, per bin.  An empty bin gives zeros.  Differences and products are formed in
 * fp64 from the fp32 inputs and accumulated in fp64.
 * Determinism: the reduction tree of aurora_hip_scores (lane -> wavefront -> workgroup -> one partial per plane, row chunk and
 * bin in `workspace` -> partials added in chunk order by a second launch; no atomics).  A point enters every bin but its own
 * as exactly +0, so the five sums of a bin are repeatable bit for bit and depend on the points of THAT bin, row_w, n_lat and
 * n_lon alone: not on n_planes, on the other planes, on pointer alignment, or on how many other edges the call has (the bin
 * [e1, e2) of a 2-edge call has the bits of that bin in an 8-edge call).
 * The four plane arrays are DEVICE arrays of n_planes plane pointers (4-byte aligned; 16-byte loads are used where all of a
 * plane's pointers and n_lon allow; an array may name the same plane for several k); edges: n_planes x n_edges DEVICE floats,
 * 1 <= n_edges <= 8; row_w: n_lat device doubles; sums: n_planes x (n_edges + 1) x 5 device doubles; workspace:
 * aurora_hip_conditional_scores_workspace_bytes(n_planes, n_lat, n_lon, n_edges) device bytes, 8-byte aligned, no
 * initialisation needed (0 bytes for an argument out of range).  Arguments are checked before anything is enqueued
 * (AURORA_E_ARG and aurora_hip_last_error()).  n_planes = 0 is a no-op.  The inputs are not modified.  Two launches, no host
 * synchronisation, no allocation, no environment variable: capturable in a hipGraph. */
size_t aurora_hip_conditional_scores_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_edges);
int aurora_hip_conditional_scores(const float* const* pred_planes, const float* const* truth_planes,
                                  const float* const* centre_planes, const float* const* scale_planes, int n_planes, int n_lat,
                                  int n_lon, const float* edges, int n_edges, int by_pred, const double* row_w, double* sums,
                                  void* workspace, void* stream);

/* ---- derived fields on the device (aurora_amd.diagnostics: relative vorticity, divergence, wind speed, total column water
 * vapour, integrated vapour transport; not in the reference) -----------------------------------------------------------------
 * Planes as above (n_lat x n_lon fp32, row-major), n_lat >= 2, n_lon >= 2.  Constants of the caller's tables: the Earth's
 * radius a = 6 371 229 m and g = 9.80665 m s^-2.  All inputs are fp32; every expression is evaluated in fp64 and the result
 * is rounded to fp32 ONCE; a result that is not finite is stored as NaN.  Every term of a formula is evaluated, also where
 * its coefficient is 0, so a NaN or an infinity that a stencil reads propagates by the IEEE rules (inf x 0 = NaN).
 * WIND GROUP, n_wind items, ONE launch.  Item k reads the planes wind_u[k] and wind_v[k] and writes vo_planes[k],
 * div_planes[k] and ws_planes[k]; a table that is NULL as a whole, or a NULL entry of a table, skips that output.
 *   row_table: n_lat x 4 device doubles (A, m0, m1, m2)_i, computed by the caller in fp64 from the latitudes phi_i (radians):
 *     A_i = 1 / (a cos phi_i), NaN for a pole row (|lat_i| >= 90 - 1e-9 degrees): pole rows come out NaN, no polar-cap formula;
 *     (m0, m1, m2)_i = (c0 cos phi_{i-1}, c1 cos phi_i, c2 cos phi_{i+1}) with the three-point first-derivative formula for
 *     unequal spacing, h1 = phi_i - phi_{i-1}, h2 = phi_{i+1} - phi_i:
 *       c0 = -h2 / (h1 (h1 + h2)),   c1 = (h2 - h1) / (h1 h2),   c2 = h1 / (h2 (h1 + h2));
 *     first row c = (0, -1 / h2, 1 / h2), last row c = (-1 / h1, 1 / h1, 0); a row that does not exist has the coefficient 0
 *     and is read at the clamped index.  The true phi enter, so descending latitudes need no sign flag.
 *   L = 1 / (2 dlambda), dlambda the longitude step in radians.  With wrap != 0 the grid covers the full circle:
 *     d_lambda f = (f[j + 1 mod n_lon] - f[j - 1 mod n_lon]) L.  With wrap == 0 the grid is regional: interior columns
 *     likewise, column 0 takes (f[1] - f[0]) 2 L and column n_lon - 1 takes (f[n_lon - 1] - f[n_lon - 2]) 2 L.
 *   vo  = A_i (d_lambda v - (m0 u[i-1] + m1 u[i] + m2 u[i+1]))            relative vorticity, s^-1
 *   div = A_i (d_lambda u + (m0 v[i-1] + m1 v[i] + m2 v[i+1]))            horizontal divergence, s^-1
 *   ws  = fp32(sqrt((double)u^2 + (double)v^2))                           the expression of aurora_hip_field_stats_update
 *   u and v of an item are read from memory once for all three outputs (a wavefront walks down a strip of 256 columns with a
 *   rolling three-row window in registers; the east and west neighbours across a lane's four columns are overlapping 4-byte
 *   loads of the row just fetched).  An item without vo and div reads no neighbour rows.  row_table may be NULL when both
 *   vo_planes and div_planes are.
 * COLUMN GROUP, n_cols items (one per batch element), ONE launch.  Item k reads the n_levels planes q_planes[k C + c] and,
 * where needed, col_u[k C + c] and col_v[k C + c] (C = n_levels, 2..64), and writes, each table and each entry nullable,
 *   tcwv[k] = sum_c w_c q_c,   ivtu[k] = sum_c w_c q_c u_c,   ivtv[k] = sum_c w_c q_c v_c,   ivt[k] = sqrt(ivtu^2 + ivtv^2)
 *   with w = level_w: C device doubles in the order of the planes, w_c = 100 (p_next - p_prev) / (2 g) with the neighbours of
 *   level c in the SORTED pressures (hPa); an end level takes half its one interval; nothing is extrapolated to the surface
 *   or to the top.  The levels are accumulated in fp64 in level order in registers (the product as (w_c q_c) u_c); ivt is
 *   formed from the fp64 sums.  col_u (col_v) may be NULL unless ivtu (ivtv) or ivt is asked for.
 * Either group may be empty (n_wind = 0, n_cols = 0: its pointers are not looked at); both empty is a no-op.  All tables are
 * DEVICE arrays of plane pointers; the entries of the input tables must not be NULL.  Plane pointers are 4-byte aligned;
 * 16-byte loads and stores are used for a plane where its pointer is 16-byte aligned and n_lon % 4 == 0 (columns: n_lat x
 * n_lon % 4 == 0 and every input plane of the item aligned): the same elements either way.  Nothing is reduced across
 * threads: a point's result depends on the values its formula names alone, is repeatable bit for bit, and does not depend
 * on the other items of the call or on pointer alignment.  The inputs are not modified.  An output plane must not overlap
 * an input plane (another wavefront may still have to read the neighbours of a point) or another output plane.
 * Arguments are checked before anything is enqueued (AURORA_E_ARG and aurora_hip_last_error()).  No workspace, no atomics, no
 * host synchronisation, no allocation, no environment variable: capturable in a hipGraph. */
int aurora_hip_diagnostics(const float* const* wind_u, const float* const* wind_v, float* const* vo_planes,
                           float* const* div_planes, float* const* ws_planes, int n_wind, const double* row_table, double L,
                           int wrap, const float* const* q_planes, const float* const* col_u, const float* const* col_v,
                           float* const* tcwv_planes, float* const* ivtu_planes, float* const* ivtv_planes,
                           float* const* ivt_planes, int n_cols, int n_levels, const double* level_w, int n_lat, int n_lon,
                           void* stream);

/* ---- verification sums by region on the device (aurora_amd.region_scores: the scores of aurora_amd.scores over latitude
 * bands, longitude boxes and masks; not in the reference) ----------------------------------------------------------------------
 * Planes as above.  For every plane k < n_planes the prediction p, the truth t and, unless clim_planes is NULL, the
 * climatology c are read once.  The point (i, j) BELONGS to region r < n_regions where bit r of
 *   row_bits[i] & col_bits[j] & mask_bits[i n_lon + j]                      (mask_bits = NULL: every bit set)
 * is set; regions may overlap.  A point is VALID as in aurora_hip_scores: p, t and (if given) c finite.  Over the valid points
 * of region r, with w = row_w[i]:
 *   sums[(k n_regions + r) 8 + slot]: the eight slots of aurora_hip_scores (count, w, w d, w d^2, w |d|, w p' t', w p'^2,
 *   w t'^2; slots 5..7 are 0 without clim_planes)
 * -- aurora_hip_scores' sums restricted to the region.  A region without a valid point gives zeros.  Differences and products
 * are formed in fp64 from the fp32 inputs and accumulated in fp64.  A row i whose byte has none of the bits 0 .. n_regions - 1
 * set is not read at all.
 * Determinism: the reduction tree of aurora_hip_scores (lane -> wavefront -> workgroup -> one partial per plane, row chunk and
 * region in `workspace` -> partials added in chunk order by a second launch; no atomics).  A point enters every region it does
 * not belong to as exactly +0, so the eight sums of a region are repeatable bit for bit and depend on the points of THAT
 * region, row_w, n_lat and n_lon alone: not on n_planes, on the other planes, on the alignment of any pointer, on which other
 * regions share the call or how many, or (slots 0..4, where c is finite wherever p and t are) on whether a climatology is given.
 * The three plane arrays are DEVICE arrays of n_planes plane pointers (4-byte aligned).  row_bits: n_lat device bytes;
 * col_bits: n_lon device bytes; mask_bits: NULL or n_lat x n_lon device bytes, row-major; any alignment.  16-byte loads of the
 * planes and 4-byte loads of col_bits and mask_bits are used where n_lon % 4 == 0, all of a plane's pointers are 16-byte
 * aligned and col_bits and mask_bits are 4-byte aligned: the same elements either way.  1 <= n_regions <= 8; bits n_regions
 * .. 7 of the tables are ignored.  row_w: n_lat device doubles; sums: n_planes x n_regions x 8 device doubles; workspace:
 * aurora_hip_region_scores_workspace_bytes(n_planes, n_lat, n_lon, n_regions) device bytes, 8-byte aligned, no
 * initialisation needed (0 bytes for an argument out of range).  Arguments are checked before anything is enqueued
 * (AURORA_E_ARG and aurora_hip_last_error()).  n_planes = 0 is a no-op.  The inputs are not modified.  Two launches, no
 * plane-sized temporary, no host synchronisation, no allocation, no environment variable: capturable in a hipGraph. */
size_t aurora_hip_region_scores_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_regions);
int aurora_hip_region_scores(const float* const* pred_planes, const float* const* truth_planes,
                             const float* const* clim_planes, int n_planes, int n_lat, int n_lon, const uint8_t* row_bits,
                             const uint8_t* col_bits, const uint8_t* mask_bits, int n_regions, const double* row_w,
                             double* sums, void* workspace, void* stream);

/* ---- threshold objects on the device (aurora_amd.objects: connected components of events with their sizes, positions and
 * peaks; not in the reference) ----------------------------------------------------------------------------------------------
 * Planes as above.  For every plane k < n_planes and threshold t < n_thresholds (thresholds[k n_thresholds + t], device fp32;
 * NaN: no event) a point is an EVENT where its value v is finite and v >= threshold (below = 1: v <= threshold).  An OBJECT is
 * a maximal connected set of events: `connectivity` 4 or 8 among grid neighbours, none beyond row 0 or row n_lat - 1; with
 * wrap = 1 column n_lon - 1 and column 0 are neighbours (diagonally too with 8).  Its FIRST POINT is its smallest flat index
 * i n_lon + j, and objects are numbered 1, 2, ... in ascending order of their first points.
 *   labels[(k n_thresholds + t) n_lat n_lon + i n_lon + j]   int32: the number of the point's object, 0 for background
 *   count[k n_thresholds + t]                                int32: the number of objects (also beyond max_objects)
 *   table[((k n_thresholds + t) max_objects + (o - 1)) 10 + c]   int64, for the objects o <= max_objects; other rows are 0:
 *     0 points   1 area_units = sum of unit[i] (device int64 per row)   2 first   3 row_min   4 row_max   5 row_sum = sum of i
 *     6 col_off_min  7 col_off_max  8 col_off_sum of d = j - j_first, with wrap reduced into [-(n_lon / 2), n_lon - n_lon / 2)
 *     9 peak_key = (K(v) << 32) | (0xffffffff - flat index), the unsigned 64-bit MAXIMUM over the points, where for the bits
 *       u of v: K = ~u if u has the sign bit, else u | 0x80000000 (ascending with v, -0 below +0), and ~K is taken with
 *       below = 1: the largest (below: smallest) value, and among equal values the smallest flat index.
 * Union-find in `workspace`, aurora_hip_objects_workspace_bytes(n_planes, n_lat, n_lon, n_thresholds) device bytes (one int32
 * per point and threshold plus one per row and threshold; 8-byte aligned; no initialisation needed; 0 for an argument out of
 * range): seven launches on `stream` (zero, rows, unite, flatten, scan, number, tabulate).  parent[x] <= x holds throughout,
 * every loop moves to a strictly smaller index or is bounded by n_lat or n_lon, and no launch waits on a value written within
 * it.  The table is filled by 64-bit integer atomics only.  labels, count and table are repeatable bit for bit and depend on
 * the plane's own values and thresholds alone: not on the other planes, not on the alignment of a plane pointer (planes are
 * read 4 bytes at a time), not on the order in which workgroups run.
 * 1 <= n_lon <= 4096, n_lat n_lon <= 2^31 - 2, 1 <= n_thresholds <= 8, max_objects >= 1; workspace_size: the bytes at
 * `workspace`, refused if too few.  Arguments are checked before anything is enqueued (AURORA_E_ARG and
 * aurora_hip_last_error()).  n_planes = 0 is a no-op.  The inputs are not modified.  No host synchronisation, no allocation,
 * no environment variable: capturable in a hipGraph. */
size_t aurora_hip_objects_workspace_bytes(int n_planes, int n_lat, int n_lon, int n_thresholds);
int aurora_hip_objects(const float* const* planes, int n_planes, int n_lat, int n_lon, const float* thresholds,
                       int n_thresholds, const int64_t* unit, int below, int connectivity, int wrap, int max_objects,
                       int32_t* labels, int32_t* count, int64_t* table, void* workspace, size_t workspace_size, void* stream);

/* ---- spatial quantiles of planes on the device (aurora_amd.field_quantiles: a plane's 0.9 / 0.99 quantile by area or by
 * count, the percentile thresholds of the event modules; not in the reference) ------------------------------------------------
 * Planes as above.  For every plane k < n_planes on its own:
 *   VALIDITY  a point is valid where its value is finite: NaN and +-Inf drop out.  valid[k] = n is their number.
 *   ORDER     by the 32-bit key K(v) of aurora_hip_objects: for the bits u of v, K = ~u if u has the sign bit, else
 *             u | 0x80000000: ascending with the value, -0 below +0.
 *   unit = NULL (kind = count): numpy's method = "linear" over the valid points, the expression of
 *             aurora_hip_ensemble_quantiles with n in place of M.  For q_i: h = (double)(n - 1) q_i, j = min(floor(h), n - 1),
 *             g = h - j, hi = min(j + 1, n - 1), and with a = (double)x_(j), b = (double)x_(hi)
 *               values[k n_q + i] = (float)(a + g (b - a)),
 *             the three fp64 operations rounded one by one (never an fma).  (j, g) are formed on the device, where n is known,
 *             by these very operations.  n = 0 gives NaN.  total[k] = n.
 *   unit != NULL (kind = area): unit[i] is the integer weight of row i (n_lat device int64, >= 0; aurora_amd.objects.area_units:
 *             llrint(w_i 2^32)).  W = sum of unit over the valid points = total[k];
 *               target = min(max((int64)ceil(q_i (double)W), 1), W),
 *               values[k n_q + i] = the smallest valid x with U(x) = sum{unit : K <= K(x)} >= target
 *             -- the inverted CDF, no interpolation.  W = 0 (no valid point, or all of them on rows of unit 0) gives NaN.
 * q: n_q HOST doubles, 1 <= n_q <= 8, finite and in [0, 1], in any order, repeats allowed; they are passed to the kernels by
 * value, so nothing is uploaded.  An exact radix select over K, most significant byte first, 8 bits per pass: a zeroing
 * launch, then four passes that each read the planes once (16-byte loads where n_lon % 4 == 0 and the plane pointer is
 * 16-byte aligned, 4-byte loads otherwise: the same elements either way) and fill 256-bin histograms of 64-bit integers in
 * `workspace`, each followed by a small launch that picks every target's bin; nine launches on `stream`.  Everything that is
 * accumulated is an integer, so values, valid and total are repeatable bit for bit, equal the rule above exactly, and depend
 * on the plane's own values, unit and q alone: not on the other planes, the alignment of a plane pointer or the order of the
 * atomics.  No launch waits on a value written within it; every loop is bounded by n_lat, n_lon, 256 or the number of targets.
 * workspace: aurora_hip_field_quantiles_workspace_bytes(n_planes, n_q) device bytes (histograms only: (2 + 6 n_q) x 256 x 8
 * bytes and a few hundred more per plane, never plane-sized; 8-byte aligned; cleared by the call's own first launch; 0 for
 * an argument out of range); workspace_bytes: the bytes at `workspace`, refused if too few.  n_lat n_lon <= 2^31 - 2, and
 * <= 2^30 with unit (the unit sum stays within int64).  values: n_planes x n_q device floats; valid, total: n_planes device
 * int64.  Arguments are checked before anything is enqueued (AURORA_E_ARG and aurora_hip_last_error()).  n_planes = 0 is a
 * no-op.  The inputs are not modified.  No plane-sized temporary, no host synchronisation, no allocation, no environment
 * variable: capturable in a hipGraph. */
size_t aurora_hip_field_quantiles_workspace_bytes(int n_planes, int n_q);
int aurora_hip_field_quantiles(const float* const* planes, int n_planes, int n_lat, int n_lon, const int64_t* unit,
                               const double* q, int n_q, float* values, int64_t* valid, int64_t* total, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- overlap pairs of two label maps on the device (aurora_amd.object_matches: which object of one field is which object of
 * another, and how much they share; not in the reference) ----------------------------------------------------------------------
 * labels_a, labels_b: n_items label maps each (an item is a plane and a threshold), n_lat x n_lon device int32, row-major, one
 * after the other, as aurora_hip_objects writes them; the maps need not be connected.  For every item on its own a point of row
 * i CONTRIBUTES where 1 <= la <= max_objects_a and 1 <= lb <= max_objects_b (any other value, negative ones and labels past
 * the tables included, is ignored), to the pair (la, lb): one point and unit[i] area units (n_lat device int64, the units of
 * aurora_hip_objects).
 *   pairs[(item max_pairs + r) 4 + c]   int64: row r = [ka, kb, points, area_units] of the r-th pair in ascending (ka, kb)
 *                                       order; rows past count are 0
 *   count[item]                         int32: the number of pairs; -1 where there are more than max_pairs: the item OVERFLOWS
 *                                       and all its rows are 0 (never a partial table, whose contents would depend on the
 *                                       order of insertion)
 * Hash aggregation in `workspace`, aurora_hip_object_matches_workspace_bytes(n_items, max_pairs) device bytes (8-byte aligned;
 * cleared by the call's own first launch; 0 for an argument out of range): per item an open-addressed table of
 * C = max(64, pow2ceil(2 max_pairs)) slots as 3 C + 1 words of 64 bits -- C key words (0 = empty, else (ka << 32) | kb), C points
 * words, C units words and one overflow word.  THE HOME SLOT of a key is
 *   home = (((uint64_t)ka << 32 | kb) * 0x9E3779B97F4A7C15) >> (64 - log2 C),
 * the product taken modulo 2^64, with linear probing upwards that wraps from slot C - 1 to slot 0 (aurora_amd/csrc/pairs_hash.h).
 * A key is claimed by one 64-bit compare-and-swap; the walk ends after C slots at the latest, then the overflow word is set and
 * the contribution dropped.  Three launches on `stream` (zero, accumulate, finish): accumulate reads both maps once, four bytes
 * at a time, a wavefront per row, the lanes that share a key combined first and a run carried across the row; finish gathers
 * the keys of an item, sorts them in LDS (8 x max(2, pow2ceil(max_pairs)) bytes) and writes the rows.  Only 64-bit integers are
 * accumulated, so pairs and count are repeatable bit for bit and depend on the item's own two maps and unit alone: not on the
 * other items, not on the alignment of a map, not on the order in which workgroups run.  No launch waits on a value written
 * within it; every loop is bounded by C, n_lon or 64.
 * n_lat n_lon <= 2^31 - 2, max_objects_a, max_objects_b >= 1, 1 <= max_pairs <= 8192; workspace_size: the bytes at `workspace`,
 * refused if too few.  Arguments are checked before anything is enqueued (AURORA_E_ARG and aurora_hip_last_error()), and then
 * nothing is written.  n_items = 0 is a no-op.  The inputs are not modified.  No host synchronisation, no allocation, no
 * environment variable: capturable in a hipGraph. */
size_t aurora_hip_object_matches_workspace_bytes(int64_t n_items, int max_pairs);
int aurora_hip_object_matches(const int32_t* labels_a, const int32_t* labels_b, int64_t n_items, int n_lat, int n_lon,
                              const int64_t* unit, int max_objects_a, int max_objects_b, int max_pairs, int32_t* count,
                              int64_t* pairs, void* workspace, size_t workspace_size, void* stream);

/* ---- the nearest event of every grid point on the sphere, and the separations of objects (aurora_amd.nearest_event,
 * aurora_amd.object_separations: minimum boundary separation, Hausdorff distance, "nearest observed object within 300 km"; not
 * in the reference) ----------------------------------------------------------------------------------------------------------
 * labels: n_items label maps as above; an EVENT is a point with label > 0.  tables: 2 n_lat + n_lon device doubles made on the
 * host: s[i] = sin(lat_i), then c[i] = max(cos(lat_i), 0), then cd[d] = cos(d dlon) for d < n_lon with cd[0] = 1, for strictly
 * monotone latitudes and equally spaced longitudes.  For every item on its own (THE RULE of aurora_amd/distances.py):
 *   GAP        of columns j and j': d = |j - j'|, with wrap = 1 min(d, n_lon - d).
 *   CANDIDATE  of target column j in source row k: the event of row k with the smallest gap, of two at the same gap the
 *              smaller column; a row without events has none.
 *   KEY        key(i, k, d) = 1 - (s_i s_k + (c_i c_k) cd[d]), every fp64 operation rounded on its own (never an fma),
 *              negative results 0; a point that is itself an event is its own candidate with key exactly 0.
 *   NEAREST    of (i, j): the row candidate with the smallest key, of equal keys the smallest flat index k n_lon + j';
 *              candidates with key > key_max are ignored (key_max = +inf: no bound).
 *   index[item n_lat n_lon + i n_lon + j]   int32: the flat index of the nearest event, -1 where there is none
 *   key[...]                                fp64: its key, 1 - cos(angle); +inf where index is -1
 * Three launches on `stream` (rows, extent, search): the candidates of every row as int16 in `workspace`,
 * aurora_hip_nearest_event_workspace_bytes(n_items, n_lat, n_lon) device bytes (2 bytes per point, 4 per row, 8 per item;
 * 8-byte aligned; no initialisation needed; 0 for an argument out of range); then every point walks the rows outward from its
 * own and stops a direction at the first row whose zero-gap key exceeds min(best, key_max) by more than 2^-46, which proves
 * that no farther row can win or tie (the derivation is in aurora_amd/csrc/nearest_event_search.h).  The walk is bounded by
 * n_lat per direction, stays within the rows that have events, and waits for nobody; an item without events walks no row.
 * index and key are repeatable bit for bit and depend on the item's own map and the tables alone.
 *
 * aurora_hip_object_separations: labels_a as above, key and index as written by aurora_hip_nearest_event for the OTHER map b,
 * count_a[item] the number of objects of a (device int32).  For every object o <= max_objects of a, over its points:
 *   table[(item max_objects + (o - 1)) 3 + c]   int64: 0 key_bits, the least key as the int64 of its fp64 bits (keys are not
 *              negative, so they order like their bits); 1 a_point, the smallest flat index among the object's points that
 *              attain it; 2 b_point = index[a_point].  Rows at or past count_a are 0; an object none of whose points has a
 *              nearest event (or that has no point) is [bits of +inf, -1, -1].
 *   hausdorff[item]                             int64: the greatest key over ALL events of a (labels past max_objects
 *              included) as bits; 0 without events, the bits of +inf where an event has no nearest event.
 * Four launches (init, least, point, finish); 64-bit integer minima and maxima by vector atomics only, the lanes of a wave
 * that share a label combined first, so the result does not depend on the order of the atomics.  No workspace.
 * 1 <= n_lon <= 4096 (nearest_event), n_lat n_lon <= 2^31 - 2, max_objects >= 1, key_max >= 0; workspace_size: the bytes at
 * `workspace`, refused if too few.  Arguments are checked before anything is enqueued (AURORA_E_ARG and
 * aurora_hip_last_error()), and then nothing is written.  n_items = 0 is a no-op.  The inputs are not modified.  No host
 * synchronisation, no allocation, no environment variable: capturable in a hipGraph. */
size_t aurora_hip_nearest_event_workspace_bytes(int64_t n_items, int n_lat, int n_lon);
int aurora_hip_nearest_event(const int32_t* labels, int64_t n_items, int n_lat, int n_lon, const double* tables, int wrap,
                             double key_max, int32_t* index, double* key, void* workspace, size_t workspace_size, void* stream);
int aurora_hip_object_separations(const int32_t* labels_a, const double* key, const int32_t* index, const int32_t* count_a,
                                  int64_t n_items, int n_lat, int n_lon, int max_objects, int64_t* table, int64_t* hausdorff,
                                  void* stream);

/* ---- fields smoothed over a great-circle disc on the device (aurora_amd.smooth: the mean over all points within R km, the
 * first step of object-based verification; not in the reference) ----------------------------------------------------------------
 * Planes as above; out: n_planes x n_lat x n_lon device fp32, one output plane after the other (4-byte aligned).  The disc
 * is given as a TABLE made on the host in fp64 (aurora_amd/smooth.py: disc_table), and nothing else decides membership:
 *   row_lo[i], row_count[i]   int32 per target row i: its source rows are k = row_lo[i] + r, r < row_count[i] <= max_rows <= 255
 *   half[i max_rows + r]      int32: the columns j - n .. j + n of source row k belong to the target (i, j); n = -1: none.  n is
 *                             the largest gap d with sin_i sin_k + cos_i cos_k cos(d dlambda) >= cos(R / a), a = 6371.229 km
 *   w[k]                      fp64 per row: cos(lat_k), exactly 0 for a pole row
 * A point is VALID where it is finite; an invalid point enters as value 0 with count 0.  Per row of a plane the EXCLUSIVE
 * PREFIX tables P[0 .. n_lon] (fp64 sums of the valid values, P[0] = 0) and N[0 .. n_lon] (int32 counts) give the sum S and
 * the count C of a window lo = j - n, hi = j + n + 1 (aurora_amd/csrc/smooth_window.h), with W = n_lon:
 *   wrap = 1 (full circle):  2 n + 1 >= W: P[W];   lo < 0: (P[W] - P[lo + W]) + P[hi];   hi > W: (P[W] - P[lo]) + P[hi - W];
 *                            otherwise P[hi] - P[lo]
 *   wrap = 0 (regional):     P[min(hi, W)] - P[max(lo, 0)]
 * and over the source rows in ascending k, in fp64:
 *   num = sum w_k S_k,   den = sum w_k C_k,   full = sum w_k F_k,   F = 2 n + 1 (wrap = 1: at most W)
 *   out = (float)(num / den); NaN where den <= 0, where den / full < min_valid (columns clipped off a regional grid count as
 *   invalid), where the result is not finite and, with keep_mask = 1, where the centre point itself is not finite.
 * Two launches on `stream`.  prefix: a wavefront owns one row, walks it in chunks of 256 columns (a lane adds its four values
 * in order, the lanes' totals go through an inclusive scan with a fixed shuffle tree, the running sum is carried from chunk to
 * chunk) and writes P and N into `workspace`: aurora_hip_smooth_workspace_bytes(n_planes, n_lat, n_lon) device bytes, 12 per
 * entry of n_planes x n_lat x (n_lon + 1), PLANE-SIZED, 8-byte aligned, no initialisation needed (0 for an argument out of
 * range).  gather: a workgroup owns 4 target rows x 256 adjacent columns; a lane reads P and N at its window's ends and writes
 * one fp32.  No atomics; nothing is reduced across threads; every index is clamped into its row.  16-byte loads are used for a
 * plane whose pointer is 16-byte aligned where n_lon % 4 == 0: the same elements in the same association either way, so the
 * output is repeatable bit for bit and depends on the plane's own values and the table alone: not on the other planes, not on
 * n_planes, not on pointer alignment.  out must not overlap an input plane or the workspace.
 * n_lat n_lon <= 2^31 - 1, 1 <= max_rows <= 255, 0 <= min_valid <= 1; workspace_size: the bytes at `workspace`, refused if too
 * few.  Arguments are checked before anything is enqueued (AURORA_E_ARG and aurora_hip_last_error()).  n_planes = 0 is a
 * no-op.  The inputs are not modified.  No host synchronisation, no allocation, no environment variable: capturable in a
 * hipGraph. */
size_t aurora_hip_smooth_workspace_bytes(int n_planes, int n_lat, int n_lon);
int aurora_hip_smooth(const float* const* planes, float* out, int n_planes, int n_lat, int n_lon, const int32_t* row_lo,
                      const int32_t* row_count, const int32_t* half, int max_rows, const double* w, int wrap,
                      double min_valid, int keep_mask, void* workspace, size_t workspace_size, void* stream);

/* ---- local extrema over a great-circle disc on the device (aurora_amd.extrema: where a point is the minimum or maximum of
 * all points within R km -- the candidates of cyclone detection and storm counts -- and the minimum / maximum filter itself;
 * not in the reference) ---------------------------------------------------------------------------------------------------------
 * Planes as above.  MEMBERSHIP is the table of aurora_hip_smooth (row_lo, row_count, half; max_rows <= 255) and nothing else:
 * the columns j - n .. j + n of source row k, around the circle with wrap = 1 (the whole row once 2 n + 1 >= n_lon) and
 * clipped into the row with wrap = 0; and the target point is always a member of its own disc: in its own row n counts as
 * max(n, 0).  A point is VALID where it is finite; NaN and +-Inf are never members and never extrema.
 * ORDER.  For the bits u of a valid value v, K = ~u where u has the sign bit, else u | 0x80000000 (ascending with v, -0 below
 * +0; the key of aurora_hip_objects); with is_max = 1 the key is ~K.  The COMPOSITE of a valid point is the uint64
 * (key << 32) | flat index, flat index = k n_lon + c.  The disc's extreme point is the MINIMUM composite over its valid
 * members: the extreme value and, among equal values, the smallest flat index.  A valid point is an EXTREMUM where that
 * minimum is its own composite.
 *   index     n_planes x n_lat x n_lon int32: the flat index of the disc's extreme point, -1 where the disc holds no valid point
 *   filtered  the same shape in fp32: the value at that index, bit for bit (NaN where index is -1)
 *   count     n_planes int32: the number of extrema of the plane, also above max_points
 *   table     n_planes x max_points x 2 int64: (flat index, K(v) widened -- K, not ~K, for either kind) of the extrema in
 *             ascending flat index; zero from row min(count, max_points) on
 * Everything is an integer or a copied fp32, so the outputs are repeatable bit for bit and depend on the plane's own values
 * and the table alone: not on the other planes, not on n_planes, not on pointer alignment (planes are read 4 bytes at a time).
 * Four launches on `stream`.  row extremes: a wavefront folds the composites of a row.  filter: a 256-thread workgroup owns 4
 * adjacent target rows and all columns; for every source row of their union, in ascending order, it stages the composites in
 * LDS and builds the doubling levels m[l + 1][c] = min(m[l][c], m[l][c + 2^l]) between two buffers (16 bytes per column of
 * LDS: 64 KiB at n_lon = 4096, the limit), answering a target row at the step l = floor(log2(2 n + 1)) with two LDS reads per
 * column (aurora_amd/csrc/extrema_window.h); a window that is the whole row reads the row's extreme instead.  scan: a
 * workgroup per plane turns the rows' numbers of extrema into row bases and `count` and zeroes the table's tail.  number: a
 * wavefront per row finds its extrema by ballot and writes their table rows.  No atomics; every trip count comes from the
 * tables and every table value is clamped into its row or plane before use.
 * `workspace`: aurora_hip_extrema_workspace_bytes(n_planes, n_lat, n_lon) = 16 n_planes n_lat device bytes -- per row of every
 * plane the extreme composite (uint64), the number of extrema and the base (int32 each); NOT plane-sized; 8-byte aligned, no
 * initialisation needed (0 for an argument out of range).  The outputs must not overlap an input plane, each other or the
 * workspace.  n_lon <= 4096, n_lat n_lon <= 2^31 - 1, 1 <= max_rows <= 255, 1 <= max_points <= 65536, wrap and is_max 0 or 1;
 * table 8-byte aligned, the other outputs and the disc table 4-byte aligned; workspace_size: the bytes at `workspace`, refused
 * if too few.  Arguments are checked before anything is enqueued (AURORA_E_ARG and aurora_hip_last_error()).  n_planes = 0 is
 * a no-op.  The inputs are not modified.  No host synchronisation, no allocation, no environment variable: capturable in a
 * hipGraph. */
size_t aurora_hip_extrema_workspace_bytes(int n_planes, int n_lat, int n_lon);
int aurora_hip_extrema(const float* const* planes, int32_t* index, float* filtered, int64_t* table, int32_t* count,
                       int n_planes, int n_lat, int n_lon, const int32_t* row_lo, const int32_t* row_count,
                       const int32_t* half, int max_rows, int wrap, int is_max, int max_points, void* workspace,
                       size_t workspace_size, void* stream);

/* ---- the closed-contour test of local extrema on the device (aurora_amd.closed_contours: does the field rise -- for maxima,
 * fall -- by at least delta on every path from a candidate to the rim of a disc of R km; the DetectNodes criterion that turns
 * the candidates of aurora_hip_extrema into storm counts; not in the reference) -------------------------------------------------
 * Planes as above.  THE RULE, per plane and per delta:
 *   CANDIDATE   row s < min(count, max_points) of the plane's extrema table: the flat index p0 = i0 n_lon + j0 (column 0 of the
 *               row; column 1 is not read) and the value v0 = x[p0].
 *   DOMAIN      the MEMBERS of the disc of row i0 around column j0 by the table of aurora_hip_smooth (row_lo, row_count, half;
 *               max_rows <= 255) and nothing else: the columns j0 - n .. j0 + n of source row k, around the circle with
 *               wrap = 1 (the whole row once 2 n + 1 >= n_lon), clipped into the row with wrap = 0; in row i0 n counts as
 *               max(n, 0), so p0 is always a member.
 *   PASSABLE    a point q is passable where x[q] is not finite, and where (double)x[q] - (double)v0 < (double)delta (is_max = 1:
 *               (double)v0 - (double)x[q] < (double)delta): one fp64 subtraction and one comparison.  A non-finite point can
 *               never hold a contour.
 *   NEIGHBOURS  those of aurora_hip_objects: 4 (rows and columns) or 8 (diagonals too); none across rows 0 and n_lat - 1; with
 *               wrap = 1 column n_lon - 1 joins column 0.
 *   FILL        F is the smallest set that holds p0 and every passable member adjacent to a point of F.
 *   EXIT        a point of F is an exit where a neighbour of it is passable and not a member, and, with wrap = 0 (a regional
 *               grid: every edge is open), where it lies in row 0, row n_lat - 1, column 0 or column n_lon - 1.  With wrap = 1
 *               the first and the last row are walls.
 *   RESULT      out: n_planes x n_deltas x max_points x 2 int32: (points = |F|, exits = the number of exits); zero from row
 *               min(count, max_points) on, and for a delta that is NaN (padding).  The contour is CLOSED where the row is live
 *               and exits = 0.  Everything is an integer, so the output is repeatable bit for bit and depends on the plane's own
 *               values and tables alone: not on the other planes, not on n_planes, not on pointer alignment (planes are read 4
 *               bytes at a time).
 * One launch on `stream`: a 256-thread workgroup per (plane, table row); one past min(count, max_points) stores its zero rows
 * and exits.  The others lay out the candidate's WINDOW (aurora_amd/csrc/contour_fill.h) -- the source rows and columns of the
 * disc and one ring of each around them -- as rows of 64-bit words in LDS and, per delta, build three bitmaps by ballot
 * (passable member A, passable non-member X, reached R = the bit of p0), repeat R |= A & dilate(R) with a whole-run horizontal
 * shortcut until a sweep changes nothing (at most |members| + 1 sweeps), and count points = popcount(R) and exits =
 * popcount(R & (dilate(X) | edge)).  No atomics on global memory, no workspace, no workgroup waits for another; every trip count
 * comes from the tables and every table value is clamped into its row or plane before use.
 * LDS: the caller announces the largest window as max_rows source rows and max_words words of 64 local columns per row -- on a
 * full circle n_lon columns where a disc row is the whole row, else 2 n + 3, on a regional grid at most n_lon + 2 -- and the
 * three bitmaps take 24 (max_rows + 2) max_words bytes, at most 159744 (156 KiB of the CU's 160 KiB); more is refused here,
 * before any launch.  A candidate whose window has more words than max_words is not filled (zero rows).
 * n_lon <= 4096, n_lat n_lon <= 2^31 - 1, 1 <= n_deltas <= 8, 1 <= max_points <= 65536, 1 <= max_rows <= 255, 1 <= max_words <=
 * 65, wrap and is_max 0 or 1, connectivity 4 or 8; table 8-byte aligned, the others 4-byte aligned; out must not overlap an
 * input.  Arguments are checked before anything is enqueued (AURORA_E_ARG and aurora_hip_last_error()).  n_planes = 0 is a
 * no-op.  The inputs are not modified.  No host synchronisation, no allocation, no environment variable: capturable in a
 * hipGraph (after one eager call on the device, which raises the kernel's dynamic LDS limit). */
int aurora_hip_closed_contours(const float* const* planes, const int64_t* table, const int32_t* count, const float* delta,
                               int32_t* out, int n_planes, int n_lat, int n_lon, int n_deltas, int max_points,
                               const int32_t* row_lo, const int32_t* row_count, const int32_t* half, int max_rows, int max_words,
                               int wrap, int is_max, int connectivity, void* stream);

/* ---- linking the extrema of two steps on the device (aurora_amd.link_extrema: for every candidate of step t the nearest
 * candidate of step t + 1 within max_km and the reverse, the all-pairs search under the StitchNodes half of DetectNodes /
 * StitchNodes; not in the reference) ---------------------------------------------------------------------------------------------
 * table_a: n_planes x max_points_a x 2 int64 and count_a: n_planes int32 as written by aurora_hip_extrema (column 0, the flat
 * index i n_lon + j, is read; column 1 is not); keep_a: n_planes x max_points_a bytes, non-zero = keep the row, or NULL = keep
 * every row; the same for b, whose max_points may differ.  tables: 2 n_lat + n_lon fp64, the tables of aurora_hip_nearest_event:
 * s[i] = sin(lat_i), c[i] = max(cos(lat_i), 0), cd[d] = cos(d dlon).  THE RULE (aurora_amd/links.py states it), per plane:
 *   LIVE       row r of a side is live where r < min(count, max_points) (a count below 0 counts as 0) and its keep byte is set.
 *   POINT      (i, j) = divmod(flat index, n_lon); the flat index is clamped into 0 .. n_lat n_lon - 1 before it addresses a table.
 *   KEY        0 exactly for two rows with the same flat index; otherwise 1 - (s_i s_k + (c_i c_k) cd[gap]) with gap = |j - j'|,
 *              with wrap = 1 min(gap, n_lon - gap): every fp64 operation rounded on its own, never a fused multiply-add, negative
 *              results 0 -- the key of aurora_hip_nearest_event, symmetric in its two points bit for bit.
 *   SEARCH     forward[p] = the live row q of b with the smallest (key, q) among keys <= key_max; backward[q] = the live row p of
 *              a with the smallest (key, p).
 *   RESULT     forward: n_planes x max_points_a x 2 int64 and backward: n_planes x max_points_b x 2 int64 -- the bits of the fp64
 *              key, the partner's row; the bits of +inf and -1 for a row that is not live or has no partner in reach.  Every
 *              row of both is written.  The result is repeatable bit for bit and depends on the plane's own tables alone.
 * One launch on `stream`: a 256-thread workgroup per (chunk of 256 rows, plane, direction); a thread owns one row and scans the
 * other side, staged through LDS in tiles of 1024 gathered rows, with cd in LDS (8 n_lon + 24576 bytes in all); the scan covers
 * min(count, max_points) rows of the other side, and a workgroup past the rows of its own side stores "none" and exits.  No
 * atomics, no workspace, no reduction across threads, plain vector stores.
 * n_lon <= 4096, n_lat n_lon <= 2^31 - 1, 1 <= max_points <= 65536, wrap 0 or 1, key_max >= 0 (+inf: no limit; a HOST number);
 * tables and outputs 8-byte aligned, counts 4-byte aligned; forward and backward must not overlap each other or an input.
 * Arguments are checked before anything is enqueued (AURORA_E_ARG and aurora_hip_last_error()).  n_planes = 0 is a no-op.  The
 * inputs are not modified.  No host synchronisation, no allocation, no environment variable: capturable in a hipGraph. */
int aurora_hip_link_extrema(const int64_t* table_a, const int32_t* count_a, const uint8_t* keep_a, int max_points_a,
                            const int64_t* table_b, const int32_t* count_b, const uint8_t* keep_b, int max_points_b,
                            int n_planes, const double* tables, int n_lat, int n_lon, int wrap, double key_max,
                            int64_t* forward, int64_t* backward, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AURORA_HIP_H */
