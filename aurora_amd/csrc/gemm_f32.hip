// fp32 linear layers on the bf16 / fp16 matrix pipe by operand splitting (dispatch: linear_impl of gemm.hip, through
// aurora_f32_launch at the end of this file):
//   linear_kernel_256_f32x3<3>  fp32 by three bf16 terms (6 MFMAs)   -- fp32 linears, any input range
//   linear_kernel_256_f32x3<2>  fp32 by two fp16 terms (3 MFMAs)     -- fp32 linears with inputs bounded by construction
//   linear_kernel_f32pp         two fp16 terms, ping-pong schedule   -- the same when K % 32 == 0, K >= 96; pre-split operands
//   split_f16_kernel            fp32 rows -> the fp16-pair layout (aurora_hip_split_f16)
#include "gemm_tile.h"

#ifndef F32PP_PARTS   // passes of the two-term fp32 kernel's whole-row epilogue (1, 2 or 4): see linear_kernel_f32pp
#define F32PP_PARTS 4
#endif

namespace aurora {

namespace {

// =================================================================================================
// fp32 linear layers on the bf16 matrix pipe: "3 x bf16" operand splitting.
//
// gfx950 multiplies bf16 sixteen times faster than fp32 on the matrix cores (v_mfma_f32_16x16x32_bf16:
// 16 Ki FLOP in 16 cycles; v_mfma_f32_16x16x4_f32: 2 Ki FLOP in 32 cycles).  An fp32 number is EXACTLY the
// sum of three bf16 numbers (8 + 8 + 8 significand bits, by truncation): a = a_h + a_m + a_l.  Then
//     a.b = a_h b_h + (a_h b_m + a_m b_h) + (a_h b_l + a_l b_h + a_m b_m) + O(2^-24 |a||b|)
// and every bf16 x bf16 product is exact in the fp32 accumulator, so six bf16 MFMAs reproduce the fp32
// product to ~1.2e-7 relative (the three dropped terms), the same order as the 2^-24 rounding an fp32 FMA
// chain commits per step: an fp32-grade GEMM at 16/6 = 2.7x the fp32 MFMA rate.  (The encoder and decoder of
// Aurora are fp32 upstream, outside autocast; this keeps them fp32-accurate.  tests/test_gpu_ops.py measures
// both this kernel and the native-fp32 one against an fp64 product.)
//
// Same 256 x 256 tile, LDS-DMA staging, swizzles and epilogue as linear_kernel_256<float>; a K-stage is 16
// fp32 per row, so two stages (a "pair") make the K = 32 of one bf16 MFMA: lane (row, g) holds fp32
// k = 4g..4g+3 of both stages, which become its 8 bf16 k-slots (the k order is free as long as both operands
// agree).  Splitting is done on the fragments in registers: ~36 VALU ops per 8-value fragment, 12 fragments
// per pair and wave against 192 MFMAs (3072 matrix-pipe cycles), so the VALU work hides under the MFMAs.
// Ring: pair j is consumed while pair j+1 (64 KiB) is in flight; one barrier per pair.
// =================================================================================================
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

struct Split3 { u32x4 h, m, l; };

__device__ __forceinline__ void split_pair(uint32_t a0, uint32_t a1, uint32_t& h, uint32_t& m, uint32_t& l) {
  // top 16 bits of two fp32 -> one packed bf16x2 word (truncation), remainder exact in fp32
  constexpr uint32_t SEL = 0x07060302u;
  h = __builtin_amdgcn_perm(a1, a0, SEL);
  const float r0 = __uint_as_float(a0) - __uint_as_float(a0 & 0xffff0000u);
  const float r1 = __uint_as_float(a1) - __uint_as_float(a1 & 0xffff0000u);
  const uint32_t q0 = __float_as_uint(r0), q1 = __float_as_uint(r1);
  m = __builtin_amdgcn_perm(q1, q0, SEL);
  const float s0 = r0 - __uint_as_float(q0 & 0xffff0000u);
  const float s1 = r1 - __uint_as_float(q1 & 0xffff0000u);
  l = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), SEL);
}

__device__ __forceinline__ Split3 split8(u32x4 a, u32x4 b) {
  uint32_t h[4], m[4], l[4];
  split_pair(a.x, a.y, h[0], m[0], l[0]);
  split_pair(a.z, a.w, h[1], m[1], l[1]);
  split_pair(b.x, b.y, h[2], m[2], l[2]);
  split_pair(b.z, b.w, h[3], m[3], l[3]);
  return Split3{u32x4{h[0], h[1], h[2], h[3]}, u32x4{m[0], m[1], m[2], m[3]}, u32x4{l[0], l[1], l[2], l[3]}};
}

__device__ __forceinline__ f32x4 mma_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                 c, 0, 0, 0);
}

// ---- second variant: two fp16 terms ----
// With round-to-nearest, a = a_h + a_l where a_h = fp16(a) and a_l = fp16(a - a_h) reproduces a to 2^-24 |a| (the
// remainder is exact in fp32, has <= 14 significant bits and loses at most its last three to the 11-bit fp16
// significand), so  a.b = a_h b_h + a_h b_l + a_l b_h + O(2^-24 |a||b|)  needs THREE MFMAs (fp16 x fp16 products are
// exact in the fp32 accumulator) and 5 VALU operations per operand pair instead of six MFMAs and 9.  The price is
// fp16's range: a_h overflows at |a| >= 65520, and a_l is a subnormal for |a| < 0.25, i.e. carries an ABSOLUTE error
// of up to 3e-8.  The weight operand is therefore scaled by 2^6 on the fly (nn.Linear weights are O(1e-2); the
// accumulators are scaled back exactly in the epilogue) and the variant is only used where the caller vouches for
// activations that are bounded by construction (f32_gemm = 2 of aurora_hip_linear_ex: LayerNorm outputs and their GELU'd linears).
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
struct Split2 { u32x4 h, l; };

template <bool SCALE>
__device__ __forceinline__ Split2 split8_f16(u32x4 a, u32x4 b) {
  constexpr float S = SCALE ? 64.0f : 1.0f;
  uint32_t h[4], l[4];
  split_pair_f16(__uint_as_float(a.x) * S, __uint_as_float(a.y) * S, h[0], l[0]);
  split_pair_f16(__uint_as_float(a.z) * S, __uint_as_float(a.w) * S, h[1], l[1]);
  split_pair_f16(__uint_as_float(b.x) * S, __uint_as_float(b.y) * S, h[2], l[2]);
  split_pair_f16(__uint_as_float(b.z) * S, __uint_as_float(b.w) * S, h[3], l[3]);
  return Split2{u32x4{h[0], h[1], h[2], h[3]}, u32x4{l[0], l[1], l[2], l[3]}};
}
__device__ __forceinline__ f32x4 mma_f16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}

template <int TERMS>   // 3: three bf16 terms, six MFMAs;  2: two fp16 terms, three MFMAs
__global__ __launch_bounds__(THREADS2, 2) void linear_kernel_256_f32x3(const LinearArgs p_in) {
  const LinearArgs p = batch_problem(p_in);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // Guarded launch: the host has launched BOTH variants; the word the caller left in device memory (max |activation|
  // or a bound of it) decides which one does the work -- two fp16 terms inside the safe range, three bf16 terms
  // otherwise -- and the other one retires at once.  Uniform: every workgroup reads the same word.
  if (p.guard != nullptr && (*p.guard < p.guard_limit) != (TERMS == 2)) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;

  uint32_t tile_m, tile_n;
  tile_of_block(blockIdx.x, (uint32_t)p.n_blocks, (uint32_t)(p.n_blocks / p.tiles_n), (uint32_t)p.tiles_n, tile_m, tile_n);
  const int64_t m0 = (int64_t)tile_m * BM2;
  const int n0 = (int)tile_n * BN2;

  const char* src_x[2];
  const char* src_w[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int id = r * THREADS2 + tid;
    const int row = id >> 2, c = id & 3;
    int64_t gm = m0 + row;
    gm = gm < p.M ? gm : p.M - 1;
    int gn = n0 + row;
    gn = gn < p.N ? gn : p.N - 1;
    src_x[r] = p.A + gm * p.lda_b + piece_x(row, c);
    src_w[r] = p.W + (int64_t)gn * p.ldw_b + piece_w(row, c);
  }
  auto stage = [&](int kt) {
    const int64_t koff = (int64_t)kt * ROW2;
    char* base = smem + (kt & (NSTAGE2 - 1)) * STAGE2;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int off = (r * THREADS2 + wave * 64) * 16;
      dma16(src_x[r] + koff, base + off);
      dma16(src_w[r] + koff, base + OPER2 + off);
    }
  };

  const int i16 = lane & 15, g = lane >> 4;
  int off_x[8], off_w[4];
#pragma unroll
  for (int f = 0; f < 8; ++f) {
    const int row = wm * 128 + 16 * f + i16;
    off_x[f] = row * ROW2 + piece_x(row, g);
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int row = wn * 64 + 16 * (i16 >> 2) + 4 * f + (i16 & 3);
    off_w[f] = OPER2 + row * ROW2 + piece_w(row, g);
  }

  f32x4 acc[4][8];  // [fn][fm]  (zeroed in place, not by zero_acc: the helper changes the code of the three-term form)
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int np = p.k_tiles >> 1;  // pairs of stages (k_tiles is even)
  stage(0);
  stage(1);
  if (np > 1) {
    stage(2);
    stage(3);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  constexpr bool use_two = TERMS == 2;
  auto pair3 = [&](const char* bufa, const char* bufb) {
      Split3 w[4];
#pragma unroll
      for (int f = 0; f < 4; ++f)
        w[f] = split8(*reinterpret_cast<const u32x4*>(bufa + off_w[f]), *reinterpret_cast<const u32x4*>(bufb + off_w[f]));
      u32x4 ra = *reinterpret_cast<const u32x4*>(bufa + off_x[0]);
      u32x4 rb = *reinterpret_cast<const u32x4*>(bufb + off_x[0]);
#pragma unroll
      for (int fm = 0; fm < 8; ++fm) {
        const Split3 x = split8(ra, rb);
        if (fm + 1 < 8) {
          ra = *reinterpret_cast<const u32x4*>(bufa + off_x[fm + 1]);
          rb = *reinterpret_cast<const u32x4*>(bufb + off_x[fm + 1]);
        }
        // smallest terms first; consecutive MFMAs go to different accumulators
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_bf16(w[fn].l, x.h, acc[fn][fm]);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_bf16(w[fn].h, x.l, acc[fn][fm]);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_bf16(w[fn].m, x.m, acc[fn][fm]);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_bf16(w[fn].m, x.h, acc[fn][fm]);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_bf16(w[fn].h, x.m, acc[fn][fm]);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_bf16(w[fn].h, x.h, acc[fn][fm]);
      }
  };
  auto pair2 = [&](const char* bufa, const char* bufb) {
      Split2 w[4];
#pragma unroll
      for (int f = 0; f < 4; ++f)
        w[f] = split8_f16<true>(*reinterpret_cast<const u32x4*>(bufa + off_w[f]),
                                *reinterpret_cast<const u32x4*>(bufb + off_w[f]));
      u32x4 ra = *reinterpret_cast<const u32x4*>(bufa + off_x[0]);
      u32x4 rb = *reinterpret_cast<const u32x4*>(bufb + off_x[0]);
#pragma unroll
      for (int fm = 0; fm < 8; ++fm) {
        const Split2 x = split8_f16<false>(ra, rb);
        if (fm + 1 < 8) {
          ra = *reinterpret_cast<const u32x4*>(bufa + off_x[fm + 1]);
          rb = *reinterpret_cast<const u32x4*>(bufb + off_x[fm + 1]);
        }
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_f16(w[fn].l, x.h, acc[fn][fm]);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_f16(w[fn].h, x.l, acc[fn][fm]);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_f16(w[fn].h, x.h, acc[fn][fm]);
      }
  };
  for (int j = 0; j < np; ++j) {
    const char* bufa = smem + ((2 * j) & (NSTAGE2 - 1)) * STAGE2;
    const char* bufb = smem + ((2 * j + 1) & (NSTAGE2 - 1)) * STAGE2;
    if constexpr (TERMS == 3) pair3(bufa, bufb);
    else pair2(bufa, bufb);
    if (j + 1 < np) {
      // RAW: my pieces of pair j+1 (issued a whole pair ago) have landed; WAR: everyone has read pair j.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (j + 2 < np) {
        stage(2 * j + 4);
        stage(2 * j + 5);
      }
    }
  }
  if constexpr (use_two) {   // undo the 2^6 weight scale (exact)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 8; ++b) acc[a][b] *= 0.015625f;
  }
  if (p.C2 == nullptr && p.vec_store) {   // (uniform)
    __syncthreads();   // every wave is done with the ring
    epilogue_256_f32_coalesced(p, acc, m0, n0, wm, wn, wave, lane, smem);
    return;
  }
  epilogue_256<float>(p, acc, m0, n0, wm, wn, i16, g);
}


// =================================================================================================
// fp32 linears by two fp16 terms, ping-pong form: 128 x 256 tile, whole-line K-stages, three-stage ring.
//
// linear_kernel_256_f32x3<2> above runs all eight waves in phase through "read fragments, split, 96 MFMAs" with one
// barrier and a full drain (vmcnt(0)) per K = 32: the two waves of a SIMD fight over its matrix pipe and its VALU issue
// (the split costs ~240 VALU instructions per wave and K = 32 against 96 MFMAs), and the kernel sits at 290 TFLOP/s
// fp32-equivalent = 0.87 PFLOP/s of fp16 MFMA work where the bf16 kernels reach 1.15-1.4.  The ping-pong schedule of
// linear_kernel_256pp needs every LDS read of a stage inside the LOAD phase (the partner's DMA refills the ring during
// the MATRIX phase) and a ring at least three K-steps deep; fp32 operands of a 256 x 256 tile are 64 KiB per K = 32,
// i.e. two steps.  Hence this geometry:
//   * tile 128 x 256, 8 waves as 2 (m) x 4 (n), wave tile 64 x 64 = 4 x 4 fragments (64 accumulator registers);
//   * a K-stage is 128 BYTES of every operand row (32 fp32 = one fp16 MFMA of K = 32): 16 KiB of activations + 32 KiB of
//     weights, staged by LDS-DMA in whole cache lines (8 rows x 128 B per wave instruction -- the pattern the vector
//     memory front end moves 4x faster than 16 rows x 64 B), XOR-swizzled as in the 128 x 128 kernel; 3 stages = 144 KiB;
//   * L(s): 16 fragment reads (raw fp32: 32 registers of activations; the weights are split to fp16 pairs at once),
//     DMA of stage s+2, counted wait for the wave's pieces of stage s+1;  M(s): per activation fragment one split
//     (20 VALU) + 12 MFMAs, the VALU work overlapping the wave's own matrix instructions;
//   * waves 4-7 run one phase behind waves 0-3 (one extra barrier in front, one behind for the others): a SIMD's matrix
//     pipe always belongs to exactly one wave.
// Same range contract and guard as the kernel above (which remains the fallback for K % 32 != 0).
// =================================================================================================
constexpr int VROW = 128, VTHREADS = 512, VNST = 3;
constexpr int VOPER_X = VM * VROW, VOPER_W = VN * VROW, VSTAGE = VOPER_X + VOPER_W;   // 16 + 32 = 48 KiB

// A_PRE / W_PRE: operand already in the fp16-pair layout: its split (all of its VALU work) disappears.
// TALL: the tile is 256 (m) x 128 (n) -- waves 4 x 2, the same 64 x 64 wave tile, the same 48 KiB stage (32 KiB of
// activations + 16 KiB of weights) and the same six LDS-DMA instructions per lane and stage -- for the narrow linears: the
// decoder's output heads have 80 real columns (5 variables x 16 pixels), which the 256-wide tile pads to 256 (69 % of
// its MFMAs on zeros), this one to 128.
template <bool A_PRE, bool W_PRE, bool TALL = false>
__global__ __launch_bounds__(VTHREADS, 2) void linear_kernel_f32pp(const LinearArgs p_in) {
  constexpr int TM = TALL ? 256 : VM, TN = TALL ? 128 : VN, OPX = TM * VROW, XP = TM / 64, WP = TN / 64;
  static_assert(OPX + TN * VROW == VSTAGE && XP + WP == 6, "stage size / DMA count the waitcnt immediates assume");
  const LinearArgs p = batch_problem(p_in);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (p.guard != nullptr && !(*p.guard < p.guard_limit)) return;   // guarded launch: the three-term kernel does the work
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int late = wave >> 2;   // waves w and w+4 share a SIMD; the late half runs one phase behind
  const int wm = TALL ? wave >> 1 : wave >> 2, wn = TALL ? wave & 1 : wave & 3;

  uint32_t tile_m, tile_n;
  tile_of_block<2>(blockIdx.x, (uint32_t)p.n_blocks, (uint32_t)(p.n_blocks / p.tiles_n), (uint32_t)p.tiles_n, tile_m, tile_n);
  const int64_t m0 = (int64_t)tile_m * TM;
  const int n0 = (int)tile_n * TN;

  const char* src_x[XP];
  const char* src_w[WP];
#pragma unroll
  for (int r = 0; r < XP; ++r) {
    const int id = r * VTHREADS + tid;
    const int row = id >> 3, c = id & 7;
    int64_t gm = m0 + row;
    gm = gm < p.M ? gm : p.M - 1;
    src_x[r] = p.A + gm * p.lda_b + ((c ^ swz_x(row)) << 4);
  }
#pragma unroll
  for (int r = 0; r < WP; ++r) {
    const int id = r * VTHREADS + tid;
    const int row = id >> 3, c = id & 7;
    src_w[r] = p.W + (int64_t)(n0 + row) * p.ldw_b + ((c ^ swz_w(row)) << 4);
  }
  auto stage = [&](int kt) {
    const int64_t koff = (int64_t)kt * VROW;
    char* base = smem + (kt % VNST) * VSTAGE;
#pragma unroll
    for (int r = 0; r < XP; ++r)   // wave-uniform LDS address; the hardware adds lane * 16
      dma16(src_x[r] + koff, base + (r * VTHREADS + wave * 64) * 16);
#pragma unroll
    for (int r = 0; r < WP; ++r)
      dma16(src_w[r] + koff, base + OPX + (r * VTHREADS + wave * 64) * 16);
  };
  // fragment read offsets.  Lane group g multiplies k = 8g..8g+7 of the stage: as fp32 that is chunks 2g and 2g + 1 of the
  // row, in the fp16-pair layout chunk g (high halves) and chunk g + 4 (remainders) -- the same k order either way, so
  // an operand may arrive split or not without changing a bit of the result.
  const int i16 = lane & 15, g = lane >> 4;
  int off_x[4][2], off_w[4][2];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int row_x = wm * 64 + 16 * f + i16;
    const int row_w = wn * 64 + 16 * (i16 >> 2) + 4 * f + (i16 & 3);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int cx = A_PRE ? g + 4 * ks : 2 * g + ks, cw = W_PRE ? g + 4 * ks : 2 * g + ks;
      off_x[f][ks] = row_x * VROW + ((cx ^ swz_x(row_x)) << 4);
      off_w[f][ks] = OPX + row_w * VROW + ((cw ^ swz_w(row_w)) << 4);
    }
  }
  f32x4 acc[4][4];  // [fn][fm]
  zero_acc(acc);

  const int nt = p.k_tiles;   // K / 32, >= 3 (dispatch)
  stage(0);
  stage(1);
  stage(2);
  asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  __builtin_amdgcn_s_barrier();   // stage 0 is complete
  asm volatile("" ::: "memory");
  if (late == 1) __builtin_amdgcn_s_barrier();   // the late half: one phase behind from here on

  for (int s = 0; s < nt; ++s) {
    // ---- L(s) ----
    const char* buf = smem + (s % VNST) * VSTAGE;
    u32x4 xa[4], xb[4];
    Split2 w[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      xa[f] = *reinterpret_cast<const u32x4*>(buf + off_x[f][0]);
      xb[f] = *reinterpret_cast<const u32x4*>(buf + off_x[f][1]);
    }
#pragma unroll
    for (int f = 0; f < 4; ++f)
      if constexpr (W_PRE)   // chunk g = high halves of k = 8g..8g+7, chunk g + 4 = their remainders
        w[f] = Split2{*reinterpret_cast<const u32x4*>(buf + off_w[f][0]), *reinterpret_cast<const u32x4*>(buf + off_w[f][1])};
      else
        w[f] = split8_f16<true>(*reinterpret_cast<const u32x4*>(buf + off_w[f][0]), *reinterpret_cast<const u32x4*>(buf + off_w[f][1]));
    if (s >= 1 && s + 2 < nt) stage(s + 2);   // into the buffer of stage s-1
    if (s + 2 < nt) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");   // own pieces of stage s+1 have landed
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    // ---- M(s): smallest terms first; consecutive MFMAs go to different accumulators ----
#pragma unroll
    for (int fm = 0; fm < 4; ++fm) {
      Split2 x;
      if constexpr (A_PRE) x = Split2{xa[fm], xb[fm]};
      else x = split8_f16<false>(xa[fm], xb[fm]);
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_f16(w[fn].l, x.h, acc[fn][fm]);
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_f16(w[fn].h, x.l, acc[fn][fm]);
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = mma_f16(w[fn].h, x.h, acc[fn][fm]);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
  }
  if (late == 0) __builtin_amdgcn_s_barrier();   // the early half waits for the late half's last phase
  asm volatile("" ::: "memory");

  // ---- epilogue: lane owns row m (per fm) x 16 consecutive features; undo the 2^6 weight scale (exact) ----
  const int nbase = n0 + wn * 64 + 16 * g;
  float bias_v[16];   // (requested before the main loop instead, as in linear_kernel_256pp: measured, no gain here -- the tiles are long)
#pragma unroll
  for (int t = 0; t < 16; ++t) bias_v[t] = p.bias ? p.bias[nbase + t] : 0.f;
  const bool vec = p.vec_store != 0;
  if (vec && p.C2 == nullptr && p.res == nullptr) {   // (uniform)
    // Plain result (fp32 or fp16 pairs): through LDS, so that a store instruction writes four whole 256-byte row
    // segments with consecutive lanes on consecutive 16-byte pieces.  The direct form below has lane (i16, g) write 16
    // bytes of row i16 at a 64-byte stride -- every instruction touches 32 cache lines, 32 bytes each, and the CU's
    // store path takes as long over a tile's 128 KiB as 6-8 K-stages of MFMAs.  The ring is dead after the main loop;
    // each wave takes 16 KiB of it for its 64 x 64 results, stored as the exact bytes of the output rows (the pair
    // layout keeps a wave's 64 features in 256 contiguous bytes too: two groups of 32 high halves + 32 remainders),
    // 16-byte pieces XOR-swizzled by row & 7.
    // (both halves are past their last LDS read: the barrier above is the late half's last in-loop one)
    // In F32PP_PARTS parts (32 / 16 of the wave's 64 rows at a time): a part's stores are in flight while the next part's
    // scaling, activation and splitting run on the VALU (as epilogue_256_bf16_coalesced; profiles/r06_ab_epilogue_parts.log).
    char* mine = smem + wave * 16384;
    const int rr = lane >> 4, cc = lane & 15;
    float* cbase = reinterpret_cast<float*>(p.C) + n0 + wn * 64 + cc * 4;
#pragma unroll
    for (int part = 0; part < F32PP_PARTS; ++part) {
#pragma unroll
    for (int fm = part * (4 / F32PP_PARTS); fm < (part + 1) * (4 / F32PP_PARTS); ++fm) {
      float v[16];
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) {
        v[4 * fn + 0] = fmaf(acc[fn][fm].x, 0.015625f, bias_v[4 * fn + 0]);
        v[4 * fn + 1] = fmaf(acc[fn][fm].y, 0.015625f, bias_v[4 * fn + 1]);
        v[4 * fn + 2] = fmaf(acc[fn][fm].z, 0.015625f, bias_v[4 * fn + 2]);
        v[4 * fn + 3] = fmaf(acc[fn][fm].w, 0.015625f, bias_v[4 * fn + 3]);
      }
      if (p.act == AURORA_ACT_GELU || p.act == ACT_GELU_FAST) gelu_fast16x2(v);
      else if (p.act == AURORA_ACT_SILU) silu16(v);
      const int row = 16 * fm + i16, sw = row & 7;
      char* lrow = mine + row * 256;
      if (p.out_split) {
        uint32_t h[8], l[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) split_pair_f16(v[2 * t], v[2 * t + 1], h[t], l[t]);
        // features 16g..16g+15 = halves 16 (g & 1).. of group g >> 1: pieces 8 (g >> 1) + 2 (g & 1) + {0, 1}, remainders + 4
        const int pc = 8 * (g >> 1) + 2 * (g & 1);
        *reinterpret_cast<u32x4*>(lrow + (((pc + 0) ^ sw) << 4)) = u32x4{h[0], h[1], h[2], h[3]};
        *reinterpret_cast<u32x4*>(lrow + (((pc + 1) ^ sw) << 4)) = u32x4{h[4], h[5], h[6], h[7]};
        *reinterpret_cast<u32x4*>(lrow + (((pc + 4) ^ sw) << 4)) = u32x4{l[0], l[1], l[2], l[3]};
        *reinterpret_cast<u32x4*>(lrow + (((pc + 5) ^ sw) << 4)) = u32x4{l[4], l[5], l[6], l[7]};
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<f32x4*>(lrow + (((4 * g + q) ^ sw) << 4)) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
      }
    }
#pragma unroll
    for (int it = part * (16 / F32PP_PARTS); it < (part + 1) * (16 / F32PP_PARTS); ++it) {
      const int row = it * 4 + rr;
      const f32x4 d = *reinterpret_cast<const f32x4*>(mine + row * 256 + ((cc ^ (row & 7)) << 4));
      const int64_t m = m0 + wm * 64 + row;
      if (m < p.M) *reinterpret_cast<f32x4*>(cbase + m * p.ldc) = d;
    }
    }
    return;
  }
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    const int64_t m = m0 + wm * 64 + 16 * fm + i16;
    if (m >= p.M) continue;
    float v[16];
#pragma unroll
    for (int fn = 0; fn < 4; ++fn) {
      v[4 * fn + 0] = fmaf(acc[fn][fm].x, 0.015625f, bias_v[4 * fn + 0]);
      v[4 * fn + 1] = fmaf(acc[fn][fm].y, 0.015625f, bias_v[4 * fn + 1]);
      v[4 * fn + 2] = fmaf(acc[fn][fm].z, 0.015625f, bias_v[4 * fn + 2]);
      v[4 * fn + 3] = fmaf(acc[fn][fm].w, 0.015625f, bias_v[4 * fn + 3]);
    }
    if (p.act == AURORA_ACT_GELU || p.act == ACT_GELU_FAST) gelu_fast16x2(v);
    else if (p.act == AURORA_ACT_SILU) silu16(v);
    if (p.res) {
      const float* rp = p.res + m * p.ldr + nbase;
      if (vec) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 rv = reinterpret_cast<const f32x4*>(rp)[q];
          v[4 * q] += rv.x; v[4 * q + 1] += rv.y; v[4 * q + 2] += rv.z; v[4 * q + 3] += rv.w;
        }
      } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) v[t] += rp[t];
      }
    }
    if (p.out_split) {
      // fp16-pair layout: the 16 features nbase.. are halves (nbase % 32) .. +15 of group nbase / 32 -- 32 bytes of high
      // halves, and 32 bytes of remainders 64 bytes further on
      uint32_t h[8], l[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) split_pair_f16(v[2 * t], v[2 * t + 1], h[t], l[t]);
      char* dst = p.C + (m * p.ldc + (nbase & ~31)) * 4 + (nbase & 31) * 2;
      reinterpret_cast<u32x4*>(dst)[0] = u32x4{h[0], h[1], h[2], h[3]};
      reinterpret_cast<u32x4*>(dst)[1] = u32x4{h[4], h[5], h[6], h[7]};
      reinterpret_cast<u32x4*>(dst + 64)[0] = u32x4{l[0], l[1], l[2], l[3]};
      reinterpret_cast<u32x4*>(dst + 64)[1] = u32x4{l[4], l[5], l[6], l[7]};
      continue;
    }
    store16<float>(reinterpret_cast<float*>(p.C) + m * p.ldc + nbase, v, vec, 16);
    if (p.C2) store16<bf16_t>(reinterpret_cast<bf16_t*>(p.C2) + m * p.ldc2 + nbase, v, vec, 16);
  }
}

// fp32 rows -> the fp16-pair layout the two-term kernels can take directly: per 32 features 128 bytes, the 32 fp16 high
// halves  h = fp16(s x)  followed by the 32 remainders  l = fp16(s x - h).  One lane per 8 features.
__global__ __launch_bounds__(256) void split_f16_kernel(const float* __restrict__ src, int64_t ld_src, char* __restrict__ dst,
                                                        int64_t ld_dst, int64_t rows, int K, float scale) {
  const int per_row = K >> 3;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= rows * per_row) return;
  const int64_t r = id / per_row;
  const int c = (int)(id - r * per_row) * 8;
  const f32x4 a = *reinterpret_cast<const f32x4*>(src + r * ld_src + c);
  const f32x4 b = *reinterpret_cast<const f32x4*>(src + r * ld_src + c + 4);
  uint32_t h[4], l[4];
  split_pair_f16(a.x * scale, a.y * scale, h[0], l[0]);
  split_pair_f16(a.z * scale, a.w * scale, h[1], l[1]);
  split_pair_f16(b.x * scale, b.y * scale, h[2], l[2]);
  split_pair_f16(b.z * scale, b.w * scale, h[3], l[3]);
  char* d = dst + (r * ld_dst + (c & ~31)) * 4 + (c & 31) * 2;
  *reinterpret_cast<u32x4*>(d) = u32x4{h[0], h[1], h[2], h[3]};
  *reinterpret_cast<u32x4*>(d + 64) = u32x4{l[0], l[1], l[2], l[3]};
}

}  // namespace

}  // namespace aurora

using namespace aurora;

namespace {
// This file's GEMM kernels by F32Kernel id.
constexpr LinearKernel F32_TABLE[F32_KERNELS] = {
    /* F32_THREE      */ {linear_kernel_256_f32x3<3>, THREADS2, NSTAGE2 * STAGE2},
    /* F32_TWO        */ {linear_kernel_256_f32x3<2>, THREADS2, NSTAGE2 * STAGE2},
    /* F32_PP         */ {linear_kernel_f32pp<false, false>, VTHREADS, VNST * VSTAGE},
    /* F32_PP_W       */ {linear_kernel_f32pp<false, true>, VTHREADS, VNST * VSTAGE},
    /* F32_PP_AW      */ {linear_kernel_f32pp<true, true>, VTHREADS, VNST * VSTAGE},
    /* F32_PP_W_TALL  */ {linear_kernel_f32pp<false, true, true>, VTHREADS, VNST * VSTAGE},
    /* F32_PP_AW_TALL */ {linear_kernel_f32pp<true, true, true>, VTHREADS, VNST * VSTAGE},
};
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int aurora_f32_launch(int kernel, const void* linear_args, unsigned n_blocks,
                                                                      unsigned batch, void* stream) {
  const LinearArgs& p = *static_cast<const LinearArgs*>(linear_args);
  AURORA_CHECK_ARG(kernel >= 0 && kernel < F32_KERNELS, "linear: no fp32 kernel %d", kernel);
  once_per_device([] {
    for (const LinearKernel& k : F32_TABLE) (void)hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes);
  });
  const LinearKernel& k = F32_TABLE[kernel];
  hipLaunchKernelGGL(k.fn, dim3(n_blocks, batch), dim3(k.threads), k.lds_bytes, as_stream(stream), p);
  return 0;
}

extern "C" int aurora_hip_split_f16(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int K,
                                    float scale, void* stream) {
  AURORA_CHECK_ARG(src != nullptr && dst != nullptr && rows > 0 && K > 0 && K % 32 == 0, "split_f16: K=%d must be a positive multiple of 32", K);
  AURORA_CHECK_ARG(ld_src >= K && ld_dst >= K && ld_src % 4 == 0 && ld_dst % 32 == 0 && ((uintptr_t)src % 16) == 0 &&
                   ((uintptr_t)dst % 16) == 0, "split_f16: strides / alignment");
  const int64_t n = rows * (K >> 3);
  hipLaunchKernelGGL(split_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), src, ld_src,
                     (char*)dst, ld_dst, rows, K, scale);
  return check_launch("split_f16");
}
