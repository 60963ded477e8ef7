// What the GEMM translation units share (gemm.hip, gemm_f32.hip, gemm_ln512.hip, gemm_a4.hip): the launch arguments, the LDS
// images' swizzles, the pieces of the tile preamble (piece_x / piece_w: where a 16-byte piece lies in its row, for the staging
// source and the fragment read alike; dma16; zero_acc), the tile order, the MFMA step, the core of every epilogue (biased16, the
// activations over a lane's 16 values, activate16) and the epilogues of the 256 x 256 tiles.  Each kernel family documents
// its own tile in its own file; the 128 x 128 kernel's description at the top of gemm.hip introduces the layouts used here.
// Every helper here is held to "the kernels compile to the same machine code as with the text in place"
// (tools/compare_isa.py): where one did not -- zero_acc and dma16 in linear_kernel_256, zero_acc in linear_kernel_256_f32x3 --
// the kernel keeps the text; so does the packed ladder of epilogue_256_bf16_coalesced (the four-wave kernel's branch layout).
#pragma once

#include "common.h"

namespace aurora {

namespace {

constexpr int ACT_GELU_FAST = 4;  // internal: fp32 results of the operand-splitting kernels, erf to 1.5e-7 (packed)

struct LinearArgs {
  const char* A; int64_t lda_b;   // byte strides
  const char* W; int64_t ldw_b;
  const float* bias;
  char* C; int64_t ldc;           // element strides from here on
  char* C2; int64_t ldc2;
  const float* res; int64_t ldr;
  int64_t M; int N; int k_tiles; int act;
  int tiles_n; int64_t n_blocks;
  int vec_store;                  // 1: every C/C2/res row piece is 16-byte aligned
  const float* guard; float guard_limit;   // f32 split kernels (guarded launch): two fp16 terms iff *guard < guard_limit
  int out_split;                  // two-term ping-pong kernel: C is written in the fp16-pair layout (see aurora_hip_split_f16)
  // strided batch (aurora_hip_linear_batched): problem blockIdx.y adds these to A / W / C (bytes) and bias (floats)
  int64_t bs_a, bs_w, bs_c, bs_bias;
  // split-K (linear_kernel_256pp, MODE 1): workgroup b multiplies K-slice b / n_blocks of tile b % n_blocks; slices
  // meet through fp32 slabs (256 KiB per slice and tile) and a ticket per tile -- the last arriver adds up and finishes
  int split; float* slabs; int32_t* tickets;
  // head planes (aurora_hip_linear_planes; 0: rows of ldc elements): the 64-column blocks of the result are q | k | v of
  // the attention heads (block sel * plane_heads + h); head h owns a plane of [M rows][q | k | v = 192 elements],
  // plane_stride elements after the previous head's
  int64_t plane_stride; int plane_heads;
};

// Element (m, n) of the result (n a multiple of 16: a 16-element piece never straddles two 64-column blocks).
template <typename T>
__device__ __forceinline__ T* out_piece(const LinearArgs& p, int64_t m, int n) {
  T* const c = reinterpret_cast<T*>(p.C);
  if (!p.plane_stride) return c + m * p.ldc + n;
  const int blk = n >> 6, sel = blk / p.plane_heads, h = blk - sel * p.plane_heads;
  return c + (int64_t)h * p.plane_stride + m * 192 + sel * 64 + (n & 63);
}

// The problem of a strided batch this workgroup belongs to (blockIdx.y; a plain launch has one problem and zero strides).
__device__ __forceinline__ LinearArgs batch_problem(const LinearArgs& in) {
  LinearArgs p = in;
  const int64_t g = blockIdx.y;
  p.A += g * in.bs_a;
  p.W += g * in.bs_w;
  p.C += g * in.bs_c;
  if (in.bias) p.bias += g * in.bs_bias;
  return p;
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;

__device__ __forceinline__ int swz_x(int row) { return row & 7; }
__device__ __forceinline__ int swz_w(int row) { return (((row >> 4) & 3) << 1) | ((row >> 1) & 1); }

// One 16 x 16 x (128 bytes of K / 2) MFMA step on 16-byte operand pieces.
template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  __device__ static __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct Mma<float> {
  // The K order inside a tile is free as long as both operands agree: lane group g supplies
  // k = 16*chunk + 4*g + s to the s-th of four 16x16x4 steps.
  __device__ static __forceinline__ f32x4 run(u32x4 a, u32x4 b, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
    return c;
  }
};

template <typename T>
__device__ __forceinline__ void store16(T* dst, const float (&v)[16], bool vec, int n_left);

template <>
__device__ __forceinline__ void store16<float>(float* dst, const float (&v)[16], bool vec, int n_left) {
  if (vec && n_left >= 16) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      reinterpret_cast<f32x4*>(dst)[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  } else {
#pragma unroll
    for (int t = 0; t < 16; ++t)
      if (t < n_left) dst[t] = v[t];
  }
}
template <>
__device__ __forceinline__ void store16<bf16_t>(bf16_t* dst, const float (&v)[16], bool vec, int n_left) {
  if (vec && n_left >= 16) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      reinterpret_cast<u32x4*>(dst)[q] =
          u32x4{pack_bf16x2(v[8 * q], v[8 * q + 1]), pack_bf16x2(v[8 * q + 2], v[8 * q + 3]),
                pack_bf16x2(v[8 * q + 4], v[8 * q + 5]), pack_bf16x2(v[8 * q + 6], v[8 * q + 7])};
  } else {
#pragma unroll
    for (int t = 0; t < 16; ++t)
      if (t < n_left) dst[t] = f32_to_bf16(v[t]);
  }
}

template <typename T> struct Other;
template <> struct Other<float> { typedef bf16_t type; };
template <> struct Other<bf16_t> { typedef float type; };

// Tiles and stages of the 256 x 256 kernels (gemm.hip, "Big-tile kernel"): K-stages of 64 bytes per row, 4-stage ring.
constexpr int BM2 = 256, BN2 = 256, ROW2 = 64, THREADS2 = 512, NSTAGE2 = 4;
constexpr int OPER2 = 256 * ROW2;      // 16 KiB per operand per stage
constexpr int STAGE2 = 2 * OPER2;      // 32 KiB per stage

// Tile of linear_kernel_f32pp (gemm_f32.hip); the dispatcher sizes its grid.
constexpr int VM = 128, VN = 256;

__device__ __forceinline__ int swz2(int a) { return ((a >> 1) & 1) * 3; }
__device__ __forceinline__ int swz2_x(int row) { return swz2((row >> 2) & 3); }
__device__ __forceinline__ int swz2_w(int row) { return swz2((row >> 4) & 3); }

// ---- the tile preamble of the kernels that stage 64-byte rows (ROW2) by LDS-DMA ----
// Byte offset of 16-byte piece c inside row `row` of an operand image (the swizzle of "Big-tile kernel", gemm.hip).  LDS-DMA
// writes lane-linearly, so the thread that stages a piece applies it to its SOURCE address and the lane that multiplies the
// piece to its fragment read: both sides through these two, or neither.
__device__ __forceinline__ int piece_x(int row, int c) { return (c ^ swz2_x(row)) << 4; }
__device__ __forceinline__ int piece_w(int row, int c) { return (c ^ swz2_w(row)) << 4; }
// One LDS-DMA piece: 16 bytes per lane from `src` to the wave-uniform LDS address `dst` + lane * 16 (the hardware adds it).
__device__ __forceinline__ void dma16(const char* src, char* dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (lds_ptr_t)dst, 16, 0, 0);
}
template <int FN, int FM>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[FN][FM]) {
#pragma unroll
  for (int a = 0; a < FN; ++a)
#pragma unroll
    for (int b = 0; b < FM; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// XCD-aware, L2-friendly tile order shared by both kernels: each XCD owns a contiguous range of
// logical ids; inside it n-tiles are visited in groups of `GN` with the m-tile index in between,
// so the workgroups that run together on one XCD share a few activation tiles AND a few weight
// tiles (both then come out of that XCD's 4 MiB L2).
// (GN = 8 for the 256 x 256 bf16 tiles; the fp32 ping-pong kernel's 128 x 256 tiles stage twice the weight bytes per
// activation byte and do best with 16 m-tiles x 2 n-tiles per XCD -- in-step A/B over GN = 2 .. 32, profiles/r02_ab_tile_group.log)
template <uint32_t GN = 8>
__device__ __forceinline__ void tile_of_block(uint32_t bid, uint32_t nb, uint32_t tiles_m, uint32_t tiles_n,
                                              uint32_t& tile_m, uint32_t& tile_n) {
  const uint32_t q8 = nb >> 3, r8 = nb & 7;
  const uint32_t xcd = bid & 7, idx = bid >> 3;
  const uint32_t logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const uint32_t full = (tiles_n / GN) * GN;          // n-tiles covered by complete groups
  const uint32_t per_group = GN * tiles_m;
  if (logical < (full / GN) * per_group) {
    const uint32_t grp = logical / per_group, rem = logical - grp * per_group;
    tile_m = rem / GN;
    tile_n = grp * GN + (rem - tile_m * GN);
  } else {                                             // last, narrower group
    const uint32_t rem = logical - (full / GN) * per_group, gw = tiles_n - full;
    tile_m = rem / gw;
    tile_n = full + (rem - tile_m * gw);
  }
}

// ---- what every epilogue starts with: the lane's 16 consecutive features of row fragment fm, and the activation ----
template <int FMS>
__device__ __forceinline__ void biased16(const f32x4 (&acc)[4][FMS], int fm, const float (&bias_v)[16], float (&v)[16]) {
#pragma unroll
  for (int fn = 0; fn < 4; ++fn) {
    v[4 * fn + 0] = acc[fn][fm].x + bias_v[4 * fn + 0];
    v[4 * fn + 1] = acc[fn][fm].y + bias_v[4 * fn + 1];
    v[4 * fn + 2] = acc[fn][fm].z + bias_v[4 * fn + 2];
    v[4 * fn + 3] = acc[fn][fm].w + bias_v[4 * fn + 3];
  }
}
// Activations over those 16 values (x2: as packed pairs).
__device__ __forceinline__ void silu16(float (&v)[16]) {
#pragma unroll
  for (int t = 0; t < 16; ++t) v[t] = v[t] / (1.0f + expf(-v[t]));
}
__device__ __forceinline__ void gelu_fast16x2(float (&v)[16]) {
#pragma unroll
  for (int t = 0; t < 16; t += 2) {
    const f32x2_hw r = gelu_erf_fast2(f32x2_hw{v[t], v[t + 1]});
    v[t] = r.x;
    v[t + 1] = r.y;
  }
}
// the ladder of the direct epilogues (the coalesced ones choose packed forms in place)
template <typename T>
__device__ __forceinline__ void activate16(int act, float (&v)[16]) {
  if (act == AURORA_ACT_GELU) {
#pragma unroll
    for (int t = 0; t < 16; ++t) v[t] = gelu_for<T>(v[t]);
  } else if (act == ACT_GELU_FAST) {
#pragma unroll
    for (int t = 0; t < 16; ++t) v[t] = gelu_erf_fast(v[t]);
  } else if (act == AURORA_ACT_SILU) {
    silu16(v);
  }
}

// Epilogue of the 256 x 256 kernels: a lane owns a row x 16 consecutive features (same ownership as the
// 128 x 128 kernel) -> bias, activation, fp32 residual, dual-dtype 16-byte stores.
template <typename T>
__device__ __forceinline__ void epilogue_256(const LinearArgs& p, f32x4 (&acc)[4][8], int64_t m0, int n0,
                                             int wm, int wn, int i16, int g) {
  const int nbase = n0 + wn * 64 + 16 * g;
  const int n_left = p.N - nbase;
  if (n_left <= 0) return;
  float bias_v[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) bias_v[t] = (p.bias && t < n_left) ? p.bias[nbase + t] : 0.f;
  const bool vec = p.vec_store != 0;
  typedef typename Other<T>::type T2;
#pragma unroll
  for (int fm = 0; fm < 8; ++fm) {
    const int64_t m = m0 + wm * 128 + 16 * fm + i16;
    if (m >= p.M) continue;
    float v[16];
    biased16(acc, fm, bias_v, v);
    activate16<T>(p.act, v);
    if (p.res) {
      const float* rp = p.res + m * p.ldr + nbase;
      if (vec && n_left >= 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 rv = reinterpret_cast<const f32x4*>(rp)[q];
          v[4 * q] += rv.x; v[4 * q + 1] += rv.y; v[4 * q + 2] += rv.z; v[4 * q + 3] += rv.w;
        }
      } else {
#pragma unroll
        for (int t = 0; t < 16; ++t)
          if (t < n_left) v[t] += rp[t];
      }
    }
    store16<T>(out_piece<T>(p, m, nbase), v, vec, n_left);
    if (p.C2) store16<T2>(reinterpret_cast<T2*>(p.C2) + m * p.ldc2 + nbase, v, vec, n_left);
  }
}

// bf16-only outputs (every backbone linear): transpose the wave's 128 x 64 result through LDS so that a
// store instruction writes 8 whole 128-byte row segments with CONSECUTIVE lanes on consecutive 16-byte pieces.
// The direct epilogue above has lane (j, g) write row j, i.e. 64 separate 16-byte requests per instruction,
// and the CU's store path then takes ~8 us per 256 x 256 tile (measured: a K = 512 tile costs 24.7 us with
// its stores and 16.9 us without) -- as long as half the tile's MFMA time.  The ring is dead after the main
// loop, so each wave borrows 16 KiB of it; LDS rows are XOR-swizzled (piece ^ (row & 7)): conflict-free for the
// b128 writes (8 rows per lane group) and reads (4 rows x 4 pieces per lane group).
template <int PARTS>   // 1: a wave's 128 x 64 results in one pass (16 KiB of the dead ring); 2 / 4: passes of 64 / 32 rows (8 / 4 KiB)
__device__ __forceinline__ void epilogue_256_bf16_coalesced(const LinearArgs& p, f32x4 (&acc)[4][8], int64_t m0,
                                                            int n0, int wm, int wn, int wave, int lane, char* smem,
                                                            const float (*bias_pre)[16] = nullptr) {
  const int i16 = lane & 15, g = lane >> 4;
  char* mine = smem + wave * (16384 / PARTS);
  const int nbase = n0 + wn * 64 + 16 * g;
  // (`bias_pre`: the lane's 16 bias values, requested by the caller before its main loop -- requested here, the first use
  //  waits out an L2 round trip with nothing else in flight)
  float bias_v[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) bias_v[t] = bias_pre ? (*bias_pre)[t] : (p.bias ? p.bias[nbase + t] : 0.f);
  const int rr = lane >> 3, cc = lane & 7;
  // (head planes: the wave's 64 columns are q, k or v of ONE head: 128-byte pieces of its plane's 384-byte rows)
  bf16_t* cbase = out_piece<bf16_t>(p, 0, n0 + wn * 64) + cc * 8;
  const int64_t ld_rows = p.plane_stride ? 192 : p.ldc;
#pragma unroll
  for (int part = 0; part < PARTS; ++part) {
#pragma unroll
    for (int f = 0; f < 8 / PARTS; ++f) {
      const int fm = part * (8 / PARTS) + f;
      float v[16];
      biased16(acc, fm, bias_v, v);
      if (p.act == AURORA_ACT_GELU) {   // (packed form of gelu_for<bf16_t>: same operations, same bits)
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
          const f32x2_hw r = gelu_sig2(f32x2_hw{v[t], v[t + 1]});
          v[t] = r.x;
          v[t + 1] = r.y;
        }
      } else if (p.act == AURORA_ACT_SILU) {
#pragma unroll
        for (int t = 0; t < 16; ++t) v[t] = v[t] / (1.0f + expf(-v[t]));
      }
      const int row = 16 * f + i16, sw = row & 7;
#pragma unroll
      for (int q = 0; q < 2; ++q)
        *reinterpret_cast<u32x4*>(mine + row * 128 + (((2 * g + q) ^ sw) << 4)) =
            u32x4{pack_bf16x2(v[8 * q], v[8 * q + 1]), pack_bf16x2(v[8 * q + 2], v[8 * q + 3]),
                  pack_bf16x2(v[8 * q + 4], v[8 * q + 5]), pack_bf16x2(v[8 * q + 6], v[8 * q + 7])};
    }
#pragma unroll
    for (int it = 0; it < 16 / PARTS; ++it) {
      const int row = it * 8 + rr;
      const u32x4 d = *reinterpret_cast<const u32x4*>(mine + row * 128 + ((cc ^ rr) << 4));
      const int64_t m = m0 + wm * 128 + part * (128 / PARTS) + row;
      if (m < p.M) __builtin_nontemporal_store(d, reinterpret_cast<u32x4*>(cbase + m * ld_rows));
    }
  }
}

// fp32 outputs, same idea in two halves (a wave's 128 x 64 fp32 results are 32 KiB, its share of the dead ring
// 16 KiB): rows of 256 bytes, pieces XOR-swizzled by (row & 7); a store instruction writes 4 whole row segments.
__device__ __forceinline__ void epilogue_256_f32_coalesced(const LinearArgs& p, f32x4 (&acc)[4][8], int64_t m0,
                                                           int n0, int wm, int wn, int wave, int lane, char* smem) {
  const int i16 = lane & 15, g = lane >> 4;
  char* mine = smem + wave * 16384;
  const int nbase = n0 + wn * 64 + 16 * g;
  float bias_v[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) bias_v[t] = p.bias ? p.bias[nbase + t] : 0.f;
  const int rr = lane >> 4, cc = lane & 15;
  float* cbase = reinterpret_cast<float*>(p.C) + n0 + wn * 64 + cc * 4;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int fm = 4 * half + f;
      float v[16];
      biased16(acc, fm, bias_v, v);
      if (p.act == AURORA_ACT_GELU) {
#pragma unroll
        for (int t = 0; t < 16; ++t) v[t] = gelu_for<float>(v[t]);
      } else if (p.act == ACT_GELU_FAST) {
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
          const f32x2_hw r = gelu_erf_fast2(f32x2_hw{v[t], v[t + 1]});
          v[t] = r.x;
          v[t + 1] = r.y;
        }
      } else if (p.act == AURORA_ACT_SILU) {
        silu16(v);
      }
      if (p.res) {
        const int64_t m = m0 + wm * 128 + 16 * fm + i16;
        const float* rp = p.res + (m < p.M ? m : p.M - 1) * p.ldr + nbase;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 rv = reinterpret_cast<const f32x4*>(rp)[q];
          v[4 * q] += rv.x; v[4 * q + 1] += rv.y; v[4 * q + 2] += rv.z; v[4 * q + 3] += rv.w;
        }
      }
      const int row = 16 * f + i16, sw = row & 7;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f32x4*>(mine + row * 256 + (((4 * g + q) ^ sw) << 4)) =
            f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int row = it * 4 + rr;
      const f32x4 d = *reinterpret_cast<const f32x4*>(mine + row * 256 + ((cc ^ (row & 7)) << 4));
      const int64_t m = m0 + wm * 128 + 64 * half + row;
      if (m < p.M) __builtin_nontemporal_store(d, reinterpret_cast<f32x4*>(cbase + m * p.ldc));
    }
  }
}

// A row of a dispatcher's kernel table (gemm.hip by plan id, gemm_f32.hip by F32Kernel): what a launch and the per-device
// LDS attribute need.
struct LinearKernel { void (*fn)(LinearArgs); unsigned threads; int lds_bytes; };

// The fp32 kernels of gemm_f32.hip, as the dispatcher of gemm.hip names them to aurora_f32_launch.
// F32_PP*: linear_kernel_f32pp with pre-split weights (W), pre-split activations and weights (AW), 256 x 128 tiles (TALL).
enum F32Kernel { F32_THREE, F32_TWO, F32_PP, F32_PP_W, F32_PP_AW, F32_PP_W_TALL, F32_PP_AW_TALL, F32_KERNELS };

}  // namespace

}  // namespace aurora

// The kernels of the other translation units, launched from the dispatcher: `linear_args` is a LinearArgs (it lives in each
// unit's anonymous namespace; all see this definition).
extern "C" __attribute__((visibility("hidden"))) int aurora_a4_launch(const void* linear_args, unsigned n_blocks, unsigned batch,
                                                                     void* stream);
extern "C" __attribute__((visibility("hidden"))) int aurora_f32_launch(int kernel, const void* linear_args, unsigned n_blocks,
                                                                      unsigned batch, void* stream);
