// Dense linear layers on the gfx950 matrix cores:  C = act(A . W^T + bias) (+ residual).
//
// Kernels in this file (dispatch: linear_impl at the end):
//   linear_kernel<T>            128 x 128 tile, two workgroups per CU -- small / ragged shapes, few-tile shapes
//   linear_kernel_256<T,4,4>    256 x 256 tile, 4-stage LDS ring     -- native-fp32 mode, bf16 with K < 128
//   linear_kernel_256pp         the same tile, ping-pong schedule    -- the backbone linears (bf16)
// and elsewhere: the operand-splitting fp32 kernels (gemm_f32.hip), the fused linear + AdaLN kernel (gemm_ln512.hip), the
// four-wave hand-scheduled tile (gemm_a4.hip); LinearArgs, swizzles, the preamble's pieces (piece_x / piece_w, dma16, zero_acc),
// tile order, the epilogue core (biased16, activate16) and epilogue_256* are shared (gemm_tile.h).
// The description below is the 128 x 128 kernel; the others document their differences in place.
//
// One kernel template serves bf16 (v_mfma_f32_16x16x32_bf16) and fp32
// (v_mfma_f32_16x16x4_f32, exact fp32 FMA chains) because both are tiled in BYTES: a K-tile
// is 128 bytes of every operand row (64 bf16 / 32 fp32), staged by 16-byte LDS-DMA pieces
// (global_load_lds_dwordx4, no VGPR round trip) into two LDS buffers per operand.
//
// Block tile 128 (m) x 128 (n), 256 threads = 4 waves as 2 (m) x 2 (n), wave tile 64 x 64 =
// 4 x 4 MFMA fragments of 16 x 16.  The MFMA "A" operand is the WEIGHT tile and the "B"
// operand the activation tile, i.e. every fragment holds C^T: lane (j = lane & 15, g = lane >> 4)
// owns activation row m = 16*fm + j and 4 consecutive output features per fragment.  Weight rows
// are interleaved over the 4 n-fragments (row = 16*(i>>2) + 4*fn + (i&3) for operand row i), so
// that the lane ends up with 16 CONSECUTIVE output features n = 16*g + 0..15 of one row: the
// epilogue (bias, exact GELU, residual, dual-dtype store) then works on whole 32/64-byte row
// pieces with 16-byte stores.
//
// LDS image of a tile: [128 rows][8 chunks of 16 B], chunk c of row r stored at position
// c ^ f(r).  LDS-DMA writes lane-linearly, so the swizzle is applied to the per-lane SOURCE
// address and again on the fragment read (both sides or neither).  f is chosen per operand so
// that the 16 rows touched by one ds_read_b128 lane group fall on 16 distinct 16-byte bank slots:
//   activations: rows i, i+1, ...          f(r) = r & 7
//   weights    : rows 16a + 4fn + b        f(r) = ((r >> 4) & 3) << 1 | ((r >> 1) & 1)
//
// Workgroup ids are remapped so that each XCD (8 of them, private L2s, block b runs on XCD b % 8)
// owns a contiguous range of tiles with the n-tiles of one m-tile adjacent: the activation tile
// is then fetched from HBM once per XCD and re-used out of that XCD's L2.
#include <stdlib.h>

#include <algorithm>

#include "gemm_tile.h"

namespace aurora {

namespace {

constexpr int BM = 128;       // activation rows per block
constexpr int BN = 128;       // output features per block
constexpr int ROW_BYTES = 128;  // bytes of K per tile row
constexpr int TILE_BYTES = 128 * ROW_BYTES;  // 16 KiB per operand per buffer
constexpr int THREADS = 256;
constexpr int A4_DEFAULT_MIN_K = 0;   // (0: the four-wave kernel of gemm_a4.hip is off unless AURORA_GEMM_A4_MIN_K says otherwise)

template <typename T>
__global__ __launch_bounds__(THREADS, 2) void linear_kernel(const LinearArgs p_in) {
  const LinearArgs p = batch_problem(p_in);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // Per buffer: X tile then W tile; 2 buffers.
  auto lds_x = [&](int buf) { return smem + buf * 2 * TILE_BYTES; };
  auto lds_w = [&](int buf) { return smem + buf * 2 * TILE_BYTES + TILE_BYTES; };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // ---- XCD-aware, L2-friendly tile assignment (tile_of_block, below) ----
  uint32_t tile_m, tile_n_u;
  tile_of_block(blockIdx.x, (uint32_t)p.n_blocks, (uint32_t)(p.n_blocks / p.tiles_n), (uint32_t)p.tiles_n, tile_m, tile_n_u);
  const int64_t m0 = (int64_t)tile_m * BM;
  const int n0 = (int)tile_n_u * BN;

  // ---- per-thread staging addresses: 4 pieces of X and 4 of W per K-tile ----
  const char* src_x[4];
  const char* src_w[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r * 32 + (tid >> 3);
    const int c = tid & 7;
    int64_t gm = m0 + row;
    gm = gm < p.M ? gm : p.M - 1;
    int gn = n0 + row;
    gn = gn < p.N ? gn : p.N - 1;
    src_x[r] = p.A + gm * p.lda_b + ((c ^ swz_x(row)) << 4);
    src_w[r] = p.W + (int64_t)gn * p.ldw_b + ((c ^ swz_w(row)) << 4);
  }

  auto stage = [&](int kt, int buf) {
    const int64_t koff = (int64_t)kt * ROW_BYTES;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // wave-uniform LDS base; the hardware adds lane * 16.
      const int base = (r * 256 + wave * 64) * 16;
      dma16(src_x[r] + koff, lds_x(buf) + base);
      dma16(src_w[r] + koff, lds_w(buf) + base);
    }
  };

  // ---- fragment read offsets (bytes inside a tile), one per (fragment, k-half) ----
  const int i16 = lane & 15, g = lane >> 4;
  int off_w[4][2], off_x[4][2];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int row_w = wn * 64 + 16 * (i16 >> 2) + 4 * f + (i16 & 3);
    const int row_x = wm * 64 + 16 * f + i16;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = g + 4 * ks;
      off_w[f][ks] = row_w * ROW_BYTES + ((c ^ swz_w(row_w)) << 4);
      off_x[f][ks] = row_x * ROW_BYTES + ((c ^ swz_x(row_x)) << 4);
    }
  }

  f32x4 acc[4][4];  // [fn][fm]
  zero_acc(acc);

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < p.k_tiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < p.k_tiles) stage(kt + 1, buf ^ 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4 fw[4], fx[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        fw[f] = *reinterpret_cast<const u32x4*>(lds_w(buf) + off_w[f][ks]);
        fx[f] = *reinterpret_cast<const u32x4*>(lds_x(buf) + off_x[f][ks]);
      }
#pragma unroll
      for (int fn = 0; fn < 4; ++fn)
#pragma unroll
        for (int fm = 0; fm < 4; ++fm) acc[fn][fm] = Mma<T>::run(fw[fn], fx[fm], acc[fn][fm]);
    }
    // The LDS-DMA of tile kt+1 must have landed, and every wave must be done reading tile kt,
    // before the next iteration reads one buffer and overwrites the other.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: lane owns row m (per fm) x 16 consecutive features ----
  const int nbase = n0 + wn * 64 + 16 * g;
  const int n_left = p.N - nbase;
  if (n_left <= 0) return;
  float bias_v[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) bias_v[t] = (p.bias && t < n_left) ? p.bias[nbase + t] : 0.f;
  const bool vec = p.vec_store != 0;
  typedef typename Other<T>::type T2;

#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    const int64_t m = m0 + wm * 64 + 16 * fm + i16;
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


// =================================================================================================
// Big-tile kernel for the backbone shapes (M >= 1024, N % 256 == 0): 256 x 256 tile, 512 threads =
// 8 waves as 2 (m) x 4 (n), wave tile 128 x 64 = 8 x 4 fragments.
//
// Why: the 128 x 128 kernel above keeps one 32 KiB K-tile in flight per workgroup; with ~1-2 us of
// HBM/L2 latency and ~0.2 us of MFMA work per tile the short-K GEMMs of stage 0 (K = 512) run at
// ~500 TFLOP/s, latency-bound.  Latency hiding capacity is (bytes in flight per CU) x (FLOP per
// byte of tile).  A 256 x 256 tile doubles the FLOP per byte (128), and K-tiles of 64 BYTES per
// row (32 bf16) make a stage 32 KiB, so a 4-stage LDS ring (128 KiB) keeps THREE tiles = 96 KiB
// in flight per CU: 3x the capacity.  The ring needs counted waits: `s_waitcnt vmcnt(8)` (two
// younger stages x 4 LDS-DMA instructions per lane stay in flight across the barrier) and a raw
// `s_barrier` -- a __syncthreads() would drain the LDS-DMA queue (vmcnt(0)).
//
// One barrier per stage does double duty: (RAW) every wave has waited for its own pieces of
// stage t before arriving, so after the barrier all of stage t is in LDS; (WAR) every wave has
// finished reading stage t-1 (its MFMAs consumed the fragments), so the DMA of stage t+3 may
// overwrite that buffer.
//
// LDS image per operand tile: [256 rows][4 pieces of 16 B]; piece c of row r at position c ^ f(r)
// with f = 0,0,3,3 over (r >> 2) & 3 (activations) / (r >> 4) & 3 (interleaved weight rows): the
// 16 rows of one ds_read_b128 lane group then hit 16 distinct 16-byte slots of the 256-byte bank row.
// =================================================================================================
// WN = number of wave columns, NST = ring depth.  Two forms are instantiated, and plan_linear picks between them:
//   WN = 4, NST = 4: 256 x 256 tile, 512 threads, one workgroup per CU (128 KiB ring) -- K_RING: native-fp32 mode, and
//                    bf16 launches with fewer than four K-stages;
//   WN = 2, NST = 3: 256 x 128 tile, 256 threads, two workgroups per CU (three stages of 24 KiB each) -- K_RING_MID, bf16
//                    only: the few-tile problems where plan_linear's cost model has the smaller tiles fill the chip better.
//                    (On the full-size backbone shapes this form is 5-15 % slower -- co-resident workgroups start
//                    together and stay in phase --, which is what the model's per-round costs say.)
constexpr int RING_LDS = NSTAGE2 * STAGE2;          // WN = 4, NST = 4
constexpr int MID_LDS = 3 * (BM2 + 128) * ROW2;     // WN = 2, NST = 3
// (Two co-resident 8-wave workgroups per CU -- a two-stage 64 KiB ring each -- do not fit: the 128 x 64 wave tile alone
// holds 128 accumulator registers, the kernel needs ~250 of the 256 a wave gets at two waves per SIMD.)
// PRIO: static s_setprio(1) for the second-dispatched half of the waves (the arbitration loser of every K-stage).
template <typename T, int WN, int NST, int PRIO = 0>
__global__ __launch_bounds__(128 * WN, 2) void linear_kernel_256(const LinearArgs p_in) {
  const LinearArgs p = batch_problem(p_in);
  constexpr int NTHR = 128 * WN;
  constexpr int XP = (BM2 * 4) / NTHR;            // 16-byte pieces of the activation tile per thread and stage
  constexpr int WP = (64 * WN * 4) / NTHR;        // ... of the weight tile (= 2)
  constexpr int LPS = XP + WP;                    // LDS-DMA instructions per lane and stage
  constexpr int OPER_X = BM2 * ROW2, OPER_W = 64 * WN * ROW2, STAGE = OPER_X + OPER_W;
  static_assert((NST == 4 && LPS == 4) || (NST == 3 && LPS == 6), "waitcnt immediates below assume these");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  if constexpr (PRIO != 0) {
    if (wave >= 2 * WN) __builtin_amdgcn_s_setprio(1);
  }

  uint32_t tile_m, tile_n;
  tile_of_block(blockIdx.x, (uint32_t)p.n_blocks, (uint32_t)(p.n_blocks / p.tiles_n), (uint32_t)p.tiles_n, tile_m, tile_n);
  const int64_t m0 = (int64_t)tile_m * BM2;
  const int n0 = (int)tile_n * 64 * WN;

  const char* src_x[XP];
  const char* src_w[WP];
#pragma unroll
  for (int r = 0; r < XP; ++r) {
    const int id = r * NTHR + tid;
    const int row = id >> 2, c = id & 3;
    int64_t gm = m0 + row;
    gm = gm < p.M ? gm : p.M - 1;
    src_x[r] = p.A + gm * p.lda_b + piece_x(row, c);
  }
#pragma unroll
  for (int r = 0; r < WP; ++r) {
    const int id = r * NTHR + tid;
    const int row = id >> 2, c = id & 3;
    int gn = n0 + row;
    gn = gn < p.N ? gn : p.N - 1;
    src_w[r] = p.W + (int64_t)gn * p.ldw_b + piece_w(row, c);
  }
  // (The LDS-DMA builtin spelled out, not dma16: through the helper two s_add of this kernel's prologue trade places, and
  // the kernel's machine code is pinned -- gemm_tile.h, top.)
  auto stage = [&](int kt) {
    const int64_t koff = (int64_t)kt * ROW2;
    char* base = smem + (kt % NST) * STAGE;
#pragma unroll
    for (int r = 0; r < XP; ++r)  // wave-uniform LDS address; the hardware adds lane * 16
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src_x[r] + koff),
                                       (lds_ptr_t)(base + (r * NTHR + wave * 64) * 16), 16, 0, 0);
#pragma unroll
    for (int r = 0; r < WP; ++r)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src_w[r] + koff),
                                       (lds_ptr_t)(base + OPER_X + (r * NTHR + wave * 64) * 16), 16, 0, 0);
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
    off_w[f] = OPER_X + row * ROW2 + piece_w(row, g);
  }

  f32x4 acc[4][8];  // [fn][fm]  (zeroed in place, not by zero_acc: the helper changes this kernel's register assignment)
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Software pipeline (nt is even: K * sizeof(T) is a multiple of 128 bytes):
  //   LDS ring   : stages kt+2 .. kt+NST in flight while stage kt is multiplied
  //   registers  : the fragments of stage kt+1 are read from LDS while the 32 MFMAs of stage kt
  //                run on the other fragment set -- the matrix pipe never waits for a ds_read.
  const int nt = p.k_tiles;
  auto read_frags = [&](int kt, u32x4 (&fw)[4], u32x4 (&fx)[8]) {
    const char* buf = smem + (kt % NST) * STAGE;
#pragma unroll
    for (int f = 0; f < 4; ++f) fw[f] = *reinterpret_cast<const u32x4*>(buf + off_w[f]);
#pragma unroll
    for (int f = 0; f < 8; ++f) fx[f] = *reinterpret_cast<const u32x4*>(buf + off_x[f]);
  };
  // One pipeline step.  Order matters: the first MFMAs of stage kt need only registers (their
  // ds_reads were issued a whole step ago, so the compiler's lgkmcnt(0) in front of them is free);
  // then stage kt+1 is made visible (counted vmcnt + raw barrier), the ring is refilled and the
  // fragments of stage kt+1 are requested; the remaining MFMAs of stage kt cover that latency.
  auto mma_rows = [&](u32x4 (&cw)[4], u32x4 (&cx)[8], int fm_lo, int fm_hi) {
#pragma unroll
    for (int fm = fm_lo; fm < fm_hi; ++fm)
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = Mma<T>::run(cw[fn], cx[fm], acc[fn][fm]);
  };
  auto step = [&](int kt, u32x4 (&cw)[4], u32x4 (&cx)[8], u32x4 (&nw)[4], u32x4 (&nx)[8]) {
    mma_rows(cw, cx, 0, 2);
    __builtin_amdgcn_sched_barrier(0);
    // my pieces of stage kt+1 have landed once only the younger stages (NST - 2 of them) remain outstanding
    if constexpr (NST == 4) {
      if (kt + 3 < nt) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (kt + 2 < nt) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      if (kt + 2 < nt) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();  // RAW: stage kt+1 complete.  WAR: everyone has read stage kt.
    asm volatile("" ::: "memory");
    if (kt + NST < nt) stage(kt + NST);  // into stage kt's buffer
    read_frags(kt + 1, nw, nx);
    __builtin_amdgcn_sched_barrier(0);
    mma_rows(cw, cx, 2, 8);
  };

  stage(0);
  stage(1);  // nt >= 2
  if (nt > 2) stage(2);
  if constexpr (NST == 4) {
    if (nt > 3) stage(3);
    if (nt > 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (nt > 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    if (nt > 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  u32x4 fwA[4], fxA[8], fwB[4], fxB[8];
  read_frags(0, fwA, fxA);
  for (int kt = 0; kt + 2 < nt; kt += 2) {
    step(kt, fwA, fxA, fwB, fxB);
    step(kt + 1, fwB, fxB, fwA, fxA);
  }
  step(nt - 2, fwA, fxA, fwB, fxB);  // fetches the last stage
  mma_rows(fwB, fxB, 0, 8);

  if constexpr (sizeof(T) == 2) {
    if (p.C2 == nullptr && p.res == nullptr && p.vec_store) {   // (uniform)
      __syncthreads();   // every wave is done with the ring
      // (in parts, as in linear_kernel_256pp below)
      if (p.act == AURORA_ACT_GELU) epilogue_256_bf16_coalesced<4>(p, acc, m0, n0, wm, wn, wave, lane, smem);
      else epilogue_256_bf16_coalesced<2>(p, acc, m0, n0, wm, wn, wave, lane, smem);
      return;
    }
  } else if constexpr (WN == 4) {
    if (p.C2 == nullptr && p.vec_store) {
      __syncthreads();
      epilogue_256_f32_coalesced(p, acc, m0, n0, wm, wn, wave, lane, smem);
      return;
    }
  }
  epilogue_256<T>(p, acc, m0, n0, wm, wn, i16, g);
}


// =================================================================================================
// Ping-pong form of the 256 x 256 ring kernel (bf16): the two waves that share a SIMD never issue MFMAs at the same time.
//
// In linear_kernel_256 all eight waves run the same stream in phase -- 8 MFMAs, wait, barrier, DMA issue, 12 fragment
// reads, 24 MFMAs -- and the two waves of a SIMD compete for its matrix pipe and issue slots (measured in round 1:
// 1668 cycles per K-stage for 1024 cycles of MFMA work, one wave of each pair parked ~580 cycles per stage).  Here every
// wave alternates a LOAD phase L(s) (12 fragment reads of stage s, DMA issue of stage s+3, counted waits) and a MATRIX
// phase M(s) (32 back-to-back MFMAs), with a barrier after each -- and waves 4-7 (the SIMD partners of waves 0-3) run
// ONE PHASE BEHIND, by a single extra barrier in front (balanced by one for waves 0-3 at the end).  So in every
// wall-clock phase a SIMD's matrix pipe belongs to exactly one wave while its partner does the LDS / DMA work; the
// instruction stream is the same for all waves, and fragments are read one phase before they are multiplied (one
// register set instead of two).
// Ring bookkeeping (per wave, iteration s): stage s+1 is published by the barrier that ends L(s) -- every wave has by
// then waited for ITS pieces of it (vmcnt(8): stages s+2, s+3 are younger) -- and is read no earlier than L(s+1); the
// DMA of stage s+3 in L(s) overwrites the buffer of stage s-1, whose last reader (a late wave's L(s-1), finished with
// lgkmcnt(0) before its barrier) is at least one barrier in the past for early and late waves alike.
// =================================================================================================
// 16 bytes written THROUGH to memory (sc1): the payload of an in-launch hand-off needs no release fence then, only the
// writing wave's own `s_waitcnt vmcnt(0)` before the flag (MI355X guide, "publish-large": 3.0 against 8.2 us per 64 KiB).
// hipcc does not count an asm store: the callers drain explicitly.
__device__ __forceinline__ void store_through(float* dst, f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
}

constexpr int PP_LDS = NSTAGE2 * STAGE2;            // the ring: 128 KiB

// SPLIT: split-K.  Launches with fewer tiles than CUs and a long K (a latitude band's coarse stages: 72 tiles, K = 8192)
//   cut every tile's K range into `split` slices, one workgroup each.  A slice publishes its fp32 accumulators to its
//   slab (write-through stores, drained), takes a ticket of the tile; whoever draws the last ticket -- no workgroup ever
//   waits for another, so nothing depends on dispatch order or co-residency -- adds the slices up IN SLICE ORDER (two
//   slices: its registers + the other slab, commutative; more: all slabs from memory, its own included, so that the sum
//   does not depend on who came last), resets the ticket for the next launch and runs the ordinary epilogue.
// Built, measured and deleted again in round 4 (profiles/r04_ab_gemm_variants_isolated.log, r04_ab_gemm_persistent_instep.json):
//   * a persistent form (workgroups walk over tiles; the next tile's bias row and first K-stages are requested before the
//     epilogue, which keeps the buffer of stage 3 for its transposition; counted waits raised by the 16 result stores that
//     sit behind the prologue in the in-order counter): -0.8 % over the step's shapes in isolation (-2...-4 % on the
//     K = 512 ones), 134.6 against 134.2 ms inside the step -- the cold start of a tile is not what its fixed cost is;
//   * a register-only epilogue (lanes i16 and i16 ^ 8 trade 16-byte pieces by a DPP rotation, stores cover whole 128-byte
//     rows): +1 % -- a 16-lane group then writes eight 32-byte pieces, the LDS-transposed form two whole rows;
//   * narrower n-groups of the tile order (4 or 2 n-tiles instead of 8, so that the weight panels of a round might survive
//     in L2 at K >= 1024): L2 -> fabric reads unchanged (-4 %; the activation panels streaming through evict them anyway),
//     time unchanged (profiles/r04_pmc_gemm_fetch_by_group_width.txt).
template <bool SPLIT>
__global__ __launch_bounds__(THREADS2, 2) void linear_kernel_256pp(const LinearArgs p_in) {
  const LinearArgs p = batch_problem(p_in);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;   // waves w and w+4 share a SIMD; wm = 1 runs one phase behind
  const uint32_t nb = (uint32_t)p.n_blocks;

  uint32_t item = blockIdx.x;   // tile, in launch order
  int kb = 0, nt = p.k_tiles, part = 0;
  if constexpr (SPLIT) {
    part = (int)(item / nb);
    item -= (uint32_t)part * nb;
    kb = (int)((int64_t)part * p.k_tiles / p.split);
    nt = (int)((int64_t)(part + 1) * p.k_tiles / p.split) - kb;   // >= 4 (dispatch)
  }
  uint32_t tile_m, tile_n;
  tile_of_block(item, nb, nb / (uint32_t)p.tiles_n, (uint32_t)p.tiles_n, tile_m, tile_n);
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
    src_x[r] = p.A + gm * p.lda_b + piece_x(row, c) + (int64_t)kb * ROW2;
    src_w[r] = p.W + (int64_t)gn * p.ldw_b + piece_w(row, c) + (int64_t)kb * ROW2;
  }
  auto stage = [&](int kt) {
    const int64_t koff = (int64_t)kt * ROW2;
    char* base = smem + (kt & (NSTAGE2 - 1)) * STAGE2;
#pragma unroll
    for (int r = 0; r < 2; ++r)
      dma16(src_x[r] + koff, base + (r * THREADS2 + wave * 64) * 16);
#pragma unroll
    for (int r = 0; r < 2; ++r)
      dma16(src_w[r] + koff, base + OPER2 + (r * THREADS2 + wave * 64) * 16);
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
  f32x4 acc[4][8];  // [fn][fm]
  zero_acc(acc);
  // The lane's 16 bias values, for the epilogue: requested NOW, in front of (and so older than) every piece the counted waits
  // below leave in flight; 16 registers the main loop does not need (201 of 256 before).  In the step 127.6 -> 127.3 ms
  // (profiles/r06_ab_epilogue_parts.log).
  float bias_pre[16];
  {
    const int nb16 = n0 + wn * 64 + 16 * g;
#pragma unroll
    for (int t = 0; t < 16; ++t) bias_pre[t] = p.bias ? p.bias[nb16 + t] : 0.f;   // (N is a multiple of the tile width here)
  }
  asm volatile("" ::: "memory");
  stage(0);
  stage(1);
  stage(2);
  stage(3);
  asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  __builtin_amdgcn_s_barrier();   // stage 0 is complete
  asm volatile("" ::: "memory");
  if (wm == 1) __builtin_amdgcn_s_barrier();   // the late half: one phase behind from here on

  for (int s = 0; s < nt; ++s) {
    // ---- L(s): fragments of stage s, refill the ring, settle what the next barrier publishes ----
    u32x4 fw[4], fx[8];
    {
      const char* buf = smem + (s & (NSTAGE2 - 1)) * STAGE2;
#pragma unroll
      for (int f = 0; f < 4; ++f) fw[f] = *reinterpret_cast<const u32x4*>(buf + off_w[f]);
#pragma unroll
      for (int f = 0; f < 8; ++f) fx[f] = *reinterpret_cast<const u32x4*>(buf + off_x[f]);
    }
    if (s >= 1 && s + 3 < nt) stage(s + 3);   // into the buffer of stage s-1
    if (s + 3 < nt) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");        // own pieces of stage s+1 have landed
    else if (s + 2 < nt) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // ---- M(s): the matrix pipe is this wave's alone ----
#pragma unroll
    for (int fm = 0; fm < 8; ++fm)
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) acc[fn][fm] = Mma<bf16_t>::run(fw[fn], fx[fm], acc[fn][fm]);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();   // the early half waits for the late half's last phase: the ring is dead
  asm volatile("" ::: "memory");

  if constexpr (SPLIT) {
    // ---- publish this slice, take a ticket; the last arriver combines ----
    float* const slab0 = p.slabs + (int64_t)item * p.split * (BM2 * BN2);
    const int64_t mine_off = (int64_t)(wave * 32 * 64 + lane) * 4;
    {
      float* const mine = slab0 + (int64_t)part * (BM2 * BN2) + mine_off;
#pragma unroll
      for (int fn = 0; fn < 4; ++fn)
#pragma unroll
        for (int fm = 0; fm < 8; ++fm) store_through(mine + (fn * 8 + fm) * 256, acc[fn][fm]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its own stores ...
    __syncthreads();                                    // ... before ONE lane takes the ticket
    int* const s_ticket = reinterpret_cast<int*>(smem);
    if (tid == 0) *s_ticket = __hip_atomic_fetch_add(p.tickets + item, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int ticket = *s_ticket;
    if (ticket != p.split - 1) return;   // (uniform) someone else will finish this tile
    if (tid == 0) __hip_atomic_store(p.tickets + item, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
    if (wave == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // drop this CU's stale L1 lines, once
    __syncthreads();
    const float* const src = slab0 + mine_off;
    // Two slices: registers + the other slab (commutative).  More: every slab from memory, this one's own included,
    // in slice order -- the sum must not depend on who drew the last ticket.  Eight loads in flight per lane (the
    // accumulators hold 128 registers; the fence keeps hipcc from hoisting a slab's 32 loads above the first add).
    const bool two = p.split == 2;
    if (!two) {
#pragma unroll
      for (int fn = 0; fn < 4; ++fn)
#pragma unroll
        for (int fm = 0; fm < 8; ++fm) acc[fn][fm] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int j = 0; j < p.split; ++j) {
      if (two && j == part) continue;
      const float* const o = src + (int64_t)j * (BM2 * BN2);
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) {
        f32x4 t[8];
#pragma unroll
        for (int fm = 0; fm < 8; ++fm) t[fm] = *reinterpret_cast<const f32x4*>(o + (fn * 8 + fm) * 256);
        asm volatile("" ::: "memory");
#pragma unroll
        for (int fm = 0; fm < 8; ++fm) acc[fn][fm] += t[fm];
      }
    }
  }
  if (p.C2 == nullptr && p.res == nullptr && p.vec_store) {   // (uniform)
    // In parts (64 / 32 rows of the wave's 128 at a time): the stores of one part are in flight while the next part's bias,
    // activation and packing run on the VALU -- in one pass the GELU of a stage-0 fc1 tile (11 VALU instructions per two
    // values, 9 K cycles per SIMD) ran with no memory operation in flight.  In the step: 129.7 -> 128.2 ms
    // (profiles/r06_ab_epilogue_parts.log); the same values either way.
    if (p.act == AURORA_ACT_GELU) epilogue_256_bf16_coalesced<4>(p, acc, m0, n0, wm, wn, wave, lane, smem, &bias_pre);
    else epilogue_256_bf16_coalesced<2>(p, acc, m0, n0, wm, wn, wave, lane, smem, &bias_pre);
    return;
  }
  epilogue_256<bf16_t>(p, acc, m0, n0, wm, wn, i16, g);
}

}  // namespace

}  // namespace aurora

using namespace aurora;

namespace {
// Process default of how large fp32 linears are multiplied (read once from AURORA_F32_GEMM, never changed afterwards):
// 0: native fp32 MFMA (v_mfma_f32_16x16x4_f32); 1: 3 x bf16 operand splitting (default); 2: 2 x fp16 splitting.
int default_f32_mode() {
  static const int mode = [] {
    const char* e = getenv("AURORA_F32_GEMM");
    return !e ? 1 : (e[0] == 'n' || e[0] == '0') ? 0 : (e[0] == 'f' || e[0] == '2') ? 2 : 1;   // native | bf16 | f16
  }();
  return mode;
}

// Smallest K (elements) of a plain bf16 linear on 256 x 256 tiles that takes the four-wave kernel with the hand-scheduled
// main loop (gemm_a4.hip) instead of the eight-wave ping-pong one.  A read-once process default like AURORA_F32_GEMM
// (AURORA_GEMM_A4_MIN_K; 0 = never): both kernels accumulate K in the same 32-wide steps -- the same bits either way.
int a4_min_k() {
  static const int v = [] {
    const char* e = getenv("AURORA_GEMM_A4_MIN_K");
    const int k = e ? atoi(e) : A4_DEFAULT_MIN_K;
    return k <= 0 ? 0x7fffffff : k;
  }();
  return v;
}

// Scratch of a split-K launch, owned by the caller: fp32 slabs (split x 256 KiB per tile; contents do not matter) and one
// ticket per tile (zero on entry, left zero).
struct SplitWs { float* slabs; int64_t slab_bytes; int32_t* tickets; int n_tickets; int split; };

// K split of a plain bf16 linear on 256 x 256 tiles (1 = none).  Only launches that leave most of the chip idle and
// have K to spare: tiles * split <= CUs (one round), >= 64 K-steps (K = 2048) per slice -- below that the slab round trip
// costs more than the idle CUs were worth (measured: 72 tiles, K = 2048: 31.6 -> 37 us; K = 8192: 108 -> 80 us) --, at most 8.
int choose_split(int64_t M, int N, int K, int64_t cus) {
  if (N % BN2 != 0 || M < 1024 || K % 32 != 0) return 1;
  const int64_t tiles = ((M + BM2 - 1) / BM2) * (N / BN2);
  const int kt = K / 32;
  int s = (int)std::min<int64_t>(std::min<int64_t>(8, cus / tiles), kt / 64);
  return s < 1 ? 1 : s;
}

// One linear, as an entry point asks for it.  The defaults are the plain call: one output, no residual, the process's fp32
// mode, no guard, one problem, no split-K scratch, rows of ldc elements.
struct LinearCall {
  const void* A; int64_t lda; const void* W; int64_t ldw; const float* bias; void* C; int64_t ldc;
  int64_t M; int N; int K; int dtype; void* stream;
  int act = AURORA_ACT_NONE;
  void* C2 = nullptr; int64_t ldc2 = 0; const float* residual = nullptr; int64_t ldr = 0;
  int f32_gemm = -1; const float* guard = nullptr; float guard_limit = 0.f;   // (check_call: f32_gemm loses its AURORA_F32_*_SPLIT bits)
  int batch = 1; int64_t stride_a = 0, stride_w = 0, stride_bias = 0, stride_c = 0;
  const SplitWs* ws = nullptr;
  int64_t plane_stride = 0; int plane_heads = 0;
  int pre = 0, mode = 0;   // set by check_call: the AURORA_F32_*_SPLIT bits of f32_gemm, the fp32 mode in force
  int es() const { return dtype == AURORA_F32 ? 4 : 2; }   // bytes per element
};

// Kernels of a plan: the fp32 ones of gemm_f32.hip (F32Kernel) and this file's.
enum { K_TILE_128 = F32_KERNELS, K_RING, K_RING_MID, K_PP, K_PP_SPLITK, K_A4 };
struct LinearPlan {
  int kernel; bool twin;   // twin: a guarded two-term launch, followed by its three-term twin
  int bm, bn, rowb;        // tile and bytes of K per stage row, as LinearArgs counts them (linear_kernel_f32pp: see launch_linear)
  int ksplit;
};

int check_call(LinearCall& c) {
  AURORA_CHECK_ARG(c.dtype == AURORA_F32 || c.dtype == AURORA_BF16, "linear: bad dtype %d", c.dtype);
  AURORA_CHECK_ARG(c.plane_stride == 0 || (c.dtype == AURORA_BF16 && c.plane_heads > 0 && c.N % (64 * c.plane_heads) == 0 &&
                                           c.N <= 192 * c.plane_heads && c.plane_stride >= c.M * 192 &&
                                           c.plane_stride % 8 == 0 && c.C2 == nullptr && c.residual == nullptr && c.batch == 1),
                   "linear: head planes need bf16, N = 64 heads x (1, 2 or 3), planes of >= M rows, one output, no residual");
  c.pre = c.f32_gemm < 0 ? 0 : c.f32_gemm & (AURORA_F32_A_SPLIT | AURORA_F32_W_SPLIT | AURORA_F32_C_SPLIT);
  if (c.pre) c.f32_gemm &= ~c.pre;
  AURORA_CHECK_ARG(c.f32_gemm >= -1 && c.f32_gemm <= 2, "linear: bad fp32 GEMM mode %d", c.f32_gemm);
  c.mode = c.f32_gemm < 0 ? default_f32_mode() : c.f32_gemm;
  // pre-split operands / output: the two-term ping-pong kernel only.  An A-split launch cannot fall back to three terms
  // (they need the fp32 values), so it takes no guard; a W-split launch with a guard runs iff the guard holds and the
  // caller pairs it with a mode-1 launch on the fp32 weights carrying the same guard, which runs iff it does not.
  AURORA_CHECK_ARG(!c.pre || (c.dtype == AURORA_F32 && c.mode == 2 && c.N % 128 == 0 && c.K % 32 == 0 && c.K >= 96),
                   "linear: fp16-pair operands need fp32, mode 2, N %% 128 == 0, K %% 32 == 0, K >= 96 (N=%d K=%d)", c.N, c.K);
  // (an A-split launch WITH a guard is for buffers whose format was itself decided by that guard on the device -- written
  // as pairs by a guarded two-term producer iff it holds, as fp32 by its three-term twin otherwise)
  AURORA_CHECK_ARG(!(c.pre & AURORA_F32_A_SPLIT) || (c.pre & AURORA_F32_W_SPLIT),
                   "linear: a pre-split activation operand needs pre-split weights");
  AURORA_CHECK_ARG(!(c.pre & AURORA_F32_C_SPLIT) || (c.C2 == nullptr && c.ldc % 32 == 0 && ((uintptr_t)c.C % 16) == 0),
                   "linear: fp16-pair output needs ldc %% 32 == 0, 16-byte alignment and no second output");
  if (!(c.mode == 2 || (c.mode == 1 && c.dtype == AURORA_F32))) c.guard = nullptr;
  AURORA_CHECK_ARG(c.M > 0 && c.N > 0 && c.K > 0, "linear: empty problem M=%lld N=%d K=%d", (long long)c.M, c.N, c.K);
  const int es = c.es();
  AURORA_CHECK_ARG(((int64_t)c.K * es) % ROW_BYTES == 0,
                   "linear: K=%d must be a multiple of %d elements", c.K, ROW_BYTES / es);
  AURORA_CHECK_ARG((c.lda * es) % 16 == 0 && (c.ldw * es) % 16 == 0 && c.lda >= c.K && c.ldw >= c.K,
                   "linear: operand strides must be 16-byte multiples >= K");
  AURORA_CHECK_ARG(((uintptr_t)c.A % 16) == 0 && ((uintptr_t)c.W % 16) == 0, "linear: unaligned operand");
  AURORA_CHECK_ARG(c.act >= AURORA_ACT_NONE && c.act <= AURORA_ACT_SILU, "linear: bad activation %d", c.act);
  AURORA_CHECK_ARG(c.C != nullptr && c.ldc >= c.N && (!c.C2 || c.ldc2 >= c.N) && (!c.residual || c.ldr >= c.N || c.ldr == 0),
                   "linear: bad output strides");
  return AURORA_OK;
}

// Kernel and tiling of a checked call on a device of `cus` compute units.
LinearPlan plan_linear(const LinearCall& c, int64_t cus) {
  const int64_t M = c.M;
  const int N = c.N, K = c.K, dtype = c.dtype, pre = c.pre, mode = c.mode;
  // Big backbone shapes take the 256 x 256 ring kernel; everything else the 128 x 128 one.
  // (fp32 in split mode: the kernel choice must not depend on M, or a latitude band of a sharded model
  // would round differently from the same rows of the un-sharded one.)
  const bool split = dtype == AURORA_F32 && mode >= 1;
  const bool tall = pre != 0 && N % VN != 0;   // pre-split operands, N a multiple of 128 only: the 256 x 128 two-term tiles
  bool big = (M >= 1024 || split) && (N % BN2 == 0 || tall);
  bool mid = false;   // bf16 only: 256 x 128 tiles of the ring kernel, two 4-wave workgroups per CU
  // split-K on 256 x 256 tiles when the caller brought scratch for it (aurora_hip_linear_ws) and the launch would
  // otherwise leave most of the chip idle
  int ksplit = 1;
  if (big && dtype == AURORA_BF16 && c.batch == 1 && c.ws != nullptr) {
    ksplit = c.ws->split > 0 ? std::min(c.ws->split, K / 128) : choose_split(M, N, K, cus);
    const int64_t tiles = ((M + BM2 - 1) / BM2) * (N / BN2);
    if (ksplit > 1 && (tiles > c.ws->n_tickets || tiles * ksplit * (int64_t)(BM2 * BN2 * 4) > c.ws->slab_bytes)) ksplit = 1;
  }
  if (big && !split && ksplit <= 1) {
    // Few tiles (a latitude band of a sharded model, the coarse stages): 256 x 256 tiles leave CUs idle or end in a
    // thin last round.  Smaller tiles fill the chip: 256 x 128 tiles of the same ring kernel (two 4-wave workgroups per
    // CU, each with the full 128 x 64 wave tile) or 128 x 128 tiles.  The choice is a cost model fitted to measurements
    // (profiles/r02_ab_gemm_tiles.log): a round of tiles costs a + b K microseconds -- 256^2: 10.1 + 0.0266 K (256 per
    // round), 256 x 128: 7.7 + 0.0317 K (512 per round), 128^2: 7.6 + 0.0153 K (512 per round) -- and a last round that
    // leaves every CU with at most one of its two workgroups runs in ~0.65 of that.  (Results do not depend on the
    // tiling: every kernel accumulates K in the same 32-wide steps.)
    const int64_t nb_big = ((M + BM2 - 1) / BM2) * (N / BN2), nb_small = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    const int64_t nb_mid = ((M + BM2 - 1) / BM2) * (N / 128);
    if (dtype == AURORA_BF16) {
      auto cost = [&](int64_t nb, int64_t slots, double a, double b) {
        const int64_t full = nb / slots, rem = nb % slots;
        const double part = rem == 0 ? 0.0 : (slots > cus && rem <= cus) ? 0.65 : 1.0;
        return ((double)full + part) * (a + b * (double)K);
      };
      const double t_big = cost(nb_big, cus, 10.1, 0.0266), t_mid = cost(nb_mid, 2 * cus, 7.7, 0.0317),
                   t_small = cost(nb_small, 2 * cus, 7.6, 0.0153);
      if (t_mid < 0.97 * t_big && t_mid <= t_small) mid = true;
      else if (t_small < 0.97 * t_big) big = false;
    } else {
      auto fill = [&](int64_t nb, int64_t slots) { return (double)nb / (double)(((nb + slots - 1) / slots) * slots); };
      if (0.8 * fill(nb_small, 2 * cus) > fill(nb_big, cus)) big = false;
    }
  }
  LinearPlan plan{K_TILE_128, false, big ? BM2 : BM, mid ? 128 : big ? BN2 : BN, big ? ROW2 : ROW_BYTES, ksplit};
  const int k_tiles = (int)(((int64_t)K * c.es()) / plan.rowb);
  // two fp16 terms: the ping-pong kernel (128 x 256 tiles, K-stages of 32) when K allows, else the in-phase 256 x 256 one
  const bool f32pp = big && split && mode == 2 && K % 32 == 0 && K >= 96;
  const int pp = tall ? ((pre & AURORA_F32_A_SPLIT) ? F32_PP_AW_TALL : F32_PP_W_TALL)
                      : (pre & AURORA_F32_A_SPLIT) ? F32_PP_AW : (pre & AURORA_F32_W_SPLIT) ? F32_PP_W : F32_PP;
  if (mid) plan.kernel = K_RING_MID;
  else if (!big) plan.kernel = K_TILE_128;
  else if (pre) plan.kernel = pp;
  else if (split && mode == 1 && c.guard != nullptr) plan.kernel = F32_THREE;   // the three-term half of a guarded pair (see check_call)
  else if (split && mode == 2 && c.guard != nullptr) {                         // both variants; the device word picks one
    plan.kernel = f32pp ? pp : F32_TWO;
    plan.twin = true;
  } else if (f32pp) plan.kernel = pp;
  else if (split && mode == 2) plan.kernel = F32_TWO;
  else if (split) plan.kernel = F32_THREE;
  else if (dtype == AURORA_F32) plan.kernel = K_RING;
  else if (ksplit > 1) plan.kernel = K_PP_SPLITK;   // ping-pong main loop, one workgroup per K-slice of a tile
  else if (k_tiles >= 8 && k_tiles % 2 == 0 && K >= a4_min_k()) plan.kernel = K_A4;   // four waves, hand-scheduled loop (gemm_a4.hip)
  else if (k_tiles >= 4) plan.kernel = K_PP;        // ping-pong main loop, one workgroup per tile
  else plan.kernel = K_RING;
  return plan;
}

// This file's kernels by plan id (from K_TILE_128 on) and dtype (bf16 | fp32; a kernel of one dtype leaves the other
// empty).  K_A4 lives in gemm_a4.hip and launches itself.
constexpr LinearKernel KERNELS[K_A4 - K_TILE_128][2] = {
    /* K_TILE_128  */ {{linear_kernel<bf16_t>, THREADS, 4 * TILE_BYTES}, {linear_kernel<float>, THREADS, 4 * TILE_BYTES}},
    /* K_RING      */ {{linear_kernel_256<bf16_t, 4, 4>, THREADS2, RING_LDS}, {linear_kernel_256<float, 4, 4>, THREADS2, RING_LDS}},
    /* K_RING_MID  */ {{linear_kernel_256<bf16_t, 2, 3>, 256, MID_LDS}, {}},
    /* K_PP        */ {{linear_kernel_256pp<false>, THREADS2, PP_LDS}, {}},
    /* K_PP_SPLITK */ {{linear_kernel_256pp<true>, THREADS2, PP_LDS}, {}},
};

// LinearArgs::vec_store of a checked call: 1 iff every row piece of C, C2 and the residual is 16-byte aligned.
int vec_store_of(const LinearCall& c) {
  const int es = c.es(), es2 = es == 4 ? 2 : 4;
  if (c.plane_stride) return ((uintptr_t)c.C % 16) == 0 ? 1 : 0;   // (rows of a plane are 128 bytes: ldc plays no part)
  bool vec = ((uintptr_t)c.C % 16) == 0 && (c.ldc * es) % 16 == 0;
  if (c.C2) vec = vec && ((uintptr_t)c.C2 % 16) == 0 && (c.ldc2 * es2) % 16 == 0;
  if (c.residual) vec = vec && ((uintptr_t)c.residual % 16) == 0 && (c.ldr * 4) % 16 == 0;
  return vec ? 1 : 0;
}

int launch_linear(const LinearCall& c, const LinearPlan& plan) {
  const int64_t M = c.M;
  const int N = c.N, K = c.K, es = c.es();
  const bool split = c.dtype == AURORA_F32 && c.mode >= 1, big = plan.bm == BM2;
  LinearArgs p;
  p.A = (const char*)c.A; p.lda_b = c.lda * es;
  p.W = (const char*)c.W; p.ldw_b = c.ldw * es;
  p.bias = c.bias;
  p.C = (char*)c.C; p.ldc = c.ldc; p.C2 = (char*)c.C2; p.ldc2 = c.ldc2;
  p.res = c.residual; p.ldr = c.ldr;
  p.M = M; p.N = N; p.k_tiles = (int)(((int64_t)K * es) / plan.rowb); p.act = c.act;
  p.tiles_n = (N + plan.bn - 1) / plan.bn;
  p.n_blocks = ((M + plan.bm - 1) / plan.bm) * p.tiles_n;
  p.vec_store = vec_store_of(c);
  if (split && big && c.act == AURORA_ACT_GELU) p.act = ACT_GELU_FAST;
  p.guard = split ? c.guard : nullptr;
  p.guard_limit = c.guard_limit;
  p.out_split = (c.pre & AURORA_F32_C_SPLIT) ? 1 : 0;
  AURORA_CHECK_ARG(p.n_blocks < (int64_t)1 << 31, "linear: too many tiles");

  p.bs_a = c.stride_a * es; p.bs_w = c.stride_w * es; p.bs_c = c.stride_c * es; p.bs_bias = c.stride_bias;
  p.split = plan.ksplit; p.slabs = plan.ksplit > 1 ? c.ws->slabs : nullptr; p.tickets = plan.ksplit > 1 ? c.ws->tickets : nullptr;
  p.plane_stride = c.plane_stride; p.plane_heads = c.plane_heads;
  once_per_device([] {
    for (const auto& row : KERNELS)
      for (const LinearKernel& k : row)
        if (k.fn) (void)hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes);
  });
  if (plan.kernel < F32_KERNELS) {   // gemm_f32.hip
    if (plan.kernel >= F32_PP) {   // linear_kernel_f32pp counts its own tiles: 128 x 256 (tall: 256 x 128), K-stages of 32
      const bool tall = plan.kernel >= F32_PP_W_TALL;
      LinearArgs q = p;
      q.k_tiles = K / 32;
      q.tiles_n = tall ? N / 128 : N / VN;
      q.n_blocks = tall ? ((M + 255) / 256) * q.tiles_n : ((M + VM - 1) / VM) * q.tiles_n;
      if (const int err = aurora_f32_launch(plan.kernel, &q, (unsigned)q.n_blocks, (unsigned)c.batch, c.stream)) return err;
    } else {
      if (const int err = aurora_f32_launch(plan.kernel, &p, (unsigned)p.n_blocks, (unsigned)c.batch, c.stream)) return err;
    }
    if (plan.twin) (void)aurora_f32_launch(F32_THREE, &p, (unsigned)p.n_blocks, (unsigned)c.batch, c.stream);
  } else if (plan.kernel == K_A4) {   // gemm_a4.hip
    (void)aurora_a4_launch(&p, (unsigned)p.n_blocks, (unsigned)c.batch, c.stream);
  } else {
    const LinearKernel& k = KERNELS[plan.kernel - K_TILE_128][c.dtype == AURORA_F32];
    // K_PP_SPLITK (batch 1): one workgroup per K-slice of a tile.  (Any other plan may carry a ksplit of 0 or 1.)
    const int64_t slices = plan.kernel == K_PP_SPLITK ? plan.ksplit : 1;
    const dim3 grid((unsigned)(p.n_blocks * slices), (unsigned)c.batch);
    hipLaunchKernelGGL(k.fn, grid, dim3(k.threads), k.lds_bytes, as_stream(c.stream), p);
  }
  return check_launch("linear");
}

// check arguments, choose kernel and tiling, fill LinearArgs and launch
int linear_impl(LinearCall c) {
  if (const int err = check_call(c)) return err;
  return launch_linear(c, plan_linear(c, device_cus()));
}

// The ids aurora_hip_linear_plan reports are this dispatcher's own.
static_assert(F32_THREE == AURORA_PLAN_F32_THREE && F32_TWO == AURORA_PLAN_F32_TWO && F32_PP == AURORA_PLAN_F32_PP &&
              F32_PP_W == AURORA_PLAN_F32_PP_W && F32_PP_AW == AURORA_PLAN_F32_PP_AW &&
              F32_PP_W_TALL == AURORA_PLAN_F32_PP_W_TALL && F32_PP_AW_TALL == AURORA_PLAN_F32_PP_AW_TALL &&
              K_TILE_128 == AURORA_PLAN_TILE128 && K_RING == AURORA_PLAN_RING && K_RING_MID == AURORA_PLAN_RING_MID &&
              K_PP == AURORA_PLAN_PP && K_PP_SPLITK == AURORA_PLAN_PP_SPLITK && K_A4 == AURORA_PLAN_A4,
              "include/aurora_hip.h: AURORA_PLAN_* out of step with the dispatcher's kernel ids");

// The call aurora_hip_linear's arguments describe; the other entry points add what is their own to it.
LinearCall plain_call(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C, int64_t ldc, void* C2,
                      int64_t ldc2, const float* residual, int64_t ldr, int64_t M, int N, int K, int dtype, int act, void* stream) {
  LinearCall c{A, lda, W, ldw, bias, C, ldc, M, N, K, dtype, stream, act};
  c.C2 = C2; c.ldc2 = ldc2; c.residual = residual; c.ldr = ldr;
  return c;
}
}  // namespace

extern "C" int aurora_hip_default_f32_gemm(void) { return default_f32_mode(); }

extern "C" int64_t aurora_hip_linear_workspace(int64_t M, int N, int K, int dtype) {
  if (dtype != AURORA_BF16 || M <= 0 || N <= 0 || K <= 0) return 0;
  const int s = choose_split(M, N, K, device_cus());
  return s <= 1 ? 0 : ((M + BM2 - 1) / BM2) * (N / BN2) * s * (int64_t)(BM2 * BN2 * 4);
}

extern "C" int aurora_hip_linear(const void* A, int64_t lda, const void* W, int64_t ldw,
                                 const float* bias, void* C, int64_t ldc, void* C2, int64_t ldc2,
                                 const float* residual, int64_t ldr, int64_t M, int N, int K,
                                 int dtype, int act, void* stream) {
  return aurora_hip_linear_ex(A, lda, W, ldw, bias, C, ldc, C2, ldc2, residual, ldr, M, N, K, dtype, act, -1, nullptr,
                              0.f, stream);
}

extern "C" int aurora_hip_linear_ex(const void* A, int64_t lda, const void* W, int64_t ldw,
                                    const float* bias, void* C, int64_t ldc, void* C2, int64_t ldc2,
                                    const float* residual, int64_t ldr, int64_t M, int N, int K,
                                    int dtype, int act, int f32_gemm, const float* guard, float guard_limit,
                                    void* stream) {
  LinearCall c = plain_call(A, lda, W, ldw, bias, C, ldc, C2, ldc2, residual, ldr, M, N, K, dtype, act, stream);
  c.f32_gemm = f32_gemm; c.guard = guard; c.guard_limit = guard_limit;
  return linear_impl(c);
}

extern "C" int aurora_hip_linear_planes(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C,
                                        int64_t plane_stride, int heads, int64_t M, int N, int K, int dtype, void* stream) {
  AURORA_CHECK_ARG(plane_stride > 0 && heads > 0, "linear_planes: plane_stride=%lld heads=%d", (long long)plane_stride, heads);
  LinearCall c = plain_call(A, lda, W, ldw, bias, C, N, nullptr, 0, nullptr, 0, M, N, K, dtype, AURORA_ACT_NONE, stream);
  c.plane_stride = plane_stride; c.plane_heads = heads;
  return linear_impl(c);
}

extern "C" int aurora_hip_linear_ws(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C,
                                    int64_t ldc, void* C2, int64_t ldc2, const float* residual, int64_t ldr, int64_t M, int N,
                                    int K, int dtype, int act, void* workspace, int64_t workspace_bytes, int32_t* tickets,
                                    int n_tickets, int split, void* stream) {
  AURORA_CHECK_ARG(workspace_bytes >= 0 && n_tickets >= 0 && split >= 0 && ((uintptr_t)workspace % 16) == 0,
                   "linear_ws: bad workspace arguments");
  const SplitWs ws{(float*)workspace, workspace ? workspace_bytes : 0, tickets, tickets ? n_tickets : 0, split};
  LinearCall c = plain_call(A, lda, W, ldw, bias, C, ldc, C2, ldc2, residual, ldr, M, N, K, dtype, act, stream);
  c.ws = &ws;
  return linear_impl(c);
}

extern "C" int aurora_hip_linear_batched(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* C,
                                         int64_t ldc, int64_t M, int N, int K, int dtype, int act, int f32_gemm,
                                         const float* guard, float guard_limit, int batch, int64_t stride_a,
                                         int64_t stride_w, int64_t stride_bias, int64_t stride_c, void* stream) {
  AURORA_CHECK_ARG(batch >= 1 && batch <= 65535, "linear_batched: 1 <= batch <= 65535 (got %d)", batch);
  const int es = dtype == AURORA_F32 ? 4 : 2;
  AURORA_CHECK_ARG((stride_a * es) % 16 == 0 && (stride_w * es) % 16 == 0 && (stride_c * es) % 16 == 0 && stride_bias % 4 == 0,
                   "linear_batched: batch strides must keep every problem 16-byte aligned");
  LinearCall c = plain_call(A, lda, W, ldw, bias, C, ldc, nullptr, 0, nullptr, 0, M, N, K, dtype, act, stream);
  c.f32_gemm = f32_gemm; c.guard = guard; c.guard_limit = guard_limit;
  c.batch = batch; c.stride_a = stride_a; c.stride_w = stride_w; c.stride_bias = stride_bias; c.stride_c = stride_c;
  return linear_impl(c);
}

// What linear_impl would launch for a call, without launching: check_call and plan_linear as the launch path runs them.
extern "C" int aurora_hip_linear_plan(int64_t M, int N, int K, int dtype, int f32_gemm, int has_guard, int batch, int64_t ldc,
                                      int64_t c_addr, int64_t ldc2, int64_t c2_addr, int64_t ldr, int64_t residual_addr,
                                      int64_t workspace_bytes, int n_tickets, int split, int64_t plane_stride, int plane_heads,
                                      int cus, int32_t* plan_out) {
  AURORA_CHECK_ARG(plan_out != nullptr && c_addr != 0 && cus >= 0 && batch >= 1, "linear_plan: bad query");
  // Operands as the tightest legal call has them (16-byte aligned, rows of K elements); of the output addresses only the
  // alignment is read.  The guard is never dereferenced here.
  static const float guard_word = 0.f;
  LinearCall c = plain_call((const void*)16, K, (const void*)16, K, nullptr, (void*)(uintptr_t)c_addr, ldc,
                            (void*)(uintptr_t)c2_addr, ldc2, (const float*)(uintptr_t)residual_addr, ldr, M, N, K, dtype,
                            AURORA_ACT_NONE, nullptr);
  c.f32_gemm = f32_gemm; c.guard = has_guard ? &guard_word : nullptr;
  c.batch = batch;
  const SplitWs ws{nullptr, workspace_bytes, nullptr, n_tickets, split};
  if (workspace_bytes >= 0) c.ws = &ws;
  c.plane_stride = plane_stride; c.plane_heads = plane_heads;
  if (const int err = check_call(c)) return err;
  const LinearPlan plan = plan_linear(c, cus > 0 ? cus : device_cus());
  const bool pp = plan.kernel >= F32_PP && plan.kernel < F32_KERNELS, tall = pp && plan.kernel >= F32_PP_W_TALL;
  plan_out[0] = plan.kernel;
  plan_out[1] = plan.twin ? 1 : 0;
  plan_out[2] = pp ? (tall ? 256 : VM) : plan.bm;    // (linear_kernel_f32pp counts its own tiles: launch_linear)
  plan_out[3] = pp ? (tall ? 128 : VN) : plan.bn;
  plan_out[4] = plan.ksplit;
  plan_out[5] = vec_store_of(c);
  return AURORA_OK;
}
