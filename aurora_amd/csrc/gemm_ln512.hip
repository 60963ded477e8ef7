// Fused bf16 linear + (adaptive) LayerNorm + residual for rows of 512 (aurora_hip_linear_layernorm, at the end).
#include "gemm_tile.h"

namespace aurora {

namespace {

// =================================================================================================
// bf16 linear + (adaptive) LayerNorm + residual in one launch, for D = 512 (stage 0 of the backbone):
//     x_out = x_in + LN(A W^T + bias) * gain + shift,   shadow = bf16(x_out)
// i.e. `x = shortcut + norm(proj(...), c)` / `x = x + norm(mlp(x), c)` of a Swin block (swin3d.py:507-508, film.py:38-49)
// without the bf16 round trip of the linear's result through HBM (2 of the 14 bytes per element the linear + LayerNorm
// pair moves) and without the second launch.  A workgroup must own whole rows: the tile is 128 x 512 -- 8 waves as
// 2 (m) x 4 (n), wave tile 64 x 128 (128 accumulator registers, the same as the 128 x 64 tile of the square kernels),
// K-stages of 64 bytes per row (8 KiB of activations + 32 KiB of weights), three-stage ring, ping-pong schedule.
// Epilogue: bias, rounding to bf16 (the reference's linear yields bf16 under autocast; statistics are taken of the
// rounded values, as the separate kernels do), two-pass fp32 row statistics (lane -> 4 lane groups by permlane swaps ->
// 4 waves through LDS), then 16 rows at a time through LDS so that every global access of the residual stream covers
// whole cache lines: a lane reads 4 consecutive features of a row, normalises, adds the fp32 residual, writes fp32 and
// bf16.  D = 1024 / 2048 would need 64 / 32-row tiles (fetch-bound) or a cross-workgroup statistics exchange: not built.
// =================================================================================================
constexpr int FM = 128, FN = 512, FTHREADS = 512, FNST = 3;
constexpr int FOPER_X = FM * ROW2, FOPER_W = FN * ROW2, FSTAGE = FOPER_X + FOPER_W;   // 8 + 32 = 40 KiB

struct LinearLnArgs {
  const char* A; int64_t lda_b; const char* W; int64_t ldw_b;
  const float* bias; const float* gain; const float* shift;
  const float* x_in; int64_t ldx; float* x_out; int64_t ldo; bf16_t* xb; int64_t ldb;
  int64_t M; int k_tiles; float eps;
  int64_t tile0;   // first tile of this launch
};

__device__ __forceinline__ float group4_sum(float v) {   // over the 4 lane groups (lanes l, l^16, l^32, l^48)
  typedef uint32_t u32x2_sw __attribute__((ext_vector_type(2)));
  u32x2_sw r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(r.x) + __uint_as_float(r.y);
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r.x) + __uint_as_float(r.y);
}

template <bool FULL>   // FULL: every row of every tile of the launch exists
__global__ __launch_bounds__(FTHREADS, 2) void linear_ln512_kernel(const LinearLnArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;   // waves w and w+4 share a SIMD; wm = 1 runs one phase behind
  const int64_t m0 = (p.tile0 + blockIdx.x) * FM;
  // (Do the CUs of a launch run in lockstep -- every main loop at once with HBM idle, then every epilogue at once?  Holding
  // the first-round workgroups of every other CU back by 8 ... 55 us changed nothing but the delay itself,
  // profiles/r04_ab_ln512_stagger.log: a CU's epilogue is as fast as the bytes it keeps in flight allow, whatever its
  // neighbours do.)
  const char* src_x;
  const char* src_w[4];
  {
    const int row = tid >> 2, c = tid & 3;
    int64_t gm = m0 + row;
    gm = gm < p.M ? gm : p.M - 1;
    src_x = p.A + gm * p.lda_b + piece_x(row, c);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int id = r * FTHREADS + tid;
    const int row = id >> 2, c = id & 3;
    src_w[r] = p.W + (int64_t)row * p.ldw_b + piece_w(row, c);
  }
  auto stage = [&](int kt) {
    const int64_t koff = (int64_t)kt * ROW2;
    char* base = smem + (kt % FNST) * FSTAGE;
    dma16(src_x + koff, base + (wave * 64) * 16);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dma16(src_w[r] + koff, base + FOPER_X + (r * FTHREADS + wave * 64) * 16);
  };
  const int i16 = lane & 15, g = lane >> 4;
  int off_x[4], off_w[8];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int row = wm * 64 + 16 * f + i16;
    off_x[f] = row * ROW2 + piece_x(row, g);
  }
#pragma unroll
  for (int f = 0; f < 8; ++f) {   // weight rows interleaved so that a lane ends up with 32 CONSECUTIVE output features
    const int row = wn * 128 + 32 * (i16 >> 2) + 4 * f + (i16 & 3);
    off_w[f] = FOPER_X + row * ROW2 + piece_w(row, g);
  }
  f32x4 acc[8][4];  // [fn][fm]: features wn*128 + 32g + 4fn .. +3 of row wm*64 + 16fm + i16
  zero_acc(acc);
  const int nt = p.k_tiles;   // >= 3 (dispatch)
  stage(0);
  stage(1);
  stage(2);
  asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  __builtin_amdgcn_s_barrier();   // stage 0 is complete
  asm volatile("" ::: "memory");
  if (wm == 1) __builtin_amdgcn_s_barrier();   // the late half: one phase behind from here on

  for (int s = 0; s < nt; ++s) {
    u32x4 fw[8], fx[4];
    {
      const char* buf = smem + (s % FNST) * FSTAGE;
#pragma unroll
      for (int f = 0; f < 8; ++f) fw[f] = *reinterpret_cast<const u32x4*>(buf + off_w[f]);
#pragma unroll
      for (int f = 0; f < 4; ++f) fx[f] = *reinterpret_cast<const u32x4*>(buf + off_x[f]);
    }
    if (s >= 1 && s + 2 < nt) stage(s + 2);   // into the buffer of stage s-1
    if (s + 2 < nt) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");   // own pieces of stage s+1 have landed
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int fn = 0; fn < 8; ++fn) acc[fn][fm] = Mma<bf16_t>::run(fw[fn], fx[fm], acc[fn][fm]);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();   // the early half waits for the late half's last phase: the ring is dead
  asm volatile("" ::: "memory");

  // ---- epilogue.  Where a tile's time goes (profiles/r04_ln512_phases.log, K = 512: 40 us): prologue 3.3, main loop
  // 15.6, residual requests + bias + rounding 4-6, statistics 2-4, the four passes 12-13.  Every global address below is
  // a UNIFORM base (scalar arithmetic: tile, wave, pass, row pair) plus one per-lane 32-bit offset computed once, and whole
  // tiles run without row predicates: 64-bit per-row multiplies and clamps were a quarter of the epilogue's ~3,000
  // instructions per wave (profiles/r04_ln512_pmc.log).  That bought 1 % (r04_ab_ln512_addressing.log): the epilogue
  // waits for memory, not for the VALU -- without the residual reads a K = 512 launch takes 318 instead of 385 us, without
  // the stores 272, without both 234 (r04_ln512_probe_no_residual_no_store.log).  Normalising in the MFMA layout with
  // packed arithmetic (a lane holds its rows' statistics there) needs ~40 registers more than the 256 there are.
  const int L = lane & 31, half = lane >> 5;
  const int col = wn * 128 + 4 * L;
  // rows of this tile that exist, counted from this wave's first row (uniform; FULL: all of them, nothing is predicated):
  // row r of the wave (r = 16 fm + 2 j + half) exists iff r < wave_rows
  const int wave_rows = FULL ? 64 : (int)(p.M - m0 < FM ? p.M - m0 : FM) - wm * 64;
  const uint32_t lane_x = (uint32_t)((half * p.ldx + col) * 4);
  const uint32_t lane_o = (uint32_t)((half * p.ldo + col) * 4);
  const uint32_t lane_b = (uint32_t)((half * p.ldb + col) * 2);
  const char* const x_wave = reinterpret_cast<const char*>(p.x_in) + (m0 + wm * 64) * p.ldx * 4;
  char* const o_wave = reinterpret_cast<char*>(p.x_out) + (m0 + wm * 64) * p.ldo * 4;
  char* const b_wave = reinterpret_cast<char*>(p.xb) + (m0 + wm * 64) * p.ldb * 2;
  // The residual rows of the first two 16-row passes are requested NOW, before bias / rounding / the two statistics passes:
  // nothing they need depends on the product, and the statistics hide their HBM round trip.
  f32x4 xr[3][8];
  auto fetch_x = [&](int fm, f32x4 (&dst)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = 16 * fm + 2 * j;   // (uniform: scalar address arithmetic)
      if constexpr (!FULL) dst[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (FULL || r + half < wave_rows) dst[j] = *reinterpret_cast<const f32x4*>(x_wave + (int64_t)(r * (int)p.ldx) * 4 + lane_x);
    }
  };
  fetch_x(0, xr[0]);
  fetch_x(1, xr[1]);
  // ---- bias, rounding to bf16 ----
  const int nb = wn * 128 + 32 * g;
#pragma unroll
  for (int fn = 0; fn < 8; ++fn) {
    const f32x4 b4 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + nb + 4 * fn) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int fm = 0; fm < 4; ++fm) {
      const uint32_t lo = pack_bf16x2(acc[fn][fm].x + b4.x, acc[fn][fm].y + b4.y);
      const uint32_t hi = pack_bf16x2(acc[fn][fm].z + b4.z, acc[fn][fm].w + b4.w);
      acc[fn][fm] = f32x4{__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
                          __uint_as_float(hi & 0xffff0000u)};
    }
  }
  // ---- row statistics: two passes over the registers; partial sums of the four n-waves meet in LDS ----
  float* const st_sum = reinterpret_cast<float*>(smem + 65536);   // [128 rows][4 n-waves]
  float* const st_sq = st_sum + 512;
  float* const st_mr = st_sq + 512 + wave * 128;                  // this wave's own copy: [64 rows][mean, rstd]
  float mean[4], rstd[4];
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    float t = 0.f;
#pragma unroll
    for (int fn = 0; fn < 8; ++fn) t += (acc[fn][fm].x + acc[fn][fm].y) + (acc[fn][fm].z + acc[fn][fm].w);
    t = group4_sum(t);
    if (g == 0) st_sum[(wm * 64 + 16 * fm + i16) * 4 + wn] = t;
  }
  __syncthreads();
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(st_sum + (wm * 64 + 16 * fm + i16) * 4);
    mean[fm] = ((t.x + t.y) + (t.z + t.w)) * (1.0f / FN);
    float q = 0.f;
#pragma unroll
    for (int fn = 0; fn < 8; ++fn) {
      const float d0 = acc[fn][fm].x - mean[fm], d1 = acc[fn][fm].y - mean[fm], d2 = acc[fn][fm].z - mean[fm],
                  d3 = acc[fn][fm].w - mean[fm];
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    q = group4_sum(q);
    if (g == 0) st_sq[(wm * 64 + 16 * fm + i16) * 4 + wn] = q;
  }
  __syncthreads();
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(st_sq + (wm * 64 + 16 * fm + i16) * 4);
    rstd[fm] = rsqrtf(((t.x + t.y) + (t.z + t.w)) * (1.0f / FN) + p.eps);
    if (g == 0) {
      st_mr[(16 * fm + i16) * 2] = mean[fm];
      st_mr[(16 * fm + i16) * 2 + 1] = rstd[fm];
    }
  }
  // ---- 16 rows at a time through this wave's 8 KiB: [16 rows][32 pieces of 16 B], piece P of row r at P ^ c(r) with
  //      c(r) = r ^ 2 (r >> 2): conflict-free for the b128 writes (a lane writes pieces 8g..8g+7 of row i16) and for the
  //      row-major b128 reads (two rows per instruction) under gfx950's 16-lane service groups ----
  char* const mine = smem + wave * 8192;
  f32x4 gn = f32x4{1.f, 1.f, 1.f, 1.f}, sh = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p.gain) gn = *reinterpret_cast<const f32x4*>(p.gain + col);
  if (p.shift) sh = *reinterpret_cast<const f32x4*>(p.shift + col);
  const int cw = (i16 ^ ((i16 >> 2) << 1)) & 31;
  // The residual rows of a 16-row pass are fetched ahead of it, all eight loads of a lane at once: x_out may alias x_in, so
  // a load written behind the previous row's store would have to wait for it -- 32 exposed round trips per tile.  TWO
  // passes ahead (round 4; one before): the 32 accumulator registers a pass has parked in LDS are free from there on, so
  // the third buffer costs no register the main loop needs, and the epilogue is a latency chain on 8 waves -- the bytes
  // in flight are what its bandwidth is made of.
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
#pragma unroll
    for (int q = 0; q < 8; ++q) *reinterpret_cast<f32x4*>(mine + i16 * 512 + (((8 * g + q) ^ cw) << 4)) = acc[q][fm];
    if (fm + 2 < 4) fetch_x(fm + 2, xr[(fm + 2) % 3]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r16 = 2 * j + half;
      const int cr = (r16 ^ ((r16 >> 2) << 1)) & 31;
      const f32x4 v = *reinterpret_cast<const f32x4*>(mine + r16 * 512 + ((L ^ cr) << 4));
      const float mu = st_mr[(16 * fm + r16) * 2], rs = st_mr[(16 * fm + r16) * 2 + 1];
      const f32x4 x = xr[fm % 3][j];
      f32x4 o;
      o.x = fmaf((v.x - mu) * rs, gn.x, sh.x) + x.x;
      o.y = fmaf((v.y - mu) * rs, gn.y, sh.y) + x.y;
      o.z = fmaf((v.z - mu) * rs, gn.z, sh.z) + x.z;
      o.w = fmaf((v.w - mu) * rs, gn.w, sh.w) + x.w;
      const int rr = 16 * fm + 2 * j;   // (uniform: scalar address arithmetic)
      if (FULL || rr + half < wave_rows) {
        *reinterpret_cast<f32x4*>(o_wave + (int64_t)(rr * (int)p.ldo) * 4 + lane_o) = o;
        if (p.xb)
          *reinterpret_cast<u32x2*>(b_wave + (int64_t)(rr * (int)p.ldb) * 2 + lane_b) = u32x2{pack_bf16x2(o.x, o.y), pack_bf16x2(o.z, o.w)};
      }
    }
  }
}

}  // namespace

}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_linear_layernorm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                                           const float* gain, const float* shift, const float* x_in, int64_t ldx,
                                           float* x_out, int64_t ldo, void* x_bf16, int64_t ldb, int64_t M, int N, int K,
                                           float eps, void* stream) {
  AURORA_CHECK_ARG(N == FN, "linear_layernorm: N=%d (only D = 512 rows are owned by one workgroup)", N);
  AURORA_CHECK_ARG(M > 0 && K % 32 == 0 && K >= 96, "linear_layernorm: K=%d must be a multiple of 32, >= 96", K);
  AURORA_CHECK_ARG(A && W && x_in && x_out && lda >= K && ldw >= K && (lda * 2) % 16 == 0 && (ldw * 2) % 16 == 0 &&
                       ((uintptr_t)A % 16) == 0 && ((uintptr_t)W % 16) == 0,
                   "linear_layernorm: operand strides / alignment");
  AURORA_CHECK_ARG(ldx >= N && ldo >= N && ldx % 4 == 0 && ldo % 4 == 0 && ((uintptr_t)x_in % 16) == 0 &&
                       ((uintptr_t)x_out % 16) == 0 && (!x_bf16 || (ldb >= N && ldb % 4 == 0 && ((uintptr_t)x_bf16 % 8) == 0)),
                   "linear_layernorm: residual / output strides / alignment");
  AURORA_CHECK_ARG((!bias || ((uintptr_t)bias % 16) == 0) && (!gain || ((uintptr_t)gain % 16) == 0) &&
                       (!shift || ((uintptr_t)shift % 16) == 0), "linear_layernorm: unaligned bias / gain / shift");
  LinearLnArgs p{(const char*)A, lda * 2, (const char*)W, ldw * 2, bias, gain, shift, x_in, ldx, x_out, ldo, (bf16_t*)x_bf16, ldb,
                 M, K / 32, eps, 0};
  once_per_device([] {
    (void)hipFuncSetAttribute((const void*)linear_ln512_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, FNST * FSTAGE);
    (void)hipFuncSetAttribute((const void*)linear_ln512_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, FNST * FSTAGE);
  });
  // whole tiles by the kernel without row predicates; the ragged last tile, if any, by its own one-workgroup launch
  const int64_t whole = M / FM;
  AURORA_CHECK_ARG(whole < (int64_t)1 << 31, "linear_layernorm: too many tiles");
  if (whole > 0)
    hipLaunchKernelGGL(linear_ln512_kernel<true>, dim3((unsigned)whole), dim3(FTHREADS), FNST * FSTAGE, as_stream(stream), p);
  if (M % FM != 0) {
    p.tile0 = whole;
    hipLaunchKernelGGL(linear_ln512_kernel<false>, dim3(1), dim3(FTHREADS), FNST * FSTAGE, as_stream(stream), p);
  }
  return check_launch("linear_layernorm");
}
