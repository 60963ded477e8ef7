// Encoder front end / decoder back end kernels (all HBM-bound, fp32 pixels on one side):
//   * patchify            : Batch.normalise + pre-encoder transforms + unfold into the patch-embed
//                           GEMM operand (LevelPatchEmbed's conv3d == GEMM over unfolded patches)
//   * assemble_tokens     : surface/latent concat + position/scale/time embeddings
//   * unpatchify          : head outputs -> (B, V, C, H, W) fields, clamp + Batch.unnormalise fused
// (The Perceiver attentions that run between them are perceiver_attention.hip.)
#include <math.h>

#include "common.h"

namespace aurora {
namespace {

// ------------------------------------------------------------------------------------------------
// patchify
// ------------------------------------------------------------------------------------------------
constexpr int MAX_VARS = 32;

struct PatchVar {
  const float* src; int64_t sb, st, sc, sh, sw;
  const float* loc; const float* inv_scale;
  int32_t transform; float tw0, tw1, tb;
};
struct PatchArgs {
  PatchVar v[MAX_VARS];
  void* out; int64_t Kpad; int k_offset; int K_total;
  int n_vars, B, T, n_lvl, Hp, Wp, P;
  float* absmax;   // nullable: max |value written| is folded into this word (non-negative floats order like their bits)
};

// max over the wave, then at most one atomic per wave -- and only if it can still raise the word (a relaxed look first):
// the guard word of the encoder's operand-split decision (step.hip) costs the producer of the values nothing but this,
// where a separate absmax pass re-read all of them (0.6 GB per step at 0.25 degree).
__device__ __forceinline__ void fold_absmax(float* word, float m) {
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) {
    const unsigned int bits = __float_as_uint(m);
    if (bits > __hip_atomic_load(reinterpret_cast<unsigned int*>(word), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(reinterpret_cast<unsigned int*>(word), bits);
  }
}

__device__ __forceinline__ float patch_transform(float z, const PatchVar& d) {
  if (d.transform == 1) return fmaxf(z, 0.f);
  if (d.transform == 2) {
    // reference aurora.py:733-742: Linear(2,1)([clamp(z,0,2.5), (log(max(z,eps)) - log eps) / -log eps])
    z = fmaxf(z, 0.f);  // positive variables are clamped at 0 before the hook (aurora.py:301-317)
    const float eps = 1e-4f, log_eps = -9.210340371976182f;  // log(1e-4)
    const float f0 = fminf(z, 2.5f);
    const float f1 = (logf(fmaxf(z, eps)) - log_eps) / (-log_eps);
    return d.tw0 * f0 + d.tw1 * f1 + d.tb;
  }
  // ocean-wave variant (reference aurora.py:892-912): missing values are NaN in the input
  if (d.transform == 3) return isnan(z) ? 0.f : 1.f;                       // density channel
  if (d.transform == 4) return isnan(z) ? 0.f : z;                         // value, nan_to_num(0)
  if (d.transform == 5) { const float r = sinf(z * 0.017453292519943295f); return isnan(r) ? 0.f : r; }
  if (d.transform == 6) { const float r = cosf(z * 0.017453292519943295f); return isnan(r) ? 0.f : r; }
  return z;
}

// Patch size 4, fp32, every piece 16-byte aligned (the 0.25-degree models).  A workgroup owns a run of 8 * PATCH4_GROUPS
// patches of one patch row at one level; lane = (piece q = (variable, time, image row i) of the output row, patch s of 8):
// the eight lanes of a q read 128 contiguous bytes of one image row of one field, the eight q of an s write 128 contiguous
// bytes of one output row -- whole cache lines on both sides, the position decoded once per PATCH4_GROUPS pieces.  (The
// first form, one thread per piece in output order, decoded a flat 64-bit index with six 64-bit divisions: ~700 VALU
// instructions per 16 bytes, 0.27 ms per launch where the bytes take 0.09.)
constexpr int PATCH4_GROUPS = 4;

__global__ __launch_bounds__(1024) void patchify_kernel(const PatchArgs p) {
  // grid: x = run of 8 * PATCH4_GROUPS patches, y = patch row, z = (level, batch); blockDim = 8 * pieces per row, rounded up
  const int q_per_row = p.n_vars * p.T * 4;
  const int q = (int)(threadIdx.x >> 3);
  float m = 0.f;
  if (q < q_per_row) {
    const int i = q & 3, vt = q >> 2;
    const int v = vt / p.T, t = vt - v * p.T;
    const unsigned hp = blockIdx.y;
    const unsigned c = blockIdx.z / (unsigned)p.B, b = blockIdx.z - c * (unsigned)p.B;
    const int wp = (int)(blockIdx.x * (8u * PATCH4_GROUPS) + (threadIdx.x & 7u));
    const PatchVar& d = p.v[v];
    const float loc = d.loc[c], inv = d.inv_scale[c];
    const float* src = d.src + b * d.sb + t * d.st + c * d.sc + (int64_t)(hp * 4 + i) * d.sh + (int64_t)wp * 4;   // (stride_w == 1)
    const int64_t row = ((int64_t)blockIdx.z * p.Hp + hp) * p.Wp + wp;   // rows are (level, batch, patch)
    float* out_row = reinterpret_cast<float*>(p.out) + row * p.Kpad;
    float* dst = out_row + p.k_offset + q * 4;
    // the K padding of a row is zeroed by the thread of its last piece, if this call ends the row
    const bool pads = q == q_per_row - 1 && p.k_offset + q_per_row * 4 == p.K_total;
    f32x4 z[PATCH4_GROUPS];
#pragma unroll
    for (int g = 0; g < PATCH4_GROUPS; ++g)
      if (wp + 8 * g < p.Wp) z[g] = *reinterpret_cast<const f32x4*>(src + 32 * g);
#pragma unroll
    for (int g = 0; g < PATCH4_GROUPS; ++g)
      if (wp + 8 * g < p.Wp) {
        const f32x4 r4 = f32x4{patch_transform((z[g].x - loc) * inv, d), patch_transform((z[g].y - loc) * inv, d),
                               patch_transform((z[g].z - loc) * inv, d), patch_transform((z[g].w - loc) * inv, d)};
        *reinterpret_cast<f32x4*>(dst + 8 * g * p.Kpad) = r4;
        m = fmaxf(m, fmaxf(fmaxf(fabsf(r4.x), fabsf(r4.y)), fmaxf(fabsf(r4.z), fabsf(r4.w))));
        if (pads)
          for (int64_t k = p.K_total; k < p.Kpad; ++k) out_row[8 * g * p.Kpad + k] = 0.f;
      }
  }
  if (p.absmax) fold_absmax(p.absmax, m);
}

// Any patch size (10 at 0.1 degree, 3 for the air-pollution model): one thread per OUTPUT element, consecutive threads on
// consecutive columns k = (v, t, i, j) of one patch's row of the GEMM operand -- every store instruction of a wave writes
// 256 contiguous bytes; the loads are runs of P pixels per image row (the neighbouring patches, handled by the next rows'
// threads, use the rest of those cache lines out of L1 / L2).  The first form gave a thread one P-value piece and looped
// over it (one 4-byte load per lane and instruction, 64 cache lines each: 1.1 TB/s on the 0.1-degree grid); a
// pixel-per-thread form with coalesced loads and scattered 40-byte stores was no faster: partial-line WRITES are what hurts.
// An LDS-staged form (a workgroup loads span * P pixel runs of all planes of `span` adjacent patches coalesced, parks them in
// LDS, then writes each patch's columns as one contiguous piece through a column -> LDS-word table) measured SLOWER on both
// grids, 5.5 vs 4.4 ms at 0.1 degree and 2.2 vs 1.8 ms at 0.4 degree, with eight loads in flight per lane slower still: the
// two phases of a workgroup do not overlap and 48 KiB of staging leaves three workgroups per CU to hide them.
// What bounded that form was neither: ~200 VALU instructions per 4-byte element (five 32-bit divisions to decode the
// column, a wave reduction for the range word) -- 14 M wave passes of 200 x 4 cycles are the 4.4 ms.  A thread now decodes
// its column ONCE and walks PATCH_SPAN patches along the latitude circle with it (source += P pixels, destination += one
// row): ~12 instructions per element, PATCH_SPAN independent loads in flight, one range-word reduction per thread.
constexpr int PATCH_SPAN = 16;   // 16 patches x 10 pixels = 640 B of every image row: whole cache lines at 0.1 degree

template <typename T>
__global__ __launch_bounds__(256) void patchify_cols_kernel(const PatchArgs p, const int k_end, const int chunks) {
  // grid: x = (group of PATCH_SPAN patch columns, 256-column chunk of the row), y = patch row, z = (level, batch) -- 32-bit
  // index arithmetic only.  k runs over this call's columns [k_offset, k_end): its variables, plus the zero padding if the
  // call ends at K_total.
  const int n_k = k_end - p.k_offset;
  const unsigned g = blockIdx.x / (unsigned)chunks, chunk = blockIdx.x - g * (unsigned)chunks;
  const int kk = (int)(chunk * 256u + threadIdx.x);
  const unsigned wp0 = g * (unsigned)PATCH_SPAN;
  const int n = min(PATCH_SPAN, p.Wp - (int)wp0);
  float m = 0.f;
  if (kk < n_k) {
    const unsigned hp = blockIdx.y;
    const unsigned c = blockIdx.z / (unsigned)p.B, b = blockIdx.z - c * (unsigned)p.B;
    const int64_t row = ((int64_t)blockIdx.z * p.Hp + hp) * p.Wp + wp0;   // rows are (level, batch, patch)
    T* dst = reinterpret_cast<T*>(p.out) + row * p.Kpad + p.k_offset + kk;
    const unsigned PP = (unsigned)(p.P * p.P);
    const unsigned vt = (unsigned)kk / PP;
    if ((int)vt >= p.n_vars * p.T) {   // K padding
      for (int s = 0; s < n; ++s) elem<T>::store(dst + s * p.Kpad, 0.f);
    } else {
      const unsigned ij = (unsigned)kk - vt * PP;
      const unsigned i = ij / (unsigned)p.P, j = ij - i * (unsigned)p.P;
      const unsigned v = vt / (unsigned)p.T, t = vt - v * (unsigned)p.T;
      const PatchVar& d = p.v[v];
      const float* src = d.src + b * d.sb + t * d.st + c * d.sc + (int64_t)(hp * p.P + i) * d.sh + (int64_t)(wp0 * p.P + j) * d.sw;
      const int64_t step = (int64_t)p.P * d.sw;
      const float loc = d.loc[c], inv = d.inv_scale[c];
      float z[PATCH_SPAN];
#pragma unroll
      for (int s = 0; s < PATCH_SPAN; ++s)
        if (s < n) z[s] = src[s * step];
#pragma unroll
      for (int s = 0; s < PATCH_SPAN; ++s)
        if (s < n) {
          const float r = patch_transform((z[s] - loc) * inv, d);
          elem<T>::store(dst + s * p.Kpad, r);
          m = fmaxf(m, fabsf(r));
        }
    }
  }
  if (p.absmax) fold_absmax(p.absmax, m);
}

// ------------------------------------------------------------------------------------------------
// assemble tokens
// ------------------------------------------------------------------------------------------------
struct AsmArgs {
  const float* surf; const float* agg; const float* pos_scale; const float* time_emb;
  float* out_f32; void* out_t; int B, Cl; int64_t L; int D;
};

template <typename T>
__global__ __launch_bounds__(256) void assemble_kernel(const AsmArgs p) {
  const int pieces = p.D >> 3;
  const int64_t total = (int64_t)p.B * p.Cl * p.L * pieces;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += stride) {
    const int e = (int)(it % pieces) * 8;
    const int64_t tokn = it / pieces;        // (b, c, l)
    const int64_t l = tokn % p.L;
    const int c = (int)((tokn / p.L) % p.Cl);
    const int b = (int)(tokn / (p.L * p.Cl));
    float v[8], a[8];
    if (c == 0) load8(p.surf + ((int64_t)b * p.L + l) * p.D + e, v);
    else load8(p.agg + (((int64_t)b * p.L + l) * (p.Cl - 1) + (c - 1)) * p.D + e, v);
    load8(p.pos_scale + l * p.D + e, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += a[j];
    load8(p.time_emb + (int64_t)b * p.D + e, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += a[j];
    store8(p.out_f32 + tokn * p.D + e, v);
    if (p.out_t) store8(reinterpret_cast<T*>(p.out_t) + tokn * p.D + e, v);
  }
}

// ------------------------------------------------------------------------------------------------
// unpatchify
// ------------------------------------------------------------------------------------------------
struct UnpatchVar {
  float* dst; const float* loc; const float* scale; int32_t clamp_min0, col0, lvl_stride, mod_col0;
  const float* prev; int64_t prev_sb, prev_sc, prev_sh; const float* inv_scale; uint32_t clamp_max1_levels;
  int32_t angle_col0, dens_col0; const float* mask; int64_t mask_sh; float mask_thresh;
};
struct UnpatchArgs {
  UnpatchVar v[MAX_VARS];
  const float* y; int64_t ldy; int n_vars, B, n_lvl, Hp, Wp, P;
  int vec4;   // P == 4 and every source / destination piece is 16-byte aligned
};

// VEC = 4: patch size 4, every piece 16-byte aligned.  A workgroup owns a run of 8 * UNPATCH_GROUPS patches of one patch
// row at one level; lane = (piece q = (variable, image row i) of the head row, patch s of 8): the eight lanes of a q write
// 128 contiguous bytes of one image row of one field, the eight q of an s read 128 contiguous bytes of one head row --
// whole cache lines on both sides.  (One thread per piece in (variable, ..., patch) order read a 16-byte piece per line and
// instruction and came back for the rest of each line a variable later: the head outputs crossed the fabric up to eight
// times, 0.38 ms per step where the bytes take 0.1, and six 64-bit divisions per thread did not help.)
// VEC = 1: any patch size: a thread owns one pixel COLUMN of a patch row -- consecutive threads on consecutive longitudes,
// so that every store of a wave writes 256 contiguous bytes of the output field -- and walks the P image rows of that
// patch row with it (head outputs += P, field += one image row): its position is decoded once per P pixels, and the
// P x P head outputs of a patch, one contiguous run, are used up by the same wave while they sit in L1.
constexpr int UNPATCH_GROUPS = 4;

template <int VEC>
__global__ __launch_bounds__(VEC == 4 ? 1024 : 256) void unpatchify_kernel(const UnpatchArgs p) {
  int v, wp, j0, i, hp, c, b;
  if constexpr (VEC == 4) {
    // grid: x = run of 8 * UNPATCH_GROUPS patches, y = patch row, z = (batch, level)
    const int q = (int)(threadIdx.x >> 3);
    if (q >= p.n_vars * 4) return;
    v = q >> 2; i = q & 3; j0 = 0;
    wp = (int)(blockIdx.x * (8u * UNPATCH_GROUPS) + (threadIdx.x & 7u));
    hp = (int)blockIdx.y;
    b = (int)(blockIdx.z / (unsigned)p.n_lvl); c = (int)(blockIdx.z - (unsigned)b * (unsigned)p.n_lvl);
  } else {
    // grid: x = 256-pixel chunk of an image row, y = patch row, z = (variable, batch, level): 32-bit index arithmetic only
    const unsigned x = blockIdx.x * 256u + threadIdx.x;
    if (x >= (unsigned)(p.Wp * p.P)) return;
    wp = (int)(x / (unsigned)p.P); j0 = (int)(x - (unsigned)wp * (unsigned)p.P);
    hp = (int)blockIdx.y; i = 0;
    const unsigned vb = blockIdx.z / (unsigned)p.n_lvl;
    c = (int)(blockIdx.z - vb * (unsigned)p.n_lvl);
    v = (int)(vb / (unsigned)p.B); b = (int)(vb - (unsigned)v * (unsigned)p.B);
  }
  const UnpatchVar& d = p.v[v];
  const int64_t L = (int64_t)p.Hp * p.Wp;
  const int64_t W = (int64_t)p.Wp * p.P, H = (int64_t)p.Hp * p.P;
  const float loc = d.loc[c], sc = d.scale[c];
  const bool has_mod = d.mod_col0 >= 0;
  const float inv = has_mod ? d.inv_scale[c] : 0.f;
  const bool cap1 = (d.clamp_max1_levels >> c) & 1u;
  // everything of patch column `wp` (image rows hp * P + i ...)
  auto patch = [&](int wp) {
    const float* row = p.y + (((int64_t)b * L + (int64_t)hp * p.Wp + wp) * p.n_lvl + c) * p.ldy + c * d.lvl_stride + i * p.P;
    const float* src = row + d.col0;
    const int64_t hh = (int64_t)hp * p.P + i, ww = (int64_t)wp * p.P;
    float* dst = d.dst + (((int64_t)b * p.n_lvl + c) * H + hh) * W + ww;
    const float* mod = row + (has_mod ? d.mod_col0 : 0);
    const float* prev = has_mod ? d.prev + b * d.prev_sb + c * d.prev_sc + hh * d.prev_sh + ww : nullptr;
    const float* cosp = d.angle_col0 >= 0 ? row + d.angle_col0 : nullptr;   // wave: col0 = sin head, this = cos head
    const float* dens = d.dens_col0 >= 0 ? row + d.dens_col0 : nullptr;     // wave: density head
    const float* maskp = dens ? d.mask + hh * d.mask_sh + ww : nullptr;     // raw water-body mask plane
    // j indexes the head outputs; the fields' own rows are prev_sh / mask_sh apart, not P (VEC = 1 walks image rows)
    auto finish = [&](float z, int j, int64_t prev_j, int64_t mask_j) -> float {
      if (has_mod) z = z + (1.0f + mod[j]) * ((prev[prev_j] - loc) * inv);
      if (cap1) z = fminf(z, 1.0f);
      if (d.clamp_min0) z = fmaxf(z, 0.f);
      if (cosp) {  // direction from its sin / cos heads: rad2deg(atan2(sin, cos)) mod 360 in [0, 360)
        z = atan2f(z, cosp[j]) * 57.29577951308232f;
        z = fmodf(z, 360.0f);
        if (z < 0.f) z += 360.0f;
      }
      if (dens) {  // present only over water AND where sigmoid(density) >= 0.5 (aurora.py:924-930)
        const bool water = maskp[mask_j] > d.mask_thresh;
        z = (water && !(dens[j] < 0.f)) ? z : __int_as_float(0x7fc00000);
      }
      return z * sc + loc;
    };
    if constexpr (VEC == 4) {
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(src);
      *reinterpret_cast<f32x4*>(dst) = f32x4{finish(s4.x, 0, 0, 0), finish(s4.y, 1, 1, 1), finish(s4.z, 2, 2, 2), finish(s4.w, 3, 3, 3)};
    } else {
      for (int ii = 0; ii < p.P; ++ii) {
        const int j = ii * p.P + j0;
        dst[ii * W + j0] = finish(src[j], j, has_mod ? ii * d.prev_sh + j0 : 0, dens ? ii * d.mask_sh + j0 : 0);
      }
    }
  };
  if constexpr (VEC == 4) {
#pragma unroll
    for (int g = 0; g < UNPATCH_GROUPS; ++g)
      if (wp + 8 * g < p.Wp) patch(wp + 8 * g);
  } else {
    patch(wp);
  }
}

}  // namespace
}  // namespace aurora

using namespace aurora;

extern "C" int aurora_hip_patchify(const aurora_patch_var* desc, int n_vars, void* out, int64_t Kpad,
                                   int k_offset, int K_total, int B, int T, int n_lvl, int Hp, int Wp, int P,
                                   int dtype, void* stream) {
  return aurora_hip_patchify_absmax(desc, n_vars, out, Kpad, k_offset, K_total, B, T, n_lvl, Hp, Wp, P, dtype, nullptr, stream);
}

extern "C" int aurora_hip_patchify_absmax(const aurora_patch_var* desc, int n_vars, void* out, int64_t Kpad,
                                          int k_offset, int K_total, int B, int T, int n_lvl, int Hp, int Wp, int P,
                                          int dtype, float* absmax, void* stream) {
  AURORA_CHECK_ARG(dtype == AURORA_F32 || dtype == AURORA_BF16, "patchify: bad dtype");
  AURORA_CHECK_ARG(n_vars > 0 && n_vars <= MAX_VARS, "patchify: %d variables per call (max %d)", n_vars, MAX_VARS);
  AURORA_CHECK_ARG(k_offset >= 0 && k_offset + n_vars * T * P * P <= K_total && K_total <= Kpad,
                   "patchify: column range does not fit (k_offset=%d K_total=%d Kpad=%lld)", k_offset, K_total,
                   (long long)Kpad);
  PatchArgs p;
  for (int v = 0; v < n_vars; ++v) {
    const aurora_patch_var& s = desc[v];
    p.v[v] = PatchVar{s.src, s.stride_b, s.stride_t, s.stride_c, s.stride_h, s.stride_w,
                      s.loc, s.inv_scale, s.transform, s.tw0, s.tw1, s.tb};
  }
  p.out = out; p.Kpad = Kpad; p.k_offset = k_offset; p.K_total = K_total;
  p.n_vars = n_vars; p.B = B; p.T = T; p.n_lvl = n_lvl; p.Hp = Hp; p.Wp = Wp; p.P = P;
  p.absmax = absmax;
  AURORA_CHECK_ARG(B > 0 && T > 0 && n_lvl > 0 && Hp > 0 && Wp > 0 && P > 0, "patchify: bad problem size");
  bool vec4 = P == 4 && dtype == AURORA_F32 && (uintptr_t)out % 16 == 0 && Kpad % 4 == 0 && k_offset % 4 == 0 &&
              n_vars * T * 32 <= 1024 && Hp <= 65535 && (int64_t)n_lvl * B <= 65535;
  for (int v = 0; v < n_vars && vec4; ++v) {
    const aurora_patch_var& s = desc[v];
    vec4 = s.stride_w == 1 && (uintptr_t)s.src % 16 == 0 && s.stride_b % 4 == 0 && s.stride_t % 4 == 0 && s.stride_c % 4 == 0 &&
           s.stride_h % 4 == 0;
  }
  if (vec4) {
    const int run = 8 * PATCH4_GROUPS;
    const dim3 grid((unsigned)((Wp + run - 1) / run), (unsigned)Hp, (unsigned)(n_lvl * B));
    hipLaunchKernelGGL(patchify_kernel, grid, dim3((unsigned)((n_vars * T * 32 + 63) / 64 * 64)), 0, as_stream(stream), p);
  } else {
    const int k_end = k_offset + n_vars * T * P * P == K_total ? (int)Kpad : k_offset + n_vars * T * P * P;
    const int chunks = (k_end - k_offset + 255) / 256;
    const int groups = (Wp + PATCH_SPAN - 1) / PATCH_SPAN;
    AURORA_CHECK_ARG((int64_t)groups * chunks < ((int64_t)1 << 31) && Hp <= 65535 && (int64_t)n_lvl * B <= 65535,
                     "patchify: grid too large (%d x %d patches, %d levels x %d)", Hp, Wp, n_lvl, B);
    const dim3 grid((unsigned)(groups * chunks), (unsigned)Hp, (unsigned)(n_lvl * B));
    if (dtype == AURORA_F32)
      hipLaunchKernelGGL(patchify_cols_kernel<float>, grid, dim3(256), 0, as_stream(stream), p, k_end, chunks);
    else
      hipLaunchKernelGGL(patchify_cols_kernel<bf16_t>, grid, dim3(256), 0, as_stream(stream), p, k_end, chunks);
  }
  return check_launch("patchify");
}

extern "C" int aurora_hip_assemble_tokens(const float* surf, const float* agg, const float* pos_scale,
                                          const float* time_emb, float* out_f32, void* out_t, int B, int Cl,
                                          int64_t L, int D, int dtype, void* stream) {
  AURORA_CHECK_ARG(D % 8 == 0 && Cl >= 2, "assemble_tokens: D=%d must be a multiple of 8, Cl=%d >= 2", D, Cl);
  AsmArgs p{surf, agg, pos_scale, time_emb, out_f32, out_t, B, Cl, L, D};
  const int64_t total = (int64_t)B * Cl * L * (D / 8);
  const unsigned blocks = (unsigned)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  if (dtype == AURORA_F32) {
    p.out_t = nullptr;  // the fp32 stream is its own GEMM operand
    hipLaunchKernelGGL(assemble_kernel<float>, dim3(blocks), dim3(256), 0, as_stream(stream), p);
  } else {
    hipLaunchKernelGGL(assemble_kernel<bf16_t>, dim3(blocks), dim3(256), 0, as_stream(stream), p);
  }
  return check_launch("assemble_tokens");
}

extern "C" int aurora_hip_unpatchify(const float* y, int64_t ldy, const aurora_unpatch_var* desc, int n_vars,
                                     int B, int n_lvl, int Hp, int Wp, int P, void* stream) {
  AURORA_CHECK_ARG(n_vars > 0 && n_vars <= MAX_VARS, "unpatchify: %d variables per call (max %d)", n_vars, MAX_VARS);
  UnpatchArgs p;
  for (int v = 0; v < n_vars; ++v)
    p.v[v] = UnpatchVar{desc[v].dst, desc[v].loc, desc[v].scale, desc[v].clamp_min0, desc[v].col0,
                        desc[v].lvl_stride, desc[v].mod_col0, desc[v].prev, desc[v].prev_sb, desc[v].prev_sc,
                        desc[v].prev_sh, desc[v].inv_scale, desc[v].clamp_max1_levels, desc[v].angle_col0,
                        desc[v].dens_col0, desc[v].mask, desc[v].mask_sh, desc[v].mask_thresh};
  p.y = y; p.ldy = ldy; p.n_vars = n_vars; p.B = B; p.n_lvl = n_lvl; p.Hp = Hp; p.Wp = Wp; p.P = P;
  bool al = P == 4 && (uintptr_t)y % 16 == 0 && ldy % 4 == 0;
  for (int v = 0; v < n_vars && al; ++v)
    al = (uintptr_t)desc[v].dst % 16 == 0 && desc[v].col0 % 4 == 0 && desc[v].lvl_stride % 4 == 0;
  p.vec4 = al ? 1 : 0;
  for (int v = 0; v < n_vars && al; ++v)   // (the optional head columns and planes of the post-decoder hooks as well)
    al = (desc[v].mod_col0 < 0 || (desc[v].mod_col0 % 4 == 0 && (uintptr_t)desc[v].prev % 16 == 0 && desc[v].prev_sb % 4 == 0 &&
                                   desc[v].prev_sc % 4 == 0 && desc[v].prev_sh % 4 == 0)) &&
         (desc[v].angle_col0 < 0 || desc[v].angle_col0 % 4 == 0) &&
         (desc[v].dens_col0 < 0 || (desc[v].dens_col0 % 4 == 0 && (uintptr_t)desc[v].mask % 16 == 0 && desc[v].mask_sh % 4 == 0));
  p.vec4 = al ? 1 : 0;
  AURORA_CHECK_ARG(B > 0 && n_lvl > 0 && Hp > 0 && Wp > 0 && P > 0, "unpatchify: bad problem size");
  if (al) {
    AURORA_CHECK_ARG(Hp <= 65535 && (int64_t)B * n_lvl <= 65535, "unpatchify: grid too large");
    const int run = 8 * UNPATCH_GROUPS;
    const dim3 grid((unsigned)((Wp + run - 1) / run), (unsigned)Hp, (unsigned)(B * n_lvl));
    hipLaunchKernelGGL(unpatchify_kernel<4>, grid, dim3((unsigned)((n_vars * 32 + 63) / 64 * 64)), 0, as_stream(stream), p);
  } else {
    AURORA_CHECK_ARG(Hp <= 65535 && (int64_t)n_vars * B * n_lvl <= 65535, "unpatchify: grid too large");
    const dim3 grid((unsigned)((Wp * P + 255) / 256), (unsigned)Hp, (unsigned)(n_vars * B * n_lvl));
    hipLaunchKernelGGL(unpatchify_kernel<1>, grid, dim3(256), 0, as_stream(stream), p);
  }
  return check_launch("unpatchify");
}
