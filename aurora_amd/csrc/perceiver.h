// What the Perceiver units (perceiver_attention.hip, perceiver_out.hip) share: the lane layout of the three
// group-per-(column, head) kernels, its sum across a group, and the host-side check of a context row that carries
// pre-multiplied scores.
#pragma once

#include "common.h"

namespace aurora {

// DPP controls of the moves below (bank and row masks 0xf, a lane without a source reads zero)
constexpr int DPP_ROW_MIRROR = 0x140;        // i <-> 15 - i
constexpr int DPP_ROW_HALF_MIRROR = 0x141;   // i <-> 7 - i
constexpr int DPP_QUAD_REVERSE = 0x1B;       // quad_perm [3,2,1,0]
constexpr int DPP_PAIR_SWAP = 0xB1;          // quad_perm [1,0,3,2]: i <-> i ^ 1
constexpr int DPP_ROW_BCAST0 = 0x150;        // row_newbcast:0

template <int CTRL>
__device__ __forceinline__ float dpp_move(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// A group of HDIM / 4 adjacent lanes owns one (grid column, head): each lane holds 4 of the head's features, so a
// group reads a key / value row as one contiguous run (16 lanes x 16 B = 256 B for head_dim 64) and the four groups
// of a wave -- four adjacent heads -- read 1 KiB contiguous per load instruction.  (One thread per (column, head,
// query) with the whole head in registers reads 16 B per lane at a 256-byte stride: 1.7 TB/s on kv streams that
// should run at HBM speed.)  The q.k dot products are reduced across the group with DPP adds (mirror, half-mirror,
// quad reverse, pair swap); the keys of a column are re-read per query out of L1 (Lk * 2 * HDIM * 4 B <= 7 KiB).
// The decomposition: group = global thread / LPG = column * heads + head, the lane's features start at (thread % LPG) * 4,
// column = b * cols_per_b + l; lanes behind the last group leave (whole groups together).  Each of the three kernels
// writes those lines out itself: as a shared function they changed every kernel's machine code.
template <int LPG>   // lanes per group
__device__ __forceinline__ float group_sum(float v) {
  static_assert(LPG == 4 || LPG == 8 || LPG == 16 || LPG == 32, "lanes per group");
  if constexpr (LPG == 32) v += __shfl_xor(v, 16, 64);
  if constexpr (LPG >= 16) v += dpp_move<DPP_ROW_MIRROR>(v);
  if constexpr (LPG >= 8) v += dpp_move<DPP_ROW_HALF_MIRROR>(v);
  v += dpp_move<DPP_QUAD_REVERSE>(v);
  v += dpp_move<DPP_PAIR_SWAP>(v);
  return v;
}

// A context row of the kernels that take pre-multiplied scores is `ld` floats: [v (heads * head_dim) | ... | scores
// (Lq * heads) at s_off].  `entry` names the C entry in the message; `rest` is whatever else that entry reports with it.
inline int check_scores_row(const char* entry, const float* vs, int64_t ld, int s_off, int Lq, int heads, int head_dim,
                            bool rest = true) {
  AURORA_CHECK_ARG(rest && s_off >= heads * head_dim && ld >= (int64_t)s_off + (int64_t)Lq * heads && ld % 4 == 0 &&
                       ((uintptr_t)vs % 16) == 0,
                   "%s: a row is [v (heads * head_dim) | ... | scores (Lq * heads) at s_off], ld %% 4 == 0", entry);
  return AURORA_OK;
}

}  // namespace aurora
