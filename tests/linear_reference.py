"""fp64 definition of the dense linears of csrc/gemm*.hip, a PER-ELEMENT tolerance derived from the number formats, the table
of cases tests/test_gpu_linear.py runs, and wrong variants.

Plain torch on the CPU:  out = act(a @ w.T + bias) + residual, erf-GELU or SiLU, with the second output, the head-plane layout
(attention_reference.to_planes), the fp16-pair layout in and out (perceiver_reference.unsplit / split_pairs), the strided
batch, and  x + LN(a @ w.T + b) * gain + shift  for the fused kernel.

The tolerance (`tolerance`) is per element and comes from the formats, not from the kernels.  With
S[m, n] = sum_k |a[m, k]| |w[n, k]| + |bias[n]|  the value in front of the activation is off by at most
    E0 = (C_ACC K u + operands) S + subnormal,      u = 2^-24,
where K u S bounds fp32 accumulation in ANY order, `operands` is what the mode loses when it represents its operands (bf16
inputs: nothing, the reference sees the rounded values; native fp32 and three bf16 terms: 2 x 2^-24; two fp16 terms: 2 x 2^-22,
and `subnormal` = 3e-8 (sum_k |w| + sum_k |a| / 64): fp16 remainders of activations below 0.25, and of the weights, scaled by
64, below 0.25 / 64, are subnormal -- gemm_f32.hip).  E0 goes through the activation by its Lipschitz constant (GELU 1.13,
SiLU 1.1); the kernel's own activation adds the bound of the form it uses, stated once in tests/activation_reference.py and
pinned there against fp64 at exact inputs (gelu_sig of every bf16 kernel: 2.6e-5 absolute for x >= -9, plus 2.4e-12 |x| below,
where the clamp leaves 2.305e-12 x -- no bf16 case of this table has a pre-activation below -9; gelu_erf_fast of the
operand-splitting fp32 kernels: 4e-7 absolute + 7.5e-8 |x|; erff of the native fp32 ones: 4 ulp of erf, 2^-22 |x|; SiLU by expf
and one division: 8 x 2^-24 |x|); the residual is added exactly but the sum is rounded
once (2^-24); the store rounds once more (2^-24 |v| fp32; 2^-8 |v| bf16 -- eight significand bits, so half a spacing is up to
2^-8 of a value at the bottom of its binade, which a correctly rounded CPU store reaches; the pair layout keeps 22 bits:
2^-22 |v|).

C_ACC is fixed from CPU evidence only (`emulate`: fp32 accumulation of 32-wide K steps, ascending and pairwise):
tests/test_linear_reference.py measures the worst ratio of that emulation's error to K u S over every case of the table --
0.16 at K = 32, falling like 1 / sqrt(K) -- and asserts that it stays below C_ACC / ACC_MULTIPLE.  ACC_MULTIPLE = 6 because
the emulation rounds every add to nearest, so its errors cancel like a random walk; a matrix core may truncate inside its 32-wide
dot product, which does not cancel, and the any-order bound (ratio 1) is then the honest ceiling: 6 x 0.16 ~ 1.

The keyword `wrong` selects deliberately WRONG evaluations, each a mistake a kernel could make; the GPU tests never use them.
tests/test_linear_reference.py shows that each lands outside the tolerance on these inputs.
"""
from typing import NamedTuple, Optional

import torch

from tests import activation_reference as A
from tests.attention_reference import to_planes
from tests.perceiver_reference import hi_is_rounded_value, split_pairs, unsplit  # noqa: F401

U32 = 2.0 ** -24
ACC_MULTIPLE = 6.0
C_ACC = 1.0
F32_A_SPLIT, F32_W_SPLIT, F32_C_SPLIT = 4, 8, 16
ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2
LIPSCHITZ = {ACT_NONE: 1.0, ACT_GELU: 1.13, ACT_SILU: 1.1}
LN_F32_TOL = 3e-6          # norm_reference.F32_TOL: per-row error of an fp32 LayerNorm over its natural scale


class Case(NamedTuple):
    id: str
    kernel: str                 # what linear_plan must say on a 256-CU device ...
    tile: tuple                 # ... (bm, bn)
    form: str                   # epilogue form: coalesced | direct_vec | direct_scalar | pair_coalesced | pair_direct | planes | planes_kv
    dtype: str                  # "bf16" | "f32"
    M: int
    N: int
    K: int
    mode: int = -1              # fp32 mode (0 native, 1 three bf16 terms, 2 two fp16 terms) with its F32_*_SPLIT flags
    act: int = ACT_NONE
    bias: bool = True
    res: str = "none"           # none | full | row (ldr == 0)
    out2: bool = False
    misalign: str = "none"      # none | c | c2 | res: whose leading dimension breaks 16-byte alignment
    guard: Optional[bool] = None   # a guard word that holds / does not hold
    entry: str = "linear"       # linear | ws | planes | batched
    split: int = 0              # ws: requested K slices (0: the library's choice)
    ksplit: int = 1             # what the plan must say
    heads: int = 0              # planes
    sel0: int = 0
    batch: int = 1
    a4: bool = False            # also run in the child process whose AURORA_GEMM_A4_MIN_K sends it to the four-wave kernel

    @property
    def vec(self) -> bool:
        return self.form != "direct_scalar"

    @property
    def pre(self) -> int:
        return self.mode & (F32_A_SPLIT | F32_W_SPLIT | F32_C_SPLIT) if self.mode > 0 else 0

    @property
    def base_mode(self) -> int:
        return self.mode & 3 if self.mode > 0 else self.mode


# The table.  Shapes are the smallest that reach their kernel on 256 CUs (found with linear_plan(cus=256), written down here).
# What cannot be reached, on any CU count, because the cost model of plan_linear never keeps 256 x 256 bf16 tiles below
# K = 355 (a round of 256 x 128 tiles costs 7.7 + 0.0317 K against 0.97 x (10.1 + 0.0266 K) and never needs more rounds):
#   * the bf16 form of `ring` (K < 128, i.e. K = 64: bf16 K is a multiple of 64, so one or three 32-wide stages, K = 32 or 96,
#     are refused by the argument check) -- `ring` is reached in its fp32 form only;
#   * `pp` with 4 or 6 stages (an odd count needs K % 64 != 0: refused): its shortest reachable K is 384, twelve stages.
_BIG = dict(dtype="bf16", M=8193, N=1024)            # 33 m-tiles x 4: ragged last m-tile, more tiles than one XCD's share
_F = dict(dtype="f32", M=300, N=256)                 # the fp32 split kernels do not depend on M: one whole tile + a ragged one
CASES = [
    # ---- 128 x 128 tiles: ragged M and N, N not a multiple of 16, M = 1 ----
    Case("t128-bf16-ragged", "tile128", (128, 128), "direct_vec", "bf16", 300, 200, 128, act=ACT_GELU, res="full", out2=True),
    Case("t128-bf16-n27", "tile128", (128, 128), "direct_scalar", "bf16", 130, 27, 64, act=ACT_SILU, misalign="c"),
    Case("t128-bf16-m1", "tile128", (128, 128), "direct_vec", "bf16", 1, 512, 64, bias=False),
    Case("t128-f32-ragged", "tile128", (128, 128), "direct_vec", "f32", 257, 100, 96, mode=0, act=ACT_GELU, res="row", out2=True),
    Case("t128-f32-n27-c2", "tile128", (128, 128), "direct_scalar", "f32", 129, 27, 32, mode=1, out2=True, misalign="c2"),
    Case("t128-f32-m1", "tile128", (128, 128), "direct_vec", "f32", 1, 144, 32, mode=2, act=ACT_SILU),
    # ---- ring, fp32 mode 0 (K-stages of 16 fp32: K = 32 is its two-stage minimum; 4, 6 and 10 stages) ----
    Case("ring-f32-coalesced-k32", "ring", (256, 256), "coalesced", "f32", 8193, 1024, 32, mode=0, act=ACT_GELU, res="full"),
    Case("ring-f32-coalesced-row", "ring", (256, 256), "coalesced", "f32", 8193, 1024, 96, mode=0, act=ACT_SILU, res="row"),
    Case("ring-f32-coalesced-plain", "ring", (256, 256), "coalesced", "f32", 8193, 1024, 64, mode=0, bias=False),
    Case("ring-f32-direct", "ring", (256, 256), "direct_vec", "f32", 8193, 1024, 160, mode=0, res="full", out2=True),
    Case("ring-f32-scalar-c", "ring", (256, 256), "direct_scalar", "f32", 8193, 1024, 32, mode=0, act=ACT_GELU, misalign="c"),
    # ---- ring_mid (256 x 128 tiles, three-stage ring): two stages (K = 64), four, and a longer K ----
    Case("mid-coalesced-k64", "ring_mid", (256, 128), "coalesced", "bf16", 8193, 512, 64),
    Case("mid-coalesced-gelu", "ring_mid", (256, 128), "coalesced", "bf16", 8193, 512, 128, act=ACT_GELU),
    Case("mid-coalesced-silu-nobias", "ring_mid", (256, 128), "coalesced", "bf16", 8193, 512, 320, act=ACT_SILU, bias=False),
    Case("mid-direct", "ring_mid", (256, 128), "direct_vec", "bf16", 8193, 512, 128, act=ACT_GELU, res="full", out2=True),
    Case("mid-scalar-res", "ring_mid", (256, 128), "direct_scalar", "bf16", 8193, 512, 192, res="full", misalign="res"),
    # ---- pp: twelve stages (its shortest reachable K) and a long K; the same rows are the a4 cases of the child ----
    Case("pp-coalesced", "pp", (256, 256), "coalesced", **_BIG, K=384, a4=True),
    Case("pp-coalesced-gelu", "pp", (256, 256), "coalesced", **_BIG, K=512, act=ACT_GELU, a4=True),
    Case("pp-coalesced-silu-nobias", "pp", (256, 256), "coalesced", **_BIG, K=448, act=ACT_SILU, bias=False, a4=True),
    Case("pp-direct", "pp", (256, 256), "direct_vec", **_BIG, K=384, act=ACT_GELU, res="full", out2=True, a4=True),
    Case("pp-direct-out2", "pp", (256, 256), "direct_vec", **_BIG, K=512, out2=True),
    Case("pp-scalar-c", "pp", (256, 256), "direct_scalar", **_BIG, K=384, act=ACT_SILU, misalign="c", a4=True),
    Case("pp-scalar-c2", "pp", (256, 256), "direct_scalar", **_BIG, K=384, out2=True, misalign="c2"),
    Case("pp-long-k", "pp", (256, 256), "coalesced", "bf16", 16385, 512, 2048, act=ACT_GELU, a4=True),
    Case("pp-planes", "pp", (256, 256), "planes", "bf16", 8193, 1536, 512, entry="planes", heads=8),
    Case("t128-planes-kv", "tile128", (128, 128), "planes_kv", "bf16", 300, 256, 128, entry="planes", heads=2, sel0=1),
    # ---- split-K: a requested split (slices of four stages, the minimum), three slices, the library's own choice ----
    Case("splitk-2", "pp_splitk", (256, 256), "coalesced", "bf16", 1030, 256, 256, entry="ws", split=2, ksplit=2, act=ACT_GELU),
    Case("splitk-3-direct", "pp_splitk", (256, 256), "direct_vec", "bf16", 1030, 512, 512, entry="ws", split=3, ksplit=3,
         res="full", out2=True),
    Case("splitk-own", "pp_splitk", (256, 256), "coalesced", "bf16", 1024, 256, 4096, entry="ws", split=0, ksplit=2),
    # ---- the operand-splitting fp32 kernels ----
    Case("three-coalesced", "f32_three", (256, 256), "coalesced", **_F, K=32, mode=1, act=ACT_GELU, res="full"),
    Case("three-direct", "f32_three", (256, 256), "direct_vec", **_F, K=96, mode=1, act=ACT_SILU, res="row", out2=True),
    Case("three-scalar-res", "f32_three", (256, 256), "direct_scalar", **_F, K=64, mode=1, res="full", misalign="res"),
    Case("two-k32", "f32_two", (256, 256), "coalesced", **_F, K=32, mode=2, act=ACT_GELU, res="row"),
    Case("two-k64-direct", "f32_two", (256, 256), "direct_vec", **_F, K=64, mode=2, out2=True),
    Case("pp2-k96", "f32_pp", (128, 256), "coalesced", **_F, K=96, mode=2, act=ACT_GELU),
    Case("pp2-k160-silu-nobias", "f32_pp", (128, 256), "coalesced", **_F, K=160, mode=2, act=ACT_SILU, bias=False),
    Case("pp2-direct", "f32_pp", (128, 256), "direct_vec", **_F, K=160, mode=2, act=ACT_GELU, res="full", out2=True),
    Case("pp2-scalar-c", "f32_pp", (128, 256), "direct_scalar", **_F, K=96, mode=2, misalign="c"),
    Case("pp2-w", "f32_pp_w", (128, 256), "coalesced", **_F, K=96, mode=2 | F32_W_SPLIT, act=ACT_GELU),
    Case("pp2-aw-direct", "f32_pp_aw", (128, 256), "direct_vec", **_F, K=128, mode=2 | F32_W_SPLIT | F32_A_SPLIT, res="full"),
    Case("pp2-w-tall", "f32_pp_w_tall", (256, 128), "coalesced", "f32", 300, 384, 96, mode=2 | F32_W_SPLIT, act=ACT_SILU),
    Case("pp2-aw-tall", "f32_pp_aw_tall", (256, 128), "direct_vec", "f32", 300, 128, 160, mode=2 | F32_W_SPLIT | F32_A_SPLIT,
         res="row"),
    Case("pp2-pair-coalesced", "f32_pp_w", (128, 256), "pair_coalesced", **_F, K=96, mode=2 | F32_W_SPLIT | F32_C_SPLIT,
         act=ACT_GELU),
    Case("pp2-pair-direct", "f32_pp_aw", (128, 256), "pair_direct", **_F, K=96,
         mode=2 | F32_W_SPLIT | F32_A_SPLIT | F32_C_SPLIT, res="full"),
    # ---- guarded twins: the device word picks the two-term kernel or its three-term twin ----
    Case("twin-pp2-holds", "f32_pp", (128, 256), "coalesced", **_F, K=96, mode=2, guard=True, act=ACT_GELU),
    Case("twin-pp2-fails", "f32_pp", (128, 256), "coalesced", **_F, K=96, mode=2, guard=False, act=ACT_GELU),
    Case("twin-two-holds", "f32_two", (256, 256), "direct_vec", **_F, K=64, mode=2, guard=True, res="full", out2=True),
    Case("twin-two-fails", "f32_two", (256, 256), "direct_vec", **_F, K=64, mode=2, guard=False, res="full", out2=True),
    # ---- strided batch of 3: distinct strides for A, W, bias and C; and without a bias ----
    Case("batched-t128", "tile128", (128, 128), "direct_vec", "bf16", 130, 100, 64, entry="batched", batch=3, act=ACT_GELU),
    Case("batched-three-guard", "f32_three", (256, 256), "coalesced", **_F, K=64, mode=1, guard=False, entry="batched", batch=3),
    Case("batched-mid", "ring_mid", (256, 128), "coalesced", "bf16", 8193, 512, 64, entry="batched", batch=3, act=ACT_SILU),
    Case("batched-nobias", "f32_pp", (128, 256), "coalesced", **_F, K=96, mode=2, entry="batched", batch=3, bias=False),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
KERNELS = ("tile128", "ring", "ring_mid", "pp", "pp_splitk", "a4", "f32_three", "f32_two", "f32_pp", "f32_pp_w", "f32_pp_aw",
           "f32_pp_w_tall", "f32_pp_aw_tall")
FORMS = ("coalesced", "direct_vec", "direct_scalar", "pair_coalesced", "pair_direct", "planes", "planes_kv")
LN_CASES = [(65, 512), (128, 512), (300, 2048)]      # (M, K): ragged only, whole only, both; N = 512


def plan_kwargs(c: Case, cus: int = 0) -> dict:
    """Keyword arguments of lib.linear_plan for a case, as its launch lays the buffers out (`layout`)."""
    ld = layout(c)
    kw = dict(f32_gemm=c.mode, guard=c.guard is not None, batch=c.batch, ldc=ld["ldc"], cus=cus)
    if c.out2:
        kw["ldc2"] = ld["ldc2"]
    if c.res != "none":
        kw["ldr"] = 0 if c.res == "row" else ld["ldr"]
    if c.entry == "ws":
        kw.update(workspace_bytes=8 * tiles(c) * 256 * 256 * 4, n_tickets=64, split=c.split)
    if c.entry == "planes":
        kw.update(plane_stride=(c.M + 2) * 192, plane_heads=c.heads, ldc=c.N)
    return kw


def tiles(c: Case) -> int:
    return ((c.M + 255) // 256) * (c.N // 256)


def layout(c: Case) -> dict:
    """Leading dimensions of C, C2 and the residual: 8 guard columns (rows stay 16-byte aligned) or 3 (they do not)."""
    ld = lambda who: (c.N + 7) // 8 * 8 + (11 if c.misalign == who else 8)   # noqa: E731
    ldc = ld("c")
    if c.pre & F32_C_SPLIT:
        ldc = c.N + 32                                # the pair layout wants ldc % 32 == 0
    return {"ldc": ldc, "ldc2": ld("c2"), "ldr": ld("res")}


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1).double() * scale


def _decades(*shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return 10.0 ** (torch.rand(*shape, generator=g, dtype=torch.float32).double() * (hi - lo) + lo)


class Problem(NamedTuple):
    a: torch.Tensor             # (G, M, K) fp64, holding values the case's dtype represents exactly
    w: torch.Tensor             # (G, N, K)
    bias: Optional[torch.Tensor]   # (G, N)
    res: Optional[torch.Tensor]    # (M, N) or (1, N)


def problem(c: Case) -> Problem:
    """Mixed magnitudes: every column k of the operands has its own decade (two and a half across K, the LAST 32-wide step at
    the top so that a dropped stage shows in every element); bias and residual have a scale per output column (a decade and
    a half across N), so a neighbour's value is a visible error.  Values are rounded to the case's dtype here."""
    G = c.batch
    kmag = _decades(c.K, seed=11, lo=-2.0, hi=0.5)
    kmag[-32:] = _decades(32, seed=12, lo=0.0, hi=0.5)
    a = rnd(G, c.M, c.K, seed=1) * kmag
    w = rnd(G, c.N, c.K, seed=2) * _decades(G, c.N, 1, seed=13, lo=-0.5, hi=0.5) * (c.K ** -0.5)
    nmag = _decades(c.N, seed=14, lo=-1.0, hi=0.5)
    bias = rnd(G, c.N, seed=3) * nmag if c.bias else None
    res = None if c.res == "none" else rnd(1 if c.res == "row" else c.M, c.N, seed=4) * nmag.flip(0) * 2
    dt = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    q = lambda t: None if t is None else t.to(dt).double()            # noqa: E731
    q32 = lambda t: None if t is None else t.float().double()         # noqa: E731
    return Problem(q(a), q(w), q32(bias), q32(res))


# ------------------------------------------------------------------------------------------
# the operation
# ------------------------------------------------------------------------------------------
def activate(v: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * 0.5 ** 0.5))
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    return v


WRONG = ("drop_last_k_step", "swap_pieces", "bias_n16", "res_row_m1", "res_clamped_row", "skip_act_fragment", "drop_split_slice",
         "batch_prev_weights", "batch_prev_bias", "row_read_with_stride")


def linear_ref(c: Case, p: Problem, wrong: Optional[str] = None):
    """(out (G, M, N) fp64, pre-activation (G, M, N), S (G, M, N)).  `wrong`: see WRONG; each touches one tile / fragment /
    problem only, as the mistake of one workgroup or lane would."""
    a, w, bias = p.a, p.w, p.bias
    bm, bn = c.tile
    last_m = (c.M - 1) // bm * bm                   # first row of the ragged (or last) m-tile
    if wrong == "batch_prev_weights":
        w = torch.cat([w[:1], w[:-1]])
    if wrong == "batch_prev_bias":
        bias = torch.cat([bias[:1], bias[:-1]])
    pre = a @ w.transpose(1, 2)
    if wrong == "drop_last_k_step":                 # one tile: the first bm x bn
        pre[:, :bm, :bn] -= a[:, :bm, -32:] @ w[:, :bn, -32:].transpose(1, 2)
    if wrong == "drop_split_slice":                 # slice 1 of ksplit, K-stages kb .. of 32, the tile of the last rows
        k0, k1 = (c.K // 32) * 1 // c.ksplit * 32, (c.K // 32) * 2 // c.ksplit * 32
        pre[:, last_m:, :bn] -= a[:, last_m:, k0:k1] @ w[:, :bn, k0:k1].transpose(1, 2)
    S = a.abs() @ w.abs().transpose(1, 2)
    if bias is not None:
        b = bias[:, None, :]
        if wrong == "bias_n16":
            b = b.clone()
            hi = min(bn, c.N)
            b[..., :hi - 16] = b[..., 16:hi].clone()
        pre = pre + b
        S = S + p.bias.abs()[:, None, :]
    out = activate(pre, c.act)
    if wrong == "skip_act_fragment":                # rows 16 .. 31 of the last m-tile (or the tile's only rows)
        r0 = min(last_m + 16, c.M - 1)
        out[:, r0:r0 + 16] = pre[:, r0:r0 + 16]
    if p.res is not None:
        r = p.res.expand(c.M, c.N)
        if wrong == "res_row_m1":                   # the ragged tile reads the row above
            r = r.clone()
            r[last_m:] = p.res.expand(c.M, c.N)[last_m - 1:-1]
        if wrong == "res_clamped_row":              # the valid row M - 2 reads the clamped row M - 1
            r = r.clone()
            r[c.M - 2] = p.res.expand(c.M, c.N)[c.M - 1]
        if wrong == "row_read_with_stride":         # the broadcast row (ldr == 0) read with the stride of a padded matrix
            idx = (torch.arange(c.M)[:, None] * (c.N + 8) + torch.arange(c.N)) % c.N
            r = p.res[0][idx]
        out = out + r
    if wrong == "swap_pieces":                      # two 16-column pieces of one tile's rows
        o = out.clone()
        o[:, :bm, 0:16], o[:, :bm, 16:32] = out[:, :bm, 16:32], out[:, :bm, 0:16]
        out = o
    return out, pre, S


def tolerance(c: Case, p: Problem, out, pre, S, store: str, three_term_twin: bool = False) -> torch.Tensor:
    """Per-element bound of |stored - out| for a result stored as `store` (f32 | bf16 | pair); the module docstring derives it.
    three_term_twin: a guarded launch whose guard does not hold runs the three-term kernel."""
    mode = 1 if three_term_twin else c.base_mode
    native = c.dtype == "f32" and (mode == 0 or c.kernel == "tile128")
    operands, sub = 0.0, 0.0
    if c.dtype == "f32":
        operands = 2 * 2.0 ** -22 if (mode == 2 and not native) else 2 * U32
        if mode == 2 and not native:
            sub = 3e-8 * (p.w.abs().sum(-1)[:, None, :] + p.a.abs().sum(-1)[:, :, None] / 64)
    e0 = (C_ACC * c.K * U32 + operands) * S + sub
    if c.ksplit > 1:
        e0 = e0 + (c.ksplit - 1) * U32 * S          # the slices are added in fp32
    if c.act == ACT_GELU:
        act_err = A.bound("gelu_sig" if c.dtype == "bf16" else "erff" if native else "gelu_erf_fast", pre)
    elif c.act == ACT_SILU:
        act_err = A.bound("silu", pre)
    else:
        act_err = 0.0
    v = activate(pre, c.act).abs()
    tol = LIPSCHITZ[c.act] * e0 + act_err + 2 * U32 * v
    if p.res is not None:
        tol = tol + U32 * (v + p.res.abs())
    return tol + {"f32": U32, "bf16": 2.0 ** -8, "pair": 2.0 ** -22}[store] * out.abs()


def worst_ratio(stored: torch.Tensor, out: torch.Tensor, tol: torch.Tensor) -> float:
    """max |stored - out| / tol over every element; NaN if anything stored is NaN."""
    r = (stored.double() - out).abs() / tol
    return float("nan") if torch.isnan(r).any() else r.max().item()


def emulate(c: Case, p: Problem, order: str = "ascending"):
    """A correct fp32 evaluation on the CPU: products of 32-wide K steps accumulated in fp32, `ascending` or `pairwise`;
    bias, activation, residual in fp32.  Returns the fp32 result (G, M, N) and the fp32 pre-activation."""
    a, w = p.a.float(), p.w.float()
    parts = [a[:, :, k:k + 32] @ w[:, :, k:k + 32].transpose(1, 2) for k in range(0, c.K, 32)]
    if order == "ascending":
        acc = parts[0]
        for t in parts[1:]:
            acc = acc + t
    else:
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        acc = parts[0]
    pre = acc if p.bias is None else acc + p.bias.float()[:, None, :]
    out = torch.nn.functional.gelu(pre) if c.act == ACT_GELU else torch.nn.functional.silu(pre) if c.act == ACT_SILU else pre
    if p.res is not None:
        out = out + p.res.float()
    return out, pre


def round_bf16_rne(x32: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by round-to-nearest-even, written out on the bits (finite values)."""
    b = x32.contiguous().view(torch.int32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16).view(torch.float32).bfloat16()


def truncate_bf16(x32: torch.Tensor) -> torch.Tensor:
    """WRONG store: the low 16 bits dropped."""
    return (x32.contiguous().view(torch.int32) >> 16 << 16).view(torch.float32).bfloat16()


def planes_of(out: torch.Tensor, heads: int) -> torch.Tensor:
    """(M, sel x heads x 64) rows -> (heads, M, sel, 64): what linear_planes stores at out[:, :M, sel0:]."""
    M, N = out.shape
    sel = N // (64 * heads)
    if sel == 3:
        return to_planes(out.reshape(1, M, N), heads)
    return out.reshape(M, sel, heads, 64).permute(2, 0, 1, 3).contiguous()


def pairs_of(x32: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    return split_pairs(x32, scale)


def from_pairs(t: torch.Tensor):
    return unsplit(t)


# ------------------------------------------------------------------------------------------
# the fused linear + AdaLN kernel (gemm_ln512.hip): x + LN(bf16(a @ w.T + b)) * gain + shift
# ------------------------------------------------------------------------------------------
def ln_problem(M: int, K: int, N: int = 512):
    bf = lambda t: t.bfloat16().double()   # noqa: E731
    return dict(a=bf(rnd(M, K, seed=21)), w=bf(rnd(N, K, seed=22) * K ** -0.5), b=rnd(N, seed=23).float().double(),
                gain=(rnd(N, seed=24) + 1).float().double(), shift=rnd(N, seed=25).float().double(),
                x=(rnd(M, N, seed=26) * 2).float().double())


def linear_ln_ref(q: dict, eps: float = 1e-5, wrong: Optional[str] = None):
    """(out, tol) per element.  The kernel rounds the linear's result to bf16 before the statistics (the reference's
    autocast linear yields bf16); the fp64 reference does not, and the tolerance carries that rounding through the
    normalisation: dy_j <= 2^-9 |y_j| moves LN_j by at most (dy_j + mean dy) / sigma + |LN_j| rms(dy) / sigma, times |gain_j|;
    plus the fp32 LayerNorm's own LN_F32_TOL of the row's natural scale (norm_reference) and the accumulation bound."""
    y = q["a"] @ q["w"].T + q["b"]
    if wrong == "stats_without_bias":
        mean, var = (y - q["b"]).mean(-1, keepdim=True), (y - q["b"]).var(-1, unbiased=False, keepdim=True)
    else:
        mean, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
    sigma = torch.sqrt(var + eps)
    ln = (y - mean) / sigma
    x = q["x"]
    if wrong == "residual_row_above":
        x = torch.cat([x[:1], x[:-1]])
    out = x + ln * q["gain"] + q["shift"]
    K = q["a"].shape[1]
    dy = 2.0 ** -9 * y.abs() + K * U32 * (q["a"].abs() @ q["w"].abs().T + q["b"].abs())
    dln = (dy + dy.mean(-1, keepdim=True)) / sigma + ln.abs() * torch.sqrt((dy * dy).mean(-1, keepdim=True)) / sigma
    scale = ((ln * q["gain"]).abs() + q["shift"].abs() + q["x"].abs()).amax(-1, keepdim=True)
    return out, q["gain"].abs() * dln + LN_F32_TOL * scale
