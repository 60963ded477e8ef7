"""fp64 definition of the Perceiver kernels of csrc/perceiver_attention.hip and csrc/perceiver_out.hip, the cases and inputs their GPU tests
use, CPU models of their rounding points, and wrong variants.

Plain torch on the CPU, NOT through F.scaled_dot_product_attention.  Per (b, column, head):

    out[(b * cols + col) * Lq + i, head] = softmax_j(q_i . k_j / sqrt(head_dim)) . v_j        j < Lk

optionally followed by to_out (`F.linear(., W, bias)`) for the re-associated pair perceiver_probs + perceiver_out.  Every
input is addressed the way the C entry points address it, from the flat buffers the kernels get:

  * query i of global column c is row `c * q_col_stride + i` of `q` (q_col_stride = 0: the queries are model constants);
  * key j of column `col` of batch element b is row `b * kv_bstride + col + j * kv_lstride` of `kv` = [k (inner) | v (inner)];
  * for the kernels that take pre-multiplied scores a row is `ld` floats: [v (inner) | ... | scores at s_off], the scaled
    score of (query i, head h) at `s_off + i * heads + h`.

so a stride mistake in a test shows as a failure and is not mirrored.  Rows and columns between the addressed ones hold NaN.

Errors are judged per row, never against a maximum over the whole tensor:

  * attention outputs: per (row, head), max_d |out - ref| / max_{j, d} |v[col, j, head, d]| -- an output is a convex
    combination of those values (`head_error`);
  * perceiver_out: per (row, n), |out - ref| / (sum_k |W[n, k]| max_j |v[col, j, k]| + |bias[n]|) (`out_error`);
  * P: absolute, against the fp64 weights in the kernel's layout (`p_layout`).

NaN in a row makes the row's error NaN, so that `<= tol` fails.

The keyword `wrong` selects deliberately WRONG evaluations, each a mistake a kernel could plausibly make.  The GPU tests
never use them; tests/test_perceiver_reference.py shows that the inputs below tell each from the right result.
"""
from dataclasses import dataclass, replace
from functools import lru_cache
from typing import Optional

import torch

NAN = float("nan")
PO_PS = 64            # floats of P per (column, head) (perceiver_out.hip)

# ------------------------------------------------------------------------------------------
# Tolerances.  NOT taken from the kernels: measured on the CPU over every case of the lists below
# (`python -m tests.perceiver_reference` prints the table; tests/test_perceiver_reference.py re-measures and fails if a
# constant is out of date), rounded up in the fourth digit, then multiplied by 8 -- the margin for a different but legitimate summation order and __expf
# against exp.
#
#   worst head_error(fp32 evaluation, fp64)    flat       1.887e-7
#                                              peaked     1.194e-5   (scores of +-60 carry |s| 2^-24 into the exponent)
#                                              ascending  9.781e-7
#                                              descending 2.562e-7
#                                              edge       1.975e-7   (the pair cases with the guard not holding)
#   tagged: one-hot weights (the other keys 120 below the maximum: their exponentials underflow to zero in fp32) times
#   exactly representable values are EXACT in every summation order; the tolerance is one fp32 ulp of the scale, 2^-23,
#   and is not multiplied.
#   worst head_error(bf16 model, fp64)         all sets   2.196e-3   (one bf16 rounding of an output near the scale: 2^-9)
#   worst head_error(pair model, fp64)         flat 2.014e-7, edge 2.256e-7   (hi + lo carries 22 bits: the fp32
#                                              evaluation's error and a rounding at 2^-22); tagged: exact, as above
#   worst out_error(probs + out model, fp64)   flat 9.556e-8, peaked 4.633e-7, nearequal 7.506e-8, edge 1.005e-7,
#                                              tagged 6.751e-8
#   worst |P of the fp32 evaluation - P fp64|  flat 1.202e-7, peaked 4.739e-6
# ------------------------------------------------------------------------------------------
FACTOR = 8.0
F32_MEASURED = {"flat": 1.887e-7, "peaked": 1.194e-5, "ascending": 9.781e-7, "descending": 2.562e-7, "edge": 1.975e-7}
BF16_MEASURED = 2.196e-3
PAIR_MEASURED = {"flat": 2.014e-7, "edge": 2.256e-7}
OUT_MEASURED = {"flat": 9.556e-8, "peaked": 4.633e-7, "nearequal": 7.506e-8, "edge": 1.005e-7, "tagged": 6.751e-8}
P_MEASURED = {"flat": 1.202e-7, "peaked": 4.739e-6}
ULP32 = 2.0 ** -23
F32_TOL = {**{k: FACTOR * v for k, v in F32_MEASURED.items()}, "tagged": ULP32}
BF16_TOL = FACTOR * BF16_MEASURED                                      # 1.76e-2
PAIR_TOL = {**{k: FACTOR * v for k, v in PAIR_MEASURED.items()}, "tagged": ULP32}
OUT_TOL = {k: FACTOR * v for k, v in OUT_MEASURED.items()}
P_TOL = {k: FACTOR * v for k, v in P_MEASURED.items()}
TEETH = 10.0

INPUT_SETS = ("flat", "peaked", "ascending", "descending", "nearequal", "edge", "tagged")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def round_bf16(x: torch.Tensor) -> torch.Tensor:
    return x.float().bfloat16().to(x.dtype)


def worst(err: torch.Tensor) -> float:
    """The largest error; NaN if any is NaN (so that `worst(e) <= tol` fails on NaN)."""
    if err.numel() == 0:
        return 0.0
    return float("nan") if torch.isnan(err).any() else err.max().item()


# ------------------------------------------------------------------------------------------
# the fp16-pair layout (gemm_f32.hip): per 32 features 32 high halves, then 32 remainders, in an fp32 container
# ------------------------------------------------------------------------------------------
def split_halves(x: torch.Tensor):
    """fp32 x -> (hi, lo) as fp32: hi = half(x), lo = half(x - hi)."""
    x = x.float()
    hi = x.half().float()
    return hi, (x - hi).half().float()


def split_pairs(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """What aurora_hip_split_f16 makes of fp32 rows (M, K), K % 32 == 0: the same shape, float32 as a container."""
    M, K = x.shape
    assert K % 32 == 0
    hi, lo = split_halves(x.float() * scale)
    h16 = torch.stack([hi.half().reshape(M, K // 32, 32), lo.half().reshape(M, K // 32, 32)], dim=2)
    return h16.reshape(M, 2 * K).view(torch.float32)


def unsplit(t: torch.Tensor):
    """fp16-pair layout -> (high halves, remainders) as fp32 tensors of the logical shape."""
    M, K = t.shape
    h16 = t.contiguous().view(torch.float16).view(M, K // 32, 2, 32)
    return h16[:, :, 0].reshape(M, K).float(), h16[:, :, 1].reshape(M, K).float()


def hi_is_rounded_value(hi: torch.Tensor, lo: torch.Tensor) -> bool:
    """hi == half(hi + lo) bit for bit, except where hi + lo lies EXACTLY between two fp16 numbers: rounding the remainder to
    fp16 can move x - hi up to half a spacing of hi (about 4 in 10,000 values), half() then picks the even neighbour, which
    need not be hi.  There hi has to be one of the two."""
    s = hi + lo                                     # exact in fp32: 22 bits
    r = s.half().float()
    return bool(((r == hi) | ((s - hi).abs() == (s - r).abs())).all())


# ------------------------------------------------------------------------------------------
# the operation
# ------------------------------------------------------------------------------------------
WRONG = ("scale_1_hd", "drop_key", "admit_key", "pad_query", "q_stride_ignored", "batch_stride_ignored", "next_head",
         "swap_pieces", "swap_lane_halves")
WRONG_OUT = ("no_level0", "third_weight_p2", "drop_lo", "no_bias")


def kv_rows(B, cols, Lk, kv_bstride, kv_lstride):
    """(B * cols, Lk) row numbers: key j of column col of batch element b is row b * kv_bstride + col + j * kv_lstride."""
    b = torch.arange(B)[:, None, None]
    c = torch.arange(cols)[None, :, None]
    j = torch.arange(Lk)[None, None, :]
    return (b * kv_bstride + c + j * kv_lstride).reshape(B * cols, Lk)


# The fp32 evaluations accumulate term by term in a fixed order and take exp in fp64, rounded once: IEEE operations only, so
# the figures the tolerances are multiples of do not depend on the machine's BLAS or vector width.
def _seq_sum(terms):
    acc = None
    for t in terms:
        acc = t if acc is None else acc + t
    return acc


def _softmax32(s):
    e = torch.exp((s - s.amax(dim=-1, keepdim=True)).double()).float()
    return e / _seq_sum(e[..., j] for j in range(e.shape[-1]))[..., None]


def _combine(s, v, work, wrong=None):
    """s (n_cols, heads, Lq, Lk) scaled scores, v (n_cols, Lk, heads, hd) -> out (n_cols * Lq, inner), the weights, and the
    natural scale (n_cols, heads) = max_{j, d} |v|."""
    n_cols, heads, Lq, Lk = s.shape
    hd = v.shape[-1]
    p = torch.softmax(s.to(work), dim=-1) if work == torch.float64 else _softmax32(s.to(work))
    scale = v.double().abs().amax(dim=(1, 3))
    if wrong == "next_head":
        v = v.roll(-1, dims=2)
    if work == torch.float64:
        o = torch.einsum("chij,cjhd->cihd", p, v.to(work)).reshape(n_cols * Lq, heads * hd)
    else:
        vw = v.to(work)
        o = _seq_sum(p[..., j].permute(0, 2, 1)[..., None] * vw[:, j, None] for j in range(Lk)).reshape(n_cols * Lq, heads * hd)
    if wrong == "swap_pieces":         # an 8-feature piece lands where its neighbour belongs
        o = o.reshape(-1, heads * hd // 16, 2, 8).flip(2).reshape(n_cols * Lq, heads * hd)
    if wrong == "swap_lane_halves":    # the two lanes of a pair store each other's four features
        o = o.reshape(-1, heads * hd // 8, 2, 4).flip(2).reshape(n_cols * Lq, heads * hd)
    return o, p, scale


def attention_eval(q, q_col_stride, kv, B, cols, kv_bstride, kv_lstride, Lq, Lk, heads, hd, mode="f64", wrong=None):
    """aurora_hip_perceiver_attention on its own arguments.  mode f64: the reference; f32: the same formula in fp32.
    Returns (out (B * cols * Lq, inner), weights (n_cols, heads, Lq, Lk), scale (n_cols, heads))."""
    assert mode in ("f64", "f32") and (wrong is None or wrong in WRONG)
    work = torch.float64 if mode == "f64" else torch.float32
    inner, n_cols = heads * hd, B * cols
    assert q.shape[1] == inner and kv.shape[1] == 2 * inner
    nk = Lk + 1 if wrong == "admit_key" else Lk
    idx = kv_rows(B, cols, nk, 0 if wrong == "batch_stride_ignored" else kv_bstride, kv_lstride) % kv.shape[0]
    rows = kv[idx]                                                # (n_cols, nk, 2 inner)
    k = rows[..., :inner].reshape(n_cols, nk, heads, hd)
    v = rows[..., inner:].reshape(n_cols, nk, heads, hd)
    qi = torch.arange(n_cols)[:, None] * (0 if wrong == "q_stride_ignored" else q_col_stride) + torch.arange(Lq)[None, :]
    if wrong == "pad_query":          # the slot behind the last query read the row behind it and was stored over the last query
        qi[:, Lq - 1] = (qi[:, Lq - 1] + 1) % q.shape[0]
    qq = q[qi].reshape(n_cols, Lq, heads, hd)
    if mode == "f64":
        s = torch.einsum("cihd,cjhd->chij", qq, k)
    else:
        qw, kw = qq.to(work).permute(0, 2, 1, 3), k.to(work).permute(0, 2, 1, 3)          # (c, h, i, d), (c, h, j, d)
        s = _seq_sum(qw[..., :, None, d] * kw[..., None, :, d] for d in range(hd))
    s = s * (1.0 / hd if wrong == "scale_1_hd" else hd ** -0.5)
    if wrong == "drop_key":
        s = s[..., :Lk - 1]
        v_used = v[:, :Lk - 1]
    else:
        v_used = v
    o, p, _ = _combine(s, v_used, work, wrong)
    return o, p, v[:, :Lk].double().abs().amax(dim=(1, 3))


def scores_eval(vs, s_off, B, cols, kv_bstride, kv_lstride, Lq, Lk, heads, hd, mode="f64", wrong=None):
    """aurora_hip_perceiver_attention_scores on its own arguments (`vs` (rows, ld))."""
    work = torch.float64 if mode == "f64" else torch.float32
    inner, n_cols = heads * hd, B * cols
    assert vs.shape[1] >= s_off + Lq * heads and s_off >= inner
    rows = vs[kv_rows(B, cols, Lk, kv_bstride, kv_lstride)]       # (n_cols, Lk, ld)
    v = rows[..., :inner].reshape(n_cols, Lk, heads, hd)
    s = rows[..., s_off:s_off + Lq * heads].reshape(n_cols, Lk, Lq, heads).permute(0, 3, 2, 1)
    return _combine(s, v, work, wrong)


def head_error(out, ref, scale, Lq):
    """max_d |out - ref| / scale per (row, head): (n_cols * Lq, heads), fp64."""
    n_cols, heads = scale.shape
    diff = (out.detach().double().cpu() - ref.double()).abs().reshape(n_cols, Lq, heads, -1)
    err = diff.amax(dim=-1) / scale[:, None, :]
    return torch.where(torch.isnan(diff).any(dim=-1), torch.full_like(err, NAN), err).reshape(n_cols * Lq, heads)


def p_layout(p):
    """fp64 weights (n_cols, heads, Lq, 3) -> P (n_cols, heads, 64) as perceiver_probs lays them out: the weights of keys 0
    and 1 (the third follows from their sum), level 0 as it is, the other levels as differences to level 0, as 16 pairs per
    (column, head): pair j * NLP + lp = levels (2 lp, 2 lp + 1) of key j, NLP = ceil(Lq / 2); zeros everywhere else."""
    n_cols, heads, Lq, _ = p.shape
    nlp = (Lq + 1) // 2
    P = torch.zeros(n_cols, heads, PO_PS, dtype=p.dtype)
    for j in (0, 1):
        w = p[..., j].clone()
        w[:, :, 1:] -= p[:, :, :1, j]
        P[:, :, 2 * nlp * j:2 * nlp * j + Lq] = w
    return P


def out_scale(W, bias, v, Lq):
    """(n_cols * Lq, N): sum_k |W[n, k]| max_j |v[col, j, k]| + |bias[n]|; v (n_cols, Lk, inner)."""
    s = v.double().abs().amax(dim=1) @ W.double().abs().T
    if bias is not None:
        s = s + bias.double().abs()
    return s.repeat_interleave(Lq, dim=0)


def out_error(out, ref, scale):
    diff = (out.detach().double().cpu() - ref.double()).abs()
    return torch.where(torch.isnan(diff), torch.full_like(diff, NAN), diff / scale)


def out_model(p32, v, W, bias, wrong=None):
    """The rounding points of perceiver_probs + perceiver_out.  p32 (n_cols, heads, Lq, 3): fp32 softmax weights; v (n_cols, 3,
    heads, 64) fp32 values; W (N, inner).  Values as (v0 - v2, v1 - v2, v2) in fp32, each split hi = half(x), lo = half(x - hi);
    weights x 64 split the same way; products hi hi + hi lo + lo hi (lo lo dropped) accumulated in fp32; the softmax weights as
    level 0 and differences to it, combined in fp32; level 0 added back; / 64, + bias."""
    assert wrong is None or wrong in WRONG_OUT
    n_cols, heads, Lq, _ = p32.shape
    v = v.float()
    d = torch.stack([v[:, 0] - v[:, 2], v[:, 1] - v[:, 2], v[:, 2]], dim=1)        # (n_cols, 3, heads, 64)
    dh, dl = split_halves(d)
    wh, wl = split_halves(W.float() * 64.0)
    wh, wl = wh.reshape(-1, heads, 64), wl.reshape(-1, heads, 64)
    if wrong == "drop_lo":
        dl, wl = torch.zeros_like(dl), torch.zeros_like(wl)
    wh, wl = wh.permute(1, 2, 0), wl.permute(1, 2, 0)                               # (heads, 64, N)
    U = _seq_sum(_seq_sum(a[..., k, None] * b[:, k] for k in range(64)) for a, b in ((dh, wh), (dh, wl), (dl, wh)))   # (n_cols, 3, heads, N)
    p32 = p32.float()
    p0, p1 = p32[..., 0], p32[..., 1]                                               # (n_cols, heads, Lq)
    w0, w1 = p0.clone(), p1.clone()
    w0[:, :, 1:] -= p0[:, :, :1]
    w1[:, :, 1:] -= p1[:, :, :1]
    acc = _seq_sum(w0[:, h, :, None] * U[:, 0, h, None] + w1[:, h, :, None] * U[:, 1, h, None] for h in range(heads))   # (n_cols, Lq, N)
    if wrong == "third_weight_p2":    # the rewritten third row weighted by p2: its weight is 1, p0 + p1 + p2 is in the rewrite
        acc[:, 0] += _seq_sum(p32[:, h, 0, 2, None] * U[:, 2, h] for h in range(heads))
    else:
        acc[:, 0] += _seq_sum(U[:, 2, h] for h in range(heads))
    if wrong != "no_level0":
        acc[:, 1:] += acc[:, :1]
    out = acc.reshape(n_cols * Lq, -1) * 0.015625
    if bias is not None and wrong != "no_bias":
        out = out + bias.float()
    return out


# ------------------------------------------------------------------------------------------
# cases and inputs
# ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    B: int
    cols: int
    Lq: int
    Lk: int
    heads: int
    hd: int
    inputs: str = "flat"
    q_per_col: bool = False     # q_col_stride = Lq, per-column queries
    kv_pad: tuple = (0, 0)      # rows added to kv_lstride and kv_bstride beyond the packed cols, Lk * kv_lstride
    # the scores form
    s_gap: int = 0              # s_off = inner + s_gap
    ld_extra: int = 0
    # to_out
    N: int = 0
    bias: bool = False
    ldo_extra: int = 0
    ldw_extra: int = 0

    @property
    def inner(self):
        return self.heads * self.hd

    @property
    def n_cols(self):
        return self.B * self.cols

    @property
    def kv_lstride(self):
        return self.cols + self.kv_pad[0]

    @property
    def kv_bstride(self):
        return self.Lk * self.kv_lstride + self.kv_pad[1]

    @property
    def q_col_stride(self):
        return self.Lq if self.q_per_col else 0

    @property
    def s_off(self):
        return self.inner + self.s_gap

    @property
    def ld(self):
        return (self.s_off + self.Lq * self.heads + 3) // 4 * 4 + self.ld_extra


def tag_values(n_cols, Lk, heads, hd):
    """v[col, j, head, d] = a linear code of its own indices modulo the prime 4093, spread over +-1 in steps of 2^-11 (exact in
    fp32): any single wrong index moves the value by a sizeable fraction of the scale."""
    col = torch.arange(n_cols)[:, None, None, None]
    j = torch.arange(Lk)[None, :, None, None]
    h = torch.arange(heads)[None, None, :, None]
    d = torch.arange(hd)[None, None, None, :]
    code = (1237 * d + 611 * j + 1789 * h + 2903 * col + 977) % 4093
    return code.double() / 2048.0 - 1.0


@dataclass
class Problem:
    case: Case
    q: torch.Tensor          # (Lq or n_cols * Lq, inner) fp64, already rounded to the compute type
    kv: torch.Tensor         # (B * kv_bstride, 2 inner) fp64, NaN in the rows no column addresses
    W: Optional[torch.Tensor] = None
    bias: Optional[torch.Tensor] = None

    def args(self):
        c = self.case
        return (self.q, c.q_col_stride, self.kv, c.B, c.cols, c.kv_bstride, c.kv_lstride, c.Lq, c.Lk, c.heads, c.hd)

    def score_rows(self):
        """(B * kv_bstride, ld) fp32: [v | NaN | the scaled scores q_i . k_j / sqrt(hd), rounded to fp32, at s_off | NaN]."""
        c = self.case
        assert not c.q_per_col
        inner = c.inner
        vs = torch.full((self.kv.shape[0], c.ld), NAN, dtype=torch.float32)
        vs[:, :inner] = self.kv[:, inner:].float()
        k = self.kv[:, :inner].reshape(-1, c.heads, c.hd)
        s = torch.einsum("ihd,rhd->rih", self.q.reshape(c.Lq, c.heads, c.hd), k) * c.hd ** -0.5
        vs[:, c.s_off:c.s_off + c.Lq * c.heads] = s.reshape(-1, c.Lq * c.heads).float()
        return vs

    def score_args(self, vs):
        c = self.case
        return (vs, c.s_off, c.B, c.cols, c.kv_bstride, c.kv_lstride, c.Lq, c.Lk, c.heads, c.hd)

    def values(self):
        """(n_cols, Lk, inner) fp64 as addressed."""
        c = self.case
        return self.kv[kv_rows(c.B, c.cols, c.Lk, c.kv_bstride, c.kv_lstride)][..., c.inner:]


def problem(case: Case, dtype: str = "f32") -> Problem:
    """The inputs of a case, rounded to `dtype` (f32 / bf16) and held as fp64."""
    c = case
    assert c.inputs in INPUT_SETS and dtype in ("f32", "bf16")
    n_cols, inner, hd, heads, Lq, Lk = c.n_cols, c.inner, c.hd, c.heads, c.Lq, c.Lk
    seed = 7 * Lq + 31 * Lk + 101 * heads + hd
    nq = n_cols if c.q_per_col else 1
    q = rnd(nq, Lq, heads, hd, seed=seed + 1)
    k = rnd(n_cols, Lk, heads, hd, seed=seed + 2)
    v = rnd(n_cols, Lk, heads, hd, seed=seed + 3)
    if c.inputs == "peaked":
        # uniform +-1: q . k / sqrt(hd) has standard deviation 1 / 3; x 90 -> 30: scaled scores span about +-60, the largest
        # one wherever the draw puts it -- another key per query and per head
        q, k = q * 90 ** 0.5, k * 90 ** 0.5
    elif c.inputs in ("ascending", "descending"):
        # positive queries, keys (j + 1) x one positive direction per (column, head): scores monotone in j, ~2 apart
        q = q * 0.25 + 0.75
        w = (k[:, :1] * 0.25 + 0.75) * (2.0 / (0.5625 * hd ** 0.5))
        step = torch.arange(1, Lk + 1, dtype=torch.float64)[None, :, None, None]
        k = w * step * (1.0 if c.inputs == "ascending" else -1.0)
    elif c.inputs == "nearequal":
        sign = torch.where(rnd(n_cols, 1, heads, 1, seed=seed + 4) < 0, -1.0, 1.0)
        v = 1000.0 * sign + v
    elif c.inputs == "edge":
        # |v| in [16000, 16383], a quarter exactly 16383; keys 0 and 2 of opposite sign: |v0 - v2| up to 32766
        mag = torch.where(v.abs() < 0.25, torch.full_like(v, 16383.0), (16000.0 + 383.0 * v.abs()).round())
        sign = torch.where(rnd(n_cols, 1, heads, hd, seed=seed + 4) < 0, -1.0, 1.0).expand(-1, Lk, -1, -1).clone()
        if Lk >= 3:
            sign[:, 2] = -sign[:, 0]
        v = mag * sign
    elif c.inputs == "tagged":
        # one-hot scores: query i is a multiple of unit vector i of every head, key j holds +a there if it is the target of
        # (column, head, query) and -a otherwise, a^2 / sqrt(hd) = 60: the target 120 above the others
        assert Lq <= hd
        a = (60.0 * hd ** 0.5) ** 0.5
        a = float(torch.tensor(a).bfloat16()) if dtype == "bf16" else float(torch.tensor(a).float())
        q = torch.zeros(nq, Lq, heads, hd, dtype=torch.float64)
        q[:, torch.arange(Lq), :, torch.arange(Lq)] = a
        col = torch.arange(n_cols)[:, None, None, None]
        j = torch.arange(Lk)[None, :, None, None]
        h = torch.arange(heads)[None, None, :, None]
        i = torch.arange(hd)[None, None, None, :]
        k = torch.where(j == (col + 2 * h + i) % Lk, a, -a).double()
        v = tag_values(n_cols, Lk, heads, hd)
    q = q.reshape(nq * Lq, inner)
    kv = torch.full((c.B * c.kv_bstride, 2 * inner), NAN, dtype=torch.float64)
    kv[kv_rows(c.B, c.cols, Lk, c.kv_bstride, c.kv_lstride)] = torch.cat([k.reshape(n_cols, Lk, inner), v.reshape(n_cols, Lk, inner)], -1)
    q, kv = q.float().double(), kv.float().double()
    if dtype == "bf16":
        q, kv = round_bf16(q), round_bf16(kv)
    W = bias = None
    if c.N:
        W = rnd(c.N, inner, seed=seed + 5, scale=inner ** -0.5).float().double()
        bias = rnd(c.N, seed=seed + 6).float().double() if c.bias else None
    return Problem(c, q, kv, W, bias)


COLS = (37, 5, 11, 23, 3, 17)
HEADS = (1, 3, 4)
LK_ALL = (1, 2, 3, 4, 5, 13)
# per Lq class of the dispatch in aurora_hip_perceiver_attention_unless: QC = 3 (Lq % 3 == 0, Lq <= 6), QC = 7 (Lq > 8, head_dim
# <= 64; FEWK with Lk <= 4), QC = 4 otherwise (head_dim 128: every Lq that is not 3 or 6)
LQ_QC3, LQ_QC7, LQ_QC4 = (3, 6), (9, 13, 14, 15), (1, 2, 4, 7, 8)
EXTRA_SETS = ("peaked", "ascending", "descending", "tagged")


def _pick_B(k, cols, heads, lpg):
    """B = 2 on odd k unless that alone makes the lane count a multiple of the wave."""
    if k % 2 and not ((2 * cols * heads * lpg) % 64 == 0 and (cols * heads * lpg) % 64 != 0):
        return 2
    return 1


def _cover(prefix, hd, lqs, lks, **kw):
    n = max(len(lqs), len(lks), len(HEADS))
    out = []
    for k in range(n):
        Lq, Lk, heads, cols = lqs[k % len(lqs)], lks[k % len(lks)], HEADS[(k + hd // 16) % 3], COLS[k % len(COLS)]
        B = _pick_B(k, cols, heads, hd // 4)
        out.append(Case(f"{prefix}-hd{hd}-q{Lq}-k{Lk}-h{heads}-{B}x{cols}", B, cols, Lq, Lk, heads, hd, **kw))
    return out


def instantiations(hd):
    """{name: (Lq values, Lk values)} of perceiver_attention_kernel<T, hd, QC, FEWK>."""
    if hd == 128:
        return {"QC3": (LQ_QC3, LK_ALL), "QC4": (LQ_QC4 + LQ_QC7, LK_ALL)}
    return {"QC3": (LQ_QC3, LK_ALL), "QC7-FEWK": (LQ_QC7, (1, 2, 3, 4)), "QC7": (LQ_QC7, (5, 13)), "QC4": (LQ_QC4, LK_ALL)}


@lru_cache(maxsize=None)
def attention_cases(hd):
    """A covering list: every Lq, Lk and head count meets every instantiation it can reach; flat inputs everywhere, the other
    input sets on the first case of each instantiation (tagged needs Lq <= hd)."""
    out = []
    for name, (lqs, lks) in instantiations(hd).items():
        cs = _cover(name, hd, lqs, lks)
        out += cs
        out += [replace(cs[0], id=cs[0].id + "-" + s, inputs=s) for s in EXTRA_SETS]
    return tuple(out)


@lru_cache(maxsize=None)
def stride_cases():
    """q_col_stride = Lq with per-column queries for QC 3, 7, 7 + FEWK and 4; kv strides larger than packed."""
    shapes = [("QC3", 6, 5, 3, 64), ("QC7", 14, 5, 3, 64), ("QC7-FEWK", 13, 3, 4, 64), ("QC4", 7, 13, 1, 64),
              ("QC3", 3, 2, 3, 16), ("QC4", 15, 4, 1, 128), ("QC7-FEWK", 9, 4, 3, 32)]
    out = []
    for n, (name, Lq, Lk, heads, hd) in enumerate(shapes):
        for s in ("flat", "peaked"):
            out.append(Case(f"stride-{name}-hd{hd}-q{Lq}-k{Lk}-h{heads}-{s}", 2, 11, Lq, Lk, heads, hd, inputs=s, q_per_col=True,
                            kv_pad=(3 + n % 2, 5)))
    return tuple(out)


@lru_cache(maxsize=None)
def pair_cases():
    """fp16-pair output, inner % 32 == 0; head_dim 16: two groups share one 32-byte piece."""
    shapes = [(3, 13, 4, 16), (13, 3, 2, 16), (6, 4, 3, 32), (9, 5, 1, 32), (13, 3, 3, 64), (4, 2, 1, 64), (15, 3, 1, 128),
              (3, 5, 3, 128)]
    out = []
    for Lq, Lk, heads, hd in shapes:
        for s in ("flat", "tagged") + (("edge",) if Lk == 3 else ()):
            out.append(Case(f"pair-hd{hd}-q{Lq}-k{Lk}-h{heads}-{s}", 1, 13, Lq, Lk, heads, hd, inputs=s, s_gap=4 * (Lq % 2), ld_extra=8))
    return tuple(out)


@lru_cache(maxsize=None)
def scores_cases(hd):
    """perceiver_attention_scores_kernel<hd, QC>: the same Lq cover, every Lk; s_off > inner and ld larger than needed on every
    other case (NaN in the gaps)."""
    out = []
    for name, lqs in (("QC3", LQ_QC3), ("QC7", LQ_QC7), ("QC4", LQ_QC4)):
        cs = _cover("s" + name, hd, lqs, LK_ALL)
        cs = [replace(c, s_gap=5 * (n % 2), ld_extra=8 * (n % 2)) for n, c in enumerate(cs)]
        out += cs
        out += [replace(cs[1], id=cs[1].id + "-" + s, inputs=s) for s in ("peaked", "tagged")]
    return tuple(out)


@lru_cache(maxsize=None)
def probs_cases():
    """Lq x heads of perceiver_probs_kernel<LQ, SCORES>; heads = 2 with an odd column count ends in the middle of a wave."""
    out = []
    for Lq in (3, 4, 13):
        for heads, B, cols in ((2, 1, 37), (4, 2, 9), (16, 1, 5)):
            for s in ("flat", "peaked"):
                out.append(Case(f"probs-q{Lq}-h{heads}-{B}x{cols}-{s}", B, cols, Lq, 3, heads, 64, inputs=s, s_gap=4 * (heads == 4),
                                ld_extra=8 * (heads == 2)))
    return tuple(out)


@lru_cache(maxsize=None)
def out_cases():
    """probs -> perceiver_out.  Tiles = ceil(n_cols / 32) * N / 128; the remainder by the 8 XCDs is in the id."""
    shapes = [  # Lq, heads, N, B, cols, bias, ldo_extra, ldw_extra
        (13, 16, 128, 1, 1, True, 0, 0), (13, 2, 256, 1, 7, False, 0, 0), (13, 4, 384, 1, 31, True, 0, 0),
        (13, 6, 128, 1, 32, False, 4, 0), (13, 4, 256, 1, 33, True, 0, 0), (13, 6, 128, 1, 65, False, 0, 0),
        (3, 2, 128, 1, 221, True, 0, 0), (3, 4, 256, 1, 33, False, 4, 0), (3, 6, 384, 1, 65, True, 0, 0),
        (3, 16, 128, 1, 7, False, 0, 32), (4, 2, 256, 2, 50, True, 0, 0), (4, 4, 128, 1, 31, False, 4, 0),
        (4, 6, 384, 1, 1, True, 0, 0), (4, 16, 256, 2, 16, False, 0, 0)]
    out = []
    for Lq, heads, N, B, cols, bias, ldo_extra, ldw_extra in shapes:
        tiles = (B * cols + 31) // 32 * (N // 128)
        sets = ("flat", "peaked", "nearequal", "edge", "tagged") if (heads, cols) in ((4, 33), (4, 31)) else ("flat",)
        for s in sets:
            out.append(Case(f"out-q{Lq}-h{heads}-N{N}-{B}x{cols}-t{tiles}r{tiles % 8}-{s}", B, cols, Lq, 3, heads, 64, inputs=s, N=N,
                            bias=bias, ldo_extra=ldo_extra, ldw_extra=ldw_extra))
    return tuple(out)


HDIMS = (16, 32, 64, 128)


# ------------------------------------------------------------------------------------------
# the CPU evaluations the tolerances are multiples of
# ------------------------------------------------------------------------------------------
def f32_measure(case: Case) -> float:
    p = problem(case, "f32")
    ref, _, scale = attention_eval(*p.args())
    got, _, _ = attention_eval(*p.args(), mode="f32")
    return worst(head_error(got, ref, scale, case.Lq))


def bf16_measure(case: Case) -> float:
    """Inputs rounded to bf16, fp32 evaluation, ONE rounding of the output to bf16."""
    p = problem(case, "bf16")
    ref, _, scale = attention_eval(*p.args())
    got, _, _ = attention_eval(*p.args(), mode="f32")
    return worst(head_error(round_bf16(got), ref, scale, case.Lq))


def pair_measure(case: Case) -> float:
    p = problem(case, "f32")
    ref, _, scale = attention_eval(*p.args())
    got, _, _ = attention_eval(*p.args(), mode="f32")
    return worst(head_error(sum(split_halves(got)).double(), ref, scale, case.Lq))


def out_reference(p: Problem):
    """fp64: attention, then F.linear(., W, bias); and the scale of out_error."""
    c = p.case
    att, pw, _ = attention_eval(*p.args())
    ref = att @ p.W.T
    if p.bias is not None:
        ref = ref + p.bias
    return ref, pw, out_scale(p.W, p.bias, p.values(), c.Lq)


def out_model_of(p: Problem, wrong=None):
    c = p.case
    _, p32, _ = attention_eval(*p.args(), mode="f32")
    v = p.values().reshape(c.n_cols, 3, c.heads, 64)
    return out_model(p32, v, p.W, p.bias, wrong), p32


def out_measure(case: Case):
    p = problem(case, "f32")
    ref, pw, scale = out_reference(p)
    got, p32 = out_model_of(p)
    return worst(out_error(got, ref, scale)), (p_layout(p32.double()) - p_layout(pw)).abs().max().item()


def measure_all():
    """{name: {input set: worst}}: what the constants at the top are 8 x of."""
    table = {"f32": {}, "bf16": {}, "pair": {}, "out": {}, "P": {}}

    def fold(name, key, val):
        table[name][key] = max(table[name].get(key, 0.0), val)

    for c in [c for hd in HDIMS for c in attention_cases(hd)] + list(stride_cases()):
        fold("f32", c.inputs, f32_measure(c))
        fold("bf16", "all", bf16_measure(c))
    for c in pair_cases():
        fold("f32", c.inputs, f32_measure(c))
        fold("pair", c.inputs, pair_measure(c))
    for c in out_cases():
        o, pp = out_measure(c)
        fold("out", c.inputs, o)
    for c in probs_cases():
        p = problem(c, "f32")
        _, pw, _ = attention_eval(*p.args())
        _, p32, _ = attention_eval(*p.args(), mode="f32")
        fold("P", c.inputs, (p_layout(p32.double()) - p_layout(pw)).abs().max().item())
    return table


if __name__ == "__main__":
    for name, row in measure_all().items():
        for key, val in row.items():
            print(f"{name:5s} {key:11s} {val:.3e}")
