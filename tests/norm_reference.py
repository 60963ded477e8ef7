"""fp64 definitions of the three row normalisations of csrc/norm.hip, the inputs their GPU tests use, and wrong variants.

Plain torch on the CPU, written from the operators' definitions and not from oracle/ (tests/test_norm_reference.py
cross-checks the two).  Every reference returns `(out, scale)`: the fp64 result and the NATURAL SCALE of each row,
max_j(|LN * gain| + |shift| + |res|) -- the size of the terms an fp32 evaluation has to round.  Errors are judged row by
row as max_j |out - ref| / scale[row] (`row_error`), never against a maximum over the whole tensor: one wrong row among
thousands, or an error that is large only against a small row, then shows.

The keyword-only arguments select deliberately WRONG evaluations, each a mistake a kernel could plausibly make.  The GPU
tests never use them; tests/test_norm_reference.py shows that on the inputs below each of them lands at least 100 x the
GPU tolerance away from the right result, i.e. that the inputs could tell such a kernel from a correct one.
"""
from typing import Optional

import torch

F32_TOL = 3e-6          # per-row error over the natural scale of every fp32 result (the project's fp32 LN tolerance)
PIECE = 8               # features per lane piece of merge_ln / split_ln (two 4-feature pieces of layernorm)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def row_error(out: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """max_j |out - ref| / scale, per row (fp64, CPU).  NaN anywhere in a row makes that row's error NaN."""
    diff = (out.detach().double().cpu() - ref).abs()
    err = diff.max(dim=1).values / scale
    return torch.where(torch.isnan(diff).any(dim=1), torch.full_like(err, float("nan")), err)


def worst(err: torch.Tensor) -> float:
    """The largest per-row error; NaN if any row is NaN (so that `worst(e) <= tol` fails on NaN)."""
    return float("nan") if torch.isnan(err).any() else err.max().item()


def swap_piece(out: torch.Tensor, piece: int) -> torch.Tensor:
    """`out` with the 8-feature piece `piece` of every row exchanged with the next one (a lane's store gone astray)."""
    o = out.clone()
    a, b = piece * PIECE, (piece + 1) * PIECE
    assert b + PIECE <= out.shape[1]
    o[:, a:b], o[:, b:b + PIECE] = out[:, b:b + PIECE], out[:, a:b]
    return o


def _normalise(x: torch.Tensor, eps: float, *, one_pass_f32: bool = False, valid: Optional[torch.Tensor] = None):
    """LN without affine over the last axis of fp64 `x`: two-pass population statistics.
    WRONG `one_pass_f32`: the variance as E[x^2] - mean^2, everything in fp32 (clamped at 0, as such kernels do).
    WRONG `valid` (a 0/1 mask like x): the statistics are taken over the marked elements only."""
    if one_pass_f32:
        x32 = x.float()
        n = x32.shape[-1]
        mean = x32.sum(-1, keepdim=True) / n
        var = ((x32 * x32).sum(-1, keepdim=True) / n - mean * mean).clamp_min(0.0)
        return ((x32 - mean) * torch.rsqrt(var + eps)).double()
    if valid is not None:
        n = valid.sum(-1, keepdim=True).clamp_min(1.0)
        mean = (x * valid).sum(-1, keepdim=True) / n
        var = (((x - mean) ** 2) * valid).sum(-1, keepdim=True) / n
    else:
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps)


def layernorm_ref(y, gain=None, shift=None, res=None, res_mod: int = 0, eps: float = 1e-5, d: Optional[int] = None, *,
                  one_pass_f32: bool = False, ignore_res_mod: bool = False):
    """res[row % res_mod] + LN(y[:, :d]) * gain + shift in fp64; every operand optional.  Returns (out, scale).
    WRONG `ignore_res_mod`: residual row = row (clamped to the rows there are) instead of row % res_mod."""
    d = y.shape[1] if d is None else d
    M = y.shape[0]
    ln = _normalise(y[:, :d].detach().double().cpu(), eps, one_pass_f32=one_pass_f32)
    if gain is not None:
        ln = ln * gain[:d].double().cpu()
    out, scale = ln, ln.abs()
    if shift is not None:
        s = shift[:d].double().cpu()
        out, scale = out + s, scale + s.abs()
    if res is not None:
        r = res.detach().double().cpu()[:, :d]
        rows = torch.arange(M)
        if res_mod > 0:
            rows = rows.clamp(max=r.shape[0] - 1) if ignore_res_mod else rows % res_mod
        r = r[rows]
        out, scale = out + r, scale + r.abs()
    return out, scale.max(dim=1).values


def merge_ln_ref(x, w, b, B: int, C: int, H: int, W: int, D: int, eps: float = 1e-5, *,
                 stats_skip_padding: bool = False, seg_order_dw_dh: bool = False):
    """2x2 gather of x (B, C, H, W, D) in (dh, dw, D) order -> LN over 4D.  Cells below / right of an odd grid are zero
    and COUNT in the row's statistics.  Returns ((B*C*H2*W2, 4D), scale).
    WRONG `stats_skip_padding`: mean and variance over the cells that exist only.
    WRONG `seg_order_dw_dh`: the four cells laid out as (dw, dh)."""
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    xs = x.detach().double().cpu().reshape(B * C, H, W, D)
    rows = torch.zeros(B * C, H2, W2, 4, D, dtype=torch.float64)
    there = torch.zeros(B * C, H2, W2, 4, D, dtype=torch.float64)
    for dh in range(2):
        for dw in range(2):
            seg = dw * 2 + dh if seg_order_dw_dh else dh * 2 + dw
            src = xs[:, dh::2, dw::2]                      # cells (2 h2 + dh, 2 w2 + dw) that exist
            rows[:, :src.shape[1], :src.shape[2], seg] = src
            there[:, :src.shape[1], :src.shape[2], seg] = 1.0
    rows, there = rows.reshape(-1, 4 * D), there.reshape(-1, 4 * D)
    ln = _normalise(rows, eps, valid=there if stats_skip_padding else None) * w.double().cpu()
    bb = b.double().cpu()
    return ln + bb, (ln.abs() + bb.abs()).max(dim=1).values


def split_ln_ref(y, w, b, B: int, C: int, H: int, W: int, Dq: int, crop_h: int, crop_w: int, eps: float = 1e-5, *,
                 crop_first: bool = False):
    """Pixel shuffle of y (B, C, H, W, [dh, dw, Dq]) to (B, C, 2H, 2W, Dq), the LAST crop_h rows / crop_w columns
    dropped, LN over Dq.  Returns ((B*C*Ho*Wo, Dq), scale).
    WRONG `crop_first`: the first row / column dropped instead."""
    ys = y.detach().double().cpu().reshape(B * C, H, W, 2, 2, Dq)
    full = torch.empty(B * C, 2 * H, 2 * W, Dq, dtype=torch.float64)
    for dh in range(2):
        for dw in range(2):
            full[:, dh::2, dw::2] = ys[:, :, :, dh, dw]
    Ho, Wo = 2 * H - crop_h, 2 * W - crop_w
    g = full[:, crop_h:, crop_w:] if crop_first else full[:, :Ho, :Wo]
    ln = _normalise(g.reshape(-1, Dq), eps) * w.double().cpu()
    bb = b.double().cpu()
    return ln + bb, (ln.abs() + bb.abs()).max(dim=1).values


# ------------------------------------------------------------------------------------------
# the cases and inputs of tests/test_gpu_norm.py (shared with tests/test_norm_reference.py, which shows their teeth)
# ------------------------------------------------------------------------------------------
LN_WIDTHS = [8, 72, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4088, 4096]   # NC 1|2|4|8|16: both sides of each boundary
LN_ROWS = [1, 3, 6, 1001]
RES_MOD = 5
LARGE_MEANS = [1e2, 1e4]
LARGE_MEAN_WIDTHS = [264, 2048]
LARGE_MEAN_ROWS = 1001
SPLIT_LN_WIDTHS = [32, 96, 544, 1024, 2080]
SPLIT_LN_ROWS = [1, 7, 1001]
MERGE_WIDTHS = [8, 64, 128, 136, 256, 264, 512, 1024]                          # 4D: MAXC 1|2|4|8, both sides of each boundary
MERGE_GRIDS = [(6, 8), (7, 9), (1, 5), (5, 1), (1, 1)]
SPLIT_WIDTHS = [8, 32, 512, 520, 1024, 1032, 2048, 2056, 4096]
SPLIT_GRIDS = [(3, 4), (1, 3), (4, 1)]
CROPS = [(0, 0), (1, 0), (0, 1), (1, 1)]
BC = (2, 3)


def ln_inputs(M: int, D: int, dtype: torch.dtype):
    """(y in `dtype`, gain, shift, full residual (M rows), cyclic residual (RES_MOD rows)); the fp64 references take the
    rounded y.  Rows of mean ~0.5 and spread ~1.7, as the backbone's; the large-mean rows have their own inputs."""
    y = (rnd(M, D, seed=1, scale=3.0) + 0.5).to(dtype)
    return (y, (rnd(D, seed=2) + 1).float(), rnd(D, seed=3).float(), rnd(M, D, seed=4).float(),
            rnd(RES_MOD, D, seed=5).float())


def eps_inputs(M: int, D: int):
    """Rows of spread 1e-2 about zero for eps = 1e-3: the variance, ~3e-5, is a thirtieth of eps."""
    return rnd(M, D, seed=6, scale=1e-2).float()


def large_mean_inputs(c: float, D: int):
    """fp32 rows c + z, z uniform in +-1 (rounded to fp32 BEFORE any reference sees them)."""
    return (c + rnd(LARGE_MEAN_ROWS, D, seed=7)).float()


def merge_inputs(H: int, W: int, D: int):
    """(x (B, C, H, W, D) uniform in 2 +- 1 -- the zero padding of an odd grid visibly moves the mean --, weight, bias)"""
    B, C = BC
    return (rnd(B, C, H, W, D, seed=8) + 2.0).float(), (rnd(4 * D, seed=9) + 1).float(), rnd(4 * D, seed=10).float()


def split_inputs(H: int, W: int, Dq: int, dtype: torch.dtype):
    B, C = BC
    y = (rnd(B * C * H * W, 4 * Dq, seed=11, scale=3.0) + 0.5).to(dtype)
    return y, (rnd(Dq, seed=12) + 1).float(), rnd(Dq, seed=13).float()


LARGE_MEAN_FACTOR = 4.0   # a 64-lane tree against a sequential / cascaded sum: a small constant factor at most


def large_mean_bound(y: torch.Tensor, eps: float = 1e-5):
    """(bound, measured): the worst per-row error of torch's CPU fp32 layer_norm on these rows against fp64, and
    LARGE_MEAN_FACTOR times it -- what a two-pass fp32 kernel that sums in another order may show."""
    ref, scale = layernorm_ref(y, eps=eps)
    measured = worst(row_error(torch.nn.functional.layer_norm(y.float().cpu(), y.shape[1:], eps=eps), ref, scale))
    return LARGE_MEAN_FACTOR * measured, measured
