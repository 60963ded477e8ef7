"""fp64 definition of the window attention of csrc/attention.hip, the cases and inputs its GPU tests use, and wrong variants.

Plain torch on the CPU, written from the table contract in the header of attention.hip and NOT through
F.scaled_dot_product_attention or geometry.window_tables:

  * `tok` is (n_windows, N) int32.  tok >= 0: row `tok` of the batch element's qkv is the q | k | v of that window
    position.  tok == -1: a padded position, q = k = v = bias (zeros when bias is None).
  * score = q . k / 8 (head_dim 64), plus the LITERAL -100 where the uint8 groups of query and key differ.
  * softmax over the window's N positions, out = P V.
  * a query is stored for 0 <= tok < L_out only; rows L_out <= tok < L (halo rows of a band) are keys only.

`attention_ref` returns `(out, written, scale)`: the fp64 result (B, L_out, D), which rows a launch stores (B, L_out), and
the NATURAL SCALE (B, L_out, heads) of every (token, head): max |v| over the keys of the token's window for that head --
an output is a convex combination of those values.  Errors are judged per (token, head) as max_d |out - ref| / scale
(`row_error`), never against a maximum over the whole tensor: with outputs that are averages of up to 144 values, a
tensor-wide bound is several percent of a typical element and one dropped key passes under it.

The keyword-only `wrong` selects deliberately WRONG evaluations, each a mistake the kernel could plausibly make.  The GPU
tests never use them; tests/test_attention_reference.py shows that on the inputs below each of them lands at least
10 x BF16_TOL away from the right result (or stores other rows), i.e. that the inputs could tell such a kernel from a
correct one.
"""
from dataclasses import dataclass
from functools import lru_cache
from typing import NamedTuple, Optional

import torch

HD = 64
GROUP_IDS = (0, 1, 2, 27)     # 27: the group geometry.window_tables gives to padding (the 3 x 3 x 3 regions are 0..26)

# ------------------------------------------------------------------------------------------
# Tolerances: per-(token, head) error over the natural scale.  NOT taken from the kernels: measured on the CPU over every
# case of `all_cases()` (tools: `python -m tests.attention_reference` prints the table), then multiplied by a fixed factor.
#
#   worst row_error(f32_model, ref)   uniform    1.101e-6   (sizes, N = 144, all padding but one position, with a bias)
#                                     lowscore   6.69e-7    (sizes, N = 144, no padding)
#                                     peaked     2.151e-5   (sizes, N = 144; scores of +-100 carry |s| 2^-24 into the exponent)
#                                     mask128    1.994e-5   (groups, N = 24; scores of 128, see below)
#   worst row_error(bf16_model, ref)  all cases  3.133e-3   (items, N = 16, 2001 windows x 3 heads; the other groups of
#                                                            cases 2.5e-3 .. 2.9e-3: one bf16 rounding of an output near
#                                                            the scale is up to 2^-9 = 1.95e-3, the rounded weights add)
#
# F32_TOL = 8 x: the kernel's online softmax and expf differ from torch's two-pass softmax in order and in the last ulp.
# The factor is applied PER INPUT SET, which is never looser than 8 x the worst over all sets: the ordinary (uniform,
# lowscore) cases are held to 8.8e-6 and not to the 1.7e-4 the peaked scores would allow.  The adversarial mask input has
# its own constant, derived the same way on that input alone: a score of 128 carries an absolute rounding error of
# ~128 x 2^-23, which the exponential turns into a relative error of the weights (tests/test_gpu_ops.py).
# BF16_TOL = 4 x: the kernel adds fp32 MFMA accumulation order, a hardware exp2 and rcp to the same rounding points.
# tests/test_attention_reference.py re-measures the four worst cases and fails if a constant below is out of date.
# ------------------------------------------------------------------------------------------
F32_FACTOR, BF16_FACTOR = 8.0, 4.0
F32_MEASURED = {"uniform": 1.101e-6, "lowscore": 6.69e-7, "peaked": 2.151e-5, "mask128": 1.994e-5}
BF16_MEASURED = 3.133e-3
F32_TOL = F32_FACTOR * max(F32_MEASURED["uniform"], F32_MEASURED["lowscore"])     # 8.8e-6
F32_TOL_PEAKED = F32_FACTOR * F32_MEASURED["peaked"]                               # 1.7e-4
F32_TOL_MASK128 = F32_FACTOR * F32_MEASURED["mask128"]                             # 1.6e-4
BF16_TOL = BF16_FACTOR * BF16_MEASURED                                             # 1.25e-2
TEETH = 10.0                  # every wrong variant is >= TEETH x BF16_TOL away


def f32_tol(inputs: str) -> float:
    return {"peaked": F32_TOL_PEAKED, "mask128": F32_TOL_MASK128}.get(inputs, F32_TOL)


def rnd32(*shape, seed=0, scale=1.0):
    """Uniform in +-scale, drawn in float32 (the large cases hold > 1e8 values)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1) * scale


def round_bf16(x: torch.Tensor) -> torch.Tensor:
    return x.float().bfloat16().to(x.dtype)


def row_error(out: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """max_d |out - ref| / scale per (token, head): (B, L_out, heads), fp64 on the CPU.  NaN anywhere in a head's 64 columns
    makes that entry NaN.  Index the result with `written` -- rows no launch stores have no reference."""
    B, L_out, heads = scale.shape
    diff = (out.detach().double().cpu().reshape(B, L_out, heads, HD) - ref.reshape(B, L_out, heads, HD)).abs()
    err = diff.amax(dim=-1) / scale
    return torch.where(torch.isnan(diff).any(dim=-1), torch.full_like(err, float("nan")), err)


def worst(err: torch.Tensor) -> float:
    """The largest error; NaN if any is NaN (so that `worst(e) <= tol` fails on NaN)."""
    if err.numel() == 0:
        return 0.0
    return float("nan") if torch.isnan(err).any() else err.max().item()


def to_planes(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """(B, L, 3 D) token-major -> (heads, B * L, 3, 64): what linear_planes writes, one attention head per plane."""
    B, L, D3 = qkv.shape
    assert D3 == 3 * heads * HD
    return qkv.reshape(B * L, 3, heads, HD).permute(2, 0, 1, 3).contiguous()


WRONG = ("mask_xor", "mask_inf", "drop_last_key", "admit_zero_key", "ignore_halo_keys", "half_row_from_partner",
         "batch1_reads_batch0", "head_xor_1", "item_shift_rows", "item_shift_planes", "swap_pieces")


def _evaluate(qkv, bias, tok, grp, B, L, L_out, D, heads, mode, wrong=None, chunk=128, piece=2):
    assert mode in ("f64", "f32", "bf16") and (wrong is None or wrong in WRONG)
    assert qkv.shape == (B, L, 3 * D) and D == heads * HD and 0 < L_out <= L
    work = torch.float32 if mode == "f32" else torch.float64
    tok = torch.as_tensor(tok).long()
    nW, N = tok.shape
    assert int(tok.min()) >= -1 and int(tok.max()) < L
    g_all = None if grp is None else torch.as_tensor(grp).long()
    bias_row = torch.zeros(3 * D, dtype=work) if bias is None else bias.detach().cpu().to(work)
    if mode == "bf16":
        bias_row = round_bf16(bias_row)
    out = torch.zeros((B, L_out, D), dtype=work)
    written = torch.zeros((B, L_out), dtype=torch.bool)
    scale = torch.ones((B, L_out, heads), dtype=torch.float64)
    if wrong in ("item_shift_rows", "item_shift_planes"):
        chunk = nW          # the shift crosses windows
    for w0 in range(0, nW, chunk):
        t = tok[w0:w0 + chunk]
        c = t.shape[0]
        rows = qkv[:, t.clamp(min=0)]                                   # (B, c, N, 3 D)
        rows = (round_bf16(rows.float()) if mode == "bf16" else rows).to(work)
        rows = torch.where((t >= 0)[None, :, :, None], rows, bias_row)
        if wrong == "batch1_reads_batch0" and B > 1:
            rows[1] = rows[0]
        q, k, v = rows.reshape(B, c, N, 3, heads, HD).permute(3, 0, 1, 4, 2, 5)   # each (B, c, heads, N, 64)
        if wrong == "head_xor_1":
            hx = torch.tensor([h ^ 1 if (h ^ 1) < heads else h for h in range(heads)])
            q, k, v = q[:, :, hx], k[:, :, hx], v[:, :, hx]
        s = (q @ k.transpose(-1, -2)) * 0.125                           # (B, c, heads, N, N): [query, key]
        if g_all is not None:
            g = g_all[w0:w0 + c]
            if wrong == "mask_xor":
                m = -100.0 * (g[:, :, None] ^ g[:, None, :]).to(work)
            else:
                m = torch.where(g[:, :, None] != g[:, None, :], float("-inf") if wrong == "mask_inf" else -100.0, 0.0).to(work)
            s = s + m[None, :, None]
        if wrong == "drop_last_key" and N % 16:
            s[..., N - 1] = float("-inf")
        if wrong == "ignore_halo_keys":
            s = s.masked_fill((t >= L_out)[None, :, None, None, :], float("-inf"))
        if wrong == "admit_zero_key" and N % 16:                        # key N of the last tile: k = v = 0, score 0
            s = torch.cat((s, torch.zeros_like(s[..., :1])), dim=-1)
            v = torch.cat((v, torch.zeros_like(v[..., :1, :])), dim=-2)
        if mode == "f32":
            o = torch.softmax(s, dim=-1) @ v
        else:
            e = torch.exp(s - s.amax(dim=-1, keepdim=True))
            if mode == "bf16":
                e = round_bf16(e)
            o = (e @ v) / e.sum(dim=-1, keepdim=True)
            if mode == "bf16":
                o = round_bf16(o)
        sc = v.abs().amax(dim=(-1, -2)).double()                        # (B, c, heads)
        if wrong == "item_shift_rows":                                  # items in (b, window, head) order
            o = o.reshape(B * c * heads, N, HD).roll(1, dims=0).reshape(B, c, heads, N, HD)
        if wrong == "item_shift_planes":                                # items in (b, head, window) order
            o = o.transpose(1, 2).reshape(B * heads * c, N, HD).roll(1, dims=0).reshape(B, heads, c, N, HD).transpose(1, 2)
        o = o.permute(0, 1, 3, 2, 4)                                    # (B, c, N, heads, 64)
        if wrong == "half_row_from_partner":
            n = torch.arange(N)
            partner = torch.where((n ^ 8) < N, n ^ 8, n)
            o = torch.cat((o[..., :32], o[:, :, partner][..., 32:]), dim=-1)
        if wrong == "swap_pieces":
            o = o.clone()
            a, b_ = piece * 8, piece * 8 + 8
            o[..., a:b_], o[..., b_:b_ + 8] = o[..., b_:b_ + 8].clone(), o[..., a:b_].clone()
        live = (t >= 0) & (t < L_out)
        out[:, t[live]] = o.reshape(B, c, N, D)[:, live]
        written[:, t[live]] = True
        scale[:, t[live]] = sc[:, :, None, :].expand(B, c, N, heads)[:, live]
    return out, written, scale


def attention_ref(qkv, bias, tok, grp, B, L, L_out, D, heads, *, wrong: Optional[str] = None, chunk: int = 128):
    """The fp64 evaluation; see the module docstring.  `qkv` (B, L, 3 D) may be held in a narrower type: every chunk of
    windows is converted to fp64 as it is gathered, so that the large cases need no fp64 copy of the whole input."""
    return _evaluate(qkv, bias, tok, grp, B, L, L_out, D, heads, "f64", wrong, chunk)


def bf16_model(qkv, bias, tok, grp, B, L, L_out, D, heads, *, chunk: int = 128):
    """The same evaluation with the bf16 kernel's documented rounding points: inputs and bias rounded to bf16, the
    probabilities exp(s - max) rounded to bf16 and normalised by the sum of the ROUNDED values, the output rounded once."""
    return _evaluate(qkv, bias, tok, grp, B, L, L_out, D, heads, "bf16", None, chunk)


def f32_model(qkv, bias, tok, grp, B, L, L_out, D, heads, *, chunk: int = 128):
    """The plain evaluation in torch float32 on the CPU (matmul, torch.softmax, matmul)."""
    return _evaluate(qkv, bias, tok, grp, B, L, L_out, D, heads, "f32", None, chunk)


def stored_rows(tok, B: int, L_out: int, guard: int, wrong: Optional[str] = None) -> torch.Tensor:
    """Which of the B * L_out + guard rows of a flat output buffer a launch stores: row b * L_out + tok for
    0 <= tok < L_out.  WRONG `halo`: the `tok < L_out` test is missing (a halo row lands in the next batch element or in
    the guard rows).  WRONG `pad`: padded queries are stored too (row b * L_out - 1)."""
    tok = torch.as_tensor(tok).long().reshape(-1)
    rows = torch.zeros(B * L_out + guard, dtype=torch.bool)
    for b in range(B):
        keep = (tok >= 0) & (tok < L_out)
        if wrong == "halo":
            keep = tok >= 0
        if wrong == "pad":
            keep = keep | ((tok == -1) & (b > 0))
        rows[b * L_out + tok[keep]] = True
    return rows


# ------------------------------------------------------------------------------------------
# hand-built tables
# ------------------------------------------------------------------------------------------
def _positions(spec, n_windows: int, N: int) -> torch.Tensor:
    """None | positions (every window) | {window: positions} | bool (n_windows, N)  ->  bool (n_windows, N)"""
    m = torch.zeros((n_windows, N), dtype=torch.bool)
    if spec is None:
        return m
    if isinstance(spec, torch.Tensor):
        assert spec.shape == (n_windows, N) and spec.dtype == torch.bool
        return spec.clone()
    if isinstance(spec, dict):
        for w, pos in spec.items():
            m[w, list(pos)] = True
        return m
    m[:, list(spec)] = True
    return m


def hand_tables(n_windows: int, N: int, L: int, seed: int, pad=None, groups: Optional[str] = None, halo=None):
    """(tok int32 (n_windows, N), grp uint8 or None): a random assignment of the L tokens to window positions, each token
    at most once (tokens that find no position are in no window and are never stored; token L_out - 1 is one of them).
    `pad`: the positions that are -1 -- a list (every window), {window: positions} or a bool (n_windows, N).
    `groups`: None (no table) | "uniform" (one id per window, differing between windows) | "mixed" (a random id of
    GROUP_IDS per position).
    `halo`: (L_out, positions): those positions (same forms as `pad`; a padded one stays padded) take tokens >= L_out,
    every other one a token < L_out."""
    g = torch.Generator().manual_seed(seed)
    is_pad = _positions(pad, n_windows, N)
    L_out, halo_pos = (L, None) if halo is None else halo
    is_halo = _positions(halo_pos, n_windows, N) & ~is_pad
    is_own = ~is_pad & ~is_halo
    n_own, n_halo = int(is_own.sum()), int(is_halo.sum())
    assert n_own <= L_out and n_halo <= L - L_out, (n_own, L_out, n_halo, L)
    tok = torch.full((n_windows, N), -1, dtype=torch.int32)
    perm = torch.randperm(L_out, generator=g)
    if n_own < L_out:       # token L_out - 1 stays free: a padded query stored "at row -1" of batch element b + 1 lands there
        at = int(torch.nonzero(perm == L_out - 1))
        perm[[at, L_out - 1]] = perm[[L_out - 1, at]]
    tok[is_own] = perm[:n_own].int()
    if n_halo:
        tok[is_halo] = (L_out + torch.randperm(L - L_out, generator=g)[:n_halo]).int()
    grp = None
    ids = torch.tensor(GROUP_IDS, dtype=torch.uint8)
    if groups == "uniform":
        grp = ids[torch.arange(n_windows) % len(ids)][:, None].expand(n_windows, N).contiguous()
    elif groups == "mixed":
        grp = ids[torch.randint(len(ids), (n_windows, N), generator=g)]
    else:
        assert groups is None
    return tok, grp


# ------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_attention.py (shared with tests/test_attention_reference.py, which shows their teeth)
# ------------------------------------------------------------------------------------------
WINDOW_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 36, 47, 48, 49, 64, 95, 96, 97, 128, 129, 143, 144]
GROUP_SIZES = [24, 143, 144]
PLANE_HEADS, ROW_HEADS, WIDE_SIZES = [1, 3, 32], [5, 32], [36, 144]
PEAKED_SIZES = [17, 144]
# Item counts B x n_windows x heads on both sides of the thresholds of aurora_hip_window_attention_planes in
# csrc/attention.hip (xcd_order from 6000 items in the row layout, from 3000 on head planes) and with every kind of
# remainder of the count by the 8 XCDs.  THEY FOLLOW THOSE THRESHOLDS AND MUST MOVE WITH THEM.  An odd count cannot have
# B = 2: those run with B = 1; 6004 / 3004 add a non-zero remainder at B = 2.      (items: (B, heads, n_windows))
ITEMS_ROWS = {5999: (1, 7, 857), 6000: (2, 2, 1500), 6003: (1, 3, 2001), 6004: (2, 2, 1501), 6007: (1, 1, 6007)}
ITEMS_PLANES = {2999: (1, 1, 2999), 3000: (2, 2, 750), 3003: (1, 3, 1001), 3004: (2, 2, 751), 3007: (1, 31, 97)}
ITEMS_ROWS_144, ITEMS_PLANES_144 = (2, 2, 1501), (2, 2, 751)    # N = 144 above the threshold; 48 live tokens per window


@dataclass(frozen=True)
class Case:
    group: str
    N: int
    pad: str = "none"             # none | ends | tile | lone | live48
    bias: bool = True
    inputs: str = "uniform"       # uniform | lowscore | peaked | mask128
    groups: Optional[str] = None  # None | uniform | mixed
    halo: bool = False
    B: int = 2
    heads: int = 2
    n_windows: int = 5
    layouts: tuple = ("rows",)    # layouts the bf16 kernel runs in
    dtypes: tuple = ("f32", "bf16")

    @property
    def id(self) -> str:
        parts = [self.group, f"N{self.N}", self.pad, "bias" if self.bias else "nobias", self.inputs]
        if self.groups:
            parts.append("grp-" + self.groups)
        if self.halo:
            parts.append("halo")
        if (self.B, self.heads, self.n_windows) != (2, 2, 5):
            parts.append(f"B{self.B}h{self.heads}w{self.n_windows}")
        return "-".join(parts)


class Problem(NamedTuple):
    qkv: torch.Tensor            # (B, L, 3 D) in the kernel's type
    bias: Optional[torch.Tensor]       # fp32, what the launch receives
    bias_seen: Optional[torch.Tensor]  # what the kernel makes of it (bf16 kernel: rounded to bf16)
    tok: torch.Tensor
    grp: Optional[torch.Tensor]
    B: int
    L: int
    L_out: int
    D: int
    heads: int

    def args(self, qkv=None, bias="seen"):
        return (self.qkv if qkv is None else qkv, self.bias_seen if bias == "seen" else bias, self.tok, self.grp,
                self.B, self.L, self.L_out, self.D, self.heads)


def _pad_spec(case: Case):
    N, nW = case.N, case.n_windows
    if case.pad == "none":
        return None
    if case.pad == "ends":                    # -1 at position 0 and at position N - 1
        return [0, N - 1]
    if case.pad == "tile":                    # a whole 16-position tile of -1, another one in every window
        full = N // 16
        assert N >= 17, "a window of one tile would be all padding"
        return {w: range(16 * (w % full), 16 * (w % full) + 16) for w in range(nW)}
    if case.pad == "lone":                    # all -1 but one position
        keep = [0, N - 1, N // 2, min(15, N - 1), 16 if N > 16 else 0]
        return {w: [p for p in range(N) if p != keep[w % 5]] for w in range(nW)}
    if case.pad == "live48":                  # 48 live positions per window, at random (the large N = 144 cases)
        g = torch.Generator().manual_seed(77)
        return torch.rand((nW, N), generator=g).argsort(dim=1) >= 48
    raise ValueError(case.pad)


def _halo_spec(case: Case):
    """Within tile 0 of window 0: query i owned and i ^ 8 a halo row (0, 8), the reverse (1, 9), i padded and its partner
    owned (2, 10), the reverse (3, 11), a padded query with a halo partner (4, 12), a pair of halo rows (5, 13); window 1:
    tile 0 all halo rows; window 2: a third of the positions at random (and a tenth padded); window 3: none; window 4:
    nothing but halo rows (no store at all).  N >= 32: tile 1 of window 0 is all halo rows as well."""
    N, nW = case.N, case.n_windows
    assert N >= 24 and nW == 5
    g = torch.Generator().manual_seed(78)
    halo = {0: [8, 1, 12, 5, 13] + (list(range(16, 32)) if N >= 32 else []), 1: range(16),
            2: torch.nonzero(torch.rand(N, generator=g) < 1 / 3).flatten().tolist(), 4: range(N)}
    pad = {0: [2, 11, 4], 2: torch.nonzero(torch.rand(N, generator=g) < 0.1).flatten().tolist()}
    return pad, halo


_TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}


@lru_cache(maxsize=4)
def problem(case: Case, dtype: str) -> Problem:
    """The inputs of one case in the kernel's type `dtype`; the references take these ROUNDED values."""
    B, heads, nW, N = case.B, case.heads, case.n_windows, case.N
    D = heads * HD
    pad = _positions(_pad_spec(case), nW, N)
    halo = None
    if case.halo:
        pad_h, halo_h = _halo_spec(case)
        pad = _positions(pad_h, nW, N)
        is_halo = _positions(halo_h, nW, N) & ~pad
        n_halo = int(is_halo.sum())
        L_out = int((~pad & ~is_halo).sum()) + 2
        L = L_out + n_halo + 2
        halo = (L_out, is_halo)
    else:
        L = L_out = int((~pad).sum()) + 3                   # three tokens are in no window: their rows stay untouched
    tok, grp = hand_tables(nW, N, L, seed=100 + N, pad=pad, groups=case.groups, halo=halo)
    dt = _TORCH_DTYPE[dtype]
    qkv = torch.empty((B, L, 3, heads, HD), dtype=dt)
    for b in range(B):
        x = rnd32(L, 3, heads, HD, seed=11 + b, scale=2.0)
        if case.inputs == "peaked":          # scores of standard deviation ~30 (uniform: 4/3): the softmax is almost one-hot
            x[:, :2] *= (30.0 * 0.75) ** 0.5
        elif case.inputs == "lowscore":      # every score ~ -8 and every value in [1, 2]: a key of score 0 admitted by
            x[:, 0, :, :16] = 2.0            # mistake (k = 0: a row beyond the window, a padded row without its bias)
            x[:, 1, :, :16] = -2.0           # takes most of the weight, and v = 0 then moves the output by about the scale
            x[:, 2] = 1.5 + 0.25 * x[:, 2]
        elif case.inputs == "mask128":       # tests/test_gpu_ops.py: the keys of each window's largest group score 128
            assert grp is not None           # against every query, every other key about 0
            x *= 0.25
            loud = torch.zeros(L, dtype=torch.bool)
            for w in range(nW):
                there = tok[w] >= 0
                top = grp[w][there].max()
                loud[tok[w][there & (grp[w] == top)].long()] = True
            x[:, 0, :, 0] = 16.0
            x[:, 1, :, 0] = torch.where(loud[:, None], 64.0, 0.0)
        else:
            assert case.inputs == "uniform"
        qkv[b] = x.to(dt)
    bias = rnd32(3 * D, seed=12) if case.bias else None
    seen = None if bias is None else (bias.bfloat16().float() if dtype == "bf16" else bias)
    return Problem(qkv.reshape(B, L, 3 * D), bias, seen, tok, grp, B, L, L_out, D, heads)


def window_size_cases(N: int):
    """Every padding form with and without a bias on uniform inputs; the low-score inputs, where a zero key could slip in;
    the peaked inputs, where every key is the only one that counts for some query (a dropped key is a wrong row)."""
    pads = ["none", "ends"] + (["tile"] if N >= 17 else []) + ["lone"]
    out = [Case("sizes", N, pad=p, bias=b) for p in pads for b in (True, False)]
    out += [Case("sizes", N, pad="none", inputs="lowscore"), Case("sizes", N, pad="ends", inputs="lowscore"),
            Case("sizes", N, pad="ends", bias=False, inputs="lowscore"), Case("sizes", N, pad="none", inputs="peaked")]
    return out


def group_cases(N: int):
    return [Case("groups", N, groups=None, pad="ends"), Case("groups", N, groups="uniform", pad="ends"),
            Case("groups", N, groups="mixed", pad="ends"), Case("groups", N, groups="mixed", pad="ends", inputs="mask128")]


def halo_cases(N: int):
    return [Case("halo", N, halo=True, groups="mixed", layouts=("rows", "planes")),
            Case("halo", N, halo=True, bias=False, inputs="peaked", layouts=("rows", "planes"))]


def plane_cases(heads: int, N: int):
    return [Case("planes", N, pad="ends", groups="mixed", heads=heads, layouts=("planes",), dtypes=("bf16",))]


def wide_row_cases(heads: int, N: int):
    return [Case("wide", N, pad="ends", groups="mixed", heads=heads)]


def peaked_cases(N: int):
    return [Case("peaked", N, pad="ends", groups="mixed", inputs="peaked", layouts=("rows", "planes"))]


def item_cases(layout: str, items: int):
    B, heads, nW = (ITEMS_ROWS if layout == "rows" else ITEMS_PLANES)[items]
    assert B * heads * nW == items
    return [Case("items", 16, B=B, heads=heads, n_windows=nW, groups="mixed", layouts=(layout,), dtypes=("bf16",))]


def item_cases_144(layout: str):
    B, heads, nW = ITEMS_ROWS_144 if layout == "rows" else ITEMS_PLANES_144
    return [Case("items", 144, pad="live48", B=B, heads=heads, n_windows=nW, groups="mixed", layouts=(layout,), dtypes=("bf16",))]


def all_cases():
    out = []
    for N in WINDOW_SIZES:
        out += window_size_cases(N)
    for N in GROUP_SIZES:
        out += group_cases(N) + halo_cases(N)
    for N in WIDE_SIZES:
        for h in PLANE_HEADS:
            out += plane_cases(h, N)
        for h in ROW_HEADS:
            out += wide_row_cases(h, N)
    for N in PEAKED_SIZES:
        out += peaked_cases(N)
    for n in ITEMS_ROWS:
        out += item_cases("rows", n)
    for n in ITEMS_PLANES:
        out += item_cases("planes", n)
    return out + item_cases_144("rows") + item_cases_144("planes")


def measure(cases=None, verbose=False):
    """({input set: worst row_error(f32_model, ref)}, worst row_error(bf16_model, ref)) over `cases`."""
    f32, bf16 = {}, 0.0
    for case in (all_cases() if cases is None else cases):
        for dtype in case.dtypes:
            p = problem(case, dtype)
            ref, written, scale = attention_ref(*p.args())
            model = f32_model if dtype == "f32" else bf16_model
            err = worst(row_error(model(*p.args())[0], ref, scale)[written])
            if dtype == "f32":
                f32[case.inputs] = max(f32.get(case.inputs, 0.0), err)
            else:
                bf16 = max(bf16, err)
            if verbose:
                print(f"{case.id:60s} {dtype:5s} {err:.3e}", flush=True)
    return f32, bf16


if __name__ == "__main__":
    torch.set_num_threads(16)
    print(measure(verbose=True))
