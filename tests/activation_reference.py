"""The activations of the GEMM epilogues (csrc/common.h, csrc/gemm_tile.h) on their own: operands that put an EXACTLY known
fp32 value in front of the activation of any linear, the fp64 definitions, the per-form error bound, the special values, fp32
emulations of every form, and wrong variants.  Plain torch on the CPU; tests/test_gpu_activations.py runs the kernels.

Exact pre-activations.  A linear whose operands are zero except for column 0 computes, in every kernel,
    pre[m, n] = fl32(s[m] * w[n] + bias[n])              a[m, 0] = s[m],  w[n, 0] = w[n]:
the product is exact and the other K - 1 terms are exact zeros.  s has at most 8 significand bits and |s| in [2^-14, 2^15]
(or is 0): exact in bf16, in the three-term bf16 split and as an fp16 high half with a zero remainder; w is a power of two in
[2^-16, 2^6], so the fp16 weights scaled by 64 are normal.  The bias is fp32 in every kernel: any fp32 value goes in through it.
  with a bias    w = 1; s cycles through OFFSETS (0 first; quarters over [-12, 12]; halves over +-[85, 92], around the
                 overflow of expf at 88.72); bias vector 0 is a fine grid inside one quarter step, so M x N points sweep
                 [-12, 12.25) densely; the following bias vectors carry SPECIALS, N at a time (rows with s = 0 see them pure,
                 the others see s + special, just as exactly known); any further vectors are fine grids shifted by a fraction
                 of a step.  A launch takes one vector, a strided batch one per problem.  With fewer rows than quarter offsets
                 (M = 1) the bias carries the quarters as well.
  without one    pre = s * w: every 8-bit significand in both signs, row blocks of 256 at the exponents NOBIAS_EXPONENTS,
                 times w = 2^-16 .. 2^6 along the columns: |pre| from 2^-30 to 2^21, every binade of [2^-18, 2^5) complete in the first block.
                 Inf and NaN cannot be injected here.
`pre_of` evaluates the formula in fp32 arithmetic; the GPU test first asserts that a launch without activation returns
exactly that (its premise), so nothing below depends on how a kernel accumulates.

Forms (`form_of` reads the route from a case of linear_reference.CASES, as csrc/gemm.hip's launch_linear and the epilogues
choose it):
  gelu_sig        bf16 kernels, direct epilogues (activate16 -> gelu_for<bf16>)
  gelu_sig2       bf16 kernels, coalesced epilogues (packed pairs)
  gelu_erf_fast   fp32 results of the 256 x 256 operand-splitting kernels, direct epilogue (activate16, ACT_GELU_FAST)
  gelu_erf_fast2  the same kernels' coalesced epilogue, and both epilogues of linear_kernel_f32pp (gelu_fast16x2)
  erff            native fp32 (tile128 in any mode, ring), and the three-term twin of a guarded 128 x 256 launch, which keeps
                  AURORA_ACT_GELU because only 256-row plans are switched to the fast form
  silu            v / (1 + expf(-v)) everywhere

Bounds (`bound`), absolute, of |result - fp64| at the exact input x; linear_reference.tolerance takes its activation term here:
  gelu_sig, gelu_sig2         2.6e-5 for x >= -9;  + 2.4e-12 |x| below: the clamp fmed3(x, -9, 9) freezes the logistic factor at
                              sigma(2 q(-9)) = rcp(1 + exp2(38.658)) = 2.305e-12 while the multiplier stays x, so the form
                              returns 2.305e-12 x where GELU is below 1e-18 (+ 4 % for the rounding of the exp2 argument)
  gelu_erf_fast, _fast2       4e-7 + 7.5e-8 |x|
  erff                        2^-22 |x|
  silu                        8 x 2^-24 |x|
`result_bound` adds 2^-150, half the spacing of the fp32 subnormals: no fp32 result can be closer than that to 0.5 x for the
smallest subnormal x, whatever the form.  It changes no bound at any normal x.

Special values (`SPECIAL_RESULTS`, read from the code): NaN -> NaN and +inf -> +inf in every form; +-0 -> a zero; x <= -104 in
the SiLU and erf forms -> a zero of either sign (expf / exp2 have overflowed or underflowed); -inf -> -inf in gelu_sig (the
clamped factor is finite and positive) and NaN in the others (inf x 0, inf / inf); never a finite nonzero value.
"""
import math
from typing import NamedTuple, Optional

import torch

ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2
FORMS = ("gelu_sig", "gelu_sig2", "gelu_erf_fast", "gelu_erf_fast2", "erff", "silu")
SIG_ABS, SIG_TAIL, SIG_CLAMP = 2.6e-5, 2.4e-12, 9.0
SIG_TAIL_FACTOR = 2.305e-12          # sigma(2 q(-9)) of the fitted quintic
ERF_FAST_ABS, ERF_FAST_REL = 4e-7, 7.5e-8
ERFF_REL = 2.0 ** -22
SILU_REL = 8 * 2.0 ** -24
SUBNORMAL_HALF_SPACING = 2.0 ** -150
ZERO_BELOW = -104.0
SPECIAL_RESULTS = {          # form -> what -inf gives
    "gelu_sig": "-inf", "gelu_sig2": "-inf", "gelu_erf_fast": "nan", "gelu_erf_fast2": "nan", "erff": "nan", "silu": "nan"}

F32 = torch.float32
FLT_MAX, FLT_MIN = 3.4028234663852886e38, 2.0 ** -126
SUB_MIN, SUB_MAX = 2.0 ** -149, 2.0 ** -126 - 2.0 ** -149


def _f32(values) -> torch.Tensor:
    return torch.tensor(values, dtype=torch.float64).to(F32)


def _around(v: float):
    t = torch.tensor(v, dtype=F32)
    return [torch.nextafter(t, torch.tensor(-math.inf)).item(), v, torch.nextafter(t, torch.tensor(math.inf)).item()]


def specials() -> torch.Tensor:
    """The fp32 values every biased case sees in pure form (the order is fixed: tests index into it)."""
    v = [0.0, -0.0, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX]
    v += _around(9.0) + _around(-9.0)
    v += [88.0, -88.0, 88.8, -88.8, 104.0, -104.0, -1e4, -1e7, -1e8, -1e20]
    for k in range(-38, 39):
        v += [10.0 ** k, -(10.0 ** k)]
    v += [math.inf, -math.inf, math.nan]
    return _f32(v)


def _offsets() -> torch.Tensor:
    q = [0.0]
    for k in range(1, 49):
        q += [k / 4, -k / 4]
    n_quarters = len(q)
    for k in range(170, 185):                    # 85.0 .. 92.0 in halves: at most 8 significand bits
        q += [k / 2, -k / 2]
    return _f32(q), n_quarters


OFFSETS, N_QUARTERS = _offsets()
NOBIAS_EXPONENTS = (-2, 9, -14, 14, -8, 3)
STEP = 0.25


class Grid(NamedTuple):
    s: torch.Tensor                  # (M,) fp32: column 0 of the activations
    w: torch.Tensor                  # (N,) fp32: column 0 of the weights
    bias: Optional[torch.Tensor]     # (P, N) fp32: one bias vector per launch, or per problem of a strided batch


def n_special_vectors(N: int) -> int:
    return -(-specials().numel() // N)


def grid(M: int, N: int, has_bias: bool, vectors: int = 0) -> Grid:
    """The injected operands of an M x N linear.  vectors: how many bias vectors (0: the fine grid + every special)."""
    m, n = torch.arange(M), torch.arange(N)
    if not has_bias:
        sig = (128 + (m >> 1) % 128).double()
        e = torch.tensor(NOBIAS_EXPONENTS)[(m >> 8) % len(NOBIAS_EXPONENTS)].double()
        s = (sig / 128 * 2.0 ** e * (1 - 2 * (m & 1))).to(F32)
        return Grid(s, (2.0 ** ((n % 23) - 16).double()).to(F32), None)
    s = OFFSETS[m % OFFSETS.numel()]
    sp = specials()
    need = 1 + n_special_vectors(N)
    P = vectors or need
    assert P >= need, (N, P, need)
    rows = []
    for p in range(P):
        if 1 <= p < need:
            chunk = sp[(p - 1) * N:p * N]
            rows.append(torch.cat([chunk, torch.zeros(N - chunk.numel(), dtype=F32)]))
            continue
        shift = 0.382 if p == 0 else 0.382 + 0.2 * (p - need + 1)       # (never a round number: points avoid the grid of s)
        fine = STEP * (n.double() + shift) / N
        if M < N_QUARTERS:
            fine = fine + OFFSETS[n % N_QUARTERS].double()
        rows.append(fine.to(F32))
    return Grid(s, torch.ones(N, dtype=F32), torch.stack(rows))


def check_grid(g: Grid) -> None:
    """The constraints that make the product and every operand representation exact."""
    for name, t, lo, hi in (("s", g.s, 2.0 ** -14, 2.0 ** 15), ("w", g.w, 2.0 ** -16, 2.0 ** 6)):
        nz = t[t != 0].double().abs()
        assert bool(((nz >= lo) & (nz <= hi)).all()), name
        mant, _ = torch.frexp(nz)
        scaled = mant * (256 if name == "s" else 2)
        assert bool((scaled == scaled.round()).all()), name         # 8 significand bits / a power of two
    assert bool((g.w != 0).all())
    assert torch.equal(g.s.bfloat16().float(), g.s) and torch.equal(g.s.half().float(), g.s)
    assert torch.equal((g.w * 64).half().float(), g.w * 64) and torch.equal(g.w.bfloat16().float(), g.w)


def pre_of(g: Grid) -> torch.Tensor:
    """(P, M, N) fp32 pre-activations, in fp32 arithmetic: the product is exact, the sum is rounded once."""
    prod = g.s[:, None] * g.w[None, :]
    assert torch.equal(prod.double(), g.s.double()[:, None] * g.w.double()[None, :])
    return prod[None] if g.bias is None else prod[None] + g.bias[:, None, :]


# ------------------------------------------------------------------------------------------
# fp64 definitions and bounds
# ------------------------------------------------------------------------------------------
def gelu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x * 0.5 ** 0.5)          # no cancellation on the negative tail


def silu64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    e = torch.exp(-x.abs())
    return x * torch.where(x >= 0, 1 / (1 + e), e / (1 + e))


def reference(form: str, x: torch.Tensor) -> torch.Tensor:
    return silu64(x) if form == "silu" else gelu64(x)


def bound(form: str, x: torch.Tensor) -> torch.Tensor:
    """The documented bound of |form(x) - fp64| at x (fp64 tensor of the shape of x)."""
    x = x.double()
    ax = x.abs()
    if form in ("gelu_sig", "gelu_sig2"):
        return SIG_ABS + torch.where(x < -SIG_CLAMP, SIG_TAIL * ax, torch.zeros_like(ax))
    if form in ("gelu_erf_fast", "gelu_erf_fast2"):
        return ERF_FAST_ABS + ERF_FAST_REL * ax
    if form == "erff":
        return ERFF_REL * ax
    assert form == "silu", form
    return SILU_REL * ax


def result_bound(form: str, x: torch.Tensor) -> torch.Tensor:
    return bound(form, x) + SUBNORMAL_HALF_SPACING


def form_of(c, direct: bool = False) -> Optional[str]:
    """The form a case of linear_reference.CASES reaches (None without activation); direct: its launch with a second output."""
    if c.act == ACT_NONE:
        return None
    if c.act == ACT_SILU:
        return "silu"
    coalesced = c.form in ("coalesced", "pair_coalesced") and not direct
    if c.dtype == "bf16":
        return "gelu_sig2" if coalesced else "gelu_sig"
    if c.kernel.startswith("f32_pp"):
        if c.guard is False:                       # the three-term twin runs instead
            return "erff" if c.tile[0] == 128 else ("gelu_erf_fast2" if coalesced else "gelu_erf_fast")
        return "gelu_erf_fast2"
    if c.kernel in ("f32_three", "f32_two"):
        return "gelu_erf_fast2" if coalesced else "gelu_erf_fast"
    return "erff"


class Worst(NamedTuple):
    ratio: float         # max |got - fp64| / bound over the finite inputs (NaN if a result there is NaN)
    x: float             # where


def worst(form: str, x32: torch.Tensor, got: torch.Tensor, extra: Optional[torch.Tensor] = None) -> Worst:
    """Over the FINITE inputs of x32.  extra: what the store adds to the bound (a tensor of the shape of x32)."""
    x = x32.double().flatten()
    fin = torch.isfinite(x)
    b = result_bound(form, x)
    if extra is not None:
        b = b + extra.double().flatten()
    r = ((got.double().flatten() - reference(form, x)).abs() / b)[fin]
    if r.numel() == 0:
        return Worst(0.0, float("nan"))
    if bool(torch.isnan(r).any()):
        return Worst(float("nan"), x[fin][torch.isnan(r)][0].item())
    i = int(r.argmax())
    return Worst(r[i].item(), x[fin][i].item())


def special_failures(form: str, x32: torch.Tensor, got: torch.Tensor) -> list:
    """What SPECIAL_RESULTS and the module docstring say about NaN, +-inf, +-0 and x <= -104, checked; [] if all hold."""
    x, y = x32.flatten(), got.float().flatten()
    bad = []

    def need(name, where, ok):
        if bool((where & ~ok).any()):
            i = int((where & ~ok).nonzero()[0])
            bad.append(f"{name}: {form}({x[i].item()!r}) = {y[i].item()!r}")

    need("NaN in, NaN out", torch.isnan(x), torch.isnan(y))
    need("+inf in, +inf out", x == math.inf, y == math.inf)
    need("a zero in, a zero out", x == 0, y == 0)
    if form not in ("gelu_sig", "gelu_sig2"):
        need("a zero at and below -104", torch.isfinite(x) & (x <= ZERO_BELOW), y == 0)
    minus = x == -math.inf
    need("-inf", minus, (y == -math.inf) if SPECIAL_RESULTS[form] == "-inf" else torch.isnan(y))
    need("-inf never gives a finite nonzero value", minus, ~torch.isfinite(y) | (y == 0))
    return bad


# ------------------------------------------------------------------------------------------
# fp32 emulations: the operations of csrc/common.h in their order, exp2 / exp / erf / 1/x correctly rounded
# ------------------------------------------------------------------------------------------
def _c(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float64).to(F32)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).to(F32)        # the product is exact in fp64; one rounding that matters


def _exp2(x):
    return torch.exp2(x.double()).to(F32)


def _exp(x):
    return torch.exp(x.double()).to(F32)


def _rcp(x):
    return (1.0 / x.double()).to(F32)


SIG_COEF = (1.0142631e-3, -1.0677572e-1, -2.3011213)
ERF_COEF = (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)


def emu_gelu_sig(x, clamp: float = SIG_CLAMP, coef=SIG_COEF):
    """gelu_sig and gelu_sig2 (the packed form performs the same operations on each half)."""
    x = x.to(F32)
    xc = torch.where(torch.isnan(x), _c(-clamp), torch.clamp(x, -clamp, clamp))     # v_med3_f32 answers a NaN with the minimum
    x2 = xc * xc
    t = _fma(x2, _c(coef[0]), _c(coef[1]))
    t = _fma(t, x2, _c(coef[2]))
    e = _exp2(xc * t)
    return x * _rcp(1.0 + e)


def emu_gelu_erf_fast(x, packed: bool = False, coef=ERF_COEF, positive_branch_everywhere: bool = False):
    """gelu_erf_fast (expf of -z^2) and, packed, gelu_erf_fast2 (exp2 of -z^2 log2 e; 0.5 multiplied in later)."""
    x = x.to(F32)
    z = x.abs() * _c(0.70710678118654752440)
    t = _rcp(_fma(_c(0.3275911), z, _c(1.0)))
    poly = _fma(_c(coef[0]), t, _c(coef[1]))
    for k in coef[2:]:
        poly = _fma(poly, t, _c(k))
    if packed:
        q = poly * t * _c(0.5) * _exp2(z * z * _c(-1.4426950408889634))
    else:
        q = _c(0.5) * poly * t * _exp(-(z * z))
    upper = torch.ones_like(x, dtype=torch.bool) if positive_branch_everywhere else x >= 0
    return x * torch.where(upper, 1.0 - q, q)


def emu_gelu_erf(x):
    x = x.to(F32)
    return _c(0.5) * x * (1.0 + torch.erf((x * _c(0.70710678118654752440)).double()).to(F32))


def emu_silu(x, negate: bool = False):
    x = x.to(F32)
    return x / (1.0 + _exp(x if negate else -x))


def emulate(form: str, x):
    if form in ("gelu_sig", "gelu_sig2"):
        return emu_gelu_sig(x)
    if form in ("gelu_erf_fast", "gelu_erf_fast2"):
        return emu_gelu_erf_fast(x, packed=form.endswith("2"))
    return emu_gelu_erf(x) if form == "erff" else emu_silu(x)


# ------------------------------------------------------------------------------------------
# wrong variants: each a mistake a kernel could contain; (name, the form it would sit in)
# ------------------------------------------------------------------------------------------
WRONG = (("tanh_gelu", "gelu_sig"), ("tanh_gelu", "gelu_erf_fast"), ("tanh_gelu", "erff"), ("clamp_at_6", "gelu_sig"),
         ("positive_branch_for_negative_x", "gelu_erf_fast"), ("coefficient_4th_digit", "gelu_sig"),
         ("coefficient_4th_digit", "gelu_erf_fast"), ("sigmoid_of_minus_x", "silu"), ("pair_halves_swapped", "gelu_sig2"),
         ("pair_halves_swapped", "gelu_erf_fast2"))


def wrong(name: str, form: str, x: torch.Tensor) -> torch.Tensor:
    """x: (..., N) fp32 with N even (pair_halves_swapped exchanges neighbours along the last dimension)."""
    x = x.to(F32)
    if name == "tanh_gelu":
        u = 0.7978845608028654 * (x.double() + 0.044715 * x.double() ** 3)
        return (0.5 * x.double() * (1 + torch.tanh(u))).to(F32)
    if name == "clamp_at_6":
        return emu_gelu_sig(x, clamp=6.0)
    if name == "positive_branch_for_negative_x":
        return emu_gelu_erf_fast(x, positive_branch_everywhere=True)
    if name == "coefficient_4th_digit":
        if form == "gelu_sig":
            return emu_gelu_sig(x, coef=(SIG_COEF[0], SIG_COEF[1], -2.3021213))
        return emu_gelu_erf_fast(x, coef=ERF_COEF[:4] + (0.254929592,))
    if name == "sigmoid_of_minus_x":
        return emu_silu(x, negate=True)
    assert name == "pair_halves_swapped", name
    y = emulate(form, x)
    return y.reshape(*y.shape[:-1], -1, 2).flip(-1).reshape(y.shape)
