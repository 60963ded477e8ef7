"""tests/activation_reference.py on the CPU: the injected operands keep their exactness constraints and reach the regions they
are for, the fp32 emulation of every form stays inside its bound on the full grids, every wrong variant leaves it, the tail of
gelu_sig is the straight line the bound says, and linear_reference.tolerance still returns what it did on the table's cases --
the condition that makes tests/test_gpu_activations.py worth having."""
import math

import pytest
import torch

from tests import activation_reference as A
from tests import linear_reference as R

ACTED = [c for c in R.CASES if c.act != R.ACT_NONE]
SHAPES = sorted({(c.M, c.N, c.bias, c.batch if c.entry == "batched" else 0) for c in ACTED})


@pytest.fixture(scope="module")
def grids():
    return {k: A.grid(k[0], k[1], k[2], k[3]) for k in SHAPES}


def test_constants_are_the_ones_the_forms_and_the_table_use():
    assert (A.ACT_NONE, A.ACT_GELU, A.ACT_SILU) == (R.ACT_NONE, R.ACT_GELU, R.ACT_SILU)
    assert {A.form_of(c) for c in ACTED} | {A.form_of(c, direct=True) for c in ACTED} == set(A.FORMS)
    assert all(A.form_of(c) is None for c in R.CASES if c.act == R.ACT_NONE)
    assert set(A.SPECIAL_RESULTS) == set(A.FORMS)
    # a strided batch has room for the fine grid and every special
    assert all(c.batch >= 1 + A.n_special_vectors(c.N) for c in ACTED if c.entry == "batched" and c.bias)


def test_grids_are_exact_and_reach_what_they_are_for(grids):
    sp = A.specials()
    for (M, N, has_bias, _), g in grids.items():
        A.check_grid(g)
        pre = A.pre_of(g)
        assert pre.shape[1:] == (M, N) and pre.dtype == torch.float32
        if not has_bias:
            assert pre.shape[0] == 1 and bool(torch.isfinite(pre).all())
            ax = pre.abs().double()
            assert M >= 256 and N >= 23 and ax.min() <= 2.0 ** -18 and ax.max() >= 2.0 ** 5
            if M >= 256 * len(A.NOBIAS_EXPONENTS):          # every row block present
                assert ax.min() == 2.0 ** -30 and 2.0 ** 20 <= ax.max() < 2.0 ** 21
            for sign in (1, -1):          # every 8-bit significand of every binade of [2^-18, 2^5), both signs
                seen = set((pre[sign * pre > 0].double().abs()).unique().tolist())
                assert all(k / 128 * 2.0 ** e in seen for e in range(-18, 5) for k in range(128, 256)), (M, N, sign)
            continue
        # pure specials: s = 0 in row 0, every special in some vector (NaN compared as NaN)
        assert g.s[0] == 0
        pure = pre[1:1 + A.n_special_vectors(N), 0].flatten()[:sp.numel()]
        assert torch.equal(pure.view(torch.int32), (sp + 0.0).view(torch.int32)), (M, N)
        # the sweep: no gap wider than a fine step over [-12, 12]
        pts = pre[0].flatten().double()
        pts = pts[(pts >= -12) & (pts <= 12)].unique()
        if M < A.N_QUARTERS:          # (a single row: the bias carries one point per quarter offset)
            assert N >= A.N_QUARTERS and pts.numel() >= A.N_QUARTERS and pts[0] < -11.5 and pts[-1] > 11.5, (M, N)
            continue
        assert pts[0] <= -12 + A.STEP / N and pts[-1] >= 12 - A.STEP / N, (M, N)
        if M >= A.OFFSETS.numel():
            assert (pts[1:] - pts[:-1]).max().item() <= 1.01 * A.STEP / N, (M, N)
            lo, hi = pre[0].min().item(), pre[0].max().item()
            assert lo <= -88.73 and hi >= 88.73        # both sides of the overflow of expf


def test_fp64_definitions():
    x = torch.tensor([-30.0, -9.0, -1.0, 0.0, 0.5, 3.0, 800.0, -800.0], dtype=torch.float64)
    assert torch.allclose(A.gelu64(x)[1:6], 0.5 * x[1:6] * (1 + torch.erf(x[1:6] * 0.5 ** 0.5)), rtol=0, atol=1e-16)
    assert A.gelu64(x)[0].item() == pytest.approx(-30 * 0.5 * math.erfc(30 / 2 ** 0.5), rel=1e-12) and A.gelu64(x)[0] < 0
    assert torch.allclose(A.silu64(x)[:6], x[:6] * torch.sigmoid(x[:6]), rtol=1e-15, atol=0)
    assert A.silu64(x)[6] == 800 and A.silu64(x)[7] == 0 and bool(torch.isfinite(A.silu64(x)).all())


@pytest.mark.parametrize("form", A.FORMS)
def test_an_emulated_form_is_inside_its_bound_and_its_special_values_hold(grids, form):
    top = A.Worst(0.0, 0.0)
    for key, g in grids.items():
        pre = A.pre_of(g)
        got = A.emulate(form, pre)
        w = A.worst(form, pre, got)
        assert w.ratio <= 1.0, (form, key, w)
        assert A.special_failures(form, pre, got) == [], (form, key)
        core = pre.abs() <= 12
        w = A.worst(form, pre[core], got[core])
        top = max(top, w)
    print(f"EMULATED {form}: worst error / bound {top.ratio:.3f} at x = {top.x!r} (|x| <= 12)")
    if form.startswith("gelu_sig"):
        assert 0.9 < top.ratio          # the fit leaves 2 % of room: the bound is not a loose one
    if form.startswith("gelu_erf_fast"):
        assert 0.5 < top.ratio


@pytest.mark.parametrize("name,form", A.WRONG, ids=lambda v: v)
def test_a_wrong_variant_leaves_the_bound(grids, name, form):
    worst = 0.0
    for key, g in grids.items():
        pre = A.pre_of(g)
        if name == "pair_halves_swapped":          # a NaN neighbour would be a failure of its own: the sweep alone tells
            pre = pre[0, :, :pre.shape[2] // 2 * 2]
        r = A.worst(form, pre, A.wrong(name, form, pre)).ratio
        assert r > 2.0 or math.isnan(r), (name, form, key, r)
        worst = max(worst, r)
    print(f"WRONG {name} in {form}: worst error / bound {worst:.3g}")


def test_the_special_value_table_tells_forms_apart():
    x = torch.tensor([-math.inf], dtype=torch.float32)
    for form in A.FORMS:
        assert A.special_failures(form, x, A.emulate(form, x)) == []
        other = "silu" if A.SPECIAL_RESULTS[form] == "-inf" else "gelu_sig"
        assert A.special_failures(form, x, A.emulate(other, x)) != []
        assert A.special_failures(form, x, torch.tensor([-1.0])) != []          # finite and nonzero out of -inf
    nan = torch.tensor([math.nan], dtype=torch.float32)
    assert A.special_failures("gelu_sig", nan, torch.tensor([-9.0 * 2.3e-12])) != []    # a NaN swallowed by the clamp


def test_the_tail_of_gelu_sig_is_a_straight_line():
    x = -torch.logspace(1, 38, 200, dtype=torch.float64).float()
    y = A.emu_gelu_sig(x).double()
    assert ((y / x.double() / A.SIG_TAIL_FACTOR - 1).abs() < 2e-3).all()
    err = (y - A.gelu64(x)).abs()
    assert bool((err <= A.bound("gelu_sig", x)).all())
    assert bool((err[x < -1.2e7] > A.SIG_ABS).all())          # "2.6e-5 absolute" alone is false below -1.13e7
    assert A.bound("gelu_sig", torch.tensor([-9.0, 9.0, 1e30])).tolist() == [A.SIG_ABS] * 3


@pytest.mark.parametrize("case", ACTED, ids=lambda c: c.id)
def test_tolerance_of_the_table_is_unchanged(case):
    """No case of the table that runs gelu_sig has a pre-activation below -9 (a few fp32 cases of short K have, down to -9.4:
    their forms have no tail term), so the tail term adds nothing there, and the activation term of
    linear_reference.tolerance is what it was before the bounds moved to activation_reference."""
    c = case
    p = R.problem(c)
    pre = p.a @ p.w.transpose(1, 2)
    if p.bias is not None:
        pre = pre + p.bias[:, None, :]
    if c.act == R.ACT_GELU and c.dtype == "bf16":
        assert pre.min().item() > -9.0, (c.id, pre.min().item())
    x = pre.abs()
    native = c.dtype == "f32" and (c.base_mode == 0 or c.kernel == "tile128")
    if c.act == R.ACT_GELU:
        old = torch.full_like(x, 2.6e-5) if c.dtype == "bf16" else (2.0 ** -22 * x if native else 4e-7 + 7.5e-8 * x)
        new = A.bound("gelu_sig" if c.dtype == "bf16" else "erff" if native else "gelu_erf_fast", pre)
    else:
        old, new = 8 * R.U32 * x, A.bound("silu", pre)
    assert torch.equal(old, new), c.id
