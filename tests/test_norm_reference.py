"""The fp64 references of tests/norm_reference.py against the oracle, and the teeth of the inputs the GPU tests use:
every deliberately wrong variant lands at least 100 x the tolerance of the GPU assertion away from the right result.
Runs without a GPU."""
import pytest
import torch

from oracle import aurora_oracle as oracle
from tests import norm_reference as R

GRIDS = [(12, 24), (13, 26), (7, 13), (1, 5)]
TEETH = 100.0


def far(wrong, ref, scale, tol=R.F32_TOL):
    """The wrong result is >= TEETH x tol away in the metric of the GPU assertion."""
    err = R.worst(R.row_error(wrong, ref, scale))
    assert err >= TEETH * tol, err


# ---- the right references equal the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 264, 1024])
def test_layernorm_ref_equals_the_oracle(D):
    y, gain, shift, res, _ = R.ln_inputs(37, D, torch.float32)
    sd = {"n.weight": gain.double(), "n.bias": shift.double()}
    out, scale = R.layernorm_ref(y, gain, shift, res)
    assert (out - (oracle.layer_norm(sd, "n", y.double()) + res.double())).abs().max().item() <= 1e-12
    ln = oracle.layer_norm({"n.weight": torch.ones(D, dtype=torch.float64), "n.bias": torch.zeros(D, dtype=torch.float64)},
                           "n", y.double())
    want_scale = ((ln * gain.double()).abs() + shift.double().abs() + res.double().abs()).max(dim=1).values
    assert (scale - want_scale).abs().max().item() <= 1e-12
    # a column block of a wider row, and the cyclic residual
    wide = torch.cat((y, y + 7.0), dim=1)
    out_d, _ = R.layernorm_ref(wide, gain, shift, R.rnd(R.RES_MOD, D, seed=5), R.RES_MOD, d=D)
    want = oracle.layer_norm(sd, "n", y.double()) + R.rnd(R.RES_MOD, D, seed=5)[torch.arange(37) % R.RES_MOD]
    assert (out_d - want).abs().max().item() <= 1e-12
    # eps
    out_e, _ = R.layernorm_ref(y, eps=1e-3)
    assert (out_e - torch.nn.functional.layer_norm(y.double(), (D,), eps=1e-3)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("H,W", GRIDS)
def test_merge_ln_ref_equals_the_oracle(H, W):
    B, C = R.BC
    D = 24
    x, w, b = R.merge_inputs(H, W, D)
    sd = {"m.norm.weight": w.double(), "m.norm.bias": b.double(), "m.reduction.weight": torch.eye(4 * D, dtype=torch.float64)}
    want = oracle.patch_merge(sd, "m", x.double().reshape(B, C * H * W, D), (C, H, W)).reshape(-1, 4 * D)
    out, _ = R.merge_ln_ref(x, w, b, B, C, H, W, D)
    assert out.shape == want.shape and (out - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("crop", R.CROPS)
def test_split_ln_ref_equals_the_oracle(H, W, crop):
    B, C = R.BC
    Dq = 16
    y, w, b = R.split_inputs(H, W, Dq, torch.float32)
    sd = {"s.lin1.weight": torch.eye(4 * Dq, dtype=torch.float64), "s.norm.weight": w.double(), "s.norm.bias": b.double(),
          "s.lin2.weight": torch.eye(Dq, dtype=torch.float64)}
    want = oracle.patch_split(sd, "s", y.double().reshape(B, C * H * W, 4 * Dq), (C, H, W), (0, *crop)).reshape(-1, Dq)
    out, _ = R.split_ln_ref(y, w, b, B, C, H, W, Dq, *crop)
    assert out.shape == want.shape and (out - want).abs().max().item() <= 1e-12


# ---- the wrong variants are far away on the GPU tests' inputs ------------------------------------------------
@pytest.mark.parametrize("D", R.LARGE_MEAN_WIDTHS)
@pytest.mark.parametrize("c", R.LARGE_MEANS)
def test_one_pass_variance_fails_the_large_mean_bound(c, D):
    """The bound of the GPU test (LARGE_MEAN_FACTOR x the error of torch's CPU fp32 layer_norm) against E[x^2] - mean^2
    in fp32: measured 114 x and 119 x the bound at c = 1e2 (D = 264, 2048), 2.7e4 x at c = 1e4."""
    y = R.large_mean_inputs(c, D)
    bound, measured = R.large_mean_bound(y)
    assert 0 < measured < 1e-2
    ref, scale = R.layernorm_ref(y)
    wrong, _ = R.layernorm_ref(y, one_pass_f32=True)
    assert R.worst(R.row_error(wrong, ref, scale)) > TEETH * bound


def test_one_pass_variance_passes_on_the_ordinary_rows():
    """... which is why the large-mean rows exist: at mean 0.5 the one-pass form is inside the tolerance."""
    y = R.ln_inputs(1001, 264, torch.float32)[0]
    ref, scale = R.layernorm_ref(y)
    assert R.worst(R.row_error(R.layernorm_ref(y, one_pass_f32=True)[0], ref, scale)) < R.F32_TOL


@pytest.mark.parametrize("D", R.LN_WIDTHS)
@pytest.mark.parametrize("dtype", [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16")])
def test_layernorm_wrong_variants(D, dtype):
    for M in R.LN_ROWS:
        y, gain, shift, res, res5 = R.ln_inputs(M, D, dtype)
        ref, scale = R.layernorm_ref(y, gain, shift, res5, R.RES_MOD)
        if M > R.RES_MOD:
            far(R.layernorm_ref(y, gain, shift, res5, R.RES_MOD, ignore_res_mod=True)[0], ref, scale)
        # the row that follows, the gain left out, the shift left out, the residual left out: each optional-operand
        # branch taken wrongly shows as well
        far(R.layernorm_ref(y, None, shift, res5, R.RES_MOD)[0], ref, scale)
        far(R.layernorm_ref(y, gain, None, res5, R.RES_MOD)[0], ref, scale)
        far(R.layernorm_ref(y, gain, shift)[0], ref, scale)
        for piece in ([] if D < 2 * R.PIECE else sorted({0, D // R.PIECE - 2})):
            far(R.swap_piece(ref, piece), ref, scale)
            plain, pscale = R.layernorm_ref(y)
            far(R.swap_piece(plain, piece), plain, pscale)


def test_eps_rows_are_dominated_by_eps():
    y = R.eps_inputs(1001, 264)
    ref, scale = R.layernorm_ref(y, eps=1e-3)
    assert y.double().var(dim=1, unbiased=False).max().item() < 1e-3 / 20
    far(R.layernorm_ref(y, eps=1e-5)[0], ref, scale)


@pytest.mark.parametrize("D", R.MERGE_WIDTHS)
@pytest.mark.parametrize("H,W", R.MERGE_GRIDS)
def test_merge_ln_wrong_variants(H, W, D):
    B, C = R.BC
    x, w, b = R.merge_inputs(H, W, D)
    ref, scale = R.merge_ln_ref(x, w, b, B, C, H, W, D)
    if H % 2 or W % 2:       # an even grid has no padding to leave out
        far(R.merge_ln_ref(x, w, b, B, C, H, W, D, stats_skip_padding=True)[0], ref, scale)
    if (H, W) != (1, 1):     # a single cell is segment 0 in either order
        far(R.merge_ln_ref(x, w, b, B, C, H, W, D, seg_order_dw_dh=True)[0], ref, scale)
    for piece in sorted({0, D // R.PIECE - 1, 4 * D // R.PIECE - 2}):   # inside a cell, across two cells, the last pair
        far(R.swap_piece(ref, piece), ref, scale)


@pytest.mark.parametrize("Dq", R.SPLIT_WIDTHS)
@pytest.mark.parametrize("H,W", R.SPLIT_GRIDS)
@pytest.mark.parametrize("dtype", [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16")])
def test_split_ln_wrong_variants(H, W, Dq, dtype):
    B, C = R.BC
    y, w, b = R.split_inputs(H, W, Dq, dtype)
    for crop in R.CROPS:
        ref, scale = R.split_ln_ref(y, w, b, B, C, H, W, Dq, *crop)
        assert ref.shape[0] == B * C * (2 * H - crop[0]) * (2 * W - crop[1])
        if crop != (0, 0):
            far(R.split_ln_ref(y, w, b, B, C, H, W, Dq, *crop, crop_first=True)[0], ref, scale)
        for piece in ([] if Dq < 2 * R.PIECE else sorted({0, Dq // R.PIECE - 2})):
            far(R.swap_piece(ref, piece), ref, scale)
