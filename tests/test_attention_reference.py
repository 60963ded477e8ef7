"""The fp64 reference of tests/attention_reference.py against an independent evaluation, its tables and tolerances, and the
teeth of the inputs the GPU tests use: every deliberately wrong variant lands at least TEETH = 10 x BF16_TOL (the LOOSER of
the GPU assertions' tolerances) away from the right result, or stores other rows.  Runs without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_reference as R

FAR = R.TEETH * R.BF16_TOL
DTYPES = ["f32", "bf16"]


def distance(case, dtype, wrong, **kw):
    """worst row_error of the wrong evaluation against the right one, over the rows the right one stores."""
    p = R.problem(case, dtype)
    ref, written, scale = R.attention_ref(*p.args())
    out, w2, _ = R.attention_ref(*p.args(), wrong=wrong, **kw)
    assert torch.equal(written, w2)
    return R.worst(R.row_error(out, ref, scale)[written])


def far(case, dtype, wrong, **kw):
    d = distance(case, dtype, wrong, **kw)
    assert d >= FAR, (case.id, dtype, wrong, d, FAR)


# ---- the reference itself ------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,window,shifted", [((4, 12, 24), (2, 6, 12), True), ((4, 7, 13), (2, 6, 12), True),
                                                ((2, 5, 9), (2, 3, 4), False)])
def test_attention_ref_equals_sdpa_on_the_geometry_tables(res, window, shifted):
    """An evaluation that shares no code with attention_ref: the engine's tables, F.scaled_dot_product_attention."""
    from aurora_amd.engine import geometry

    B, heads = 2, 2
    D = 64 * heads
    L = res[0] * res[1] * res[2]
    tok, grp, _ = geometry.window_tables(res, window, shifted)
    qkv = R.rnd32(B, L, 3 * D, seed=5, scale=2.0).double()
    bias = R.rnd32(3 * D, seed=6).double()
    ref, written, scale = R.attention_ref(qkv, bias, tok, grp, B, L, L, D, heads)
    nW, N = tok.shape
    t = torch.from_numpy(tok.astype(np.int64))
    want = torch.zeros((B, L, D), dtype=torch.float64)
    for b in range(B):
        rows = torch.where(t[..., None] >= 0, qkv[b][t.clamp(min=0)], bias.expand(nW, N, 3 * D))
        q, k, v = rows.reshape(nW, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
        mask = None
        if grp is not None:
            g = torch.from_numpy(grp.astype(np.int64))
            mask = torch.where(g[:, None, :] != g[:, :, None], -100.0, 0.0)[:, None].double()
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(nW, N, D)
        want[b][t[t >= 0]] = o[t >= 0]
    assert bool(written.all()) and (ref - want).abs().max().item() <= 1e-12
    assert 1.0 < scale.min().item() and scale.max().item() <= 2.0


def test_scale_and_written_by_hand():
    """Two windows of three positions over five tokens, one head: token 4 is a halo row, token 2 is in no window."""
    tok = torch.tensor([[0, -1, 4], [3, 1, -1]], dtype=torch.int32)
    qkv = torch.zeros((1, 5, 192), dtype=torch.float64)
    qkv[0, :, 128] = torch.tensor([0.5, -3.0, 9.0, 1.0, -7.0])     # v_0 of the five tokens
    bias = torch.zeros(192, dtype=torch.float64)
    bias[128] = 2.0
    out, written, scale = R.attention_ref(qkv, bias, tok, None, 1, 5, 4, 64, 1)
    assert written.tolist() == [[True, True, False, True]]
    assert scale[0, :, 0].tolist() == [7.0, 3.0, 1.0, 3.0]          # the halo row and the bias rows count; unwritten: 1
    # all scores are zero: uniform weights
    assert out[0, 0, 0].item() == pytest.approx((0.5 + 2.0 - 7.0) / 3) and out[0, 3, 0].item() == pytest.approx(0.0)
    none = R.attention_ref(qkv, None, tok, None, 1, 5, 4, 64, 1)[0]
    assert none[0, 0, 0].item() == pytest.approx((0.5 - 7.0) / 3)
    err = R.row_error(out, out, scale)
    assert err.shape == (1, 4, 1) and R.worst(err[written]) == 0.0
    bad = out.clone()
    bad[0, 1, 63] = float("nan")
    assert np.isnan(R.worst(R.row_error(bad, out, scale)[written]))


def test_to_planes():
    qkv = R.rnd32(2, 7, 3 * 192, seed=1)
    pl = R.to_planes(qkv, 3)
    assert pl.shape == (3, 14, 3, 64) and pl.is_contiguous()
    for b, t, sel, h in [(0, 0, 0, 0), (1, 6, 2, 2), (1, 0, 1, 1)]:
        assert torch.equal(pl[h, b * 7 + t, sel], qkv[b, t, sel * 192 + h * 64:sel * 192 + h * 64 + 64])


def test_hand_tables():
    tok, grp = R.hand_tables(5, 24, 200, seed=3, pad={0: [0, 23], 2: range(16)}, groups="mixed",
                             halo=(150, {1: [3, 11], 2: range(24)}))
    live = tok[tok >= 0]
    assert live.numel() == live.unique().numel() == 5 * 24 - 2 - 16 and int(live.max()) < 200
    assert tok[0, 0] == tok[0, 23] == -1 and bool((tok[2, :16] == -1).all())
    assert bool((tok[2, 16:] >= 150).all()) and tok[1, 3] >= 150 and tok[1, 11] >= 150
    assert int(((tok >= 150)).sum()) == 2 + 8
    assert grp.dtype == torch.uint8 and set(grp.flatten().tolist()) == set(R.GROUP_IDS) and 27 in R.GROUP_IDS
    _, uni = R.hand_tables(5, 24, 200, seed=3, groups="uniform")
    assert bool((uni == uni[:, :1]).all()) and uni[:, 0].unique().numel() > 1
    assert R.hand_tables(5, 24, 200, seed=3)[1] is None


@pytest.mark.parametrize("N", R.GROUP_SIZES)
def test_the_band_tables_hold_every_partner_arrangement(N):
    case = R.halo_cases(N)[0]
    p = R.problem(case, "f32")
    t, Lo = p.tok, p.L_out
    own = (t >= 0) & (t < Lo)
    halo, pad = t >= Lo, t == -1
    assert p.L_out < p.L
    pairs = {(i, i ^ 8) for i in range(16)}
    w0 = [(own[0, i], halo[0, i], pad[0, i], own[0, j], halo[0, j], pad[0, j]) for i, j in sorted(pairs)]
    assert any(a[0] and a[4] for a in w0) and any(a[2] and a[3] for a in w0)      # owned | halo,  padded | owned
    assert any(a[1] and a[4] for a in w0) and any(a[2] and a[4] for a in w0)      # halo | halo,  padded | halo
    assert bool(halo[1, :16].all()) and bool(own[1, 16:].all())                  # a whole tile of halo rows, keys of owned queries
    assert bool(halo[4].all()) and bool(own[3].all())
    assert N < 32 or bool(halo[0, 16:32].all())
    for w in range(3):
        assert bool(own[w].any()) and bool(halo[w].any())


def test_the_item_counts_straddle_the_thresholds():
    for table, threshold in ((R.ITEMS_ROWS, 6000), (R.ITEMS_PLANES, 3000)):
        assert {n - threshold for n in table} == {-1, 0, 3, 4, 7}
        assert all(B * h * w == n for n, (B, h, w) in table.items())
        assert all(B == 2 for n, (B, h, w) in table.items() if n % 2 == 0)             # (an odd count has B = 1)
        assert any(B == 2 and h >= 2 and n % 8 for n, (B, h, w) in table.items() if n >= threshold)
    for (B, h, w), threshold in ((R.ITEMS_ROWS_144, 6000), (R.ITEMS_PLANES_144, 3000)):
        assert B * h * w >= threshold and (B * h * w) % 8


def test_the_recorded_errors_are_up_to_date():
    """The four cases that gave the worst figure of each kind, measured again: the constants beside F32_TOL / BF16_TOL
    are what this code yields (fp32: within a factor of two -- the order of a BLAS sum is the machine's)."""
    worst_cases = [R.Case("sizes", 144, pad="lone"), R.Case("sizes", 144, inputs="lowscore"), R.Case("sizes", 144, inputs="peaked"),
                   R.group_cases(24)[3], R.item_cases("rows", 6003)[0]]
    f32, bf16 = R.measure(worst_cases)
    for kind, recorded in R.F32_MEASURED.items():
        assert recorded / 2 <= f32[kind] <= recorded * 2, (kind, f32[kind], recorded)
    assert 0.9 * R.BF16_MEASURED <= bf16 <= R.BF16_MEASURED * 1.001, bf16
    assert R.F32_TOL == 8 * max(R.F32_MEASURED["uniform"], R.F32_MEASURED["lowscore"]) and R.BF16_TOL == 4 * R.BF16_MEASURED
    assert R.F32_TOL < min(R.F32_TOL_PEAKED, R.F32_TOL_MASK128) and max(R.F32_TOL_PEAKED, R.F32_TOL_MASK128) < R.BF16_TOL / 50


# ---- the wrong variants are far away on the GPU tests' inputs ------------------------------------------------
@pytest.mark.parametrize("N", R.GROUP_SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_masks(dtype, N):
    """-100 x (group xor) and -inf on the scores of 128; the ordinary mixed groups tell -100 from no mask at all."""
    mask128 = R.group_cases(N)[3]
    assert mask128.inputs == "mask128"
    far(mask128, dtype, "mask_xor")
    far(mask128, dtype, "mask_inf")
    p = R.problem(R.group_cases(N)[2], dtype)
    ref, written, scale = R.attention_ref(*p.args())
    unmasked = R.attention_ref(p.qkv, p.bias_seen, p.tok, None, p.B, p.L, p.L_out, p.D, p.heads)[0]
    assert R.worst(R.row_error(unmasked, ref, scale)[written]) >= FAR


@pytest.mark.parametrize("N", [n for n in R.WINDOW_SIZES if n % 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_keys_of_a_ragged_tile(dtype, N):
    """The last live key dropped: the peaked inputs (it is the one key that counts for some query).  Key N admitted with
    k = v = 0: the low-score inputs (a score of 0 is ~8 above every other)."""
    cases = {(c.pad, c.bias, c.inputs): c for c in R.window_size_cases(N)}
    if N > 1:      # (a window of one key has nothing left to compare with: its only key is the right answer)
        far(cases["none", True, "peaked"], dtype, "drop_last_key")
    far(cases["none", True, "lowscore"], dtype, "admit_zero_key")


@pytest.mark.parametrize("N", R.WINDOW_SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_padding_rows(dtype, N):
    """Zero where the bias belongs, and the bias where there is none: the windows of one live position, and the low-score
    inputs with both ends padded."""
    cases = {(c.pad, c.bias, c.inputs): c for c in R.window_size_cases(N)}
    spare = R.rnd32(3 * 128, seed=12)
    for key in [("lone", True, "uniform"), ("ends", True, "lowscore"), ("lone", False, "uniform"), ("ends", False, "lowscore")]:
        if N == 1 and key[0] == "lone":
            continue      # (one position, kept: no padding)
        case = cases[key]
        p = R.problem(case, dtype)
        ref, written, scale = R.attention_ref(*p.args())
        if N <= 2 and key[0] == "ends":
            assert not bool(written.any())      # both ends of a window of one or two: nothing is stored
            continue
        wrong = R.attention_ref(*p.args(bias=None if case.bias else spare))[0]
        d = R.worst(R.row_error(wrong, ref, scale)[written])
        assert d >= FAR, (case.id, dtype, d)


@pytest.mark.parametrize("N", R.GROUP_SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrong_bands(dtype, N):
    for case in R.halo_cases(N):
        far(case, dtype, "ignore_halo_keys")
        far(case, dtype, "half_row_from_partner")
        p = R.problem(case, dtype)
        guard = p.L - p.L_out + 2
        right = R.stored_rows(p.tok, p.B, p.L_out, guard)
        assert torch.equal(right[:p.B * p.L_out].reshape(p.B, p.L_out), R.attention_ref(*p.args())[1])
        assert not bool(right[p.B * p.L_out:].any())
        for wrong in ("halo", "pad"):
            assert not torch.equal(R.stored_rows(p.tok, p.B, p.L_out, guard, wrong), right), (case.id, wrong)
        # a stored halo row of the last batch element stays inside the guard rows: the GPU test would see it
        assert R.stored_rows(p.tok, p.B, p.L_out, guard, "halo")[p.B * p.L_out:].any()


@pytest.mark.parametrize("N", R.WINDOW_SIZES)
def test_wrong_columns_and_batch_element(N):
    case = R.Case("sizes", N)
    for dtype in DTYPES:
        far(case, dtype, "swap_pieces", )
        far(case, dtype, "batch1_reads_batch0")
        if N > 8:
            far(case, dtype, "half_row_from_partner")


@pytest.mark.parametrize("piece", range(7))
def test_every_pair_of_pieces(piece):
    p = R.problem(R.Case("sizes", 144), "bf16")
    ref, written, scale = R.attention_ref(*p.args())
    out = R._evaluate(*p.args(), "f64", "swap_pieces", piece=piece)[0]
    assert R.worst(R.row_error(out, ref, scale)[written]) >= FAR


@pytest.mark.parametrize("N", R.WIDE_SIZES)
def test_wrong_head_and_batch_element_on_planes_and_wide_rows(N):
    for case in [c for h in R.PLANE_HEADS for c in R.plane_cases(h, N)] + [c for h in R.ROW_HEADS for c in R.wide_row_cases(h, N)]:
        for dtype in case.dtypes:
            far(case, dtype, "batch1_reads_batch0")
            if case.heads > 1:
                far(case, dtype, "head_xor_1")


@pytest.mark.parametrize("layout,items", [("rows", n) for n in R.ITEMS_ROWS] + [("planes", n) for n in R.ITEMS_PLANES])
def test_an_item_off_by_one(layout, items):
    far(R.item_cases(layout, items)[0], "bf16", "item_shift_" + layout)


@pytest.mark.parametrize("N", R.PEAKED_SIZES)
def test_the_peaked_inputs_are_peaked(N):
    p = R.problem(R.peaked_cases(N)[0], "f32")
    q, k = p.qkv.double().reshape(p.B, p.L, 3, p.heads, 64)[:, :, :2].unbind(2)
    s = torch.einsum("bihd,bjhd->bhij", q, k) / 8
    assert 25.0 < s.std().item() < 35.0
