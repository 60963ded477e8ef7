"""tests/linear_reference.py on the CPU: the dispatch query puts every case of the table on the kernel it names (256 CUs), the
table covers every kernel id and epilogue form, a correct fp32 evaluation fits inside the per-element tolerance for every case,
and each seeded mistake lands outside it -- the condition that makes tests/test_gpu_linear.py worth having."""
import pytest
import torch

from tests import linear_reference as R


@pytest.fixture(scope="module")
def L():
    from aurora_amd.build import build_library
    from aurora_amd.engine import lib

    build_library(force=False, verbose=False)
    lib.load()
    return lib


def dt(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_every_case_reaches_the_kernel_it_names_on_256_cus(L, case):
    c = case
    plan = L.linear_plan(c.M, c.N, c.K, dt(c), **R.plan_kwargs(c, cus=256))
    assert (plan.kernel, (plan.bm, plan.bn), plan.vec_store) == (c.kernel, c.tile, c.vec), plan
    assert plan.ksplit == c.ksplit if c.kernel == "pp_splitk" else plan.ksplit <= 1, plan
    assert plan.twin == (c.guard is not None and c.base_mode == 2), plan


def test_the_table_covers_every_kernel_and_every_epilogue_form():
    kernels = {c.kernel for c in R.CASES} | ({"a4"} if any(c.a4 for c in R.CASES) else set())
    assert kernels == set(R.KERNELS) and len(R.KERNELS) == 13
    # each big-tile kernel meets each epilogue form it has
    forms = {}
    for c in R.CASES:
        forms.setdefault(c.kernel, set()).add(c.form)
        if c.a4:
            forms.setdefault("a4", set()).add(c.form)
    general = {"coalesced", "direct_vec", "direct_scalar"}
    for k in ("ring", "ring_mid", "pp", "a4", "f32_three", "f32_pp"):
        assert general <= forms[k], (k, forms[k])
    assert {"direct_vec", "direct_scalar"} <= forms["tile128"]
    assert {"coalesced", "direct_vec"} <= forms["pp_splitk"] and {"coalesced", "direct_vec"} <= forms["f32_two"]
    assert set().union(*forms.values()) == set(R.FORMS)
    # both coalesced bf16 ladders (<4> GELU, <2> otherwise) with and without bias; the fp32 one with a residual and the row
    co = [c for c in R.CASES if c.form == "coalesced"]
    for k in ("ring_mid", "pp"):
        assert {c.act for c in co if c.kernel == k} == {R.ACT_NONE, R.ACT_GELU, R.ACT_SILU}
        assert {c.bias for c in co if c.kernel == k} == {True, False}
    assert {c.res for c in co if c.kernel == "ring"} == {"none", "full", "row"}
    assert {c.misalign for c in R.CASES} == {"none", "c", "c2", "res"}
    assert {c.guard for c in R.CASES if c.base_mode == 2} == {None, True, False}
    assert {c.kernel for c in R.CASES if c.entry == "batched"} >= {"tile128", "f32_three", "ring_mid"}
    assert any(c.entry == "batched" and not c.bias for c in R.CASES)
    assert {c.sel0 for c in R.CASES if c.entry == "planes"} == {0, 1}
    assert all(c.M * c.N * c.K <= 8192 * 2048 * 1024 * 1.01 for c in R.CASES)


def test_the_argument_check_refuses_what_the_table_calls_unreachable(L):
    for K in (32, 96, 160):       # bf16: one, three or five 32-wide stages
        with pytest.raises(ValueError, match="multiple"):
            L.linear_plan(8193, 1024, K, torch.bfloat16, cus=256)
    for M in (1024, 4097, 8193, 16385, 32769, 65537):      # below K = 355 the cost model never keeps 256 x 256 bf16 tiles
        for N in (256, 512, 1024, 2048):
            for K in (64, 128, 192, 256, 320):
                assert L.linear_plan(M, N, K, torch.bfloat16, cus=256).kernel in ("ring_mid", "tile128")


_ratio = {}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_a_correct_fp32_evaluation_is_inside_the_tolerance(case):
    c = case
    p = R.problem(c)
    out, pre, S = R.linear_ref(c, p)
    bound = c.K * R.U32 * S
    for order in ("ascending", "pairwise"):
        got, got_pre = R.emulate(c, p, order)
        acc = ((got_pre.double() - pre).abs() / bound).max().item()
        _ratio[(c.id, order)] = acc
        assert acc * R.ACC_MULTIPLE <= R.C_ACC, (c.id, order, acc)      # the evidence C_ACC stands on
        store = "bf16" if c.dtype == "bf16" else "f32"
        stored = got.bfloat16() if store == "bf16" else got
        assert R.worst_ratio(stored, out, R.tolerance(c, p, out, pre, S, store)) <= 1.0, (c.id, order)
        if c.dtype == "bf16" or c.out2:
            assert torch.equal(R.round_bf16_rne(got), got.bfloat16())


def _pick(**want):
    for c in R.CASES:
        if all(getattr(c, k) == v for k, v in want.items()):
            return c
    raise AssertionError(want)


SEEDED = [
    ("drop_last_k_step", dict(id="pp-long-k")), ("drop_last_k_step", dict(id="mid-coalesced-k64")),
    ("drop_last_k_step", dict(id="three-coalesced")), ("drop_last_k_step", dict(id="ring-f32-direct")),
    ("swap_pieces", dict(id="pp-coalesced")), ("swap_pieces", dict(id="ring-f32-coalesced-plain")),
    ("swap_pieces", dict(id="pp2-k96")),
    ("bias_n16", dict(id="pp-coalesced-gelu")), ("bias_n16", dict(id="t128-f32-ragged")), ("bias_n16", dict(id="pp2-w")),
    ("res_row_m1", dict(id="ring-f32-coalesced-k32")), ("res_clamped_row", dict(id="ring-f32-coalesced-k32")),
    ("res_row_m1", dict(id="mid-direct")), ("res_clamped_row", dict(id="three-coalesced")),
    ("skip_act_fragment", dict(id="pp-coalesced-gelu")), ("skip_act_fragment", dict(id="mid-coalesced-silu-nobias")),
    ("skip_act_fragment", dict(id="three-coalesced")),
    ("drop_split_slice", dict(id="splitk-2")), ("drop_split_slice", dict(id="splitk-3-direct")),
    ("drop_split_slice", dict(id="splitk-own")),
    ("batch_prev_weights", dict(id="batched-t128")), ("batch_prev_weights", dict(id="batched-nobias")),
    ("batch_prev_bias", dict(id="batched-three-guard")), ("batch_prev_bias", dict(id="batched-mid")),
    ("row_read_with_stride", dict(id="ring-f32-coalesced-row")), ("row_read_with_stride", dict(id="two-k32")),
]


@pytest.mark.parametrize("wrong,which", SEEDED, ids=lambda v: v if isinstance(v, str) else v["id"])
def test_a_seeded_mistake_is_outside_the_tolerance(wrong, which):
    c = _pick(**which)
    p = R.problem(c)
    out, pre, S = R.linear_ref(c, p)
    bad, _, _ = R.linear_ref(c, p, wrong=wrong)
    store = "bf16" if c.dtype == "bf16" else "f32"
    tol = R.tolerance(c, p, out, pre, S, store)
    stored = bad.float().bfloat16() if store == "bf16" else bad.float()
    ratio = (stored.double() - out).abs() / tol
    assert ratio.max().item() > 4.0, (wrong, c.id, ratio.max().item())
    assert set(w for w, _ in SEEDED) == set(R.WRONG)


def test_a_truncating_bf16_store_is_caught_bit_for_bit_and_by_the_tolerance():
    c = R.BY_ID["pp-direct"]
    p = R.problem(c)
    out, pre, S = R.linear_ref(c, p)
    got, _ = R.emulate(c, p)
    assert torch.equal(R.round_bf16_rne(got), got.bfloat16())            # check 7 of the GPU test, on a correct store
    cut = R.truncate_bf16(got)
    assert not torch.equal(cut, got.bfloat16())
    # a truncated store is up to 2^-7 |v| off: outside 2^-8 |v| + the fp32 terms wherever the dropped bits were large
    assert R.worst_ratio(cut, out, R.tolerance(c, p, out, pre, S, "bf16")) > 1.5


def test_swapped_pair_halves_and_exchanged_head_planes_are_caught():
    c = R.BY_ID["pp2-pair-coalesced"]
    p = R.problem(c)
    out, pre, S = R.linear_ref(c, p)
    got, _ = R.emulate(c, p)
    pairs = R.pairs_of(got[0])
    hi, lo = R.from_pairs(pairs)
    tol = R.tolerance(c, p, out, pre, S, "pair")[0]
    assert R.worst_ratio(hi + lo, out[0], tol) <= 1.0
    h16 = pairs.view(torch.float16).view(c.M, c.N // 32, 2, 32)
    swapped = h16.flip(2).contiguous().view(c.M, 2 * c.N).view(torch.float32)       # remainders where the halves belong
    lo2, hi2 = R.from_pairs(swapped)
    assert torch.equal(hi2, hi) and not R.hi_is_rounded_value(lo2, hi2)
    for cid in ("pp-planes", "t128-planes-kv"):
        c = R.BY_ID[cid]
        p = R.problem(c)
        out, pre, S = R.linear_ref(c, p)
        planes = R.planes_of(out[0], c.heads)
        tol = R.planes_of(R.tolerance(c, p, out, pre, S, "bf16")[0], c.heads)
        assert planes.shape == (c.heads, c.M, 3 - c.sel0, 64)
        sel = 3 - c.sel0
        for s in range(sel):      # plane h, slot s is column block s * heads + h
            assert torch.equal(planes[1, :, s], out[0][:, (s * c.heads + 1) * 64:(s * c.heads + 2) * 64])
        wrong = planes.clone()
        wrong[0], wrong[1] = planes[1], planes[0]
        assert ((wrong.float().bfloat16().double() - planes).abs() / tol).max().item() > 4.0


@pytest.mark.parametrize("M,K", R.LN_CASES)
def test_fused_linear_layernorm_reference_has_teeth(M, K):
    q = R.ln_problem(M, K)
    out, tol = R.linear_ln_ref(q)
    # a correct evaluation as the kernel defines it: the linear's result rounded to bf16, fp32 LayerNorm
    y = (q["a"].float() @ q["w"].float().T + q["b"].float()).bfloat16().float()
    ln = torch.nn.functional.layer_norm(y, (512,), q["gain"].float(), q["shift"].float(), 1e-5)
    got = q["x"].float() + ln
    assert ((got.double() - out).abs() / tol).max().item() <= 1.0
    for wrong in ("stats_without_bias", "residual_row_above"):
        bad, _ = R.linear_ln_ref(q, wrong=wrong)
        assert ((bad - out).abs() / tol).max().item() > 4.0, wrong
