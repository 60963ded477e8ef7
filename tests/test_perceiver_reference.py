"""tests/perceiver_reference.py can tell right from wrong, and its tolerances are what it says they are.  CPU only.

Every deliberately wrong variant of the reference lands >= TEETH x the LARGEST tolerance any GPU test applies to that
output (attention outputs: BF16_TOL; perceiver_out: OUT_TOL of the input set) away from the right result, on every
input set that claims to tell it.  The distances are printed in multiples of that tolerance (pytest -s).
"""
from dataclasses import replace

import pytest
import torch

from tests import perceiver_reference as R

# per-column queries (flat, peaked) and B = 2: both strides are live; packed rows, so that a key admitted behind Lk is a number
ATT = R.Case("teeth", 2, 11, 13, 3, 4, 64, q_per_col=True, kv_pad=(0, 0))
OUT = R.Case("teeth-out", 1, 33, 13, 3, 4, 64, N=256, bias=True)

# which input sets claim to tell which mistake (the monotone and one-hot sets share their queries between the columns, and a
# key dropped or admitted at the low end of a monotone softmax weighs nothing: they make no claim there)
EVERY = ("flat", "peaked", "ascending", "descending", "tagged")
CLAIMS = {
    "scale_1_hd": ("flat", "peaked", "ascending", "descending"),
    "drop_key": ("flat", "peaked", "ascending", "tagged"),
    "admit_key": ("flat", "peaked", "descending", "tagged"),
    "pad_query": ("flat", "peaked"),
    "q_stride_ignored": ("flat", "peaked"),
    "batch_stride_ignored": EVERY,
    "next_head": EVERY,
    "swap_pieces": EVERY,
    "swap_lane_halves": EVERY,
}
EVERY_OUT = ("flat", "peaked", "nearequal", "edge", "tagged")
CLAIMS_OUT = {
    "no_level0": EVERY_OUT,
    "third_weight_p2": EVERY_OUT,
    "drop_lo": EVERY_OUT,                        # (must exceed OUT_TOL on nearequal: asserted below)
    "no_bias": ("flat", "peaked", "nearequal", "tagged"),   # next to |v| ~ 16383 a bias of +-1 is small
}


def att_case(inputs):
    return replace(ATT, inputs=inputs, q_per_col=inputs in ("flat", "peaked"))


@pytest.mark.parametrize("wrong", R.WRONG)
def test_attention_inputs_tell_the_wrong_variant(wrong):
    assert set(CLAIMS) == set(R.WRONG)
    tol = max(R.BF16_TOL, *R.F32_TOL.values(), *R.PAIR_TOL.values())
    for inputs in CLAIMS[wrong]:
        c = att_case(inputs)
        p = R.problem(c)
        ref, _, scale = R.attention_eval(*p.args())
        bad, _, _ = R.attention_eval(*p.args(), wrong=wrong)
        dist = R.head_error(bad, ref, scale, c.Lq).max().item() / tol
        print(f"{wrong} on {inputs}: {dist:.1f} x tolerance")
        assert dist >= R.TEETH, (wrong, inputs, dist)


@pytest.mark.parametrize("wrong", ["drop_key", "next_head", "swap_pieces"])
def test_score_rows_tell_the_wrong_variant(wrong):
    """The same through the [v | ... | scores] rows of the kernels that take pre-multiplied scores."""
    for inputs in ("flat", "peaked", "tagged"):
        c = replace(ATT, inputs=inputs, q_per_col=False, s_gap=5, ld_extra=8)
        p = R.problem(c)
        vs = p.score_rows().double()
        ref, _, scale = R.scores_eval(*p.score_args(vs))
        if wrong == "drop_key":
            bad, _, _ = R.scores_eval(*p.score_args(vs)[:7], c.Lk - 1, c.heads, c.hd)
        else:
            bad, _, _ = R.scores_eval(*p.score_args(vs), wrong=wrong)
        dist = R.head_error(bad, ref, scale, c.Lq).max().item() / R.BF16_TOL
        print(f"scores: {wrong} on {inputs}: {dist:.1f} x tolerance")
        assert dist >= R.TEETH


@pytest.mark.parametrize("wrong", R.WRONG_OUT)
def test_out_inputs_tell_the_wrong_variant(wrong):
    assert set(CLAIMS_OUT) == set(R.WRONG_OUT)
    for inputs in CLAIMS_OUT[wrong]:
        p = R.problem(replace(OUT, inputs=inputs))
        ref, _, scale = R.out_reference(p)
        bad, _ = R.out_model_of(p, wrong)
        dist = R.worst(R.out_error(bad, ref, scale)) / R.OUT_TOL[inputs]
        print(f"{wrong} on {inputs}: {dist:.1f} x tolerance")
        assert dist >= R.TEETH, (wrong, inputs, dist)


def test_swapped_pair_halves_break_the_bit_identity():
    """High halves and remainders exchanged leave hi + lo as it was: only `hi is the rounded value` tells.  The plain form
    hi == half(hi + lo) fails for a correct split in the rare exact ties; the check admits those and nothing else."""
    x = R.rnd(200000, 32, seed=3).float()[:4000]
    big = R.rnd(200000, seed=4).float()
    hi, lo = R.split_halves(big)
    assert not torch.equal(hi, (hi + lo).half().float()) and R.hi_is_rounded_value(hi, lo)
    hi, lo = R.unsplit(R.split_pairs(x))
    assert R.hi_is_rounded_value(hi, lo) and torch.equal(hi, x.half().float())
    assert not R.hi_is_rounded_value(lo, hi)
    assert not R.hi_is_rounded_value(hi + hi.abs() * 2.0 ** -10, lo - hi.abs() * 2.0 ** -10)    # a neighbour of the rounded value


def test_reference_equals_scaled_dot_product_attention():
    """The plain formula against torch's own, in the packed layout with shared queries (the one layout both can express)."""
    c = R.Case("sdpa", 2, 7, 5, 4, 3, 32)
    p = R.problem(c)
    ref, _, _ = R.attention_eval(*p.args())
    kvr = p.kv.reshape(c.B, c.Lk, c.cols, 2, c.heads, c.hd).permute(3, 0, 2, 4, 1, 5)
    qq = p.q.reshape(c.Lq, c.heads, c.hd).permute(1, 0, 2)[None, None].expand(c.B, c.cols, -1, -1, -1)
    want = torch.nn.functional.scaled_dot_product_attention(qq, kvr[0], kvr[1]).permute(0, 1, 3, 2, 4).reshape(-1, c.inner)
    assert (ref - want).abs().max().item() < 1e-14
    vs = p.score_rows().double()
    got, _, _ = R.scores_eval(*p.score_args(vs))
    assert (got - want).abs().max().item() < 1e-6     # (the scores were rounded to fp32)


def test_padded_layouts_hold_nan_between_the_addressed_rows():
    c = R.Case("pad", 2, 5, 3, 2, 1, 16, kv_pad=(3, 5), s_gap=5, ld_extra=8)
    p = R.problem(c)
    assert p.kv.shape[0] == 2 * (2 * 8 + 5) and int(torch.isnan(p.kv[:, 0]).sum()) == p.kv.shape[0] - 2 * 5 * 2
    ref, _, _ = R.attention_eval(*p.args())
    assert bool(torch.isfinite(ref).all())
    vs = p.score_rows()
    assert bool(torch.isnan(vs[0, c.inner:c.s_off]).all()) and bool(torch.isnan(vs[0, c.s_off + c.Lq * c.heads:]).all())


def test_case_lists_cover_what_they_say():
    for hd in R.HDIMS:
        lpg = hd // 4
        cases = R.attention_cases(hd)
        for name, (lqs, lks) in R.instantiations(hd).items():
            mine = [c for c in cases if c.id.startswith(name + "-hd")]
            assert {c.Lq for c in mine} == set(lqs) and {c.Lk for c in mine} == set(lks) and {c.heads for c in mine} == set(R.HEADS)
            assert {c.inputs for c in mine} == {"flat", *R.EXTRA_SETS}
            assert any(c.n_cols * c.heads * lpg % 64 for c in mine)          # a group count that ends inside a wave
        assert any(c.n_cols * c.heads * lpg % 256 for c in cases)
        assert all(c.cols <= 37 and c.B <= 2 for c in cases)
        for name, lqs in (("sQC3", R.LQ_QC3), ("sQC7", R.LQ_QC7), ("sQC4", R.LQ_QC4)):
            mine = [c for c in R.scores_cases(hd) if c.id.startswith(name + "-hd")]
            assert {c.Lq for c in mine} == set(lqs) and {c.Lk for c in mine} == set(R.LK_ALL)
    out = R.out_cases()
    assert {c.Lq for c in out} == {3, 4, 13} and {c.heads for c in out} == {2, 4, 6, 16} and {c.N for c in out} == {128, 256, 384}
    assert {1, 7, 31, 32, 33, 65} <= {c.n_cols for c in out}
    assert {((c.n_cols + 31) // 32 * (c.N // 128)) % 8 for c in out} >= {0, 1, 3, 7}
    assert {(c.Lq, c.bias) for c in out} == {(Lq, b) for Lq in (3, 4, 13) for b in (True, False)}
    assert {c.Lq for c in out if c.ldo_extra} == {3, 4, 13} and any(c.ldw_extra for c in out)
    assert all(c.n_cols * c.Lq * c.N <= 1.1e6 for c in out)


def test_tolerances_are_eight_times_what_the_cpu_evaluations_show():
    """Re-measures every constant: an edited constant, case list or input set without a new measurement fails here."""
    table = R.measure_all()
    for name, measured in (("f32", R.F32_MEASURED), ("pair", R.PAIR_MEASURED), ("out", R.OUT_MEASURED), ("P", R.P_MEASURED)):
        for key, const in measured.items():
            now = table[name][key]
            print(f"{name} {key}: measured {now:.4e}, constant {const:.4e}")
            assert 0.9 * const <= now <= const, (name, key, now, const)
    now = table["bf16"]["all"]
    print(f"bf16: measured {now:.4e}, constant {R.BF16_MEASURED:.4e}")
    assert 0.9 * R.BF16_MEASURED <= now <= R.BF16_MEASURED
    assert table["f32"]["tagged"] < 1e-30 and table["pair"]["tagged"] < 1e-30      # exact but for exp(-120) in the fp64 reference
    assert R.F32_TOL["flat"] == 8 * R.F32_MEASURED["flat"] and R.BF16_TOL == 8 * R.BF16_MEASURED
    assert R.OUT_TOL["nearequal"] == 8 * R.OUT_MEASURED["nearequal"] and R.PAIR_TOL["edge"] == 8 * R.PAIR_MEASURED["edge"]
