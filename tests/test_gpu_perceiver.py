"""The Perceiver kernels of csrc/perceiver_attention.hip and csrc/perceiver_out.hip against the fp64 reference of tests/perceiver_reference.py.

  perceiver_attention_kernel<T, HDIM, QC, FEWK>     test_attention (the covering list of R.attention_cases: every Lq, Lk and head
                                                    count meets every instantiation it can reach, fp32 and bf16), test_strides
  perceiver_attention_scores_kernel<HDIM, QC>       test_attention_from_scores
  the fp16-pair store of both                       test_pair_output
  perceiver_probs_kernel<LQ, SCORES>                test_probs
  perceiver_probs_kernel + perceiver_out_kernel<LQ> test_probs_then_out, test_out_guard_not_holding

Every launch writes into a NaN-filled buffer with guard rows behind it (and guard columns beside it where ldo > N).  A case
asserts: every stored row is finite; the error per row -- per (row, head) over max |v| of the column's head for the attention
outputs, per (row, n) over sum_k |W[n, k]| max_j |v| + |bias[n]| for perceiver_out -- stays within the tolerance of
perceiver_reference (multiples of what CPU evaluations show, not of what the kernels show); nothing else was touched; a second
launch gives the same bits.  bf16 inputs are rounded first and the reference sees the rounded values.  Inputs sit in buffers
whose unaddressed rows and columns hold NaN.  tests/test_perceiver_reference.py shows which mistakes these inputs tell.
"""
from dataclasses import replace

import pytest
import torch

from tests import perceiver_reference as R
from tests.device_buffers import DEV, NAN, Padded, same_bits

pytestmark = pytest.mark.gpu


def lib():
    from aurora_amd.engine import lib as L

    L.load()
    return L


def nan_rows(rows, cols, dtype=torch.float32):
    """(buffer with two guard rows, the view a launch may write)."""
    buf = torch.full((rows + 2, cols), NAN, dtype=dtype, device=DEV)
    return buf, buf[:rows]


def dev(x, dtype):
    return x.to(torch.bfloat16 if dtype == "bf16" else torch.float32).to(DEV).contiguous()


def check_attention(case: R.Case, dtype: str, form: str = "keys", pair=None):
    """One case through perceiver_attention (form keys) or perceiver_attention_scores (form scores).  pair: None -- no guard
    word; True / False -- a pair guard that holds / does not hold."""
    L = lib()
    c = case
    p = R.problem(c, dtype)
    rows = c.n_cols * c.Lq
    word = None if pair is None else torch.tensor([1.0 if pair else 3.0], device=DEV)
    guard = None if pair is None else (word, 2.0)
    if form == "keys":
        ref, _, scale = R.attention_eval(*p.args())
        q_d, kv_d = dev(p.q, dtype), dev(p.kv, dtype)

        def launch(view):
            L.perceiver_attention(q_d, c.q_col_stride, kv_d, view, c.B, c.cols, c.kv_bstride, c.kv_lstride, c.Lq, c.Lk, c.heads,
                                  c.hd, pair_guard=guard)
    else:
        vs = p.score_rows()
        ref, _, scale = R.scores_eval(*p.score_args(vs.double()))
        vs_d = vs.to(DEV)

        def launch(view):
            L.perceiver_attention_scores(vs_d, c.s_off, view, c.B, c.cols, c.kv_bstride, c.kv_lstride, c.Lq, c.Lk, c.heads, c.hd,
                                         pair_guard=guard)
    bufs = [nan_rows(rows, c.inner, torch.bfloat16 if dtype == "bf16" else torch.float32) for _ in range(2)]
    for _, view in bufs:
        launch(view)
    torch.cuda.synchronize()
    what = (c.id, dtype, form, pair)
    out = bufs[0][1].cpu()
    if pair:
        hi, lo = R.unsplit(out)
        assert R.hi_is_rounded_value(hi, lo), what      # hi == half(hi + lo), exact ties aside
        out = hi + lo
        tol = R.PAIR_TOL[c.inputs]
    else:
        tol = R.BF16_TOL if dtype == "bf16" else R.F32_TOL[c.inputs]
    assert bool(torch.isfinite(out).all()), what
    err = R.worst(R.head_error(out, ref, scale, c.Lq))
    print(f"{c.id} {dtype} {form} pair={pair}: row error {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol, (what, err, tol)
    assert bool(torch.isnan(bufs[0][0][rows:]).all()), what
    assert same_bits(bufs[0][0], bufs[1][0]), what


@pytest.mark.parametrize("hd", R.HDIMS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_attention(dtype, hd):
    """QC = 3 (Lq 3, 6), QC = 7 with and without FEWK (Lq 9, 13, 14, 15: chunks 7 + 2 .. 7 + 7 + 1; Lk 1..4 / 5, 13), QC = 4 (Lq 1, 2,
    4, 7, 8; at head_dim 128 -- LPG = 32, the __shfl_xor(v, 16) step -- also Lq > 8); heads 1, 3, 4; lane counts that end
    inside a wave; flat inputs everywhere, peaked / ascending / descending / tagged on one case per instantiation."""
    for case in R.attention_cases(hd):
        check_attention(case, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_strides(dtype):
    """q_col_stride = Lq with per-column queries (every Perceiver layer after the first); kv_lstride and kv_bstride larger
    than packed, NaN rows in between."""
    for case in R.stride_cases():
        check_attention(case, dtype)


@pytest.mark.parametrize("hd", R.HDIMS)
def test_attention_from_scores(hd):
    """[v | NaN | scores at s_off > inner | NaN] rows with ld larger than needed; the two-pass maximum on peaked scores."""
    for case in R.scores_cases(hd):
        check_attention(case, "f32", form="scores")


@pytest.mark.parametrize("form", ["keys", "scores"])
@pytest.mark.parametrize("holds", [True, False])
def test_pair_output(holds, form):
    """The fp16-pair store at head_dim 16 (two groups share one 32-byte piece), 32, 64, 128: the represented value per row, and
    hi == half(hi + lo) bit for bit (exact ties aside); values of magnitude 16383; with the guard not holding, plain fp32 rows."""
    for case in R.pair_cases():
        check_attention(case, "f32", form=form, pair=holds)


@pytest.mark.parametrize("scores", [False, True])
def test_probs(scores):
    """P per element against the fp64 weights in the kernel's layout, slots 4 NLP .. 63 exactly zero, Vp bit-equal to the split
    of the fp32 differences (v0 - v2, v1 - v2, v2); nothing behind P and Vp touched."""
    L = lib()
    fn = L.load().aurora_hip_perceiver_probs_scores if scores else L.load().aurora_hip_perceiver_probs
    for c in R.probs_cases():
        p = R.problem(c, "f32")
        if scores:
            vs = p.score_rows()
            _, pw, _ = R.scores_eval(*p.score_args(vs.double()))
            src = vs.to(DEV)
        else:
            _, pw, _ = R.attention_eval(*p.args())
            q_d, src = dev(p.q, "f32"), dev(p.kv, "f32")
        bufs = []
        for _ in range(2):
            Pb, Pv = nan_rows(c.n_cols, c.heads * R.PO_PS)
            # (a lane writes one pair: the 32 floats perceiver_out reads; the 32 behind them are zero from the allocation)
            Pv.view(c.n_cols, c.heads, R.PO_PS)[:, :, 32:] = 0
            Vb, Vv = nan_rows(c.n_cols * 3, c.inner)
            tail = (c.B, c.cols, c.kv_bstride, c.kv_lstride, c.Lq, c.Lk, c.heads, c.hd, None, 0.0, L._stream())
            if scores:
                L._check(fn(src.data_ptr(), c.ld, c.s_off, Pv.data_ptr(), Vv.data_ptr(), *tail))
            else:
                L._check(fn(q_d.data_ptr(), src.data_ptr(), Pv.data_ptr(), Vv.data_ptr(), *tail))
            bufs.append((Pb, Vb))
        torch.cuda.synchronize()
        Pb, Vb = bufs[0]
        P = Pb[:c.n_cols].reshape(c.n_cols, c.heads, R.PO_PS).cpu()
        nlp = (c.Lq + 1) // 2
        assert bool(torch.isfinite(P).all()), c.id
        err = (P.double() - R.p_layout(pw)).abs().max().item()
        print(f"{c.id} scores={scores}: P error {err:.3e} (tolerance {R.P_TOL[c.inputs]:.3e})")
        assert err <= R.P_TOL[c.inputs], (c.id, err)
        assert bool((P[:, :, 4 * nlp:] == 0).all()), c.id
        if c.Lq % 2:    # the odd last level's partner slots
            assert bool((P[:, :, c.Lq] == 0).all()) and bool((P[:, :, 2 * nlp + c.Lq] == 0).all()), c.id
        v = p.values().float()
        d = torch.stack([v[:, 0] - v[:, 2], v[:, 1] - v[:, 2], v[:, 2]], dim=1).reshape(c.n_cols * 3, c.inner)
        Vp = Vb[:c.n_cols * 3]
        assert same_bits(Vp.cpu(), R.split_pairs(d)), c.id
        assert torch.equal(Vp, L.split_f16(d.to(DEV))), c.id
        assert bool(torch.isnan(Pb[c.n_cols:]).all()) and bool(torch.isnan(Vb[c.n_cols * 3:]).all()), c.id
        assert same_bits(Pb, bufs[1][0]) and same_bits(Vb, bufs[1][1]), c.id


def run_out(L, c, p, word=None):
    """probs -> out into a fresh padded buffer."""
    guard = None if word is None else (word, 2.0)
    P, Vp = L.perceiver_probs(dev(p.q, "f32"), dev(p.kv, "f32"), c.B, c.cols, c.kv_bstride, c.kv_lstride, c.Lq, c.Lk, c.heads, c.hd,
                              guard=guard)
    w_buf = torch.full((c.N, c.inner + c.ldw_extra), NAN, device=DEV)
    L.split_f16(p.W.float().to(DEV), scale=64.0, out=w_buf[:, :c.inner])
    out = Padded(c.n_cols * c.Lq, c.N, c.ldo_extra)
    L.perceiver_out(Vp, w_buf, P, out.view, c.n_cols, c.Lq, c.Lk, c.heads, c.hd,
                    bias=None if p.bias is None else p.bias.float().to(DEV), guard=guard)
    return out


@pytest.mark.parametrize("case", R.out_cases(), ids=lambda c: c.id)
def test_probs_then_out(case):
    """n_cols 1, 7, 31, 32, 33, 65 (a ragged and a single column tile), N = 128 (a single n-tile), 256, 384; 2, 4, 6, 16 heads (the
    four-stage ring exactly full, and the two smallest head counts beyond it); tile counts with remainders 1, 3, 7, 0 by the 8
    XCDs; bias; ldo = N + 4; ldw = inner + 32; flat, peaked, near-equal, fp16-edge and tagged values."""
    L = lib()
    c = case
    assert L.load().aurora_hip_perceiver_out_supported(c.Lq, c.Lk, c.heads, c.hd, c.N) == 1
    p = R.problem(c, "f32")
    ref, _, scale = R.out_reference(p)
    outs = [run_out(L, c, p) for _ in range(2)]
    torch.cuda.synchronize()
    got = outs[0].view.cpu()
    assert bool(torch.isfinite(got).all()), c.id
    err = R.worst(R.out_error(got, ref, scale))
    print(f"{c.id}: row error {err:.3e} (tolerance {R.OUT_TOL[c.inputs]:.3e})")
    assert err <= R.OUT_TOL[c.inputs], (c.id, err)
    assert outs[0].untouched(), c.id
    assert same_bits(outs[0].buf, outs[1].buf), c.id


def test_out_guard_not_holding_leaves_the_buffer_untouched():
    L = lib()
    c = replace(R.out_cases()[3], id="out-guard")
    p = R.problem(c, "f32")
    out = run_out(L, c, p, word=torch.tensor([3.0], device=DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all())
