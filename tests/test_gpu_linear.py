"""Every GEMM kernel and epilogue form of csrc/gemm*.hip against the fp64 reference of tests/linear_reference.py, per element.

  linear_kernel<T> (tile128)                 t128-*, batched-t128, t128-planes-kv
  linear_kernel_256<float, 4, 4> (ring)      ring-f32-*        (its bf16 form is unreachable: see the table's comment)
  linear_kernel_256<bf16, 2, 3> (ring_mid)   mid-*, batched-mid
  linear_kernel_256pp<false> (pp)            pp-*
  linear_kernel_256pp<true> (pp_splitk)      splitk-*
  linear_kernel_256a4 (a4)                   the a4 rows of the table, in one child process (test_four_wave_kernel)
  linear_kernel_256_f32x3<3> / <2>           three-*, two-*, the twins whose guard does not hold, batched-three-guard
  linear_kernel_f32pp<A_PRE, W_PRE, TALL>    pp2-*, twin-pp2-*, batched-nobias
  linear_ln512_kernel<true> / <false>        test_linear_layernorm

A case names the kernel, tile, K split and store path it must take; `linear_plan` for THIS device has to agree or the case fails.
Outputs are NaN-filled `Padded` buffers with guard rows and columns, operands sit in buffers whose unaddressed rows and columns
hold NaN.  Asserted: every stored element finite; |stored - reference| within the per-element tolerance; nothing else touched; a
second launch gives the same bits; a bf16 second copy is the round-to-nearest-even of the fp32 one, bit for bit.
tests/test_linear_reference.py shows which mistakes these inputs and this tolerance tell.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import linear_reference as R
from tests.device_buffers import DEV, NAN, Padded, same_bits

pytestmark = pytest.mark.gpu


def lib():
    from aurora_amd.engine import lib as L

    L.load()
    return L


def tdt(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def operand(x, dtype, pairs=0.0):
    """(rows, K) values in a NaN-surrounded device buffer; pairs: the fp16-pair layout with that scale."""
    x = R.pairs_of(x.float(), pairs) if pairs else x.to(dtype)
    return Padded(x.shape[0], x.shape[1], 8, dtype, fill=x.to(DEV)).view


def run_case(c: R.Case, expect_kernel=None):
    """Launch twice, check everything; returns (worst error / tolerance) per output."""
    L = lib()
    dt, other = tdt(c), (torch.float32 if c.dtype == "bf16" else torch.bfloat16)
    plan = L.linear_plan(c.M, c.N, c.K, dt, **R.plan_kwargs(c, cus=0))
    assert (plan.kernel, plan.vec_store) == (expect_kernel or c.kernel, c.vec), (c.id, plan)
    if expect_kernel is None:
        assert (plan.bm, plan.bn) == c.tile and (plan.ksplit == c.ksplit if c.kernel == "pp_splitk" else plan.ksplit <= 1), (c.id, plan)
        assert plan.twin == (c.guard is not None and c.base_mode == 2), (c.id, plan)
    p = R.problem(c)
    out, pre, S = R.linear_ref(c, p)
    ld, G = R.layout(c), c.batch
    bias = None
    if p.bias is not None:
        bbuf = torch.full((G, c.N + 16), NAN, device=DEV)
        bbuf[:, :c.N] = p.bias.float().to(DEV)
        bias = bbuf[:, :c.N]
    res = None
    if p.res is not None:
        rows = p.res.shape[0]
        res = Padded(rows, c.N, ld["ldr"] - c.N, fill=p.res.float().to(DEV)).view
        res = res.expand(c.M, c.N) if c.res == "row" else res
    word = None if c.guard is None else torch.tensor([1.0 if c.guard else 3.0], device=DEV)
    a_pairs, w_pairs = (1.0 if c.pre & R.F32_A_SPLIT else 0.0), (64.0 if c.pre & R.F32_W_SPLIT else 0.0)
    if G == 1:
        a_d, w_d = operand(p.a[0], dt, a_pairs), operand(p.w[0], dt, w_pairs)
    else:   # distinct batch strides: A and W problems sit in one NaN-filled buffer each, two guard rows between them
        a_b = Padded(G * (c.M + 2), c.K, 8, dt).buf.view(-1, c.K + 8)[:G * (c.M + 2)].view(G, c.M + 2, c.K + 8)
        w_b = Padded(G * (c.N + 4), c.K, 8, dt).buf.view(-1, c.K + 8)[:G * (c.N + 4)].view(G, c.N + 4, c.K + 8)
        a_d, w_d = a_b[:, :c.M, :c.K], w_b[:, :c.N, :c.K]
        a_d.copy_(p.a.to(dt).to(DEV))
        w_d.copy_(p.w.to(dt).to(DEV))
    ws = tickets = None
    if c.entry == "ws":
        ws = torch.empty(8 * R.tiles(c) * 256 * 256 * 4, dtype=torch.uint8, device=DEV)
        tickets = torch.zeros(64, dtype=torch.int32, device=DEV)
    bufs = []
    for _ in range(2):
        if c.entry == "planes":
            pl = torch.full((c.heads, c.M + 2, 3, 64), NAN, dtype=dt, device=DEV)
            L.linear_planes(a_d, w_d, bias[0], pl[:, :c.M], sel0=c.sel0)
            bufs.append((pl, None))
            continue
        if G > 1:
            cb = Padded(G * (c.M + 2), c.N, ld["ldc"] - c.N, dt)
            view = cb.buf[:G * (c.M + 2)].view(G, c.M + 2, ld["ldc"])[:, :c.M, :c.N]
            with L.f32_gemm(c.base_mode, guard=None if word is None else (word, 2.0)):
                L.linear_batched(a_d, w_d, bias, view, act=c.act)
            bufs.append((cb, None))
            continue
        cw = c.N if not (c.pre & R.F32_C_SPLIT) else c.N      # (the pair layout fills the same N containers)
        c1 = Padded(c.M, cw, ld["ldc"] - cw, dt)
        c2 = Padded(c.M, c.N, ld["ldc2"] - c.N, other) if c.out2 else None
        kw = dict(out2=None if c2 is None else c2.view, residual=res, act=c.act)
        b1 = None if bias is None else bias[0]
        if c.entry == "ws":
            L.linear_ws(a_d, w_d, b1, c1.view, ws, tickets, split=c.split, **kw)
        elif c.dtype == "bf16":
            L.linear(a_d, w_d, b1, c1.view, **kw)
        else:
            with L.f32_gemm(c.base_mode, guard=None if word is None else (word, 2.0)):
                L.linear(a_d, w_d, b1, c1.view, presplit=c.pre, **kw)
        bufs.append((c1, c2))
    torch.cuda.synchronize()
    if tickets is not None:
        assert int(tickets.abs().sum()) == 0, c.id
    twin3 = c.guard is False
    store = "bf16" if c.dtype == "bf16" else "pair" if (c.pre & R.F32_C_SPLIT) else "f32"
    tol = R.tolerance(c, p, out, pre, S, store, three_term_twin=twin3)
    worst = {}
    if c.entry == "planes":
        pl = bufs[0][0]
        got = pl[:, :c.M, c.sel0:].cpu()
        assert bool(torch.isfinite(got.float()).all()), c.id
        worst["c"] = R.worst_ratio(got, R.planes_of(out[0], c.heads), R.planes_of(tol[0], c.heads))
        assert bool(torch.isnan(pl[:, c.M:].float()).all() and torch.isnan(pl[:, :c.M, :c.sel0].float()).all()), c.id
        assert same_bits(pl, bufs[1][0]), c.id
    elif G > 1:
        cb = bufs[0][0]
        full = cb.buf[:G * (c.M + 2)].view(G, c.M + 2, ld["ldc"])
        got = full[:, :c.M, :c.N].cpu()
        assert bool(torch.isfinite(got.float()).all()), c.id
        worst["c"] = R.worst_ratio(got, out, tol)
        assert bool(torch.isnan(full[:, c.M:].float()).all() and torch.isnan(full[:, :, c.N:].float()).all()), c.id
        assert same_bits(cb.buf, bufs[1][0].buf), c.id
    else:
        c1, c2 = bufs[0]
        got = c1.view.cpu()
        if store == "pair":
            hi, lo = R.from_pairs(got)
            assert R.hi_is_rounded_value(hi, lo), c.id
            got = hi + lo
        assert bool(torch.isfinite(got.float()).all()), c.id
        worst["c"] = R.worst_ratio(got, out[0], tol[0])
        assert c1.untouched() and same_bits(c1.buf, bufs[1][0].buf), c.id
        if c2 is not None:
            got2 = c2.view.cpu()
            assert bool(torch.isfinite(got2.float()).all()), c.id
            st2 = "f32" if c.dtype == "bf16" else "bf16"
            worst["c2"] = R.worst_ratio(got2, out[0], R.tolerance(c, p, out, pre, S, st2, three_term_twin=twin3)[0])
            assert c2.untouched() and same_bits(c2.buf, bufs[1][1].buf), c.id
            f32_copy, bf_copy = (got2, got) if c.dtype == "bf16" else (got, got2)
            assert same_bits(R.round_bf16_rne(f32_copy), bf_copy), c.id     # both stored from the same registers
    for name, w in worst.items():
        print(f"PARITY {c.id} [{expect_kernel or c.kernel} {c.form}] {name}: worst error / tolerance {w:.3f}")
    return worst


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_linear(case):
    for name, w in run_case(case).items():
        assert w <= 1.0, (case.id, name, w)


def four_wave_worst():
    """The a4 rows of the table in THIS process (which must have been started with AURORA_GEMM_A4_MIN_K set)."""
    return {c.id: run_case(c, expect_kernel="a4") for c in R.CASES if c.a4}


def test_four_wave_kernel():
    """AURORA_GEMM_A4_MIN_K is read once per process: one fresh child runs every a4 row -- plan assertion included, which must
    say a4 there -- against fp64 and prints its worst errors; nothing else is added to its environment."""
    root = Path(__file__).resolve().parents[1]
    code = (f"import json, sys; sys.path.insert(0, {str(root)!r}); from tests import test_gpu_linear as t; "
            "print('WORST ' + json.dumps(t.four_wave_worst()))")
    res = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code],
                         env={**os.environ, "AURORA_GEMM_A4_MIN_K": "64"}, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    print("\n".join(l for l in res.stdout.splitlines() if l.startswith("PARITY ")))
    worst = json.loads(next(l for l in res.stdout.splitlines() if l.startswith("WORST "))[6:])
    assert set(worst) == {c.id for c in R.CASES if c.a4} and len(worst) >= 5
    for cid, w in worst.items():
        for name, v in w.items():
            assert v <= 1.0, (cid, name, v)


def test_bad_strided_batches_are_refused():
    L = lib()
    a = torch.zeros((3, 8, 64), dtype=torch.bfloat16, device=DEV)
    w = torch.zeros((3, 16, 64), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="batch strides"):
        L.linear_batched(a, w, torch.zeros((3, 18), device=DEV)[:, :16], torch.zeros((3, 8, 16), dtype=torch.bfloat16, device=DEV))


@pytest.mark.parametrize("M,K", R.LN_CASES)
@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("shadow", [True, False])
def test_linear_layernorm(M, K, in_place, shadow):
    L = lib()
    q = R.ln_problem(M, K)
    out, tol = R.linear_ln_ref(q)
    bf = torch.bfloat16
    a_d, w_d = operand(q["a"], bf), operand(q["w"], bf)
    vec = lambda t: torch.cat([t.float(), torch.full((16,), NAN)]).to(DEV)[:512]   # noqa: E731
    b_d, g_d, s_d = vec(q["b"]), vec(q["gain"]), vec(q["shift"])
    runs = []
    for _ in range(2):
        x = Padded(M, 512, 8, fill=q["x"].float().to(DEV))
        xo = x if in_place else Padded(M, 512, 8)
        xb = Padded(M, 512, 8, bf) if shadow else None
        L.linear_layernorm(a_d, w_d, b_d, g_d, s_d, x.view, xo.view, None if xb is None else xb.view)
        runs.append((x, xo, xb))
    torch.cuda.synchronize()
    x, xo, xb = runs[0]
    got = xo.view.cpu()
    assert bool(torch.isfinite(got).all())
    worst = ((got.double() - out).abs() / tol).max().item()
    print(f"PARITY linear_layernorm M={M} K={K} in_place={in_place} shadow={shadow}: worst error / tolerance {worst:.3f}")
    assert worst <= 1.0
    assert xo.untouched() and same_bits(xo.buf, runs[1][1].buf)
    if not in_place:
        assert x.untouched() and torch.equal(x.view.cpu(), q["x"].float())
    if xb is not None:
        assert xb.untouched() and same_bits(xb.buf, runs[1][2].buf)
        assert same_bits(R.round_bf16_rne(got), xb.view.cpu())
