"""Every activation form of the GEMM epilogues against fp64 at EXACTLY known inputs, over the whole fp32 range, through the
public entry points: tests/activation_reference.py injects the pre-activation (operands zero except column 0, the bias
carrying sweep and special values), so no accumulation term enters the bound.  One case per row of linear_reference.CASES with
an activation, on that row's shape, mode, flags, entry, batch, guard and layout (without residual: no form needs one):

  gelu_sig        t128-bf16-ragged, mid-direct, pp-direct, batched-t128 (activate16<bf16>), and the direct launch next to
                  every gelu_sig2 row
  gelu_sig2       mid-coalesced-gelu, pp-coalesced-gelu, pp-long-k, splitk-2 (epilogue_256_bf16_coalesced<4>); a4: <A4_EPI_PARTS>
  gelu_erf_fast   the direct launch next to three-coalesced and two-k32 (activate16, ACT_GELU_FAST)
  gelu_erf_fast2  three-coalesced, two-k32 (epilogue_256_f32_coalesced); pp2-k96, pp2-direct, pp2-w, pp2-pair-coalesced,
                  twin-pp2-holds (both epilogues of linear_kernel_f32pp: gelu_fast16x2)
  erff            t128-f32-ragged, ring-f32-coalesced-k32, ring-f32-scalar-c, twin-pp2-fails (the three-term twin of a
                  128 x 256 plan keeps AURORA_ACT_GELU)
  silu            t128-bf16-n27, t128-f32-m1, ring-f32-coalesced-row, mid-coalesced-silu-nobias, pp-coalesced-silu-nobias,
                  pp-scalar-c, three-direct, pp2-k160-silu-nobias, pp2-w-tall, batched-mid
  a4              pp-coalesced-gelu, pp-coalesced-silu-nobias, pp-direct, pp-scalar-c, pp-long-k in one child process

Per case, in this order: `linear_plan` names the row's kernel, tile and store path; the PREMISE -- the same launch without
activation returns fl32(s w + bias) bit for bit (bf16-only outputs: its round-to-nearest-even) -- ; every fp32 result within
the form's bound of the fp64 value at its input; NaN, +-inf, +-0 and x <= -104 as activation_reference.SPECIAL_RESULTS says;
a bf16 copy equal to the round-to-nearest-even of the fp32 copy bit for bit (finite values, those that round to inf
included); a second launch with the same bits; nothing outside the views touched.  A row that stores bf16 only (every coalesced
bf16 row, and the direct rows without a second output) must equal, bit for bit, the bf16 output of a launch of the same kernel
with a second fp32 output -- which takes the direct epilogue -- on the same inputs, and THAT launch's fp32 copy is held to
fp64: gelu_sig2 is gelu_sig and the packed SiLU the scalar one over the whole range.  The fp16-pair row is held to the bound
plus what its store keeps (22 bits, fp16 range), on the inputs whose result fits fp16.

gelu_erf_fast (__expf of -z^2) and gelu_erf_fast2 (exp2 of -z^2 log2 e) are each held to the bound, and to each other bit for
bit: __expf is exp2 of the argument times log2 e and the factor 0.5 is exact wherever it is multiplied in, so the two perform the
same operations; on the device they agree on every input.

Measured on an MI355X (worst error / bound, the input): gelu_sig = gelu_sig2 0.983 at 3.0738; gelu_erf_fast = gelu_erf_fast2
0.637 at 2.9672; erff 0.460 at 1.26 in the native kernels and 0.977 at 0.0433 in the three-term twin; silu 0.247 at 8.1086.
"""
import json
import math
import os
import subprocess
import sys
from pathlib import Path
from typing import NamedTuple, Optional

import pytest
import torch

from tests import activation_reference as A
from tests import linear_reference as R
from tests.device_buffers import DEV, NAN, Padded
from tests.test_gpu_linear import lib, operand, tdt

pytestmark = pytest.mark.gpu

ACTED = [c for c in R.CASES if c.act != R.ACT_NONE]
FP16_MAX = 6.0e4


def same_bits_or_nan(a: torch.Tensor, b: torch.Tensor) -> bool:
    as_int = torch.int32 if a.element_size() == 4 else torch.int16
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return bool(((a.view(as_int) == b.view(as_int)) | (torch.isnan(a) & torch.isnan(b))).all())


def bf16_of(x32: torch.Tensor) -> torch.Tensor:
    """Round to nearest even on the bits where x32 is finite (FLT_MAX rounds to inf); inf and NaN as they are."""
    return torch.where(torch.isfinite(x32), R.round_bf16_rne(x32), x32.bfloat16())


class Out(NamedTuple):
    main: torch.Tensor                 # (P, M, N) on the CPU, in the case's dtype (pair layout: its fp32 containers)
    second: Optional[torch.Tensor]     # (P, M, N), the other dtype
    bufs: list                         # whole device buffers, guard space included
    clean: bool                        # nothing outside the views touched


class Bench:
    """A case's device operands and one way to launch it: per bias vector, or, a strided batch, all vectors at once."""

    def __init__(self, c: R.Case, g: A.Grid):
        self.c, self.L, self.G, dt = c, lib(), c.batch, tdt(c)
        a = torch.zeros(c.M, c.K)
        w = torch.zeros(c.N, c.K)
        a[:, 0], w[:, 0] = g.s, g.w
        a_pairs, w_pairs = (1.0 if c.pre & R.F32_A_SPLIT else 0.0), (64.0 if c.pre & R.F32_W_SPLIT else 0.0)
        if self.G == 1:
            self.a, self.w = operand(a, dt, a_pairs), operand(w, dt, w_pairs)
        else:           # as test_gpu_linear.run_case: distinct batch strides, two / four guard rows between the problems
            G = self.G
            a_b = Padded(G * (c.M + 2), c.K, 8, dt).buf.view(-1, c.K + 8)[:G * (c.M + 2)].view(G, c.M + 2, c.K + 8)
            w_b = Padded(G * (c.N + 4), c.K, 8, dt).buf.view(-1, c.K + 8)[:G * (c.N + 4)].view(G, c.N + 4, c.K + 8)
            self.a, self.w = a_b[:, :c.M, :c.K], w_b[:, :c.N, :c.K]
            self.a.copy_(a.to(dt).to(DEV).expand(G, -1, -1))
            self.w.copy_(w.to(dt).to(DEV).expand(G, -1, -1))
        self.bias = None
        if g.bias is not None:
            bbuf = torch.full((g.bias.shape[0], c.N + 16), NAN, device=DEV)
            bbuf[:, :c.N] = g.bias.to(DEV)
            self.bias = bbuf[:, :c.N]
        self.P = 1 if g.bias is None else g.bias.shape[0]
        self.word = None if c.guard is None else torch.tensor([1.0 if c.guard else 3.0], device=DEV)
        self.ws = self.tickets = None
        if c.entry == "ws":
            self.ws = torch.empty(8 * R.tiles(c) * 256 * 256 * 4, dtype=torch.uint8, device=DEV)
            self.tickets = torch.zeros(64, dtype=torch.int32, device=DEV)

    def one(self, c: R.Case, a, w, bias, act: int):
        """One launch of a batch-1 case `c` (this case, or its twin with a second output)."""
        L, dt = self.L, tdt(c)
        ld = R.layout(c)
        c1 = Padded(c.M, c.N, ld["ldc"] - c.N, dt)
        c2 = Padded(c.M, c.N, ld["ldc2"] - c.N, torch.float32 if c.dtype == "bf16" else torch.bfloat16) if c.out2 else None
        kw = dict(out2=None if c2 is None else c2.view, residual=None, act=act)
        if c.entry == "ws":
            L.linear_ws(a, w, bias, c1.view, self.ws, self.tickets, split=c.split, **kw)
        elif c.dtype == "bf16":
            L.linear(a, w, bias, c1.view, **kw)
        else:
            with L.f32_gemm(c.base_mode, guard=None if self.word is None else (self.word, 2.0)):
                L.linear(a, w, bias, c1.view, presplit=c.pre, **kw)
        return c1, c2

    def run(self, act: int, second_output: bool = False) -> Out:
        """Every bias vector.  second_output: the launch with a second output next to a row that has none (a strided batch:
        one `linear` per problem, which the caller has checked takes the same kernel)."""
        c, L = self.c, self.L
        if self.G > 1 and not second_output:
            G, ldc = self.G, R.layout(c)["ldc"]
            cb = Padded(G * (c.M + 2), c.N, ldc - c.N, tdt(c))
            full = cb.buf[:G * (c.M + 2)].view(G, c.M + 2, ldc)
            with L.f32_gemm(c.base_mode, guard=None if self.word is None else (self.word, 2.0)):
                L.linear_batched(self.a, self.w, self.bias, full[:, :c.M, :c.N], act=act)
            torch.cuda.synchronize()
            clean = bool(torch.isnan(full[:, c.M:].float()).all() and torch.isnan(full[:, :, c.N:].float()).all()
                         and torch.isnan(cb.buf[G * (c.M + 2):].float()).all())
            return Out(full[:, :c.M, :c.N].cpu(), None, [cb.buf], clean)
        one = c._replace(entry="linear", batch=1, out2=True) if self.G > 1 else c._replace(out2=True) if second_output else c
        mains, seconds, bufs, clean = [], [], [], True
        for p in range(self.P):
            a, w = (self.a[p], self.w[p]) if self.G > 1 else (self.a, self.w)
            c1, c2 = self.one(one, a, w, None if self.bias is None else self.bias[p], act)
            torch.cuda.synchronize()
            clean = clean and c1.untouched() and (c2 is None or c2.untouched())
            mains.append(c1.view.cpu())
            bufs.append(c1.buf)
            if c2 is not None:
                seconds.append(c2.view.cpu())
                bufs.append(c2.buf)
        if self.tickets is not None:
            assert int(self.tickets.abs().sum()) == 0, c.id
        return Out(torch.stack(mains), torch.stack(seconds) if seconds else None, bufs, clean)


def check_plan(L, c: R.Case, expect_kernel: Optional[str], whole: bool = True):
    plan = L.linear_plan(c.M, c.N, c.K, tdt(c), **R.plan_kwargs(c, cus=0))
    assert (plan.kernel, plan.vec_store) == (expect_kernel or c.kernel, c.vec), (c.id, plan)
    if expect_kernel is None and whole:
        assert (plan.bm, plan.bn) == c.tile and (plan.ksplit == c.ksplit if c.kernel == "pp_splitk" else plan.ksplit <= 1), (c.id, plan)
        assert plan.twin == (c.guard is not None and c.base_mode == 2), (c.id, plan)


def held_to_fp64(tag: str, form: str, pre: torch.Tensor, got: torch.Tensor, pair: bool = False) -> A.Worst:
    if pair:           # what fits fp16, and what the two halves keep of it
        ref = A.reference(form, pre)
        fits = torch.isfinite(pre) & (ref.abs() < FP16_MAX)
        w = A.worst(form, pre[fits], got[fits], extra=2.0 ** -22 * ref[fits].abs() + 2.0 ** -24)
    else:
        normal = ~(pre.abs() < A.FLT_MIN)         # (at a subnormal input half the subnormal spacing is most of a relative bound)
        w, tiny = A.worst(form, pre[normal], got[normal]), A.worst(form, pre[~normal], got[~normal])
        assert tiny.ratio <= 1.0, (tag, form, "subnormal input", tiny)
        assert A.special_failures(form, pre, got) == [], tag
    print(f"ACT {tag} {form}: worst error / bound {w.ratio:.3f} at x = {w.x!r}")
    assert w.ratio <= 1.0, (tag, form, w)
    return w


def run_case(case: R.Case, expect_kernel: Optional[str] = None) -> dict:
    c = case._replace(res="none")
    L = lib()
    check_plan(L, c, expect_kernel)
    batched = c.entry == "batched"
    g = A.grid(c.M, c.N, c.bias, vectors=c.batch if batched else 0)
    A.check_grid(g)
    pre = A.pre_of(g)
    bench = Bench(c, g)
    tag = c.id + (" [a4]" if expect_kernel == "a4" else "")
    pair = bool(c.pre & R.F32_C_SPLIT)
    bf16 = c.dtype == "bf16"

    def value(out: Out) -> torch.Tensor:
        if not pair:
            return out.main
        hi, lo = R.from_pairs(out.main.reshape(-1, out.main.shape[-1]))
        return (hi + lo).reshape(pre.shape)

    # ---- the premise: without activation the launch returns the injected value ----
    plain = bench.run(R.ACT_NONE)
    assert plain.clean, tag
    if pair:
        fits = torch.isfinite(pre) & (pre.abs() < FP16_MAX)
        err = (value(plain).double() - pre.double()).abs()[fits]
        assert bool((err <= 2.0 ** -22 * pre.double().abs()[fits] + 2.0 ** -24).all()), ("premise", tag)
    elif bf16:
        assert same_bits_or_nan(plain.main, bf16_of(pre)), ("premise", tag)
        assert plain.second is None or same_bits_or_nan(plain.second, pre), ("premise", tag)
    else:
        assert same_bits_or_nan(plain.main, pre), ("premise", tag)
        assert plain.second is None or same_bits_or_nan(plain.second, bf16_of(pre)), ("premise", tag)

    # ---- the activation ----
    first, again = bench.run(c.act), bench.run(c.act)
    assert first.clean and again.clean, tag
    assert all(same_bits_or_nan(x.cpu(), y.cpu()) for x, y in zip(first.bufs, again.bufs)), ("second launch", tag)
    form = A.form_of(c)
    found = {}
    if not bf16:
        found[form] = held_to_fp64(tag, form, pre, value(first), pair)
        if first.second is not None:
            assert same_bits_or_nan(first.second, bf16_of(first.main)), ("bf16 copy", tag)
    elif first.second is not None:
        found[form] = held_to_fp64(tag, form, pre, first.second)
        assert same_bits_or_nan(first.main, bf16_of(first.second)), ("bf16 copy", tag)
    if bf16 and first.second is None or (form == "gelu_erf_fast2" and c.kernel in ("f32_three", "f32_two")):
        # the same kernel with a second output: the direct epilogue and its scalar forms
        twin = c._replace(entry="linear", batch=1, out2=True) if batched else c._replace(out2=True)
        check_plan(L, twin, expect_kernel or c.kernel, whole=False)
        direct = bench.run(c.act, second_output=True)
        assert direct.clean, tag
        dform = A.form_of(c, direct=True)
        if bf16:
            found[dform] = held_to_fp64(tag + " (direct)", dform, pre, direct.second)
            assert same_bits_or_nan(direct.main, bf16_of(direct.second)), ("bf16 copy", tag)
            assert same_bits_or_nan(first.main, direct.main), ("coalesced / direct bf16 bits", tag, form, dform)
            found[form] = found[dform]
            print(f"ACT {tag} {form}: bf16 only, the bits of the direct launch's")
        else:
            found[dform] = held_to_fp64(tag + " (direct)", dform, pre, direct.main)
            assert same_bits_or_nan(direct.second, bf16_of(direct.main)), ("bf16 copy", tag)
            assert same_bits_or_nan(first.main, direct.main), ("coalesced / direct fp32 bits", tag, form, dform)
    return {k: [v.ratio, v.x] for k, v in found.items()}


@pytest.mark.parametrize("case", ACTED, ids=lambda c: c.id)
def test_activation(case):
    assert run_case(case)


def four_wave_worst():
    """The a4 rows with an activation in THIS process (which must have been started with AURORA_GEMM_A4_MIN_K set)."""
    return {c.id: run_case(c, expect_kernel="a4") for c in ACTED if c.a4}


def test_four_wave_kernel_activations():
    """As test_gpu_linear.test_four_wave_kernel: one fresh child under a time limit runs every a4 row with an activation."""
    root = Path(__file__).resolve().parents[1]
    code = (f"import json, sys; sys.path.insert(0, {str(root)!r}); from tests import test_gpu_activations as t; "
            "print('WORST ' + json.dumps(t.four_wave_worst()))")
    res = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code],
                         env={**os.environ, "AURORA_GEMM_A4_MIN_K": "64"}, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    print("\n".join(l for l in res.stdout.splitlines() if l.startswith("ACT ")))
    worst = json.loads(next(l for l in res.stdout.splitlines() if l.startswith("WORST "))[6:])
    assert set(worst) == {c.id for c in ACTED if c.a4} and len(worst) >= 5
    for cid, forms in worst.items():
        for form, (ratio, x) in forms.items():
            assert ratio <= 1.0 and not math.isnan(ratio), (cid, form, ratio, x)
