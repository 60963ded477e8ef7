"""The fp16-pair range guards AT their limits.

A guarded launch runs its two-term (fp16) form iff `*word < limit` and its three-term (bf16) twin iff not.  The rest of the
suite runs every guard at words decades away from any limit; here the word is the float below the limit, the limit itself and
the float above it (op level, where the word can be set exactly), the activations attain the L1 bound the limits are derived
from, and -- step level -- the model inputs are scaled until a step's own words sit at the limits `aurora_hip_guard_limits`
reports.

Shapes: M = 257 (a ragged last m-tile of both the 128- and the 256-row tiles), N = 256 (one tile column) or 128 (the narrow
two-term tiles), K = 96 (the ping-pong two-term kernel's three-stage minimum; K = 64 reaches the in-phase two-term kernel).
"""
import json
import math
import os
from pathlib import Path

import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, normalisation
from aurora_amd.engine import lib as L
from oracle import aurora_oracle as oracle
from tests import helpers
from tests.golden_cases import CASES as GOLDEN
from tests.perceiver_reference import unsplit

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16_SAFE, PRESPLIT_W_MAX = 16384.0, 1000.0
INF, NAN = float("inf"), float("nan")
M, K = 257, 96


def _around(limit):
    """(the float below, the limit, the float above) in fp32."""
    t = torch.tensor(limit, dtype=torch.float32)
    return [float(torch.nextafter(t, torch.tensor(0.0))), float(t), float(torch.nextafter(t, torch.tensor(INF)))]


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _weights(N, K_, seed=2):
    return (_randn(N, K_, seed=seed) * K_ ** -0.5).to(DEV)


def _activations(amax, K_=K, seed=1):
    """(M, K_) of magnitude amax / 8 with max |a| == amax exactly, attained once, with a minus sign."""
    a = (_randn(M, K_, seed=seed) * (amax / 8)).clamp(-amax / 2, amax / 2)
    a[5, 7] = -amax
    return a.to(DEV)


def _same(x, y):
    nan = torch.isnan(y)
    return torch.equal(torch.isnan(x), nan) and torch.equal(x[~nan], y[~nan])


def _linear(mode, a, w, b, N, guard=None, presplit=0):
    out = torch.full((M, N), NAN, device=DEV)
    with L.f32_gemm(mode, guard=guard):
        L.linear(a, w, b, out, presplit=presplit)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# (a) the comparison itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [16384.0, 1000.0])
@pytest.mark.parametrize("K_", [96, 64], ids=["pingpong", "inphase"])
def test_guarded_linear_switches_exactly_at_the_limit(limit, K_):
    N = 256
    w, b = _weights(N, K_), _randn(N, seed=3).to(DEV)
    for amax in _around(limit):
        a = _activations(amax, K_)
        word = L.absmax(a)
        assert word.item() == amax
        two, three = _linear(2, a, w, b, N), _linear(1, a, w, b, N)
        assert torch.isfinite(two).all() and torch.isfinite(three).all()
        assert not torch.equal(two, three)                      # (else the test says nothing)
        want = two if amax < limit else three
        out = torch.full((M, N), NAN, device=DEV)
        with L.bounded_activations(guard=(word, limit)):       # one call: the kernel and its twin
            L.linear(a, w, b, out)
        assert torch.equal(out, want), (amax, limit)
        if K_ >= 96:   # the explicit pair: pre-split weights iff the guard holds, the three-term launch iff not
            out = torch.full((M, N), NAN, device=DEV)
            with L.f32_gemm(2, guard=(word, limit)):
                L.linear(a, L.split_f16(w, scale=64.0), b, out, presplit=L.F32_W_SPLIT)
            assert torch.equal(out, two) if amax < limit else bool(torch.isnan(out).all())   # (the other half has not run yet)
            with L.f32_gemm(1, guard=(word, limit)):
                L.linear(a, w, b, out)
            assert torch.equal(out, want), (amax, limit)


@pytest.mark.parametrize("limit", [16384.0, 1000.0])
def test_narrow_two_term_tiles_run_iff_the_guard_holds(limit):
    """N = 128: the 256 x 128 tiles exist in the pre-split two-term form only; guarded, they write iff word < limit."""
    N = 128
    w, b = _weights(N, K), _randn(N, seed=3).to(DEV)
    ws = L.split_f16(w, scale=64.0)
    for amax in _around(limit):
        a = _activations(amax)
        word = L.absmax(a)
        for flags, a_in in ((L.F32_W_SPLIT, a), (L.F32_W_SPLIT | L.F32_A_SPLIT, L.split_f16(a))):
            free = _linear(2, a_in, ws, b, N, presplit=flags)
            out = _linear(2, a_in, ws, b, N, guard=(word, limit), presplit=flags)
            assert torch.isfinite(free).all()
            assert torch.equal(out, free) if amax < limit else bool(torch.isnan(out).all()), (amax, flags)


@pytest.mark.parametrize("limit", [16384.0, 1000.0])
def test_guarded_chain_switches_format_and_kernels_exactly_at_the_limit(limit):
    """Producer (pair output) and consumer (pair input) with their three-term twins on one word: the buffer between them is
    fp16 pairs strictly below the limit and fp32 from the limit on, and the result is that of the unguarded kernels."""
    D, N = 256, 256
    w1, w2, b1 = _weights(D, K, seed=32), _weights(N, D, seed=33), _randn(D, seed=34).to(DEV)
    w1s, w2s = L.split_f16(w1, scale=64.0), L.split_f16(w2, scale=64.0)
    for amax in _around(limit):
        a = _activations(amax)
        word = L.absmax(a)
        ref = {}
        for mode in (2, 1):
            mid_ref = _linear(mode, a, w1, b1, D)
            with L.f32_gemm(mode):
                ref[mode] = (mid_ref, L.linear(mid_ref, w2, None, torch.empty((M, N), device=DEV)))
        assert not torch.equal(ref[1][1], ref[2][1]) and torch.isfinite(ref[1][1]).all() and torch.isfinite(ref[2][1]).all()
        mid, out = torch.full((M, D), NAN, device=DEV), torch.full((M, N), NAN, device=DEV)
        with L.f32_gemm(2, guard=(word, limit)):
            L.linear(a, w1s, b1, mid, presplit=L.F32_W_SPLIT | L.F32_C_SPLIT)
            L.linear(mid, w2s, None, out, presplit=L.F32_W_SPLIT | L.F32_A_SPLIT)
        with L.f32_gemm(1, guard=(word, limit)):
            L.linear(a, w1, b1, mid)
            L.linear(mid, w2, None, out)
        holds = amax < limit
        assert torch.equal(mid, L.split_f16(ref[2][0]) if holds else ref[1][0]), (amax, limit)
        assert torch.equal(out, ref[2][1] if holds else ref[1][1]), (amax, limit)


@pytest.mark.parametrize("limit", [2.0, 1000.0])
def test_perceiver_attention_pair_output_switches_exactly_at_the_limit(limit):
    B, cols, Lq, Lk, heads, hd = 1, 37, 13, 3, 4, 64
    inner = heads * hd
    q, kv = _randn(Lq, inner, seed=1).to(DEV), _randn(Lk * cols, 2 * inner, seed=2).to(DEV)
    ref = L.perceiver_attention(q, 0, kv, torch.empty(cols * Lq, inner, device=DEV), B, cols, cols * Lk, cols, Lq, Lk, heads, hd)
    pairs = L.split_f16(ref)
    assert not torch.equal(pairs, ref)
    for value in _around(limit):
        word = torch.tensor([value], device=DEV)
        out = L.perceiver_attention(q, 0, kv, torch.full((cols * Lq, inner), NAN, device=DEV), B, cols, cols * Lk, cols, Lq, Lk,
                                    heads, hd, pair_guard=(word, limit))
        assert torch.equal(out, pairs if value < limit else ref), (value, limit)


@pytest.mark.parametrize("limit", [2.0, 1000.0])
def test_perceiver_out_pair_form_switches_exactly_at_the_limit(limit):
    """Exactly one of {probs + out, attention (+ its three-term to_out)} runs, and which flips between the float below the
    limit and the limit."""
    B, cols, Lq, Lk, heads, hd, N = 1, 37, 13, 3, 4, 64, 256
    inner = heads * hd
    q, kv = _randn(Lq, inner, seed=1).to(DEV), _randn(Lk * cols, 2 * inner, seed=2).to(DEV)
    w_pairs = L.split_f16(_weights(N, inner, seed=3), scale=64.0)
    free_P, free_Vp = L.perceiver_probs(q, kv, B, cols, Lk * cols, cols, Lq, Lk, heads, hd)
    free_out = L.perceiver_out(free_Vp, w_pairs, free_P, torch.full((cols * Lq, N), -7.0, device=DEV), cols, Lq, Lk, heads, hd)
    free_att = L.perceiver_attention(q, 0, kv, torch.full((cols * Lq, inner), -7.0, device=DEV), B, cols, cols * Lk, cols, Lq, Lk,
                                     heads, hd)
    for value in _around(limit):
        word = torch.tensor([value], device=DEV)
        P, Vp = L.perceiver_probs(q, kv, B, cols, Lk * cols, cols, Lq, Lk, heads, hd, guard=(word, limit))
        out = L.perceiver_out(Vp, w_pairs, P, torch.full((cols * Lq, N), -7.0, device=DEV), cols, Lq, Lk, heads, hd, guard=(word, limit))
        att = L.perceiver_attention(q, 0, kv, torch.full((cols * Lq, inner), -7.0, device=DEV), B, cols, cols * Lk, cols, Lq, Lk,
                                    heads, hd, skip_guard=(word, limit))
        if value < limit:
            assert torch.equal(P, free_P) and torch.equal(Vp, free_Vp) and torch.equal(out, free_out)
            assert bool((att == -7.0).all())
        else:
            assert bool((P == 0).all()) and bool((out == -7.0).all()) and torch.equal(att, free_att)


# ---------------------------------------------------------------------------------------------------------------------
# (b) soundness at the limit: activations that attain the L1 bound
# ---------------------------------------------------------------------------------------------------------------------
def _adversarial(w, s):
    """Row 0 = s sign(w[j*]) for the row j* of the largest L1 norm (its output attains s ||w[j*]||_1), the rest randn s / 4
    kept inside [-s, s].  Returns (a, j*)."""
    j = int(w.double().abs().sum(1).argmax())
    a = (_randn(M, w.shape[1], seed=7) * (s / 4)).clamp(-s, s)
    a[0] = s * torch.sign(w[j].cpu())
    a[0][a[0] == 0] = s
    return a.to(DEV), j


def _grade(out, a, w, b=None):
    """max |out - fp64 product| / (|a| @ |w|.T), the scale of tests/test_gpu_ops.py's fp32-grade bound."""
    a64, w64 = a.double().cpu(), w.double().cpu()
    ref = a64 @ w64.T + (0 if b is None else b.double().cpu())
    return float(((out.double().cpu() - ref).abs() / (a64.abs() @ w64.abs().T)).max())


@pytest.mark.parametrize("N", [256, 128])
@pytest.mark.parametrize("w_scale", ["unit", "presplit_max"])
def test_two_term_forms_are_fp32_grade_with_the_l1_bound_attained(N, w_scale):
    """Activations at the float below F16_SAFE, signs aligned with the heaviest weight row; weights of scale K^-0.5, and once
    scaled until max |w| is just under PRESPLIT_W_MAX (times 2^6 in the kernel: just under fp16's 65504)."""
    w = _weights(N, K)
    if w_scale == "presplit_max":
        w = w * (torch.nextafter(torch.tensor(PRESPLIT_W_MAX), torch.tensor(0.0)).item() / w.abs().max().item())
        assert w.abs().max().item() < PRESPLIT_W_MAX
    s = _around(F16_SAFE)[0]
    a, j = _adversarial(w, s)
    native = torch.empty((M, N), device=DEV)
    with L.f32_gemm(0):
        L.linear(a, w, None, native)
    err_native = _grade(native, a, w)
    attained = float(a[0].double() @ w[j].double())
    assert abs(attained - s * float(w[j].double().abs().sum())) <= 1e-9 * abs(attained)
    ws, a_s = L.split_f16(w, scale=64.0), L.split_f16(a)
    forms = {"pre-split W": _linear(2, a, ws, None, N, presplit=L.F32_W_SPLIT),
             "pre-split A and W": _linear(2, a_s, ws, None, N, presplit=L.F32_W_SPLIT | L.F32_A_SPLIT)}
    if N == 256:
        forms["in-kernel split"] = _linear(2, a, w, None, N)
    for name, out in forms.items():
        err = _grade(out, a, w)
        print(f"N={N} {w_scale} {name}: err {err:.3e} (native {err_native:.3e}), attained {attained:.6g}")
        assert torch.isfinite(out).all(), name
        assert err <= 2e-6 and err <= 2 * err_native + 1e-7, (name, err, err_native)


@pytest.mark.parametrize("N", [256, 128])
@pytest.mark.parametrize("w_scale", ["unit", "presplit_max"])
def test_pair_output_at_the_limit_the_step_derives(N, w_scale):
    """The C_SPLIT form with the limit chosen as csrc/step.hip does for a chain: limit = (F16_SAFE - max|bias|) / max row L1,
    in float.  With the word at the float below it and the bound attained, the largest output is just under F16_SAFE, every
    pair is finite and hi + lo is the fp32 result to 2^-23 relative (+ 2^-25 absolute: half the fp16 subnormal spacing, for
    results whose remainder is subnormal)."""
    w = _weights(N, K)
    if w_scale == "presplit_max":
        w = w * (torch.nextafter(torch.tensor(PRESPLIT_W_MAX), torch.tensor(0.0)).item() / w.abs().max().item())
    b = _randn(N, seed=3).clamp(-1, 1).to(DEV)
    l1 = torch.tensor(0.0)
    for r in w.cpu():                                   # plain float accumulation in row order, as max_row_l1 does
        acc = torch.tensor(0.0)
        for v in r.abs():
            acc = acc + v
        l1 = torch.maximum(l1, acc)
    limit = ((torch.tensor(F16_SAFE) - b.abs().max().cpu()) / l1).item()
    s = _around(limit)[0]
    a, j = _adversarial(w, s)
    b[j] = b.abs().max() * torch.sign(a[0].double() @ w[j].double()).float()        # the bias term attained as well
    ws, a_s = L.split_f16(w, scale=64.0), L.split_f16(a)
    word = L.absmax(a)
    assert word.item() == s
    base = _linear(2, a_s, ws, b, N, presplit=L.F32_W_SPLIT | L.F32_A_SPLIT)
    out = torch.full((M, N), NAN, device=DEV)
    with L.f32_gemm(2, guard=(word, limit)):
        L.linear(a_s, ws, b, out, presplit=L.F32_W_SPLIT | L.F32_A_SPLIT | L.F32_C_SPLIT)
    hi, lo = unsplit(out.cpu())
    top = base.abs().max().item()
    err = _grade(base, a, w, b)
    print(f"N={N} {w_scale}: limit {limit:.6g}, largest |output| {top:.6f}, err {err:.3e}")
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    assert 0.999 * F16_SAFE < top < F16_SAFE * (1 + K * 2.0 ** -24 + 2e-6)   # attained, to the float L1 sum's and the GEMM's rounding
    assert err <= 2e-6
    bc = base.cpu()
    assert bool(((hi + lo - bc).abs() <= 2.0 ** -23 * bc.abs() + 2.0 ** -25).all())
    assert torch.equal(out, L.split_f16(base))


def test_pair_output_past_the_fp16_range_is_not_finite_without_a_guard():
    """Why the guard exists.  Unguarded C_SPLIT with the bound attained just under 65504: still finite; just past 65520 (where
    fp16 rounds to inf) the pair is hi = +inf, lo = -inf -- it does not saturate."""
    N = 256
    w = _weights(N, K)
    l1 = float(w.double().abs().sum(1).max())
    ws = L.split_f16(w, scale=64.0)
    for s, finite in ((_around(65504.0 / l1)[0], True), (65600.0 / l1, False)):
        a, j = _adversarial(w, s)
        out = _linear(2, L.split_f16(a), ws, None, N, presplit=L.F32_W_SPLIT | L.F32_A_SPLIT | L.F32_C_SPLIT)
        hi, lo = unsplit(out.cpu())
        assert bool(torch.isfinite(hi).all() and torch.isfinite(lo).all()) == finite
        if not finite:
            assert abs(hi[0, j].item()) == INF and lo[0, j].item() == -hi[0, j].item()


# ---------------------------------------------------------------------------------------------------------------------
# (c) small activations: the subnormal remainders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K_", [96, 512])
def test_small_activations_stay_inside_the_stated_absolute_error(K_):
    """csrc/gemm_f32.hip: below 0.25 the fp16 remainder of an activation is subnormal and carries an ABSOLUTE error of up to
    3e-8.  So |out - ref| <= 3e-8 sum_k |w[n, k]| (that claim) + 2e-6 (|a| @ |w|.T) (the fp32-grade bound)."""
    N = 256
    g = torch.Generator().manual_seed(K_)
    lo_, hi_ = math.log10(1e-6), math.log10(0.25)
    mag = 10.0 ** (torch.rand(M, K_, generator=g, dtype=torch.float64) * (hi_ - lo_) + lo_)
    sign = torch.where(torch.rand(M, K_, generator=g) < 0.5, -1.0, 1.0)
    a = (mag * sign).float()
    assert 1e-6 * 0.999 <= a.abs().min().item() and a.abs().max().item() <= 0.25
    w = _weights(N, K_)
    out = _linear(2, a.to(DEV), w, None, N).double().cpu()
    a64, w64 = a.double(), w.double().cpu()
    err = (out - a64 @ w64.T).abs()
    bound = 3e-8 * w64.abs().sum(1)[None, :] + 2e-6 * (a64.abs() @ w64.abs().T)
    print(f"K={K_}: worst |err| / bound {float((err / bound).max()):.3f}; worst |err| / (|a| @ |w|.T) {float((err / (a64.abs() @ w64.abs().T)).max()):.3e}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------------------------------
# (d) what the word can hold
# ---------------------------------------------------------------------------------------------------------------------
def test_nan_inf_and_signed_zero_words():
    N = 256
    w, b = _weights(N, K), _randn(N, seed=3).to(DEV)
    a = _activations(3.0)
    two, three = _linear(2, a, w, b, N), _linear(1, a, w, b, N)
    # NaN inputs: `absmax` ignores them, the word stays finite, the two-term kernel runs and the NaN reaches exactly its rows
    a_nan = a.clone()
    a_nan[3, 11] = NAN
    a_nan[200, :] = NAN
    word = L.absmax(a_nan)
    assert word.item() == 3.0
    out = torch.full((M, N), 0.0, device=DEV)
    with L.bounded_activations(guard=(word, F16_SAFE)):
        L.linear(a_nan, w, b, out)
    rows = torch.zeros(M, dtype=torch.bool, device=DEV)
    rows[[3, 200]] = True
    assert bool(torch.isnan(out[rows]).all()) and torch.equal(out[~rows], two[~rows])
    # +inf: the word is inf, the three-term kernel runs
    a_inf = a.clone()
    a_inf[9, 2] = INF
    word = L.absmax(a_inf)
    assert word.item() == INF
    out = torch.full((M, N), 0.0, device=DEV)
    with L.bounded_activations(guard=(word, F16_SAFE)):
        L.linear(a_inf, w, b, out)
    assert _same(out, _linear(1, a_inf, w, b, N)) and not bool(torch.isfinite(out[9]).any())
    assert torch.equal(out[torch.arange(M, device=DEV) != 9], three[torch.arange(M, device=DEV) != 9])
    # a word of +0 or -0 is below every positive limit: the guard holds
    for zero in (0.0, -0.0):
        out = torch.full((M, N), NAN, device=DEV)
        with L.bounded_activations(guard=(torch.tensor([zero], device=DEV), 1000.0)):
            L.linear(a, w, b, out)
        assert torch.equal(out, two)


# ---------------------------------------------------------------------------------------------------------------------
# step level: the limits a step derives, and its own words at them
# ---------------------------------------------------------------------------------------------------------------------
_SMALL = dict(embed_dim=256, num_heads=8, encoder_depths=(2, 2, 2), encoder_num_heads=(4, 8, 16), decoder_depths=(2, 2, 2),
              decoder_num_heads=(16, 8, 4))
# The golden cases are 64 wide: no linear of their encoder front exists in the fp16-pair form (K = 64 < 96, 64 rows), so words
# 1 and 2 are not even measured there and only words 0 and 3 carry guards.  `chain256` is the narrowest model whose front runs
# as the guarded chains (tests/test_gpu_encoder_front.py), on the smallest grid its three stages accept.
STEP_CASES = {**{k: GOLDEN[k] for k in ("small_b2", "base_pad", "patch10", "air_pollution")},
              "chain256": dict(cls="Aurora", kwargs=dict(**_SMALL), H=16, W=32, B=1, T=2, levels=(100, 250, 500, 850))}
FIXTURE = Path(__file__).parent / "golden" / "guard_limits.json"
MEAN_REL, MAX_REL = 1e-4, 1e-3   # tests/test_gpu_production.py:_compare, fp32 engine vs oracle


def _step_case(name):
    case = STEP_CASES[name]
    with torch.device("meta"):
        meta = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    sd = helpers.case_state_dict(meta, torch.float32)
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, meta.config)
    return case, meta, sd, (surf, static, atmos, lat, lon, times)


def _scaled(case, meta, inputs, atmos_scale, surf_scale):
    """The batch with its NORMALISED atmospheric / surface anomalies multiplied: x -> loc + scale (x - loc)."""
    surf, static, atmos, lat, lon, times = inputs
    levels = tuple(case["levels"])

    def grow(d, affine, k_):
        out = {}
        for k, v in d.items():
            loc, _ = affine(k)
            loc_t = torch.as_tensor(loc, dtype=torch.float64)
            loc_t = loc_t.reshape(-1, 1, 1) if loc_t.numel() > 1 else loc_t
            out[k] = ((v.double() - loc_t) * k_ + loc_t).float()
        return out

    atmos = grow(atmos, lambda k: normalisation.atmos_affine(k, levels), atmos_scale)
    surf = grow(surf, normalisation.surf_affine, surf_scale)
    static = {k: v.float() for k, v in static.items()}
    return Batch(surf, static, atmos, Metadata(lat.float(), lon.float(), times, levels))


def _engine(case, sd, monkeypatch, compose=True):
    monkeypatch.setenv("AURORA_COMPOSE_FRONT", "1" if compose else "0")
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    model.load_state_dict(sd, strict=True)
    return model.to("cuda").eval()


def _step(model, batch):
    with torch.inference_mode():
        pred = model.forward(batch.to("cuda"))
    torch.cuda.synchronize()
    native = model.engine().native
    out = {**{f"surf.{k}": v.cpu() for k, v in pred.surf_vars.items()}, **{f"atmos.{k}": v.cpu() for k, v in pred.atmos_vars.items()}}
    return out, native.guard_words(), native.guard_limits()


def _oracle(sd, meta, case, batch):
    with torch.inference_mode():
        o_s, o_a, _ = oracle.forward({k: v.double() for k, v in sd.items()}, meta.config, batch.surf_vars, batch.static_vars,
                                     batch.atmos_vars, batch.metadata.lat, batch.metadata.lon, batch.metadata.time, case["levels"], 0,
                                     normalisation.locations, normalisation.scales, variant=meta.variant)
    return {**{f"surf.{k}": v for k, v in o_s.items()}, **{f"atmos.{k}": v for k, v in o_a.items()}}


def _errors(out, ref):
    assert set(out) == set(ref)
    return (max(helpers.mean_rel_err(out[k], ref[k]) for k in ref), max(helpers.rel_err(out[k], ref[k]) for k in ref))


@pytest.mark.parametrize("name,compose", [("small_b2", True), ("base_pad", True), ("patch10", True), ("air_pollution", True),
                                          ("chain256", True), ("chain256", False)])
def test_reported_limits_are_positive_and_above_the_words_of_ordinary_inputs(name, compose, monkeypatch):
    """`aurora_hip_guard_limits` after a step on the case's own inputs: every word that a launch carried has a positive, finite
    limit no larger than F16_SAFE and sits below it; a word nothing carried reports +inf.  The numbers are the recorded results
    tests/test_guard_limits_host.py checks against fp64 (tests/golden/guard_limits.json; AURORA_WRITE_GUARD_LIMITS=1 rewrites
    this case's entry)."""
    case, meta, sd, inputs = _step_case(name)
    model = _engine(case, sd, monkeypatch, compose)
    _, words, (limits, launches) = _step(model, _scaled(case, meta, inputs, 1.0, 1.0))
    print(f"{name} compose={compose}: words {words} limits {limits} launches {launches}")
    for i in range(4):
        if launches[i] == 0:
            assert limits[i] == INF, (i, limits)
        else:
            assert 0.0 < limits[i] <= F16_SAFE and 0.0 < words[i] < limits[i], (i, words, limits)
    assert launches[3] > 0 and (launches[0] > 0) != (launches[1] > 0)      # the encoder context: its own word, or the chain's
    assert (launches[1] > 0 and launches[2] > 0) == (name == "chain256")
    key = f"{name}/{'composed' if compose else 'staged'}"
    entry = {"limits": [None if v == INF else v for v in limits], "launches": list(launches),
             "front_composed": model.engine().native.front_composed()}
    recorded = json.loads(FIXTURE.read_text()) if FIXTURE.exists() else {}
    if os.environ.get("AURORA_WRITE_GUARD_LIMITS") == "1":
        recorded[key] = entry
        FIXTURE.write_text(json.dumps(recorded, indent=1, sort_keys=True) + "\n")
    rec = recorded.get(key)
    assert rec is not None and rec["launches"] == entry["launches"] and rec["front_composed"] == entry["front_composed"], (key, entry, rec)
    for got, want in zip(entry["limits"], rec["limits"]):   # (a float ulp of the device-computed bias maximum is not a change)
        assert (got is None) == (want is None) and (got is None or abs(got - want) <= 1e-6 * want), (key, entry, rec)


def _sweep(name, compose, word_index, monkeypatch):
    """Scales the inputs until word `word_index` of a step sits just below, at and at twice its limit.  At each point: the
    word is the one computed here from the inputs; the step reports the same limit (it is a property of the weights); every
    output is finite and meets the fp64 oracle on the same inputs."""
    case, meta, sd, inputs = _step_case(name)
    model = _engine(case, sd, monkeypatch, compose)
    levels = tuple(case["levels"])

    def norm_max(batch):
        def of(d, affine):
            m = 0.0
            for k, v in d.items():
                loc, scale = affine(k)
                loc_t, scale_t = torch.tensor(loc, dtype=torch.float32), torch.tensor(scale, dtype=torch.float32)
                shape = (-1, 1, 1) if loc_t.numel() > 1 else ()
                m = max(m, float(((v.float() - loc_t.reshape(shape)) / scale_t.reshape(shape)).abs().max()))
            return m
        b = batch.crop(model.patch_size)
        return (of(b.atmos_vars, lambda k: normalisation.atmos_affine(k, levels)),
                max(of(b.surf_vars, normalisation.surf_affine), of(b.static_vars, normalisation.surf_affine)))

    def at(k_):
        return _scaled(case, meta, inputs, k_ if word_index == 1 else 1.0, k_ if word_index == 2 else 1.0)

    _, w0, (lim0, launches) = _step(model, at(1.0))
    assert launches[word_index] > 0 and model.engine().native.front_composed() == compose
    limit = lim0[word_index]
    # the word is |scale| x a fixed maximum up to rounding: aim, measure, correct once
    results = {}
    for label, target in (("below", limit * (1 - 2.0 ** -12)), ("at", limit * (1 + 2.0 ** -12)), ("twice", 2 * limit)):
        k_ = target / w0[word_index]
        for _ in range(3):
            batch = at(k_)
            got = norm_max(batch)[word_index - 1]
            if abs(got / target - 1) < 2.0 ** -14:
                break
            k_ *= target / got
        out, words, (limits, _) = _step(model, batch)
        want = norm_max(batch)[word_index - 1]
        assert abs(words[word_index] - want) <= 2e-6 * want, (label, words, want)
        assert limits[word_index] == limit
        e = _errors(out, _oracle(sd, meta, case, batch))
        results[label] = (words[word_index], e)
        print(f"{name} compose={compose} word {word_index} {label}: word {words[word_index]:.9g} limit {limit:.9g} "
              f"mean-rel {e[0]:.3e} max-rel {e[1]:.3e}")
        assert all(torch.isfinite(v).all() for v in out.values()), label
        assert e[0] <= MEAN_REL and e[1] <= MAX_REL, (label, e)
    # the path flips exactly where the word crosses the limit: two fp16 terms iff word < limit (aurora_hip_guard_words)
    assert 0.99 * limit < results["below"][0] < limit
    assert limit <= results["at"][0] < 1.01 * limit
    assert results["twice"][0] >= limit
    return results


@pytest.mark.parametrize("compose", [True, False], ids=["composed", "staged"])
@pytest.mark.parametrize("word_index", [1, 2], ids=["atmos", "surf"])
def test_step_words_at_their_limits_meet_the_oracle(word_index, compose, monkeypatch):
    _sweep("chain256", compose, word_index, monkeypatch)
