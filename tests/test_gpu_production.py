"""Parity at the PRODUCTION widths: the default constructors (embed_dim 512, heads 8/16/32, 48 blocks, D = 512 /
1024 / 2048) against the CPU oracle on grids small enough for the oracle, and every production GEMM shape of the
0.25-degree step against an fp64 product.

Why this file exists: the golden cases (tests/golden_cases.py) run tiny widths (embed_dim 64), so the kernels the
headline configuration dispatches -- the 256 x 256 ring GEMM with 6 / 12 / 24 / 32 n-tiles (incl. the narrower last tile
group of N = 3072 and 6144), the fp16-split fp32 GEMM on the decoder's 842,400-row MLP, window attention with 8 / 16 /
32 heads on zero-padded windows -- were only ever compared with each other.  Here they meet the oracle.

Tolerances (metric of the reference's own test, tests/test_model.py:45-61 upstream: mean|out-ref| / mean|ref| per
variable): fp32 engine vs fp32 oracle <= 1e-4; bf16 engine within 2x of what the oracle's own `autocast=True` run
(the reference's CPU autocast semantics) deviates from the fp32 oracle.

Beside them, per surface variable and per (variable, level) in units of normalisation.scales (tests/normalised_error.py): the
fp32 engine against the oracle in fp64 on the same fp32 weights, within 4x of what the fp32 oracle deviates from it by (or of one
fp32 ulp of the entry).  The fp64 run is made once per (model, grid) and shared.  The quarter grid (361 x 720) has no fp64 run --
it would take about four times the 21 s of the 181 x 360 one on 8 cores: its per-entry baseline is the one of the same model on
181 x 360, the reference stays the fp32 oracle, and the bound is 5x that baseline (4x for the engine + 1x for the reference).
"""
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, normalisation
from oracle import aurora_oracle as oracle
from tests import helpers
from tests import normalised_error as ne

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _seeded_model(cls, seed=0, **kw):
    """Random weights at their production shapes (no checkpoints offline); zero-initialised tensors (AdaLN modulation,
    LoRA B) are re-randomised so that those paths are not no-ops -- as tests/test_rollout.py:23-35 upstream does."""
    torch.manual_seed(seed)
    with torch.device(DEV):
        model = cls(**kw)
        with torch.no_grad():
            for p in model.parameters():
                if not p.any():
                    p.normal_(std=0.02)
    return model.eval()


def _inputs(cfg, H, W, levels, seed=1, positive=()):
    """`randn` in normalised space mapped to physical units, positive variables >= 0."""
    from bench import synthetic_batch

    b = synthetic_batch(cfg, H, W, seed, "cpu", levels=levels)
    fix = lambda d: {k: (v.abs() if k in positive else v) for k, v in d.items()}  # noqa: E731
    return Batch(fix(b.surf_vars), b.static_vars, fix(b.atmos_vars), b.metadata)


def _oracle(model, sd, batch, autocast):
    md = batch.metadata
    with torch.inference_mode():
        o_s, o_a, _ = oracle.forward(sd, model.config, batch.surf_vars, batch.static_vars, batch.atmos_vars, md.lat,
                                     md.lon, md.time, md.atmos_levels, 0, normalisation.locations,
                                     normalisation.scales, autocast=autocast, variant=model.variant)
    return {**{f"surf.{k}": v for k, v in o_s.items()}, **{f"atmos.{k}": v for k, v in o_a.items()}}


_FP64 = {}   # (class, H, W, levels) -> (the oracle in fp64, what the fp32 oracle deviates from it by per entry); read-only


def _fp64_baseline(model, sd, batch, ref32, key):
    """`key` names a seeded model and seeded inputs: both are reproducible, so one fp64 run serves every test of that geometry."""
    if key not in _FP64:
        ref64 = _oracle(model, {k: v.double() for k, v in sd.items()}, batch, autocast=False)
        _FP64[key] = (ref64, ne.per_level_errors(ref32, ref64, batch.metadata.atmos_levels))
    return _FP64[key]


def _engine(model, batch):
    with torch.inference_mode():
        pred = model.forward(batch.to(DEV))
    torch.cuda.synchronize()
    return {**{f"surf.{k}": v.cpu() for k, v in pred.surf_vars.items()},
            **{f"atmos.{k}": v.cpu() for k, v in pred.atmos_vars.items()}}


def _compare(model_cls, kw, H, W, levels, positive=()):
    """fp32 engine vs fp32 oracle, bf16 engine vs the oracle's autocast deviation: returns the worst errors."""
    model = _seeded_model(model_cls, autocast=False, **kw)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    batch = _inputs(model.config, H, W, levels, positive=positive)
    ref32 = _oracle(model, sd, batch, autocast=False)
    ref16 = _oracle(model, sd, batch, autocast=True)
    out32 = _engine(model, batch)
    model.autocast = True            # same weights, bf16 backbone
    model._engine = None
    out16 = _engine(model, batch)
    assert set(out32) == set(ref32)
    e32 = {k: helpers.mean_rel_err(out32[k], ref32[k]) for k in ref32}
    m32 = {k: helpers.rel_err(out32[k], ref32[k]) for k in ref32}
    e16 = {k: helpers.mean_rel_err(out16[k], ref32[k]) for k in ref32}
    b16 = {k: helpers.mean_rel_err(ref16[k], ref32[k]) for k in ref32}
    print(f"{model_cls.__name__} {H}x{W}: fp32 worst mean-rel {max(e32.values()):.3e} max-rel {max(m32.values()):.3e}; "
          f"bf16 worst {max(e16.values()):.3e} (oracle autocast {max(b16.values()):.3e})")
    for k in ref32:
        assert torch.isfinite(out32[k]).all() and torch.isfinite(out16[k]).all(), k
        assert e32[k] <= 1e-4 and m32[k] <= 1e-3, (k, e32[k], m32[k])
        assert e16[k] <= 2 * b16[k] + 5e-4, (k, e16[k], b16[k])
    if not kw:       # (the default constructor with seed 0: what the key stands for)
        ref64, baseline = _fp64_baseline(model, sd, batch, ref32, (model_cls.__name__, H, W, levels))
        ne.check(f"{model_cls.__name__} {H}x{W} fp32 vs fp64 oracle", out32, ref64, levels, baseline)
    del model
    torch.cuda.empty_cache()


LEVELS13 = (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)


def test_pretrained_default_geometry_matches_oracle():
    """AuroraPretrained() exactly as bench.py builds it (1.3 B parameters, depths (6,10,8)/(8,10,6)) on a 181 x 360
    grid: token grid (4, 45, 90) -- the 45 -> 48 two-sided window padding of the 0.25-degree stage 2, here at every
    stage ((45,90) -> (23,45) -> (12,23), all padded, odd merges) -- with D = 512 / 1024 / 2048 and the ring GEMM on
    6 / 12 / 24 / 32 n-tiles."""
    _compare(aurora_amd.AuroraPretrained, {}, 181, 360, LEVELS13)


def test_pretrained_default_geometry_with_fused_adaln_matches_oracle(monkeypatch):
    """The same with the stage-0 proj / fc2 linears fused with their AdaLN + residual (`linear_ln512_kernel`), which the
    engine only picks by itself when the 128-row tiles fill the chip (the 0.25-degree grid; bench.py runs that)."""
    monkeypatch.setenv("AURORA_FUSE_LN", "2")
    _compare(aurora_amd.AuroraPretrained, {}, 181, 360, LEVELS13)


def test_attention_layouts_give_the_same_prediction_bit_for_bit(monkeypatch):
    """q | k | v in head planes in front of the window attention (csrc/step.hip: m.qkv_planes) is a LAYOUT: the qkv linear and
    the attention do the same arithmetic on the same values wherever they lie.  Both settings of the switch must reproduce the
    same prediction exactly -- at the production widths, with the stage-0 proj / fc2 linears fused with their AdaLN and without.
    (Round 5 ran the same test over a third switch -- the attention's RESULT in head planes, read by the proj linear -- before
    that layout was measured and dropped: profiles/r05_ab_attention_out_planes.log.)"""
    outs = {}
    for qp, fuse in (("1", "2"), ("0", "2"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("AURORA_QKV_PLANES", qp)
        monkeypatch.setenv("AURORA_FUSE_LN", fuse)
        model = _seeded_model(aurora_amd.AuroraPretrained, autocast=True)
        batch = _inputs(model.config, 181, 360, LEVELS13)
        outs[(qp, fuse)] = _engine(model, batch)
        del model
        torch.cuda.empty_cache()
    for fuse in ("2", "0"):
        assert all(torch.equal(outs[("0", fuse)][k], v) for k, v in outs[("1", fuse)].items()), fuse


def test_decoder_reassociation_equals_attention_then_to_out_at_model_level(monkeypatch):
    """The decoder's level de-aggregation re-associated (csrc/perceiver_out.hip: to_out of a column's three value rows, the
    13 x 48 combinations in registers) against the plain pair it replaces (perceiver attention, then the 13-row `to_out`) in
    the same fp32 model at the production widths: the same function, summed in another order -- fp32 round-off apart.  (Both
    are compared with the oracle by the tests above / below; this one isolates the re-association.)"""
    outs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("AURORA_PERCEIVER_REASSOC", on)
        model = _seeded_model(aurora_amd.AuroraPretrained, autocast=False)
        batch = _inputs(model.config, 181, 360, LEVELS13)
        outs[on] = _engine(model, batch)
        del model
        torch.cuda.empty_cache()
    worst = max(helpers.mean_rel_err(outs["1"][k], outs["0"][k]) for k in outs["0"])
    print(f"re-associated vs plain decoder de-aggregation: worst mean-rel {worst:.3e}")
    assert 0 < worst < 2e-6   # (not the same launches -- and not further apart than fp32 summation orders are)


def test_scores_from_packed_query_rows_equal_key_projection_at_model_level(monkeypatch):
    """First Perceiver layers (encoder level aggregation, decoder de-aggregation): `to_kv` with its key half replaced by the
    Lq x heads rows W_k^T q / sqrt(64) (csrc/model_weights.hip:score_weights) and attention from those scores, against keys + q . k in
    the same fp32 model at the production widths -- the same function re-associated; fp32 round-off apart."""
    outs = {}
    for on in ("1", "0"):
        monkeypatch.setenv("AURORA_SCORE_WEIGHTS", on)
        model = _seeded_model(aurora_amd.AuroraPretrained, autocast=False)
        batch = _inputs(model.config, 181, 360, LEVELS13)
        outs[on] = _engine(model, batch)
        del model
        torch.cuda.empty_cache()
    worst = max(helpers.mean_rel_err(outs["1"][k], outs["0"][k]) for k in outs["0"])
    print(f"scores from packed query rows vs key projection: worst mean-rel {worst:.3e}")
    assert 0 < worst < 2e-6


def test_pretrained_quarter_grid_matches_oracle():
    """AuroraPretrained() on 361 x 720 = a quarter of the 0.25-degree tokens (token grid (4, 90, 180); stages (45, 90) and
    (23, 45) padded): M = 64,800 / 16,200 / 4,140 rows per stage, so the M-dependent dispatch of the headline step is
    met by the oracle as well -- the fused linear + AdaLN kernel in 507 row tiles (two rounds of one tile per CU), the
    8-round tile order of the 256 x 256 GEMMs, the 128 x 256 fp32 tiles on 210,600 decoder rows.  (The full grid is
    compared with the oracle inside bench.py: `parity_full_grid`.)  fp32 oracle only: bf16 is bounded absolutely."""
    model = _seeded_model(aurora_amd.AuroraPretrained, autocast=False)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    batch = _inputs(model.config, 361, 720, LEVELS13)
    ref32 = _oracle(model, sd, batch, autocast=False)
    out32 = _engine(model, batch)
    model.autocast = True
    model._engine = None
    out16 = _engine(model, batch)
    e32 = {k: helpers.mean_rel_err(out32[k], ref32[k]) for k in ref32}
    e16 = {k: helpers.mean_rel_err(out16[k], ref32[k]) for k in ref32}
    print(f"AuroraPretrained 361x720: fp32 worst {max(e32.values()):.3e}, bf16 worst {max(e16.values()):.3e}")
    for k in ref32:
        assert e32[k] <= 1e-4, (k, e32[k])
        assert e16[k] <= 3e-3, (k, e16[k])   # measured 1.0e-3; the oracle's own CPU autocast deviates 2.3-2.6e-3
    # per entry: the baseline of the same model on 181 x 360 (no fp64 run at this size), against the fp32 oracle, hence 4 + 1
    small = _inputs(model.config, 181, 360, LEVELS13)
    key = ("AuroraPretrained", 181, 360, LEVELS13)
    _, baseline = _fp64_baseline(model, sd, small, None if key in _FP64 else _oracle(model, sd, small, autocast=False), key)
    ne.check("AuroraPretrained 361x720 fp32 vs fp32 oracle, baseline of 181x360", out32, ref32, LEVELS13, baseline, margin=ne.MARGIN + 1)
    del model
    torch.cuda.empty_cache()


def test_highres_default_geometry_matches_oracle():
    """AuroraHighRes(): patch size 10, depths (6,8,8)/(8,8,6), LoRA merged (single), on a 121 x 240 grid."""
    _compare(aurora_amd.AuroraHighRes, {}, 121, 240, LEVELS13)


def test_air_pollution_default_geometry_matches_oracle():
    """AuroraAirPollution(): patch size 3, 13 level-conditioned embeddings / heads, second decoder Perceiver,
    difference prediction, on a 46 x 72 grid (token grid (4, 15, 24))."""
    m = aurora_amd.AuroraAirPollution
    with torch.device("meta"):
        cfg = m().config
    _compare(m, {}, 46, 72, LEVELS13, positive=cfg.positive_surf_vars + cfg.positive_atmos_vars)


# ---- every GEMM shape of the 0.25-degree step vs an fp64 product --------------------------------------------------
BACKBONE_SHAPES = [  # (M, N, K): qkv, proj, fc1, fc2 per stage; merge / split linears
    (259200, 1536, 512), (259200, 512, 512), (259200, 2048, 512), (259200, 512, 2048),
    (64800, 3072, 1024), (64800, 1024, 1024), (64800, 4096, 1024), (64800, 1024, 4096),
    (16200, 6144, 2048), (16200, 2048, 2048), (16200, 8192, 2048), (16200, 2048, 8192),
    (64800, 1024, 2048), (16200, 2048, 4096), (16200, 4096, 2048), (64800, 2048, 1024),
]


def _sample_rows(M, n=768, seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = torch.cat([torch.randint(0, M, (n,), generator=g), torch.arange(M - 300, M), torch.arange(0, 260)])
    return rows.unique().to(DEV)


@pytest.mark.parametrize("M,N,K", BACKBONE_SHAPES)
def test_bf16_linear_production_shapes_vs_fp64(M, N, K):
    from aurora_amd.engine import lib

    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).bfloat16()
    b = torch.randn(N, device=DEV, generator=g)
    out = lib.linear(a, w, b, torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV), act=lib.ACT_GELU)
    assert torch.isfinite(out).all()           # every tile written
    rows = _sample_rows(M)
    ref = torch.nn.functional.gelu(a[rows].double() @ w.double().t() + b.double())
    err = (out[rows].double() - ref).abs()
    # one bf16 rounding of the result (2^-9 relative) on top of the fp32-accumulated product
    assert (err <= 2.0 ** -8 * ref.abs() + 2e-3).all(), err.max().item()


@pytest.mark.parametrize("M,N,K,bounded", [(842400, 2048, 1024, True), (842400, 1024, 2048, True),
                                           (842400, 1024, 1024, False), (194400, 2048, 1024, False),
                                           (907200, 1024, 512, False), (64800, 512, 2048, True)])
def test_fp32_linear_decoder_shapes_vs_fp64(M, N, K, bounded):
    """The fp32 linears of the Perceiver encoder / decoder at their 0.25-degree sizes: three-term bf16 split, and the
    two-term fp16 split where the engine uses it (`bounded`)."""
    from aurora_amd.engine import lib

    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) * K ** -0.5
    b = torch.randn(N, device=DEV, generator=g)
    out = torch.full((M, N), float("nan"), device=DEV)
    if bounded:
        with lib.bounded_activations():
            lib.linear(a, w, b, out)
    else:
        lib.linear(a, w, b, out)
    assert torch.isfinite(out).all()
    rows = _sample_rows(M, n=512)
    ref = a[rows].double() @ w.double().t() + b.double()
    scale = (a[rows].double().abs() @ w.double().abs().t())          # sum |a||w|: the natural error scale
    err = ((out[rows].double() - ref).abs() / scale).max().item()
    assert err < 4e-6, err
