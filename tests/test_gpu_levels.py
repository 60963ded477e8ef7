"""The decoder's level de-aggregation at 2, 3, 4 and 5 pressure levels THROUGH THE STEP'S OWN WORKSPACE (csrc/step.hip:resampler,
csrc/resampler_space.h), at the Perceiver widths of both published sizes, against the CPU oracle.

tests/test_gpu_production.py meets that workspace at 13 levels only, and the goldens run embed_dim 64, where the re-associated
path (csrc/perceiver_out.hip) is not eligible; the Lq = 3 and Lq = 4 instantiations of its kernels were tested on buffers a
test allocated itself.  At 3 and 4 levels k | v (3 rows of kv_ld floats per column) is WIDER than to_out's result (Lq rows of
dim floats), and the softmax weights P, which used to start right behind that result, lay on k | v rows that the launch
writing P was still reading (tests/test_resampler_space.py is the same statement without a device).

Grid sizes.  The damage needs the workgroup that reads a k | v row to start after the one that wrote P over it has
retired.  `perceiver_probs` runs one 256-thread workgroup per 16 (column, head) groups -- 2 columns per workgroup with 8 heads,
1 with 16 -- and at most 8 such workgroups are resident on each of 256 CUs, so victim and writer have to be more than about
2,048 workgroups apart.  With P at byte Lq * dim * 4 * n_cols of a k | v of kv_ld * 4 bytes per row, key j of column c at row
j * n_cols + c:
  README widths (dim 512, 8 heads), 4 levels, scores (kv_ld 768):  8192 n / 3072 = row 2.67 n: column 0's P lies on key 2 of
    column 0.67 n.  321 x 640 = 80 x 160 = 12,800 columns = 6,400 workgroups; the nearest victim is 0.33 n columns = 2,133
    workgroups behind its writer.  (B = 2 at 161 x 320: 6,400 columns, the same distance at column 0.)
  512 widths (dim 1024, 16 heads), 3 levels: scores (kv_ld 1280) 12288 n / 5120 = row 2.4 n, column 0.4 n; keys (kv_ld 2048)
    row 1.5 n, column 0.5 n.  241 x 480 = 60 x 120 = 7,200 columns = 7,200 workgroups: 2,880 / 3,600 apart.
  AuroraAirPollution (512 widths, patch size 3): 181 x 360 = 60 x 120 = 7,200 columns as well.

Where P starts at or behind the start of key 2 (README widths at 3 levels with scores: row 2 n + 0.67 c; 512 widths at 4 levels
with keys: row 2 n + 0.5 c) the victim's workgroup runs BEFORE its writer's, and the overlap stays a race between neighbours
that these grids do not lose.

On the layout before the fix (P at round256(unit)), one run of this file on an MI355X: 4 of 11 failed -- every case the
arithmetic above puts a victim behind its writer, with 5 to 10 % mean-rel error against the oracle where the bound is 1e-4 --
and the cases with the victim in front passed; the docstrings of the tests have the figures.

Bounds: those of tests/test_gpu_production.py -- fp32 engine against the fp32 oracle mean-rel <= 1e-4 and max-rel <= 1e-3 per
variable, and per surface variable and (variable, level) in units of normalisation.scales against the oracle in fp64 on the same
weights, within 4x of what the fp32 oracle deviates from it by (tests/normalised_error.py; one fp64 run per cached geometry, 6 to 7 s
on 8 cores at these sizes); a switched path against the plain one 0 < worst mean-rel < 2e-6 (the same function summed in another order; `0 <`
proves that the switch took another path); bf16 within twice the oracle's own autocast deviation + 5e-4.

Both models run with one Swin block per stage, so that the oracle takes seconds; the Perceiver widths are the constructors'.
The weights are seeded, so the oracle's result for a (model, grid, levels) is computed once and shared.
"""
from datetime import timedelta

import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata
from tests import helpers
from tests import normalised_error as ne
from tests.test_gpu_production import DEV, LEVELS13, _engine, _inputs, _oracle, _seeded_model

pytestmark = pytest.mark.gpu

DEPTHS = dict(encoder_depths=(1, 1, 1), decoder_depths=(1, 1, 1))
SIZES = {"readme": (aurora_amd.AuroraSmallPretrained, 321, 640), "512": (aurora_amd.AuroraPretrained, 241, 480)}
LEVELS = {2: (500, 850), 3: (250, 500, 850), 4: (100, 250, 500, 850), 5: (50, 250, 500, 850, 1000)}
assert all(set(v) <= set(LEVELS13) for v in LEVELS.values())

_REFS = {}   # (class, H, W, levels, B, autocast) -> the oracle's result; read-only


class _Ref32(dict):
    """The fp32 oracle's fields of a geometry, with the fp64 oracle's and the per-entry deviation between the two."""
    fp64, baseline, levels = None, None, None


def _batch(cfg, H, W, levels, B=1, positive=()):
    """`B` members with their own seeds and times, concatenated (bench.py's synthetic batch has one member)."""
    members = [_inputs(cfg, H, W, levels, seed=1 + i, positive=positive) for i in range(B)]
    if B == 1:
        return members[0]
    cat = lambda name: {k: torch.cat([getattr(m, name)[k] for m in members]) for k in getattr(members[0], name)}  # noqa: E731
    md = members[0].metadata
    times = tuple(md.time[0] + i * timedelta(hours=6) for i in range(B))
    return Batch(cat("surf_vars"), members[0].static_vars, cat("atmos_vars"), Metadata(md.lat, md.lon, times, md.atmos_levels))


def _reference(model, batch, key, autocast=False):
    key = (*key, autocast)
    if key not in _REFS:
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        ref = _oracle(model, sd, batch, autocast=autocast)
        if not autocast:
            ref = _Ref32(ref)
            ref.levels = batch.metadata.atmos_levels
            ref.fp64 = _oracle(model, {k: v.double() for k, v in sd.items()}, batch, autocast=False)
            ref.baseline = ne.per_level_errors(ref, ref.fp64, ref.levels)
        _REFS[key] = ref
    return _REFS[key]


def _run(monkeypatch, model, batch, reassoc, scores):
    monkeypatch.setenv("AURORA_PERCEIVER_REASSOC", reassoc)
    monkeypatch.setenv("AURORA_SCORE_WEIGHTS", scores)
    model._engine = None             # the switches are read when the handle is created
    out = _engine(model, batch)
    model._engine = None
    torch.cuda.empty_cache()
    return out


def _oracle_errors(out, ref, what):
    """Worst mean-rel and max-rel error per variable against the oracle, printed; `_assert_matches_oracle` holds them to the bounds."""
    assert set(out) == set(ref)
    e = {k: helpers.mean_rel_err(out[k], ref[k]) for k in ref}
    m = {k: helpers.rel_err(out[k], ref[k]) for k in ref}
    finite = all(bool(torch.isfinite(out[k]).all()) for k in ref)
    print(f"{what}: fp32 vs oracle worst mean-rel {max(e.values()):.3e} max-rel {max(m.values()):.3e}{'' if finite else ' NOT FINITE'}")
    return what, e, m, finite, out, ref


def _assert_matches_oracle(errors):
    what, e, m, finite, out, ref = errors
    assert finite, what
    for k in e:
        assert e[k] <= 1e-4 and m[k] <= 1e-3, (what, k, e[k], m[k])
    ne.check(what + " vs fp64 oracle", out, ref.fp64, ref.levels, ref.baseline)


def _worst(a, b):
    return max(helpers.mean_rel_err(a[k], b[k]) for k in b)


def _setup(cls, H, W, levels, B=1, positive=(), **kw):
    model = _seeded_model(cls, autocast=False, **DEPTHS, **kw)
    batch = _batch(model.config, H, W, levels, B, positive)
    ref = _reference(model, batch, (cls.__name__, H, W, levels, B))
    return model, batch, ref


def _switch_combinations(monkeypatch, cls, H, W, levels, B=1, positive=()):
    """All four settings of (re-association, score weights) against the oracle and against each other."""
    model, batch, ref = _setup(cls, H, W, levels, B, positive)
    what = f"{cls.__name__} {H}x{W} B={B} {len(levels)} levels"
    outs = {}
    for reassoc in ("1", "0"):
        for scores in ("1", "0"):
            outs[reassoc, scores] = _run(monkeypatch, model, batch, reassoc, scores)
    del model
    torch.cuda.empty_cache()
    pairs = {}
    for other in ("1", "0"):
        pairs[f"reassoc on/off, scores={other}"] = _worst(outs["1", other], outs["0", other])
        pairs[f"scores on/off, reassoc={other}"] = _worst(outs[other, "1"], outs[other, "0"])
    for name, worst in pairs.items():
        print(f"{what}: {name}: worst mean-rel {worst:.3e}")
    errors = [_oracle_errors(out, ref, f"{what} reassoc={reassoc} scores={scores}") for (reassoc, scores), out in outs.items()]
    for err in errors:               # (every figure is printed before the first assertion)
        _assert_matches_oracle(err)
    for name, worst in pairs.items():
        assert 0 < worst < 2e-6, (what, name, worst)


@pytest.mark.parametrize("n_levels", [3, 4])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_three_and_four_levels_match_oracle_under_every_switch(monkeypatch, size, n_levels):
    """`perceiver_out_kernel<3 | 4>` and `perceiver_probs_kernel<3 | 4, scores>` inside the step.  On the layout before the
    fix, worst mean-rel against the oracle with re-association on: 512 widths, 3 levels: 1.05e-1 (scores) and 7.1e-2 (keys);
    README widths, 3 levels: 8.0e-2 (keys; 7.8e-7 with scores, victim in front); README widths, 4 levels: 7.0e-2 (scores; 7.9e-7
    with keys, no overlap); 512 widths, 4 levels: 9.0e-7 (scores: no overlap; keys: victim in front).  Re-association off: 8e-7 to
    9.4e-7 everywhere, which is what every setting gives now."""
    cls, H, W = SIZES[size]
    _switch_combinations(monkeypatch, cls, H, W, LEVELS[n_levels])


@pytest.mark.parametrize("n_levels", [2, 5])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_two_and_five_levels_take_the_plain_pair_whatever_the_switch_says(monkeypatch, size, n_levels):
    """No `perceiver_out` kernel exists for these level counts (aurora_hip_perceiver_out_supported), so the re-association switch
    must change nothing at all: this pins the eligibility rule.  The plain pair goes through the same workspace."""
    cls, H, W = SIZES[size]
    model, batch, ref = _setup(cls, H, W, LEVELS[n_levels])
    on = _run(monkeypatch, model, batch, "1", "1")
    off = _run(monkeypatch, model, batch, "0", "1")
    del model
    torch.cuda.empty_cache()
    _assert_matches_oracle(_oracle_errors(on, ref, f"{cls.__name__} {H}x{W} {n_levels} levels"))
    assert all(torch.equal(on[k], off[k]) for k in off)


def test_batch_of_two_at_four_levels_matches_oracle_under_every_switch(monkeypatch):
    """Two batch members (row b * kv_bstride + j * kv_lstride + l of the context): README widths, 4 levels, 161 x 320.  On the
    layout before the fix: 6.9e-2 (scores) and 4.6e-2 (keys) against the oracle with re-association on, 8.3e-7 with it off."""
    _switch_combinations(monkeypatch, aurora_amd.AuroraSmallPretrained, 161, 320, LEVELS[4], B=2)


def test_bf16_backbone_at_three_levels_matches_oracle(monkeypatch):
    """`autocast=True` (the Perceivers stay fp32; the backbone between them runs in bf16) at 3 levels, 512 widths, default
    switches: within twice what the oracle's own autocast run deviates from its fp32 run, + 5e-4
    (tests/test_gpu_production.py:_compare).  The fp32 engine at this configuration was 1.05e-1 from the oracle on the layout
    before the fix.  (The one run on that layout had this case at the README widths, where the victim lies in front of its
    writer: it passed there, 7.3e-4 against the oracle's 9.6e-4, and moved here for that reason.)"""
    cls, H, W = SIZES["512"]
    levels = LEVELS[3]
    model, batch, ref32 = _setup(cls, H, W, levels)
    ref16 = _reference(model, batch, (cls.__name__, H, W, levels, 1), autocast=True)
    model.autocast = True
    out16 = _run(monkeypatch, model, batch, "1", "1")
    del model
    torch.cuda.empty_cache()
    e16 = {k: helpers.mean_rel_err(out16[k], ref32[k]) for k in ref32}
    b16 = {k: helpers.mean_rel_err(ref16[k], ref32[k]) for k in ref32}
    print(f"{cls.__name__} {H}x{W} 3 levels: bf16 worst {max(e16.values()):.3e} (oracle autocast {max(b16.values()):.3e})")
    for k in ref32:
        assert torch.isfinite(out16[k]).all(), k
        assert e16[k] <= 2 * b16[k] + 5e-4, (k, e16[k], b16[k])


def test_second_perceiver_layers_match_oracle():
    """`enc_depth=2, dec_depth=2`: the only way to a resampler layer behind the first -- its query projection from the previous
    layer's result, keys instead of score rows, that result as the residual, no re-association.  The smallest shapes at which
    every pre-split weight of a layer exists (tests/test_gpu_encoder_front.py: embed_dim 256, 4 x 8 patches, 4 levels), against
    the oracle in fp64 on the same fp32 weights."""
    from tests import test_gpu_encoder_front as front

    case = dict(front.CASES["era5"], kwargs=dict(front._SMALL, enc_depth=2, dec_depth=2))
    sd, batch, ref = front._case(case)
    assert any(".level_agg.layers.1." in k for k in sd) and any(".level_decoder.layers.1." in k for k in sd)
    model = aurora_amd.Aurora(**case["kwargs"])
    model.load_state_dict(sd, strict=True)
    out = _engine(model.to(DEV).eval(), batch)
    ref32 = _Ref32(_oracle(model, sd, batch, autocast=False))      # `ref` is the oracle in fp64 here: the fp32 run is the baseline
    ref32.fp64, ref32.levels = ref, batch.metadata.atmos_levels
    ref32.baseline = ne.per_level_errors(ref32, ref, ref32.levels)
    what, e, m, finite, _, _ = _oracle_errors(out, ref, "Aurora 16x32 4 levels, two layers per Perceiver")
    _assert_matches_oracle((what, e, m, finite, out, ref32))


def test_air_pollution_second_decoder_perceiver_at_four_levels(monkeypatch):
    """AuroraAirPollution decodes its pollution variables with a second Perceiver (`dec_rs_alt`) over the same context, through
    the same workspace: 4 of its 13 condition levels (each level has its own patch embedding and head, so a subset is a valid
    input), default widths, patch size 3, 181 x 360.  At 4 levels and these widths the overlap exists with keys only, with the
    victim in front of its writer: on the layout before the fix this case passed (1.1e-6 against the oracle in every setting)."""
    cls = aurora_amd.AuroraAirPollution
    with torch.device("meta"):
        cfg = cls().config
    _switch_combinations(monkeypatch, cls, 181, 360, LEVELS[4], positive=cfg.positive_surf_vars + cfg.positive_atmos_vars)
