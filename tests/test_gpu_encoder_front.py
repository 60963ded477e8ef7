"""The encoder front composed: the atmospheric patch embedding folded into the level aggregation's context linears
(csrc/model_weights.hip:compose_front, csrc/step.hip:encode_levels) against the two stages it replaces, at the handle level.

Both forms are fp32-grade evaluations of the same real-valued map; only the rounding points move.  So the bound is not a
distance between the two but the one tests/test_gpu_production.py holds the fp32 engine to against the oracle (metric of the
reference's own test: mean|out - ref| / mean|ref| <= 1e-4 per variable, max-norm <= 1e-3), here against the oracle run in
fp64 on the same fp32 weights: each case prints what the two-stage path deviates by and asserts that the composed path meets
the same bound.

Shapes: a 4 x 8 patch grid (the smallest all three backbone stages accept), 4 levels, D = 256 -- the narrowest width at which
to_kv (512 rows) exists in the fp16-pair form, i.e. at which the guarded chain and its pre-split composed weights run.
What cannot be reached through the handle (the encoder latents themselves) is not compared; the step outputs are a function
of nothing else.
"""
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, normalisation
from oracle import aurora_oracle as oracle
from tests import helpers

pytestmark = pytest.mark.gpu

_SMALL = dict(embed_dim=256, num_heads=8, encoder_depths=(2, 2, 2), encoder_num_heads=(4, 8, 16), decoder_depths=(2, 2, 2),
              decoder_num_heads=(16, 8, 4))
LEVELS = (100, 250, 500, 850)
CASES = {
    "era5": dict(cls="Aurora", kwargs=dict(**_SMALL), H=16, W=32, B=1, T=2, levels=LEVELS),
    "level_conditioned": dict(cls="Aurora", kwargs=dict(**_SMALL, level_condition=LEVELS), H=16, W=32, B=1, T=2, levels=LEVELS),
    "one_variable_absent": dict(cls="Aurora", kwargs=dict(**_SMALL), H=16, W=32, B=1, T=2, levels=LEVELS, drop="q"),
    "batch_of_two": dict(cls="Aurora", kwargs=dict(**_SMALL), H=16, W=32, B=2, T=2, levels=LEVELS),
    "ln_k_q": dict(cls="Aurora", kwargs=dict(**_SMALL, stabilise_level_agg=True), H=16, W=32, B=1, T=2, levels=LEVELS),
}
MEAN_REL, MAX_REL = 1e-4, 1e-3   # tests/test_gpu_production.py:_compare, fp32 engine vs oracle


def _case(case, scale=1.0):
    """(weights fp32, batch on the host, fp64 oracle outputs) of a case; `scale` multiplies the atmospheric anomalies."""
    with torch.device("meta"):
        meta = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    sd = helpers.case_state_dict(meta, torch.float32)
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, meta.config)
    atmos = {k: v for k, v in atmos.items() if k != case.get("drop")}
    if scale != 1.0:   # the normalised inputs grow by `scale`: (x - loc) / scale_k
        atmos = {k: v * scale for k, v in atmos.items()}
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
    with torch.inference_mode():
        o_s, o_a, _ = oracle.forward({k: v.double() for k, v in sd.items()}, meta.config, batch.surf_vars, batch.static_vars,
                                     batch.atmos_vars, lat, lon, times, case["levels"], 0, normalisation.locations,
                                     normalisation.scales, variant=meta.variant)
    ref = {**{f"surf.{k}": v for k, v in o_s.items()}, **{f"atmos.{k}": v for k, v in o_a.items()}}
    return sd, batch, ref


def _run(case, sd, batch, monkeypatch, compose):
    """One step of a fresh handle with the switch on / off: (outputs, was the front composed, guard words, linear_f32 launches)."""
    monkeypatch.setenv("AURORA_COMPOSE_FRONT", "1" if compose else "0")
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda").eval()
    dev = batch.to("cuda")
    with torch.inference_mode():
        model.forward(dev)                       # (the first step builds the packs and sizes the workspace)
        native = model.engine().native
        native.profile_begin({"linear_f32"})
        pred = model.forward(dev)
        launches = native.profile_end_list()
    torch.cuda.synchronize()
    out = {**{f"surf.{k}": v.cpu() for k, v in pred.surf_vars.items()}, **{f"atmos.{k}": v.cpu() for k, v in pred.atmos_vars.items()}}
    return out, native.front_composed(), native.guard_words(), launches


def _errors(out, ref):
    assert set(out) == set(ref)
    return (max(helpers.mean_rel_err(out[k], ref[k]) for k in ref), max(helpers.rel_err(out[k], ref[k]) for k in ref))


@pytest.mark.parametrize("name", list(CASES))
def test_composed_front_meets_the_fp32_bound_the_two_stages_meet(name, monkeypatch):
    case = CASES[name]
    sd, batch, ref = _case(case)
    staged, was0, w0, l0 = _run(case, sd, batch, monkeypatch, compose=False)
    folded, was1, w1, l1 = _run(case, sd, batch, monkeypatch, compose=True)
    e0, e1 = _errors(staged, ref), _errors(folded, ref)
    between = max(helpers.mean_rel_err(folded[k], staged[k]) for k in ref)
    print(f"{name}: two stages vs fp64 oracle mean-rel {e0[0]:.3e} max-rel {e0[1]:.3e}; composed {e1[0]:.3e} {e1[1]:.3e}; "
          f"composed vs two stages {between:.3e}; linear_f32 launches {len(l0)} -> {len(l1)}")
    assert not was0 and was1, (was0, was1)
    assert all(torch.isfinite(v).all() for v in folded.values())
    assert e0[0] <= MEAN_REL and e0[1] <= MAX_REL, e0
    assert e1[0] <= MEAN_REL and e1[1] <= MAX_REL, e1
    assert between > 0                                      # (not the same launches)
    # the same guard word decides both, inside fp16's range here; the embedding's guarded pair of launches is gone
    assert w0[1] == w1[1] and 0 < w1[1] < 16384.0 and w1[0] == 0.0
    assert len(l1) == len(l0) - 2, (len(l0), len(l1))


def test_inputs_outside_the_fp16_range_take_the_three_term_kernel_and_agree(monkeypatch):
    """Atmospheric anomalies scaled until max |normalised input| passes the guard's limit: the device word sends the composed
    linear to its three-term twin (fp32 composed weights), and the step still meets the bound.  The word is read back through
    `aurora_hip_guard_words`, the handle's account of which path a step took; the plan query names the kernel of each half."""
    from aurora_amd.engine import lib

    case = CASES["era5"]
    sd, batch, ref = _case(case, scale=1e5)
    staged, _, w0, _ = _run(case, sd, batch, monkeypatch, compose=False)
    folded, was, w1, _ = _run(case, sd, batch, monkeypatch, compose=True)
    e0, e1 = _errors(staged, ref), _errors(folded, ref)
    print(f"guard failed (word {w1[1]:.3e}): two stages {e0[0]:.3e} {e0[1]:.3e}; composed {e1[0]:.3e} {e1[1]:.3e}")
    assert was and w1[1] == w0[1] and w1[1] >= 16384.0, w1   # word >= limit: the two-term launch retires, its twin runs
    rows = case["B"] * (case["H"] // 4) * (case["W"] // 4)
    two = lib.linear_plan(rows, 512, 160, torch.float32, f32_gemm=2 | lib.F32_W_SPLIT, guard=True, batch=len(LEVELS))
    three = lib.linear_plan(rows, 512, 160, torch.float32, f32_gemm=1, guard=True, batch=len(LEVELS))
    assert two.kernel == "f32_pp_w" and three.kernel == "f32_three", (two, three)
    assert all(torch.isfinite(v).all() for v in folded.values())
    assert e0[0] <= MEAN_REL and e0[1] <= MAX_REL, e0
    assert e1[0] <= MEAN_REL and e1[1] <= MAX_REL, e1


def test_patch_size_10_declines_and_runs_the_two_stages(monkeypatch):
    """Kpad = 1000 at patch size 10: the composed linear would do 0.85 of the work, the rule declines, and the switch changes
    nothing -- the same launches, the same bits."""
    case = dict(cls="AuroraHighRes", kwargs=dict(**_SMALL), H=40, W=80, B=1, T=2, levels=LEVELS)
    sd, batch, _ = _case(case)
    off, was0, _, l0 = _run(case, sd, batch, monkeypatch, compose=False)
    on, was1, _, l1 = _run(case, sd, batch, monkeypatch, compose=True)
    assert not was0 and not was1
    assert l0 and [e[2] for e in l0] == [e[2] for e in l1]   # (the work of every fp32 linear, in launch order)
    assert all(torch.equal(on[k], off[k]) for k in off)
