"""End-to-end parity of the HIP engine (through the public Aurora / rollout API).

Stated tolerances (metric = the reference test's own, tests/test_model.py:45-61 upstream:
mean|out - ref| / mean|ref| per variable, plus a max-norm guard):

  fp32 engine  vs fp64 reference goldens : <= 1e-4  (upstream accepts 1e-4 .. 5e-3 in fp64)
  bf16 engine (autocast=True) vs the same: <= 3e-2, and within 3x of what the reference's own
        CPU autocast path (the oracle with autocast=True) deviates from fp32.

Beside them, per surface variable and per (atmospheric variable, level) in units of normalisation.scales
(tests/normalised_error.py): fp32 within 4x of what the fp32 oracle deviates from the same golden by (or of one fp32 ulp of the
entry's largest value), bf16 within 3x of the oracle's autocast deviation of that entry, never tighter than the fp32 bound.
"""
import dataclasses
from datetime import timedelta

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, normalisation, rollout
from oracle import aurora_oracle as oracle
from tests import helpers
from tests import normalised_error as ne
from tests.golden_cases import CASES

pytestmark = pytest.mark.gpu


def build(name, autocast=False):
    case = CASES[name]
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"], autocast=autocast)
    sd = helpers.case_state_dict(model, torch.float32)
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda").eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
    return case, model, batch


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_engine_matches_reference_golden(name):
    case, model, batch = build(name)
    gold = helpers.load_golden(name)
    worst, preds = {}, []
    with torch.inference_mode():
        for s, pred in enumerate(rollout(model, batch, steps=case["steps"])):
            preds.append(ne.fields({k: v.cpu() for k, v in pred.surf_vars.items()}, {k: v.cpu() for k, v in pred.atmos_vars.items()}))
            assert pred.metadata.rollout_step == s + 1
            assert pred.metadata.time == tuple(t + (s + 1) * model.timestep for t in batch.metadata.time)
            for kind, d in (("surf", pred.surf_vars), ("atmos", pred.atmos_vars)):
                for k, v in d.items():
                    ref = torch.from_numpy(gold[f"s{s}.{kind}.{k}"])
                    assert v.shape == ref.shape and v.is_cuda
                    v, ref, flipped = helpers.nan_agreement(v.cpu(), ref)
                    assert flipped <= 2e-3, (k, flipped)   # (only the wave variant produces NaN at all)
                    worst[f"s{s}.{kind}.{k}"] = (helpers.mean_rel_err(v, ref), helpers.rel_err(v, ref))
            for k, v in pred.static_vars.items():
                assert torch.allclose(v.cpu(), batch.static_vars[k][: v.shape[0]])
            if name == "wave":
                assert "dwi" not in pred.surf_vars and torch.isnan(pred.surf_vars["swh"]).any()
    print(name, "worst mean-rel", max(w[0] for w in worst.values()), "worst max-rel", max(w[1] for w in worst.values()))
    assert len(worst) == len(gold)
    bad = {k: w for k, w in worst.items() if w[0] > 1e-4 or w[1] > 1e-3}
    assert not bad, bad
    # per variable and level in normalised units, against the fp32 oracle's own deviation from the same golden
    entries = [ne.per_level_errors(p, ne.golden(name)[s], case["levels"]) for s, p in enumerate(preds)]
    ratios = [ne.report(f"{name} step {s}", e, ne.oracle_fp32_errors(name, s)) for s, e in enumerate(entries)]
    print(name, "worst engine / oracle ratio over all steps", max(ratios))
    bad = [f"step {s}: {line}" for s, e in enumerate(entries) for line in ne.failures(e, ne.fp32_bounds(name, s))]
    assert not bad, bad


def test_double_model_runs_the_references_own_golden_harness():
    """The reference's golden test runs `model.double()` on float64 inputs and accepts, per variable,
    mean|out - ref| / mean|ref| <= 1e-4 (2t, msl, t) or 5e-3 (winds, q) (tests/test_model.py:18-24, 45-61 upstream).  The same
    harness against this package: a float64 model is accepted with a warning that names the precision, the predictions
    come back as float64, and they meet the tighter of the reference's own bounds on every variable."""
    case, model, batch = build("base_pad")
    model = model.double()
    assert model._engine is None and next(model.parameters()).dtype == torch.float64
    batch = batch.type(torch.float64)
    gold = helpers.load_golden("base_pad")
    with torch.inference_mode(), pytest.warns(UserWarning, match="float64.*computes in float32"):
        preds = [p for p in rollout(model, batch, steps=case["steps"])]
    for s, pred in enumerate(preds):
        for kind, d in (("surf", pred.surf_vars), ("atmos", pred.atmos_vars)):
            for k, v in d.items():
                assert v.dtype == torch.float64 and v.is_cuda
                ref = torch.from_numpy(gold[f"s{s}.{kind}.{k}"]).double()
                assert helpers.mean_rel_err(v.cpu(), ref) <= 1e-4, (s, kind, k)
    # `.float()` again: storage changes, the handle is rebuilt (no warning this time)
    model = model.float()
    assert model._engine is None


@pytest.mark.parametrize("name", ["base_pad", "small_b2", "lora_all"])
def test_bf16_engine_within_autocast_tolerance(name):
    case, model, batch = build(name, autocast=True)
    gold = helpers.load_golden(name)
    # what the reference's own bf16 path (CPU autocast, restated by the oracle) deviates by
    _, meta = helpers.case_model_meta(name)
    sd32 = helpers.case_state_dict(meta, torch.float32)
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, meta.config)
    with torch.inference_mode():
        o_s, o_a, _ = oracle.forward(sd32, meta.config, surf, static, atmos, lat, lon, times, case["levels"], 0,
                                     normalisation.locations, normalisation.scales, autocast=True,
                                     variant=meta.variant)
        pred = model.forward(batch)
    errs, base = {}, {}
    for kind, d, od in (("surf", pred.surf_vars, o_s), ("atmos", pred.atmos_vars, o_a)):
        for k, v in d.items():
            ref = torch.from_numpy(gold[f"s0.{kind}.{k}"])
            errs[f"{kind}.{k}"] = helpers.mean_rel_err(v.cpu(), ref)
            base[f"{kind}.{k}"] = helpers.mean_rel_err(od[k], ref)
    print(name, "engine bf16:", max(errs.values()), " reference autocast:", max(base.values()))
    for k in errs:
        assert errs[k] < 1e-2, (k, errs[k])
        assert errs[k] < 3 * base[k] + 1e-3, (k, errs[k], base[k])
    # per entry: 3x the oracle's autocast deviation of that entry; the entry's fp32 bound takes the place of the flat + 1e-3
    ref = ne.golden(name)[0]
    ne.check(f"{name} bf16", ne.fields({k: v.cpu() for k, v in pred.surf_vars.items()}, {k: v.cpu() for k, v in pred.atmos_vars.items()}),
             ref, case["levels"], ne.per_level_errors(ne.fields(o_s, o_a), ref, case["levels"]), margin=3.0,
             floor=ne.fp32_bounds(name, 0))


def test_guard_words_say_which_fp32_path_a_step_took():
    """The large fp32 linears of encoder and decoder pick two fp16 terms or three bf16 terms on the DEVICE, from range words the
    step leaves behind; `aurora_hip_guard_words` hands them to the host afterwards.  Word 1 / 2 are max |normalised input| of
    the atmospheric / surface patch embedding exactly (patchify folds them in, no separate pass); raw `randn` fields -- the
    upstream README example -- push them past fp16's safe range, and the step takes the three-term kernels."""
    from datetime import datetime

    model = aurora_amd.AuroraSmallPretrained()      # (the README model: its patch embeddings run as guarded chains)
    torch.manual_seed(0)
    for p in model.parameters():
        if p.abs().sum() == 0:
            torch.nn.init.normal_(p, std=0.02)
    model = model.to("cuda").eval()
    levels = (100, 250, 500, 850)
    g = torch.Generator().manual_seed(3)
    batch = Batch(
        surf_vars={k: torch.randn(1, 2, 17, 32, generator=g) for k in ("2t", "10u", "10v", "msl")},
        static_vars={k: torch.randn(17, 32, generator=g) for k in ("lsm", "z", "slt")},
        atmos_vars={k: torch.randn(1, 2, 4, 17, 32, generator=g) for k in ("z", "u", "v", "t", "q")},
        metadata=Metadata(lat=torch.linspace(90, -90, 17), lon=torch.linspace(0, 360, 32 + 1)[:-1],
                          time=(datetime(2020, 6, 1, 12, 0),), atmos_levels=levels),
    )
    with torch.inference_mode():
        model.forward(batch)
    w = model.engine().native.guard_words()
    batch = batch.crop(model.patch_size)

    def norm_max(d, affine):
        m = 0.0
        for k, v in d.items():
            loc, scale = affine(k)
            loc_t, scale_t = torch.tensor(loc, dtype=torch.float32), torch.tensor(scale, dtype=torch.float32)
            shape = (-1, 1, 1) if loc_t.numel() > 1 else ()
            m = max(m, float(((v.float().cpu() - loc_t.reshape(shape)) / scale_t.reshape(shape)).abs().max()))
        return m

    atmos = norm_max(batch.atmos_vars, lambda k: normalisation.atmos_affine(k, levels))
    surf = max(norm_max(batch.surf_vars, normalisation.surf_affine), norm_max(batch.static_vars, normalisation.surf_affine))
    assert abs(w[1] - atmos) <= 2e-6 * atmos and abs(w[2] - surf) <= 2e-6 * surf, (w, atmos, surf)
    assert 0.0 < w[3] < float("inf") and w[0] == 0.0     # the encoder ran as one guarded chain: its own word stays clear
    assert w[1] > 16384.0                                 # raw randn fields: (x - loc) / scale of q is ~1e6 -> three bf16 terms

    # the same fields in physical units (randn in NORMALISED space): inside fp16's range -> two fp16 terms
    def physical(d, affine):
        out = {}
        for k, v in d.items():
            loc, scale = affine(k)
            loc_t, scale_t = torch.tensor(loc, dtype=torch.float32), torch.tensor(scale, dtype=torch.float32)
            shape = (-1, 1, 1) if loc_t.numel() > 1 else ()
            out[k] = v * scale_t.reshape(shape) + loc_t.reshape(shape)
        return out

    phys = dataclasses.replace(batch, surf_vars=physical(batch.surf_vars, normalisation.surf_affine),
                               static_vars=physical(batch.static_vars, normalisation.surf_affine),
                               atmos_vars=physical(batch.atmos_vars, lambda k: normalisation.atmos_affine(k, levels)))
    with torch.inference_mode():
        pred = model.forward(phys)
    w2 = model.engine().native.guard_words()
    want = max(float(v.abs().max()) for v in batch.atmos_vars.values())
    assert abs(w2[1] - want) <= 1e-3 * want and w2[1] < 16384.0 and w2[2] < 16384.0, (w2, want)
    assert all(torch.isfinite(v).all() for v in pred.atmos_vars.values())


def test_readme_example_runs_unchanged():
    """README.md:77-102 upstream, with `aurora` -> `aurora_amd` and the model on the GPU."""
    from datetime import datetime

    model = aurora_amd.AuroraSmallPretrained()
    torch.manual_seed(0)
    for p in model.parameters():  # no checkpoint download offline: random weights
        if p.abs().sum() == 0:
            torch.nn.init.normal_(p, std=0.02)
    model = model.to("cuda").eval()
    batch = Batch(
        surf_vars={k: torch.randn(1, 2, 17, 32) for k in ("2t", "10u", "10v", "msl")},
        static_vars={k: torch.randn(17, 32) for k in ("lsm", "z", "slt")},
        atmos_vars={k: torch.randn(1, 2, 4, 17, 32) for k in ("z", "u", "v", "t", "q")},
        metadata=Metadata(
            lat=torch.linspace(90, -90, 17),
            lon=torch.linspace(0, 360, 32 + 1)[:-1],
            time=(datetime(2020, 6, 1, 12, 0),),
            atmos_levels=(100, 250, 500, 850),
        ),
    )
    with torch.inference_mode():
        pred = model.forward(batch)
    assert pred.surf_vars["2t"].shape == (1, 1, 16, 32) and pred.atmos_vars["t"].shape == (1, 1, 4, 16, 32)
    assert torch.isfinite(pred.surf_vars["2t"]).all()
    assert pred.metadata.time == (datetime(2020, 6, 1, 18, 0),) and pred.metadata.rollout_step == 1
    # versus the oracle on the same weights / inputs
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.inference_mode():
        o_s, o_a, _ = oracle.forward(sd, model.config, batch.surf_vars, batch.static_vars, batch.atmos_vars,
                                     batch.metadata.lat, batch.metadata.lon, batch.metadata.time,
                                     batch.metadata.atmos_levels, 0, normalisation.locations, normalisation.scales)
    for k, v in pred.surf_vars.items():
        assert helpers.mean_rel_err(v.cpu(), o_s[k]) < 1e-4
    for k, v in pred.atmos_vars.items():
        assert helpers.mean_rel_err(v.cpu(), o_a[k]) < 1e-4


def test_model_runs_wrapped_in_ddp():
    """tests/test_model.py:96-110 upstream (the reference's only collective): the model inside DistributedDataParallel,
    gloo, world size one -- "just test that it runs", and that it predicts what the bare model predicts."""
    import torch.distributed as dist

    case, model, batch = build("small_b2")
    with torch.inference_mode():
        want = model.forward(batch)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", rank=0, world_size=1, store=dist.HashStore())
    try:
        wrapped = torch.nn.parallel.DistributedDataParallel(model)
        with torch.inference_mode():
            got = wrapped.forward(batch)
        for k, v in want.surf_vars.items():
            assert torch.equal(got.surf_vars[k], v)
    finally:
        if created:
            dist.destroy_process_group()


def test_lat_lon_matrices_give_the_vector_result():
    """tests/test_model.py:126-160 upstream: latitude / longitude matrices instead of vectors, same prediction (rtol 1e-5)."""
    case, model, batch = build("small_b2")
    with torch.inference_mode():
        pred = model.forward(batch)
        n_lat, n_lon = len(batch.metadata.lat), len(batch.metadata.lon)
        meta = dataclasses.replace(batch.metadata, lat=batch.metadata.lat[:, None].expand(n_lat, n_lon),
                                   lon=batch.metadata.lon[None, :].expand(n_lat, n_lon))
        pred_matrix = model.forward(dataclasses.replace(batch, metadata=meta))
    for a, b in ((pred.surf_vars, pred_matrix.surf_vars), (pred.static_vars, pred_matrix.static_vars),
                 (pred.atmos_vars, pred_matrix.atmos_vars)):
        for k in a:
            np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), rtol=1e-5)
    assert pred_matrix.metadata.lat.dim() == 2   # the prediction carries the caller's (cropped) matrices on


def test_flags_change_the_prediction():
    """tests/test_model.py:163-200 upstream: `stabilise_level_agg` and a 12 h `timestep` each give a different model (surface
    and atmospheric predictions differ beyond rtol 5e-2 somewhere), static variables pass through unchanged."""
    case = CASES["small_b2"]
    preds = []
    for flags in ({}, {"stabilise_level_agg": True}, {"timestep": timedelta(hours=12)}):
        model = aurora_amd.AuroraSmallPretrained(**case["kwargs"], use_lora=True, **flags)
        sd = helpers.case_state_dict(model, torch.float32)
        model.load_state_dict(sd, strict=True)
        model = model.to("cuda").eval()
        surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
        f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
        batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
        with torch.inference_mode():
            preds.append(model.forward(batch).normalise(model.surf_stats).to("cpu"))
    for i, p1 in enumerate(preds):
        for p2 in preds[i + 1:]:
            for k in p1.surf_vars:
                assert not np.allclose(p1.surf_vars[k], p2.surf_vars[k], rtol=5e-2), k
            for k in p1.static_vars:
                np.testing.assert_allclose(p1.static_vars[k], p2.static_vars[k], rtol=1e-5)
            for k in p1.atmos_vars:
                assert not np.allclose(p1.atmos_vars[k], p2.atmos_vars[k], rtol=5e-2), k


def test_lora_single_vs_all_equal_at_step0_only():
    """tests/test_rollout.py:62-76 upstream: LoRA 'single' and 'all' agree at step 0, not after."""
    outs = {}
    for mode in ("single", "all"):
        kw = dict(CASES["lora_all"]["kwargs"], lora_mode=mode)
        model = aurora_amd.Aurora(**kw)
        sd = helpers.case_state_dict(model, torch.float32)
        model.load_state_dict(sd)
        model = model.to("cuda").eval()
        case = CASES["lora_all"]
        surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
        f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
        batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
        with torch.inference_mode():
            outs[mode] = [p.surf_vars["2t"].cpu() for p in rollout(model, batch, steps=2)]
    assert torch.allclose(outs["single"][0], outs["all"][0], rtol=1e-4)
    assert not torch.allclose(outs["single"][1], outs["all"][1], rtol=1e-4)


def test_inputs_are_not_mutated_and_outputs_are_fresh():
    case, model, batch = build("small_b2")
    before = {k: v.clone() for k, v in batch.surf_vars.items()}
    with torch.inference_mode():
        p1 = model.forward(batch)
        keep = p1.surf_vars["2t"].clone()
        p2 = model.forward(batch)
    for k, v in batch.surf_vars.items():
        assert torch.equal(v, before[k])
    assert torch.equal(p1.surf_vars["2t"], keep)          # a second step does not clobber the first
    assert torch.equal(p1.surf_vars["2t"], p2.surf_vars["2t"])  # deterministic


@pytest.mark.parametrize("name,autocast", [("base_pad", False), ("base_pad", True), ("lora_all", False),
                                           ("air_pollution", False), ("wave", False)])
def test_graph_captured_rollout_equals_eager(name, autocast):
    """BASELINE config 3 in miniature: roll-out with the step replayed from a hipGraph."""
    case, model, batch = build(name, autocast=autocast)
    steps = max(case["steps"], 3)
    with torch.inference_mode():
        eager = list(rollout(model, batch, steps=steps))
        graphed = list(rollout(model, batch, steps=steps, graph=True))
    torch.cuda.synchronize()
    for e, g in zip(eager, graphed):
        assert g.metadata.time == e.metadata.time and g.metadata.rollout_step == e.metadata.rollout_step
        for k in e.surf_vars:
            assert torch.equal(g.surf_vars[k].nan_to_num(-1.0), e.surf_vars[k].nan_to_num(-1.0)), k
        for k in e.atmos_vars:
            assert torch.equal(g.atmos_vars[k], e.atmos_vars[k]), k
    # predictions handed out earlier are not overwritten by later replays
    assert not torch.equal(graphed[0].surf_vars["2t"], graphed[1].surf_vars["2t"])


def test_captured_graph_refuses_to_replay_after_the_handle_reallocated():
    """A hipGraph of the step bakes in the addresses of the handle's workspace and tables.  Running the same model eagerly on
    a larger batch re-allocates them (`aurora_hip_generation` changes): `advance()` must refuse instead of replaying into
    freed memory, and `rollout(graph=True)` must capture anew by itself."""
    case, model, batch = build("base_pad")
    with torch.inference_mode():
        stepper = model.engine().capture(batch)
        first = stepper.advance()
        gen = model.engine().native.generation()
        two = dataclasses.replace(
            batch, surf_vars={k: v.repeat(2, 1, 1, 1) for k, v in batch.surf_vars.items()},
            atmos_vars={k: v.repeat(2, 1, 1, 1, 1) for k, v in batch.atmos_vars.items()},
            metadata=dataclasses.replace(batch.metadata, time=batch.metadata.time * 2))
        model.forward(two)                                   # B = 2: larger workspace, larger time buffers
        assert model.engine().native.generation() != gen
        with pytest.raises(RuntimeError, match="capture a new graph"):
            stepper.advance()
        again = next(iter(rollout(model, batch, steps=1, graph=True)))
    for k, v in first.surf_vars.items():
        assert torch.equal(again.surf_vars[k], v), k


def test_rollout_history_windows_equal_the_reference_cat_loop():
    """`rollout` slides a window over history chunks and lets the model write each prediction into the next slot; the
    reference's loop (rollout.py:39-49: forward, then `cat([old[:, 1:], pred])`) must give the same states, across a
    chunk boundary (12 steps > 8 slots) and with earlier predictions still intact afterwards."""
    case, model, batch = build("small_b2")       # B = 2: predictions are copied into the slots
    case1, model1, batch1 = build("base_pad")    # B = 1: predictions are written in place
    for mdl, bt in ((model, batch), (model1, batch1)):
        steps = 12
        with torch.inference_mode():
            got = list(rollout(mdl, bt, steps=steps))
            b = bt.type(torch.float32).crop(mdl.patch_size).to("cuda")
            want = []
            for _ in range(steps):
                p = mdl.forward(b)
                want.append(p)
                b = dataclasses.replace(
                    p, surf_vars={k: torch.cat([b.surf_vars[k][:, 1:], v], dim=1) for k, v in p.surf_vars.items()},
                    atmos_vars={k: torch.cat([b.atmos_vars[k][:, 1:], v], dim=1) for k, v in p.atmos_vars.items()})
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert g.metadata.time == w.metadata.time and g.metadata.rollout_step == w.metadata.rollout_step
            for k in w.surf_vars:
                assert torch.equal(g.surf_vars[k], w.surf_vars[k]), k
            for k in w.atmos_vars:
                assert torch.equal(g.atmos_vars[k], w.atmos_vars[k]), k


def test_rollout_to_host_overlaps_and_equals_device_rollout():
    case, model, batch = build("base_pad")
    with torch.inference_mode():
        dev = list(rollout(model, batch, steps=4))
        host = list(rollout(model, batch, steps=4, to_host=True))
    assert len(host) == 4
    for d, h in zip(dev, host):
        assert h.metadata.rollout_step == d.metadata.rollout_step and h.metadata.time == d.metadata.time
        for k, v in d.surf_vars.items():
            assert not h.surf_vars[k].is_cuda and h.surf_vars[k].is_pinned()
            assert torch.equal(h.surf_vars[k], v.cpu()), k
        for k, v in d.atmos_vars.items():
            assert torch.equal(h.atmos_vars[k], v.cpu()), k


def test_write_rollout_files_equal_the_predictions(tmp_path):
    """`write_rollout` = roll-out + pinned-host delivery + one netCDF file per step written by a
    background thread; the files hold exactly what `rollout` yields."""
    case, model, batch = build("base_pad")
    with torch.inference_mode():
        want = [p.to("cpu") for p in rollout(model, batch, steps=3)]
        paths = aurora_amd.write_rollout(model, batch, 3, str(tmp_path / "pred.{step:02d}.nc"))
    assert [p.rsplit("/", 1)[1] for p in paths] == ["pred.01.nc", "pred.02.nc", "pred.03.nc"]
    for path, ref in zip(paths, want):
        got = Batch.from_netcdf(path)
        assert got.metadata.rollout_step == ref.metadata.rollout_step
        assert tuple(got.metadata.time) == tuple(t.replace(tzinfo=None) for t in ref.metadata.time)
        for d, rd in ((got.surf_vars, ref.surf_vars), (got.atmos_vars, ref.atmos_vars)):
            for k, v in rd.items():
                assert torch.equal(d[k], v), k


def test_a_subset_of_the_variables_runs_like_the_reference():
    """The reference accepts a Batch that carries only some of the model's variables (every variable has its own patch
    embedding weight and head, patchembed.py:100-115, decoder.py:214-263).  Through the C ABI an absent variable is a NULL
    entry of the pointer lists: the embedding GEMM is packed for the present channels, only they are predicted."""
    case, model, batch = build("base_pad")
    drop_s, drop_a = "msl", "q"
    sub = dataclasses.replace(batch, surf_vars={k: v for k, v in batch.surf_vars.items() if k != drop_s},
                              atmos_vars={k: v for k, v in batch.atmos_vars.items() if k != drop_a})
    sd = helpers.case_state_dict(model, torch.float32)
    host = lambda d: {k: v.cpu() for k, v in d.items()}  # noqa: E731
    with torch.inference_mode():
        pred = model.forward(sub)
        (o_s, o_a, _), (d_s, d_a, _) = (
            oracle.forward(w, model.config, host(sub.surf_vars), host(sub.static_vars), host(sub.atmos_vars), sub.metadata.lat.cpu(),
                           sub.metadata.lon.cpu(), sub.metadata.time, case["levels"], 0, normalisation.locations, normalisation.scales)
            for w in (sd, {k: v.double() for k, v in sd.items()}))
    assert list(pred.surf_vars) == list(sub.surf_vars) and list(pred.atmos_vars) == list(sub.atmos_vars)
    for d, od in ((pred.surf_vars, o_s), (pred.atmos_vars, o_a)):
        for k, v in d.items():
            assert helpers.mean_rel_err(v.cpu(), od[k]) <= 1e-4, k
    # per entry against the oracle in fp64 on the same fp32 weights and inputs; the baseline is the fp32 oracle above
    ref = ne.fields(d_s, d_a)
    ne.check("base_pad without msl and q", ne.fields(host(pred.surf_vars), host(pred.atmos_vars)), ref, case["levels"],
             ne.per_level_errors(ne.fields(o_s, o_a), ref, case["levels"]))
    with pytest.raises(KeyError):
        model.forward(dataclasses.replace(batch, surf_vars={**batch.surf_vars, "sst": batch.surf_vars["2t"]}))
