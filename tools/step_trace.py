"""What one forecast step launches, how much workspace it takes and what it computes -- as text that two builds of the
library can be diffed on.

    AURORA_HIP_LIB=<library> python tools/step_trace.py --out FILE                       (GPU box)
    AURORA_HIP_LIB=<library> python tools/step_trace.py --out FILE --f32-gemm bf16      (its own process)

One JSON record per line:
  * every golden case of tests/golden_cases.py (built as tests/test_gpu_model.py builds them), in fp32 and under autocast:
    the ordered (kind, work) list of a warmed step's launches with every kind profiled, the handle's workspace_bytes(),
    the sha256 of every output variable's bytes, and `repeatable`: whether the next step of the same process gives the
    same hashes (where a build does not reproduce itself, its hashes say nothing about another build);
  * every rank of the band splits of tests/test_gpu_sharded.py::test_sharded_equals_unsharded (base_pad at 192x96 over
    2 and 3 ranks, at 256x96 over 5), fp32 and autocast, with a transport whose `post` / `wait` do nothing: launch list
    and workspace only -- the halo bytes are not real, the values are the sharded tests' business;
  * the production widths, built as tests/test_gpu_production.py builds them (`_seeded_model`, `_inputs`): AuroraPretrained()
    on 181 x 360 and AuroraAirPollution() on 46 x 72, 13 levels, fp32 and autocast, recorded like the golden cases.  The
    golden cases run at embed_dim 64, where most weights are too narrow for the fp16-pair form; at embed_dim 512 every
    pre-split site of the handle (Perceiver layers, score rows, patch embeddings, surface MLP, output heads) is eligible, so
    a changed eligibility rule changes these launch lists.
  * the branches of the Perceiver resampler (csrc/step.hip:resampler) at the smallest shapes that reach them -- SMALL_CASES
    below: the configuration and input builder of tests/test_gpu_encoder_front.py (embed_dim 256, the narrowest width with a
    pre-split to_kv; 16 x 32 grid, the smallest the three stages accept), every record in a handle of its own because the
    tuning switches are read when a handle is created; and the second decoder Perceiver at AuroraAirPollution's widths as
    tests/test_gpu_levels.py builds it.
Every record also carries what the handle says about its range guards after the traced step: `guard_limits` (per word the
smallest limit any launch carried, as float hex, and the number of launches that carried the word), `guard_words` (whole
steps only: the measured words, as float hex) and `front_composed`.
`--f32-gemm MODE` pins AURORA_F32_GEMM=MODE before the library is first called -- the mode is read once per process, hence a
run of its own -- and records AuroraPretrained() on 181 x 360 and the 4-level small case only: with a pinned mode the handle
makes no pre-split buffer and no guarded launch pair, and a pinned mode other than the two-term one is the only way into the
resampler's unguarded linears.
A refactor of the handle (csrc/step.hip, csrc/model*.hip) is done when the files of the two builds are equal.  Printed: one short
line per record -- workspace, launch count, the first 16 hex digits of the sha256 of the launch list and of the output
hashes -- which is what a log keeps; the launch lists themselves are some 150 kB per build.
"""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import aurora_amd  # noqa: E402
from aurora_amd import Batch, Metadata  # noqa: E402
from aurora_amd.engine import native  # noqa: E402
from aurora_amd.engine.engine import Engine, Shard  # noqa: E402
from tests import helpers  # noqa: E402
from tests import test_gpu_encoder_front as front  # noqa: E402
from tests import test_gpu_levels as levels  # noqa: E402
from tests import test_gpu_production as production  # noqa: E402
from tests.golden_cases import CASES  # noqa: E402

BANDS = ((192, 96, 2), (192, 96, 3), (256, 96, 5))
PRODUCTION = (("AuroraPretrained", 181, 360), ("AuroraAirPollution", 46, 72))
SWITCHES = ("AURORA_COMPOSE_FRONT", "AURORA_PERCEIVER_REASSOC", "AURORA_SCORE_WEIGHTS")
ERA5 = front.CASES["era5"]


def small(levels_=front.LEVELS, B=1, **kwargs):
    return dict(ERA5, levels=levels_, B=B, kwargs=dict(ERA5["kwargs"], **kwargs))


# name -> (case, environment of the handle, autocast, factor on the atmospheric anomalies)
SMALL_CASES = {f"small 4 levels compose={c} reassoc={r} scores={s}": (small(), dict(zip(SWITCHES, (c, r, s))), False, 1.0)
               for c in "01" for r in "01" for s in "01"}
SMALL_CASES.update({
    "small 3 levels": (small(levels.LEVELS[3]), {}, False, 1.0),      # re-associated, k | v wider than to_out's result
    "small 5 levels": (small(levels.LEVELS[5]), {}, False, 1.0),      # no perceiver_out kernel: the plain pair
    "small stabilised": (front.CASES["ln_k_q"], {}, False, 1.0),      # key and query LayerNorms, no score rows
    "small depth 2": (small(enc_depth=2, dec_depth=2), {}, False, 1.0),   # the only way to a layer i > 0
    "small level-conditioned": (front.CASES["level_conditioned"], {}, False, 1.0),
    "small B=2": (front.CASES["batch_of_two"], {}, False, 1.0),
    "small one variable absent": (front.CASES["one_variable_absent"], {}, False, 1.0),
    "small anomalies x 1e5": (small(), {}, False, 1e5),               # every guard fails on the device: the fall-backs run
    "small 4 levels": (small(), {}, True, 1.0),                       # bf16 backbone
})


class NoTransport(native._Transport):
    def allocate(self, n_bytes):
        super().allocate(n_bytes)
        self.send.zero_()
        self.recv.zero_()

    def _post(self, *a):
        return 0

    def _wait(self, *a):
        return 0


def build(name, autocast, H=None, W=None):
    case = dict(CASES[name])
    if H:
        case["H"], case["W"] = H, W
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"], autocast=autocast)
    model.load_state_dict(helpers.case_state_dict(model, torch.float32), strict=True)
    model = model.to("cuda").eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    return model, Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))


def build_production(cls_name, H, W, autocast):
    with torch.inference_mode(False):
        model = production._seeded_model(getattr(aurora_amd, cls_name), autocast=autocast)
    cfg = model.config
    batch = production._inputs(cfg, H, W, production.LEVELS13, positive=cfg.positive_surf_vars + cfg.positive_atmos_vars)
    return model, batch.to("cuda")


def build_small(case, env, autocast, scale):
    """The model and batch of tests/test_gpu_encoder_front.py:_case / _run (without its oracle), `env` set for the handle."""
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"], autocast=autocast)
    model.load_state_dict(helpers.case_state_dict(model, torch.float32), strict=True)
    model = model.to("cuda").eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    atmos = {k: v * scale for k, v in atmos.items() if k != case.get("drop")}
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    return model, Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"]))).to("cuda")


def build_second_perceiver():
    """tests/test_gpu_levels.py::test_air_pollution_second_decoder_perceiver_at_four_levels, default switches."""
    cls = aurora_amd.AuroraAirPollution
    with torch.inference_mode(False):
        model = production._seeded_model(cls, autocast=False, **levels.DEPTHS)
    cfg = model.config
    return model, levels._batch(cfg, 181, 360, levels.LEVELS[4], positive=cfg.positive_surf_vars + cfg.positive_atmos_vars).to("cuda")


def guards(nat, words=True):
    limits, counts = nat.guard_limits()
    out = {"guard_limits": [float(v).hex() for v in limits], "guard_launches": list(counts), "front_composed": nat.front_composed()}
    if words:
        out["guard_words"] = [float(v).hex() for v in nat.guard_words()]
    return out


def hashes(pred):
    torch.cuda.synchronize()
    return {f"{kind}.{k}": hashlib.sha256(v.contiguous().cpu().numpy().tobytes()).hexdigest()
            for kind, d in (("surf", pred.surf_vars), ("atmos", pred.atmos_vars)) for k, v in d.items()}


def traced(nat, step):
    """(launch list, workspace bytes, prediction) of one `step()` with every kind profiled."""
    nat.profile_begin()
    pred = step()
    launches = [[kind, work] for kind, _, work in nat.profile_end_list()]
    return launches, nat.workspace_bytes(), pred


def short(x):
    return hashlib.sha256(json.dumps(x, sort_keys=True).encode()).hexdigest()[:16]


def digest(r):
    where = f"{r['case']} {'autocast' if r['autocast'] else 'fp32'}" + (f" rank {r['rank']}/{r['world']}" if "world" in r else "")
    out = f" outputs {short(r['sha256'])} repeatable {r['repeatable']}" if "sha256" in r else ""
    guard = short([r[k] for k in ("guard_limits", "guard_launches", "front_composed")] + [r.get("guard_words")])
    return f"{where}: workspace_bytes {r['workspace_bytes']} launches {r['n_launches']} {short(r['launches'])} guards {guard}{out}"


def whole_step(case, autocast, model, batch):
    """The record of an un-sharded case: a warmed step traced, the next one hashed again."""
    model.forward(batch)
    nat = model.engine().native
    launches, ws, pred = traced(nat, lambda: model.forward(batch))
    h, g = hashes(pred), guards(nat)
    return {"case": case, "autocast": autocast, "workspace_bytes": ws, "n_launches": len(launches),
            "repeatable": hashes(model.forward(batch)) == h, "sha256": h, "launches": launches, **g}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--f32-gemm", choices=("native", "bf16", "f16"),
                    help="pin AURORA_F32_GEMM for this process and record AuroraPretrained() 181 x 360 and the 4-level small case only")
    args = ap.parse_args()
    records = []

    def add(r):   # (printed as it goes: a long run shows where it is)
        records.append(r)
        print(digest(r), flush=True)

    if args.f32_gemm:
        os.environ["AURORA_F32_GEMM"] = args.f32_gemm   # before the first call into the library, which reads it once
    pinned = f" AURORA_F32_GEMM={args.f32_gemm}" if args.f32_gemm else ""
    with torch.inference_mode():
        for cls_name, H, W in PRODUCTION[:1] if args.f32_gemm else PRODUCTION:
            for autocast in (False, True):
                model, batch = build_production(cls_name, H, W, autocast)
                add(whole_step(f"{cls_name} {H}x{W}{pinned}", autocast, model, batch))
                del model
                torch.cuda.empty_cache()
        for name, (case, env, autocast, scale) in SMALL_CASES.items():
            if args.f32_gemm and name != "small 4 levels compose=1 reassoc=1 scores=1":
                continue
            model, batch = build_small(case, env, autocast, scale)
            add(whole_step(name + pinned, autocast, model, batch))
            del model
        for k in SWITCHES:
            os.environ.pop(k, None)
        if not args.f32_gemm:
            model, batch = build_second_perceiver()
            add(whole_step("AuroraAirPollution 181x360 4 levels, one block per stage", False, model, batch))
            del model
            torch.cuda.empty_cache()
        for name in () if args.f32_gemm else CASES:
            for autocast in (False, True):
                model, batch = build(name, autocast)
                add(whole_step(name, autocast, model, batch))
        for H, W, world in () if args.f32_gemm else BANDS:
            for autocast in (False, True):
                model, batch = build("base_pad", autocast, H, W)
                for rank in range(world):
                    model._shard = Shard(rank, world, None, gather_output=False)
                    eng = Engine(model, transport=NoTransport(None, "cuda"))
                    model._shard = None
                    band = eng.local_band(batch)
                    eng.step(band)
                    launches, ws, _ = traced(eng.native, lambda: eng.step(band))
                    add({"case": f"base_pad {H}x{W}", "autocast": autocast, "world": world, "rank": rank,
                                    "workspace_bytes": ws, "n_launches": len(launches), "launches": launches,
                                    **guards(eng.native, words=False)})
    torch.cuda.synchronize()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(r, sort_keys=True) + "\n" for r in records))
    flaky = [f"{r['case']} autocast={r['autocast']}" for r in records if r.get("repeatable") is False]
    print(f"{len(records)} records; not repeatable within one process: {flaky or 'none'}")


if __name__ == "__main__":
    main()
