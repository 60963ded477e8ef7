"""Model-level parity per variable and level, in units of that entry's `normalisation.scales`.

`helpers.rel_err` / `helpers.mean_rel_err` divide by the max / mean of a whole variable in physical units, so the location
term (280 K, 1e5 Pa, 5e4 m^2/s^2) and the largest level set the denominator: under mean-rel <= 1e-4 and max-rel <= 1e-3 the
humidity head at 100 hPa may be 34 sigma off.  Here every surface variable and every (atmospheric variable, level) is an
entry of its own, key `msl` / `q_100`, with max and mean of |pred - ref| / scale in fp64 and the position of the max.

The bound of an entry comes from the reference's own fp32 error, never from the engine's:

    bound = MARGIN * max(what the fp32 oracle deviates from the same reference by,
                         one fp32 ulp of max|ref| of that entry / scale)

The oracle's deviation on one seed is a sample of fp32 rounding, not a bound: two correct fp32 implementations that sum in
different orders move the max by a small factor, hence MARGIN = 4.  The ulp term is the rounding floor of an fp32 output
(5.9e-6 sigma for msl).  The same formula holds the mean.

NaN (ocean-wave outputs) as `helpers.nan_agreement`: values are compared where both are finite, and the masks may differ on
at most FLIPPED_CAP of an entry's points (a density logit within rounding of 0 may legitimately flip).

Worst measured engine / oracle ratio per golden case (max error of an entry over max(oracle error, ulp floor); the bound is
at MARGIN), fp32 engine on an MI355X through `rollout`, every step: base_pad 1.50, small_b2 1.10, lora_all 2.00,
stabilised_12h 1.37, patch10 1.33, air_pollution 1.77, wave 3.00.  bf16 against 3x the oracle's autocast deviation: 0.82
(base_pad, small_b2), 0.77 (lora_all).  Stitched bands against the un-sharded step: fp32 at most 1.11 of the fp32 baseline,
bf16 0.00 of the autocast baseline; at the production widths (tests/test_gpu_sharded_widths.py) fp32 bit for bit, bf16 at most
0.19 of the 3x autocast bound.  Through the C ABI: with torch tables the same figures as through `rollout` (lora_all 2.00,
air_pollution 1.77, wave 2.18); with the handle's own tables against the oracle on those tables at most 2.83 (wave), lora_all 1.39,
air_pollution 1.66 -- against the GOLDEN those two reach 5.0 and 4.5, because their tables are other inputs (see below).
Levels and production tests against the oracle in fp64: at most 2.08 (Aurora*Pretrained), 1.89 (AuroraHighRes), 3.38 (AuroraAirPollution 181 x 360, 4 levels), 2.26 of 5 on 361 x 720.
"""
from __future__ import annotations

import contextlib
import dataclasses
import functools
from typing import Mapping, Sequence

import numpy as np
import torch

from aurora_amd import normalisation
from oracle import aurora_oracle as oracle
from tests import helpers
from tests.golden_cases import CASES

MARGIN = 4.0
FLIPPED_CAP = 2e-3      # tests/test_gpu_model.py::test_fp32_engine_matches_reference_golden


@dataclasses.dataclass(frozen=True)
class Entry:
    max: float                      # max |pred - ref| / scale over the points where both are finite
    mean: float                     # mean of the same
    where: tuple[int, int, int, int]  # (b, t, row, col) of the max
    flipped: float                  # fraction of points where exactly one of pred, ref is NaN
    floor: float                    # one fp32 ulp of max|ref| / scale


Fields = Mapping[str, torch.Tensor]     # "surf.<var>" -> (B, T, H, W), "atmos.<var>" -> (B, T, C, H, W)


def fields(surf: Fields, atmos: Fields) -> dict[str, torch.Tensor]:
    return {**{f"surf.{k}": v for k, v in surf.items()}, **{f"atmos.{k}": v for k, v in atmos.items()}}


def golden_step(gold: Mapping[str, np.ndarray], step: int) -> dict[str, torch.Tensor]:
    """The fields of one roll-out step of a golden file (keys `s<step>.surf.<var>`)."""
    pre = f"s{step}."
    return {k[len(pre):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(pre)}


def _entry(p: torch.Tensor, r: torch.Tensor, scale: float) -> Entry:
    p, r = p.detach().cpu().double(), r.detach().cpu().double()
    assert p.shape == r.shape and p.dim() == 4, (p.shape, r.shape)
    both = ~torch.isnan(p) & ~torch.isnan(r)
    flipped = (torch.isnan(p) ^ torch.isnan(r)).double().mean().item()
    if not both.any():
        return Entry(0.0, 0.0, (0, 0, 0, 0), flipped, 0.0)
    err = torch.where(both, (p - r).abs() / scale, torch.full_like(p, -1.0))
    flat = int(err.argmax())
    where = tuple(int(i) for i in np.unravel_index(flat, tuple(err.shape)))
    top = float(np.float32(r[both].abs().max().item()))
    floor = float(np.spacing(np.float32(top))) / scale
    return Entry(err.flatten()[flat].item(), err[both].mean().item(), where, flipped, floor)


def per_level_errors(pred: Fields, ref: Fields, levels: Sequence[float]) -> dict[str, Entry]:
    """One Entry per surface variable (key = its name) and per atmospheric variable and level (key `<var>_<level>`)."""
    assert set(pred) == set(ref), (sorted(pred), sorted(ref))
    out = {}
    for name, r in ref.items():
        kind, var = name.split(".", 1)
        p = pred[name]
        assert p.shape == r.shape, (name, p.shape, r.shape)
        if kind == "surf":
            out[var] = _entry(p, r, normalisation.scales[var])
        else:
            assert r.shape[2] == len(levels), (name, r.shape, levels)
            for i, lv in enumerate(levels):
                key = f"{var}_{normalisation.level_to_str(lv)}"
                out[key] = _entry(p[:, :, i], r[:, :, i], normalisation.scales[key])
    return out


def bounds(baseline: Mapping[str, Entry], margin: float = MARGIN, floor: Mapping[str, tuple[float, float]] | None = None):
    """key -> (max bound, mean bound) = margin * max(baseline, ulp floor); `floor` (key -> bounds) replaces the ulp floor."""
    out = {}
    for k, e in baseline.items():
        if floor is None:
            out[k] = (margin * max(e.max, e.floor), margin * max(e.mean, e.floor))
        else:
            out[k] = (max(margin * e.max, floor[k][0]), max(margin * e.mean, floor[k][1]))
    return out


def failures(errors: Mapping[str, Entry], bound: Mapping[str, tuple[float, float]]) -> list[str]:
    """One line per entry outside its bound: which variable and level, by how much, and where."""
    assert set(errors) == set(bound), (sorted(errors), sorted(bound))
    bad = []
    for k, e in errors.items():
        bmax, bmean = bound[k]
        if e.flipped > FLIPPED_CAP:
            bad.append(f"{k}: NaN masks differ on {e.flipped:.2e} of the points (cap {FLIPPED_CAP:.0e})")
        if not (e.max <= bmax) or not (e.mean <= bmean):
            bad.append(f"{k}: max {e.max:.3e} sigma at (b, t, row, col) = {e.where} (bound {bmax:.3e}), "
                       f"mean {e.mean:.3e} (bound {bmean:.3e})")
    return bad


def report(what: str, errors: Mapping[str, Entry], baseline: Mapping[str, Entry]) -> float:
    """Print engine / baseline per entry; returns the worst ratio of max errors (the bound sits at the margin)."""
    worst = 0.0
    for k, e in errors.items():
        base = max(baseline[k].max, baseline[k].floor)
        ratio = e.max / base if base > 0 else 0.0
        worst = max(worst, ratio)
        print(f"  {what} {k}: max {e.max:.3e} mean {e.mean:.3e} sigma; baseline max {baseline[k].max:.3e} "
              f"mean {baseline[k].mean:.3e} floor {baseline[k].floor:.3e}; ratio {ratio:.2f}")
    print(f"{what}: worst max-error ratio over the baseline {worst:.2f}")
    return worst


def check(what: str, pred: Fields, ref: Fields, levels: Sequence[float], baseline: Mapping[str, Entry],
          margin: float = MARGIN, floor=None) -> float:
    """Print every ratio, then assert every entry of pred against ref within margin * baseline (see `bounds`)."""
    errors = per_level_errors(pred, ref, levels)
    worst = report(what, errors, baseline)
    bad = failures(errors, bounds(baseline, margin, floor))
    assert not bad, f"{what}: " + "; ".join(bad)
    return worst


# ---- the fp32 oracle against the goldens ----------------------------------------------------------------------------
def handle_tables(dim: int, lat: torch.Tensor, lon: torch.Tensor, patch: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The position / scale tables a handle derives from lat / lon when its grid carries none (aurora_hip_pos_scale_encoding:
    host-only code, runs without a GPU), in the form of `oracle.pos_scale_encodings`."""
    import numpy as np
    from aurora_amd.engine import lib

    assert lat.dim() == 1 and lon.dim() == 1
    la, lo = np.ascontiguousarray(lat.double().numpy()), np.ascontiguousarray(lon.double().numpy())
    n = (len(la) // patch) * (len(lo) // patch)
    pos, scale = np.empty((n, dim), np.float32), np.empty((n, dim), np.float32)
    L = lib.load()
    code = L.aurora_hip_pos_scale_encoding(la.ctypes.data_as(lib._PD), lo.ctypes.data_as(lib._PD), len(la), len(lo), patch, dim,
                                           pos.ctypes.data_as(lib._PF), scale.ctypes.data_as(lib._PF))
    assert code == 0, L.aurora_hip_last_error()
    return torch.from_numpy(pos), torch.from_numpy(scale)


@contextlib.contextmanager
def _oracle_takes_handle_tables():
    plain = oracle.pos_scale_encodings
    oracle.pos_scale_encodings = handle_tables
    try:
        yield
    finally:
        oracle.pos_scale_encodings = plain


@functools.lru_cache(maxsize=None)
def oracle_rollout(case_name: str, dtype: torch.dtype = torch.float32, autocast: bool = False,
                   own_tables: bool = False) -> tuple[dict[str, torch.Tensor], ...]:
    """The oracle on the case's weights in `dtype`, rolled forward as the golden recipe does (`oracle.rollout`): one dict of
    fields per step.  `own_tables`: with the handle's tables in place of its own.  Computed once; read-only."""
    case, model = helpers.case_model_meta(case_name)
    sd = helpers.case_state_dict(model, dtype)
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    with torch.inference_mode(), (_oracle_takes_handle_tables() if own_tables else contextlib.nullcontext()):
        gen = oracle.rollout(sd, model.config, surf, static, atmos, lat, lon, times, case["levels"], case["steps"],
                             normalisation.locations, normalisation.scales, autocast=autocast, variant=model.variant)
        return tuple(fields(sp, ap) for sp, ap, _ in gen)


def oracle_fp32_rollout(case_name: str, autocast: bool = False) -> tuple[dict[str, torch.Tensor], ...]:
    return oracle_rollout(case_name, torch.float32, autocast)


@functools.lru_cache(maxsize=None)
def golden(case_name: str) -> tuple[dict[str, torch.Tensor], ...]:
    gold = helpers.load_golden(case_name)
    return tuple(golden_step(gold, s) for s in range(CASES[case_name]["steps"]))


@functools.lru_cache(maxsize=None)
def oracle_fp32_errors(case_name: str, step: int) -> dict[str, Entry]:
    """What the fp32 oracle deviates from the golden of that case and step by: the baseline of every fp32 bound."""
    return per_level_errors(oracle_fp32_rollout(case_name)[step], golden(case_name)[step], CASES[case_name]["levels"])


@functools.lru_cache(maxsize=None)
def oracle_autocast_errors(case_name: str, step: int) -> dict[str, Entry]:
    """The same for the oracle's own bf16 path (CPU autocast of the backbone): the baseline of the bf16 bounds."""
    return per_level_errors(oracle_fp32_rollout(case_name, True)[step], golden(case_name)[step], CASES[case_name]["levels"])


def fp32_bounds(case_name: str, step: int):
    return bounds(oracle_fp32_errors(case_name, step))


def check_fp32(what: str, pred: Fields, case_name: str, step: int, ref: Fields | None = None) -> float:
    """A prediction of golden case `case_name`, step `step`, against the golden within the case's fp32 bound.  `ref`: another
    fp32-grade evaluation of the same model (any grid) in place of the golden, held to the same per-entry bound."""
    return check(what, pred, golden(case_name)[step] if ref is None else ref, CASES[case_name]["levels"],
                 oracle_fp32_errors(case_name, step))


def check_autocast(what: str, pred: Fields, case_name: str, step: int, ref: Fields | None = None, margin: float = 3.0) -> float:
    """A bf16-backbone prediction against the golden (or `ref`): within `margin` times what the oracle's autocast run deviates
    from the golden by, per entry, and never held tighter than the entry's fp32 bound."""
    return check(what, pred, golden(case_name)[step] if ref is None else ref, CASES[case_name]["levels"],
                 oracle_autocast_errors(case_name, step), margin=margin, floor=fp32_bounds(case_name, step))


# ---- a handle that computes its own position / scale tables ---------------------------------------------------------------
# The patch root areas are fp32 upstream, and the scale expansion's shortest wavelength (1.1e-4 km against roots of hundreds of
# km) turns a last-bit difference into radians of phase; the handle's own tables take those fp32 steps through libm, not torch
# (aurora_amd/csrc/model_grid.hip:pos_scale_tables, tests/test_encodings.py), so on some grids they are OTHER inputs than the
# golden's, and the model's answer to them is not the golden.  Such a forecast is therefore compared like for like: with the
# oracle in fp64 ON THE HANDLE'S TABLES, within MARGIN of what the fp32 oracle on the same tables deviates from it by.
@functools.lru_cache(maxsize=None)
def own_tables_errors(case_name: str, step: int) -> dict[str, Entry]:
    return per_level_errors(oracle_rollout(case_name, torch.float32, False, True)[step],
                            oracle_rollout(case_name, torch.float64, False, True)[step], CASES[case_name]["levels"])


def check_own_tables(what: str, pred: Fields, case_name: str, step: int) -> float:
    return check(what, pred, oracle_rollout(case_name, torch.float64, False, True)[step], CASES[case_name]["levels"],
                 own_tables_errors(case_name, step))
