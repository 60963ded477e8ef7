"""The argument errors and the host numbers of the seven verification front ends -- `scores`, `ensemble_scores`,
`event_scores`, `probability_scores`, `spectra`, `FieldStats`, `diagnostics` -- pinned as literals (no GPU needed).

`CASES` drives every `raise` of the public entry points that the CPU can reach, on 5 x 8 grids; `MESSAGES` holds the exception
type and the exact text each case gave BEFORE the front ends were moved onto `aurora_amd/_fields.py`, so a shared helper
cannot reword a module's message unnoticed.  `DIGESTS` holds the sha256 of the raw bytes of every result tensor of one
fixed small input per entry point, recorded at the same commit.  To record again after a deliberate change:

    python tests/test_verification_messages.py

The checks of the device branch (float32 fields, row-major planes) cannot be reached without a GPU through the public
functions; `test_device_checks_keep_their_texts` calls the shared placement function with CPU tensors standing in for one
device and compares with the literals of the modules' earlier source.  `test_device_table_cache` pins the policy of the one
device-table cache."""
import dataclasses
import hashlib
import sys
from datetime import datetime
from pathlib import Path

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from aurora_amd import (Batch, FieldStats, Metadata, diagnostics, ensemble_scores, event_scores, probability_scores, scores,  # noqa: E402
                        spectra)
from aurora_amd.batch import BandBatch  # noqa: E402
from aurora_amd.scores import latitude_weights  # noqa: E402

TIME = (datetime(2022, 5, 11, 12),)


def fill(shape, seed: int) -> torch.Tensor:
    """Exactly representable float32 values around 280, a fixed function of the index and the seed."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return torch.from_numpy((270.0 + ((i * 7919 + seed * 104729) % 1013) / 32.0).astype(np.float32).reshape(shape))


def coords(n_lat: int, n_lon: int):
    lat = torch.linspace(80, -80, n_lat, dtype=torch.float64) if n_lat > 1 else torch.tensor([10.0], dtype=torch.float64)
    return lat, torch.arange(n_lon, dtype=torch.float64) * (360.0 / n_lon)


def mk(surf=("2t",), atmos=("z",), n_lat=5, n_lon=8, B=1, C=2, levels=None, seed=0, lat=None, lon=None) -> Batch:
    la, lo = coords(n_lat, n_lon)
    md = Metadata(la if lat is None else lat, lo if lon is None else lon, TIME, tuple(levels or (500, 850)[:C]))
    s = {k: fill((B, 2, n_lat, n_lon), seed + 10 * i) for i, k in enumerate(surf)}
    a = {k: fill((B, 2, C, n_lat, n_lon), seed + 10 * i + 5) for i, k in enumerate(atmos)}
    return Batch(s, {}, a, md)


def band(b: Batch) -> BandBatch:
    return BandBatch(b.surf_vars, {}, b.atmos_vars, b.metadata, full_patch_rows=4, band=(0, 4))


def matrices(b: Batch) -> Batch:
    n_lat, n_lon = b.metadata.lat.shape[0], b.metadata.lon.shape[0]
    md = Metadata(b.metadata.lat[:, None].expand(n_lat, n_lon), b.metadata.lon[None, :].expand(n_lat, n_lon), TIME,
                  b.metadata.atmos_levels)
    return dataclasses.replace(b, metadata=md)


def moved(b: Batch, lat=None, lon=None, levels=None) -> Batch:
    """The same fields under other coordinates."""
    md = Metadata(b.metadata.lat if lat is None else lat, b.metadata.lon if lon is None else lon, TIME,
                  b.metadata.atmos_levels if levels is None else levels)
    return dataclasses.replace(b, metadata=md)


def with_var(b: Batch, group: str, name: str, t: torch.Tensor) -> Batch:
    return dataclasses.replace(b, **{group: {**getattr(b, group), name: t}})


def on_meta(b: Batch) -> Batch:
    """The fields on the `meta` device (the coordinates stay): a second device without a GPU."""
    f = lambda d: {k: v.to("meta") for k, v in d.items()}  # noqa: E731
    return Batch(f(b.surf_vars), {}, f(b.atmos_vars), b.metadata)


def shifted_lat(n_lat=5):
    return torch.linspace(70, -70, n_lat, dtype=torch.float64)


def shifted_lon(n_lon=8):
    return torch.arange(n_lon, dtype=torch.float64) * (360.0 / n_lon) + 1.0


def members(M=3, **kw):
    return [mk(seed=m + 1, **kw) for m in range(M)]


THR = {"2t": [280.0], "z": [280.0]}


def pair_cases(fn, call, clim: bool):
    """The cases every (pred, truth) front end shares; `call(pred, truth)`."""
    p = mk
    out = {
        "pred_band": lambda: call(band(p()), p(seed=1)),
        "truth_band": lambda: call(p(), band(p(seed=1))),
        "pred_matrices": lambda: call(matrices(p()), p(seed=1)),
        "truth_matrices": lambda: call(p(), matrices(p(seed=1))),
        "lat_length": lambda: call(p(), p(n_lat=7)),
        "lat_length_crop_hint": lambda: call(p(), p(n_lat=6)),
        "lat_values": lambda: call(p(), moved(p(seed=1), lat=shifted_lat())),
        "lon_length": lambda: call(p(), p(n_lon=9)),
        "lon_values": lambda: call(p(), moved(p(seed=1), lon=shifted_lon())),
        "levels": lambda: call(p(), moved(p(seed=1), levels=(500, 700))),
        "both_groups": lambda: call(with_var(p(), "atmos_vars", "2t", fill((1, 2, 2, 5, 8), 3)),
                                    with_var(p(seed=1), "atmos_vars", "2t", fill((1, 2, 2, 5, 8), 4))),
        "pred_rank": lambda: call(with_var(p(), "surf_vars", "2t", fill((1, 2, 2, 5, 8), 3)), p(seed=1)),
        "truth_grid": lambda: call(p(), with_var(p(seed=1), "surf_vars", "2t", fill((1, 2, 5, 7), 3))),
        "batch_size": lambda: call(p(), p(seed=1, B=2)),
        "shape": lambda: call(p(), with_var(p(seed=1), "atmos_vars", "z", fill((1, 2, 3, 5, 8), 3))),
        "devices": lambda: call(p(), on_meta(p(seed=1))),
    }
    return {f"{fn}.{k}": v for k, v in out.items()}


def ensemble_cases(fn, call):
    """The cases both members-against-truth front ends share; `call(members, truth)`."""
    t = lambda **kw: mk(seed=0, **kw)  # noqa: E731
    out = {
        "truth_band": lambda: call(members(), band(t())),
        "truth_not_batch": lambda: call(members(), 3),
        "member_not_batch": lambda: call([mk(seed=1), "x", mk(seed=2)], t()),
        "one_member": lambda: call(members(1), t()),
        "65_members": lambda: call([mk(seed=1)] * 65, t()),
        "member_band": lambda: call([mk(seed=1), band(mk(seed=2))], t()),
        "member_matrices": lambda: call([matrices(mk(seed=1)), mk(seed=2)], t()),
        "truth_matrices": lambda: call(members(), matrices(t())),
        "lat_length": lambda: call(members(), t(n_lat=7)),
        "lat_length_crop_hint": lambda: call(members(), t(n_lat=6)),
        "lat_values": lambda: call([mk(seed=1), moved(mk(seed=2), lat=shifted_lat())], t()),
        "lon_length": lambda: call(members(), t(n_lon=9)),
        "lon_values": lambda: call(members(), moved(t(), lon=shifted_lon())),
        "levels": lambda: call(members(), moved(t(), levels=(500, 700))),
        "one_batch_band": lambda: call(band(mk(B=3)), t()),
        "one_batch_lat_crop_hint": lambda: call(mk(B=3), t(n_lat=6)),
        "one_batch_lon_values": lambda: call(mk(B=3), moved(t(), lon=shifted_lon())),
        "one_batch_levels": lambda: call(mk(B=3), moved(t(), levels=(500, 700))),
        "both_groups": lambda: call([with_var(mk(seed=m), "atmos_vars", "2t", fill((1, 2, 2, 5, 8), 3)) for m in (1, 2)],
                                    with_var(t(), "atmos_vars", "2t", fill((1, 2, 2, 5, 8), 4))),
        "truth_rank": lambda: call(members(), with_var(t(), "surf_vars", "2t", fill((1, 2, 2, 5, 8), 3))),
        "member_grid": lambda: call([mk(seed=1), with_var(mk(seed=2), "surf_vars", "2t", fill((1, 2, 5, 7), 3))], t()),
        "one_batch_grid": lambda: call(with_var(mk(B=3), "surf_vars", "2t", fill((3, 2, 4, 8), 3)), t()),
        "one_batch_truth_batch": lambda: call(mk(B=3), t(B=2)),
        "one_batch_shape": lambda: call(with_var(mk(B=3), "atmos_vars", "z", fill((3, 2, 3, 5, 8), 3)), t()),
        "batch_size": lambda: call([mk(seed=1), mk(seed=2, B=2)], t()),
        "shape": lambda: call([mk(seed=1), with_var(mk(seed=2), "atmos_vars", "z", fill((1, 2, 3, 5, 8), 3))], t()),
        "one_batch_one_member": lambda: call(mk(B=1, seed=1), t()),
        "one_batch_65_members": lambda: call(mk(B=65, seed=1), t()),
        "one_batch_sizes_differ": lambda: call(with_var(mk(B=3), "surf_vars", "2t", fill((4, 2, 5, 8), 3)), t()),
        "devices": lambda: call(members(), on_meta(t())),
        "one_batch_devices": lambda: call(on_meta(mk(B=3)), t()),
    }
    return {f"{fn}.{k}": v for k, v in out.items()}


def threshold_cases(fn, call):
    """`call(thresholds)` on a (2t; z) pair or ensemble."""
    out = {
        "thresholds_not_mapping": lambda: call([1.0]),
        "thresholds_empty": lambda: call({}),
        "thresholds_not_numbers": lambda: call({"2t": ["a"]}),
        "thresholds_surface_2d": lambda: call({"2t": np.zeros((2, 2))}),
        "thresholds_levels": lambda: call({"z": np.zeros((3, 2))}),
        "thresholds_3d": lambda: call({"z": np.zeros((2, 2, 2))}),
        "thresholds_scalar": lambda: call({"2t": 1.0}),
        "thresholds_none": lambda: call({"2t": []}),
        "thresholds_nine": lambda: call({"2t": list(range(9))}),
        "thresholds_unknown": lambda: call({"2t": [1.0], "msl": [1.0]}),
    }
    return {f"{fn}.{k}": v for k, v in out.items()}


def stats(thresholds=None, derived=(), first=None, **kw):
    s = FieldStats(thresholds, derived=derived, **kw)
    if first is not None:
        s.update(first)
    return s


WIND = dict(surf=("10u", "10v"), atmos=("u", "v", "q"))

CASES = {
    **pair_cases("scores", scores, True),
    "scores.no_common": lambda: scores(mk(), mk(surf=("msl",), atmos=("t",))),
    "scores.climatology_band": lambda: scores(mk(), mk(seed=1), band(mk(seed=2))),
    "scores.climatology_lat_crop_hint": lambda: scores(mk(), mk(seed=1), mk(seed=2, n_lat=6)),
    "scores.climatology_lon_values": lambda: scores(mk(), mk(seed=1), moved(mk(seed=2), lon=shifted_lon())),
    "scores.climatology_levels": lambda: scores(mk(), mk(seed=1), moved(mk(seed=2), levels=(500, 700))),
    "scores.climatology_lacks_surface": lambda: scores(mk(), mk(seed=1), mk(seed=2, surf=())),
    "scores.climatology_lacks_atmospheric": lambda: scores(mk(), mk(seed=1), mk(seed=2, atmos=())),
    "scores.climatology_grid": lambda: scores(mk(), mk(seed=1), with_var(mk(seed=2), "surf_vars", "2t", fill((1, 2, 5, 7), 3))),
    "scores.climatology_batch_size": lambda: scores(mk(), mk(seed=1), mk(seed=2, B=2)),
    "scores.climatology_shape": lambda: scores(mk(), mk(seed=1), with_var(mk(seed=2), "atmos_vars", "z", fill((1, 2, 3, 5, 8), 3))),
    "scores.climatology_devices": lambda: scores(mk(), mk(seed=1), on_meta(mk(seed=2))),
    "latitude_weights.matrix": lambda: latitude_weights(np.zeros((2, 2))),
    "latitude_weights.empty": lambda: latitude_weights([]),
    "latitude_weights.range": lambda: latitude_weights([0.0, 91.0]),
    "latitude_weights.nan": lambda: latitude_weights([0.0, float("nan")]),
    "latitude_weights.poles": lambda: latitude_weights(np.array([90.0, -90.0]) * (1 + 2.0 ** -52)),

    **ensemble_cases("ensemble_scores", ensemble_scores),
    "ensemble_scores.no_common": lambda: ensemble_scores(members(), mk(surf=("msl",), atmos=("t",))),

    **pair_cases("event_scores", lambda p, t: event_scores(p, t, THR), False),
    **threshold_cases("event_scores", lambda thr: event_scores(mk(), mk(seed=1), thr)),
    "event_scores.longitudes": lambda: event_scores(mk(n_lat=2, n_lon=4097, surf=(), atmos=()), mk(n_lat=2, n_lon=4097, surf=(), atmos=()), THR),
    "event_scores.scales_not_sequence": lambda: event_scores(mk(), mk(seed=1), THR, scales=3),
    "event_scores.scales_fraction": lambda: event_scores(mk(), mk(seed=1), THR, scales=(1, 2.5)),
    "event_scores.scales_bool": lambda: event_scores(mk(), mk(seed=1), THR, scales=(True,)),
    "event_scores.scales_even": lambda: event_scores(mk(), mk(seed=1), THR, scales=(1, 4)),
    "event_scores.scales_range": lambda: event_scores(mk(), mk(seed=1), THR, scales=(1, 65)),
    "event_scores.scales_wider": lambda: event_scores(mk(), mk(seed=1), THR, scales=(1, 9)),
    "event_scores.scales_twice": lambda: event_scores(mk(), mk(seed=1), THR, scales=(3, 3)),
    "event_scores.scales_nine": lambda: event_scores(mk(n_lon=32), mk(n_lon=32, seed=1), THR, scales=range(3, 21, 2)),

    **ensemble_cases("probability_scores", lambda m, t: probability_scores(m, t, THR)),
    **threshold_cases("probability_scores", lambda thr: probability_scores(members(), mk(), thr)),
    "probability_scores.thresholds_unknown_one_batch": lambda: probability_scores(mk(B=3), mk(), {"msl": [1.0]}),

    **pair_cases("spectra", spectra, False),
    "spectra.no_common": lambda: spectra(mk(), mk(surf=("msl",), atmos=("t",))),
    "spectra.no_variable": lambda: spectra(mk(surf=(), atmos=())),
    "spectra.alone_band": lambda: spectra(band(mk())),
    "spectra.alone_matrices": lambda: spectra(matrices(mk())),
    "spectra.alone_both_groups": lambda: spectra(with_var(mk(), "atmos_vars", "2t", fill((1, 2, 2, 5, 8), 3))),
    "spectra.alone_rank": lambda: spectra(with_var(mk(), "surf_vars", "2t", fill((1, 2, 2, 5, 8), 3))),
    "spectra.alone_devices": lambda: spectra(with_var(mk(), "surf_vars", "2t", fill((1, 2, 5, 8), 3).to("meta"))),
    "spectra.bands_not_pairs": lambda: spectra(mk(), bands=[1.0]),
    "spectra.bands_none": lambda: spectra(mk(), bands=[]),
    "spectra.bands_nine": lambda: spectra(mk(), bands=[(-10, 10)] * 9),
    "spectra.bands_order": lambda: spectra(mk(), bands=[(10, -10)]),
    "spectra.one_longitude": lambda: spectra(mk(n_lon=1)),
    "spectra.longitudes": lambda: spectra(mk(n_lat=2, n_lon=4097, surf=(), atmos=())),
    "spectra.longitudes_regional": lambda: spectra(moved(mk(), lon=torch.arange(8, dtype=torch.float64) * 10.0)),

    "FieldStats.thresholds_not_mapping": lambda: FieldStats([1.0]),
    "FieldStats.derived_unknown": lambda: FieldStats(derived=("vo",)),
    "FieldStats.over": lambda: stats().update(mk(), over="time"),
    "FieldStats.batch_band": lambda: stats().update(band(mk())),
    "FieldStats.minus_band": lambda: stats().update(mk(), minus=band(mk(seed=1))),
    "FieldStats.batch_not_batch": lambda: stats().update(3),
    "FieldStats.minus_not_batch": lambda: stats().update(mk(), minus=3),
    "FieldStats.batch_matrices": lambda: stats().update(matrices(mk())),
    "FieldStats.minus_matrices": lambda: stats().update(mk(), minus=matrices(mk(seed=1))),
    "FieldStats.minus_lat_length": lambda: stats().update(mk(), minus=mk(n_lat=7)),
    "FieldStats.minus_lat_crop_hint": lambda: stats().update(mk(), minus=mk(n_lat=6)),
    "FieldStats.minus_lat_values": lambda: stats().update(mk(), minus=moved(mk(seed=1), lat=shifted_lat())),
    "FieldStats.minus_lon_length": lambda: stats().update(mk(), minus=mk(n_lon=9)),
    "FieldStats.minus_lon_values": lambda: stats().update(mk(), minus=moved(mk(seed=1), lon=shifted_lon())),
    "FieldStats.minus_levels": lambda: stats().update(mk(), minus=moved(mk(seed=1), levels=(500, 700))),
    "FieldStats.batch_rank": lambda: stats().update(with_var(mk(), "surf_vars", "2t", fill((1, 2, 2, 5, 8), 3))),
    "FieldStats.minus_grid": lambda: stats().update(mk(), minus=with_var(mk(seed=1), "surf_vars", "2t", fill((1, 2, 5, 7), 3))),
    "FieldStats.holds_derived": lambda: stats(derived=("10ws",)).update(mk(surf=("10u", "10v", "10ws"))),
    "FieldStats.reference_of_derived": lambda: stats(derived=("10ws",)).update(mk(**WIND), minus=mk(seed=1, **WIND)),
    "FieldStats.derived_components": lambda: stats(derived=("ws",)).update(mk(surf=("10u",), atmos=("u",))),
    "FieldStats.both_groups": lambda: stats().update(with_var(mk(), "atmos_vars", "2t", fill((1, 2, 2, 5, 8), 3))),
    "FieldStats.no_variable": lambda: stats().update(mk(surf=(), atmos=())),
    "FieldStats.batch_sizes": lambda: stats().update(with_var(mk(B=2), "surf_vars", "msl", fill((3, 2, 5, 8), 3))),
    "FieldStats.over_batch_one": lambda: stats().update(mk(), over="batch"),
    "FieldStats.over_batch_65": lambda: stats().update(mk(B=65), over="batch"),
    "FieldStats.minus_lacks": lambda: stats().update(mk(), minus=mk(seed=1, surf=())),
    "FieldStats.minus_batch_size": lambda: stats().update(mk(B=2), minus=mk(seed=1)),
    "FieldStats.minus_shape": lambda: stats().update(mk(), minus=with_var(mk(seed=1), "atmos_vars", "z", fill((1, 2, 3, 5, 8), 3))),
    "FieldStats.minus_over_batch": lambda: stats().update(mk(B=3), over="batch", minus=mk(seed=1, B=3)),
    "FieldStats.devices": lambda: stats().update(mk(), minus=on_meta(mk(seed=1))),
    "FieldStats.thresholds_not_numbers": lambda: stats({"2t": ["a"]}).update(mk()),
    "FieldStats.thresholds_surface_2d": lambda: stats({"2t": np.zeros((2, 2))}).update(mk()),
    "FieldStats.thresholds_levels": lambda: stats({"z": np.zeros((3, 2))}).update(mk()),
    "FieldStats.thresholds_3d": lambda: stats({"z": np.zeros((2, 2, 2))}).update(mk()),
    "FieldStats.thresholds_none": lambda: stats({"2t": []}).update(mk()),
    "FieldStats.thresholds_nine": lambda: stats({"2t": list(range(9))}).update(mk()),
    "FieldStats.thresholds_unknown": lambda: stats({"msl": [1.0]}).update(mk()),
    "FieldStats.later_lat_length": lambda: stats(first=mk()).update(mk(n_lat=6)),
    "FieldStats.later_lat_values": lambda: stats(first=mk()).update(moved(mk(seed=1), lat=shifted_lat())),
    "FieldStats.later_lon_length": lambda: stats(first=mk()).update(mk(n_lon=9)),
    "FieldStats.later_lon_values": lambda: stats(first=mk()).update(moved(mk(seed=1), lon=shifted_lon())),
    "FieldStats.later_levels": lambda: stats(first=mk()).update(moved(mk(seed=1), levels=(500, 700))),
    "FieldStats.later_variables": lambda: stats(first=mk()).update(mk(surf=("msl",))),
    "FieldStats.later_batch_size": lambda: stats(first=mk()).update(mk(B=2)),
    "FieldStats.later_shape": lambda: stats(first=mk()).update(with_var(mk(seed=1), "atmos_vars", "z", fill((1, 2, 3, 5, 8), 3))),
    "FieldStats.no_update": lambda: stats().mean,
    "FieldStats.no_thresholds": lambda: stats(first=mk()).exceed_count,
    "FieldStats.no_thresholds_fraction": lambda: stats(first=mk()).exceed_fraction,
    "FieldStats.as_batch": lambda: stats(first=mk()).as_batch("median"),

    "diagnostics.band": lambda: diagnostics(band(mk(**WIND)), "ws"),
    "diagnostics.not_batch": lambda: diagnostics(3, "ws"),
    "diagnostics.matrices": lambda: diagnostics(matrices(mk(**WIND)), "ws"),
    "diagnostics.unknown": lambda: diagnostics(mk(**WIND), ("ws", "pv")),
    "diagnostics.nothing": lambda: diagnostics(mk(**WIND), ()),
    "diagnostics.one_latitude": lambda: diagnostics(mk(n_lat=1, **WIND), "ws"),
    "diagnostics.longitudes": lambda: diagnostics(moved(mk(**WIND), lon=torch.tensor([0.0, 10, 20, 30, 40, 50, 60, 75], dtype=torch.float64)), "ws"),
    "diagnostics.already_held": lambda: diagnostics(mk(surf=("10u", "10v"), atmos=("u", "v", "ws")), "ws"),
    "diagnostics.component_missing": lambda: diagnostics(mk(surf=("10u",), atmos=("u", "v")), "10vo"),
    "diagnostics.rank": lambda: diagnostics(with_var(mk(**WIND), "atmos_vars", "u", fill((1, 2, 5, 8), 3)), "ws"),
    "diagnostics.grid": lambda: diagnostics(with_var(mk(**WIND), "surf_vars", "10v", fill((1, 2, 5, 7), 3)), "10d"),
    "diagnostics.batch_sizes": lambda: diagnostics(with_var(mk(**WIND), "atmos_vars", "v", fill((2, 2, 2, 5, 8), 3)), "vo"),
    "diagnostics.level_counts": lambda: diagnostics(with_var(mk(**WIND), "atmos_vars", "v", fill((1, 2, 3, 5, 8), 3)), "vo"),
    "diagnostics.metadata_levels": lambda: diagnostics(moved(mk(**WIND), levels=(500, 700, 850)), "tcwv"),
    "diagnostics.one_level": lambda: diagnostics(mk(C=1, **WIND), "tcwv"),
    "diagnostics.levels_twice": lambda: diagnostics(mk(levels=(500, 500), **WIND), "ivt"),
    "diagnostics.devices": lambda: diagnostics(with_var(mk(**WIND), "atmos_vars", "v", fill((1, 2, 2, 5, 8), 3).to("meta")), "ws"),
}


def outcome(case):
    try:
        CASES[case]()
    except Exception as err:  # noqa: BLE001
        return type(err).__name__, str(err)
    return None, None


# ---- one fixed small input per entry point: 2 surface + 1 atmospheric variable, 2 levels, 6 x 8, NaNs, 3 members ---------
def holed(b: Batch, seed: int) -> Batch:
    """`b` with a NaN at every 11th point (offset by the seed) of every field."""
    def f(v):
        v = v.clone()
        v.view(-1)[seed % 11::11] = float("nan")
        return v
    return Batch({k: f(v) for k, v in b.surf_vars.items()}, {}, {k: f(v) for k, v in b.atmos_vars.items()}, b.metadata)


def digest_inputs():
    kw = dict(surf=("2t", "msl"), atmos=("z",), n_lat=6, n_lon=8, B=2)
    truth = holed(mk(seed=0, **kw), 0)
    pred, clim = holed(mk(seed=1, **kw), 3), holed(mk(seed=2, **kw), 7)
    ens = [holed(mk(seed=11 + m, **kw), 4 + m) for m in range(3)]
    return truth, pred, clim, ens


def digest_results() -> dict[str, list[torch.Tensor]]:
    truth, pred, clim, ens = digest_inputs()
    thr = {"2t": [280.0, 290.0], "z": [[275.0], [285.0]]}
    wind = holed(mk(seed=5, surf=("10u", "10v"), atmos=("u", "v", "q"), n_lat=6, n_lon=8, B=2), 2)
    s, e = scores(pred, truth, clim), ensemble_scores(ens, truth)
    v, p = event_scores(pred, truth, thr, scales=(1, 3, 5)), probability_scores(ens, truth, thr)
    x = spectra(pred, truth, bands=[(-90, 90), (-30, 30)])
    f = FieldStats(thr, derived=()).update(pred).update(truth, minus=clim)
    d = diagnostics(wind, ("ws", "vo", "d", "10ws", "10vo", "10d", "tcwv", "ivtu", "ivtv", "ivt"))
    one = ensemble_scores(dataclasses.replace(ens[0], metadata=ens[0].metadata), holed(mk(seed=0, surf=("2t", "msl"), n_lat=6, n_lon=8), 0))
    return {
        "scores": [s.table], "scores.no_climatology": [scores(pred, truth).table],
        "ensemble_scores": [e.table, e.hist], "ensemble_scores.one_batch": [one.table, one.hist],
        "event_scores": [v.rowsums_table, v.valid_table, v.fss_table, v.counts_table, v.rates_table],
        "probability_scores": [p.rows_table, p.counts_table, p.scores_table, p.bins_table, p.roc_table, p.forecast_probability],
        "spectra": [x.table, x.rows_table], "spectra.alone": [spectra(pred).table],
        "FieldStats": [f.state[k] for k in sorted(f.state)] + [f.mean["z"], f.exceed_fraction["2t"]],
        "diagnostics": [d.surf_vars[k] for k in sorted(d.surf_vars)] + [d.atmos_vars[k] for k in sorted(d.atmos_vars)],
        "accessors": [s.rmse["z"], s.count["2t"], e.rank_hist["z"], v.fss["z"], p.brier["2t"], x.power["msl"]],
    }


def sha(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(np.ascontiguousarray(t.detach().numpy()).tobytes())
    return h.hexdigest()


MESSAGES = {
    'scores.pred_band': ('ValueError',
        'scores: pred is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'scores.truth_band': ('ValueError',
        'scores: truth is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'scores.pred_matrices': ('ValueError',
        'scores: pred has matrices for latitudes / longitudes; vector coordinates are needed'),
    'scores.truth_matrices': ('ValueError',
        'scores: truth has matrices for latitudes / longitudes; vector coordinates are needed'),
    'scores.lat_length': ('ValueError',
        'scores: pred and truth differ in lat: 5 against 7 values'),
    'scores.lat_length_crop_hint': ('ValueError',
        "scores: pred and truth differ in lat: 5 against 6 values; the prediction was cropped to the model's patch size: use truth.crop(model.patch_size)"),
    'scores.lat_values': ('ValueError',
        'scores: pred and truth differ in lat (same length, different values)'),
    'scores.lon_length': ('ValueError',
        'scores: pred and truth differ in lon: 8 against 9 values'),
    'scores.lon_values': ('ValueError',
        'scores: pred and truth differ in lon (same length, different values)'),
    'scores.levels': ('ValueError',
        'scores: pred and truth differ in atmos_levels: (500, 850) against (500, 700)'),
    'scores.both_groups': ('ValueError',
        "scores: '2t' is both a surface and an atmospheric variable"),
    'scores.pred_rank': ('ValueError',
        "scores: pred.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'scores.truth_grid': ('ValueError',
        "scores: truth.surf_vars['2t'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'scores.batch_size': ('ValueError',
        "scores: pred and truth differ in batch size for '2t': (1, 5, 8) against (2, 5, 8)"),
    'scores.shape': ('ValueError',
        "scores: pred and truth differ in shape for 'z': (1, 2, 5, 8) against (1, 3, 5, 8)"),
    'scores.devices': ('ValueError',
        "scores: the fields are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'scores.no_common': ('ValueError',
        'scores: pred and truth have no surface or atmospheric variable in common'),
    'scores.climatology_band': ('ValueError',
        'scores: climatology is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'scores.climatology_lat_crop_hint': ('ValueError',
        "scores: pred and climatology differ in lat: 5 against 6 values; the prediction was cropped to the model's patch size: use climatology.crop(model.patch_size)"),
    'scores.climatology_lon_values': ('ValueError',
        'scores: pred and climatology differ in lon (same length, different values)'),
    'scores.climatology_levels': ('ValueError',
        'scores: pred and climatology differ in atmos_levels: (500, 850) against (500, 700)'),
    'scores.climatology_lacks_surface': ('ValueError',
        "scores: the climatology has no surf variable '2t'"),
    'scores.climatology_lacks_atmospheric': ('ValueError',
        "scores: the climatology has no atmos variable 'z'"),
    'scores.climatology_grid': ('ValueError',
        "scores: climatology.surf_vars['2t'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'scores.climatology_batch_size': ('ValueError',
        "scores: pred and climatology differ in batch size for '2t': (1, 5, 8) against (2, 5, 8)"),
    'scores.climatology_shape': ('ValueError',
        "scores: pred and climatology differ in shape for 'z': (1, 2, 5, 8) against (1, 3, 5, 8)"),
    'scores.climatology_devices': ('ValueError',
        "scores: the fields are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'latitude_weights.matrix': ('ValueError',
        'scores: latitudes must be a non-empty vector'),
    'latitude_weights.empty': ('ValueError',
        'scores: latitudes must be a non-empty vector'),
    'latitude_weights.range': ('ValueError',
        'scores: latitudes must be in the range [-90, 90]'),
    'latitude_weights.nan': ('ValueError',
        'scores: latitudes must be in the range [-90, 90]'),
    'latitude_weights.poles': ('ValueError',
        'scores: latitudes must be in the range [-90, 90]'),
    'ensemble_scores.truth_band': ('ValueError',
        'ensemble_scores: truth is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'ensemble_scores.truth_not_batch': ('TypeError',
        'ensemble_scores: truth must be a Batch, got int'),
    'ensemble_scores.member_not_batch': ('TypeError',
        'ensemble_scores: members[1] must be a Batch, got str'),
    'ensemble_scores.one_member': ('ValueError',
        'ensemble_scores: members must hold 2 to 64 batches, got 1'),
    'ensemble_scores.65_members': ('ValueError',
        'ensemble_scores: members must hold 2 to 64 batches, got 65'),
    'ensemble_scores.member_band': ('ValueError',
        'ensemble_ensemble_scores: members[1] is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'ensemble_scores.member_matrices': ('ValueError',
        'ensemble_ensemble_scores: members[0] has matrices for latitudes / longitudes; vector coordinates are needed'),
    'ensemble_scores.truth_matrices': ('ValueError',
        'ensemble_scores: truth has matrices for latitudes / longitudes; vector coordinates are needed'),
    'ensemble_scores.lat_length': ('ValueError',
        'ensemble_ensemble_scores: members[0] and truth differ in lat: 5 against 7 values'),
    'ensemble_scores.lat_length_crop_hint': ('ValueError',
        "ensemble_ensemble_scores: members[0] and truth differ in lat: 5 against 6 values; members[0] was cropped to the model's patch size: use truth.crop(model.patch_size)"),
    'ensemble_scores.lat_values': ('ValueError',
        'ensemble_ensemble_scores: members[1] and truth differ in lat (same length, different values)'),
    'ensemble_scores.lon_length': ('ValueError',
        'ensemble_ensemble_scores: members[0] and truth differ in lon: 8 against 9 values'),
    'ensemble_scores.lon_values': ('ValueError',
        'ensemble_ensemble_scores: members[0] and truth differ in lon (same length, different values)'),
    'ensemble_scores.levels': ('ValueError',
        'ensemble_ensemble_scores: members[0] and truth differ in atmos_levels: (500, 850) against (500, 700)'),
    'ensemble_scores.one_batch_band': ('ValueError',
        'ensemble_ensemble_scores: members is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'ensemble_scores.one_batch_lat_crop_hint': ('ValueError',
        "ensemble_ensemble_scores: members and truth differ in lat: 5 against 6 values; members was cropped to the model's patch size: use truth.crop(model.patch_size)"),
    'ensemble_scores.one_batch_lon_values': ('ValueError',
        'ensemble_ensemble_scores: members and truth differ in lon (same length, different values)'),
    'ensemble_scores.one_batch_levels': ('ValueError',
        'ensemble_ensemble_scores: members and truth differ in atmos_levels: (500, 850) against (500, 700)'),
    'ensemble_scores.both_groups': ('ValueError',
        "ensemble_scores: '2t' is both a surface and an atmospheric variable"),
    'ensemble_scores.truth_rank': ('ValueError',
        "ensemble_scores: truth.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'ensemble_scores.member_grid': ('ValueError',
        "ensemble_scores: members[1].surf_vars['2t'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'ensemble_scores.one_batch_grid': ('ValueError',
        "ensemble_scores: members.surf_vars['2t'] has shape (3, 2, 4, 8), which does not fit a 5 x 8 grid"),
    'ensemble_scores.one_batch_truth_batch': ('ValueError',
        "ensemble_scores: members is ONE Batch (its batch elements are the members), so truth must have batch size 1, got 2 for '2t'; pass a sequence of Batches to score a batch of ensembles"),
    'ensemble_scores.one_batch_shape': ('ValueError',
        "ensemble_scores: members and truth differ in shape for 'z': (3, 3, 5, 8) against (1, 2, 5, 8)"),
    'ensemble_scores.batch_size': ('ValueError',
        "ensemble_scores: members[1] and truth differ in batch size for '2t': (2, 5, 8) against (1, 5, 8)"),
    'ensemble_scores.shape': ('ValueError',
        "ensemble_scores: members[1] and truth differ in shape for 'z': (1, 3, 5, 8) against (1, 2, 5, 8)"),
    'ensemble_scores.one_batch_one_member': ('ValueError',
        'ensemble_scores: members is ONE Batch, whose batch size is the number of members: it must be 2 to 64, got [1]'),
    'ensemble_scores.one_batch_65_members': ('ValueError',
        'ensemble_scores: members is ONE Batch, whose batch size is the number of members: it must be 2 to 64, got [65]'),
    'ensemble_scores.one_batch_sizes_differ': ('ValueError',
        'ensemble_scores: members is ONE Batch, whose batch size is the number of members: it must be 2 to 64, got [3, 4]'),
    'ensemble_scores.devices': ('ValueError',
        "ensemble_scores: the fields of members and truth are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'ensemble_scores.one_batch_devices': ('ValueError',
        "ensemble_scores: the fields of members and truth are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'ensemble_scores.no_common': ('ValueError',
        'ensemble_scores: members and truth have no surface or atmospheric variable in common'),
    'event_scores.pred_band': ('ValueError',
        'scores: pred is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'event_scores.truth_band': ('ValueError',
        'scores: truth is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'event_scores.pred_matrices': ('ValueError',
        'scores: pred has matrices for latitudes / longitudes; vector coordinates are needed'),
    'event_scores.truth_matrices': ('ValueError',
        'scores: truth has matrices for latitudes / longitudes; vector coordinates are needed'),
    'event_scores.lat_length': ('ValueError',
        'scores: pred and truth differ in lat: 5 against 7 values'),
    'event_scores.lat_length_crop_hint': ('ValueError',
        "scores: pred and truth differ in lat: 5 against 6 values; the prediction was cropped to the model's patch size: use truth.crop(model.patch_size)"),
    'event_scores.lat_values': ('ValueError',
        'scores: pred and truth differ in lat (same length, different values)'),
    'event_scores.lon_length': ('ValueError',
        'scores: pred and truth differ in lon: 8 against 9 values'),
    'event_scores.lon_values': ('ValueError',
        'scores: pred and truth differ in lon (same length, different values)'),
    'event_scores.levels': ('ValueError',
        'scores: pred and truth differ in atmos_levels: (500, 850) against (500, 700)'),
    'event_scores.both_groups': ('ValueError',
        "event_scores: '2t' is both a surface and an atmospheric variable"),
    'event_scores.pred_rank': ('ValueError',
        "event_scores: pred.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'event_scores.truth_grid': ('ValueError',
        "event_scores: truth.surf_vars['2t'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'event_scores.batch_size': ('ValueError',
        "event_scores: pred and truth differ in batch size for '2t': (1, 5, 8) against (2, 5, 8)"),
    'event_scores.shape': ('ValueError',
        "event_scores: pred and truth differ in shape for 'z': (1, 2, 5, 8) against (1, 3, 5, 8)"),
    'event_scores.devices': ('ValueError',
        "event_scores: the fields are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'event_scores.thresholds_not_mapping': ('ValueError',
        'event_scores: thresholds must be a non-empty mapping from variable name to values'),
    'event_scores.thresholds_empty': ('ValueError',
        'event_scores: thresholds must be a non-empty mapping from variable name to values'),
    'event_scores.thresholds_not_numbers': ('ValueError',
        "event_scores: the thresholds of '2t' must be numbers"),
    'event_scores.thresholds_surface_2d': ('ValueError',
        "event_scores: the thresholds of '2t' have shape (2, 2); a sequence is needed"),
    'event_scores.thresholds_levels': ('ValueError',
        "event_scores: the thresholds of 'z' have shape (3, 2); a (C, T) array needs C = 2 levels"),
    'event_scores.thresholds_3d': ('ValueError',
        "event_scores: the thresholds of 'z' have shape (2, 2, 2); a sequence or a (2, T) array is needed"),
    'event_scores.thresholds_scalar': ('ValueError',
        "event_scores: the thresholds of '2t' have shape (); a sequence is needed"),
    'event_scores.thresholds_none': ('ValueError',
        "event_scores: 1 to 8 thresholds per variable, '2t' has 0"),
    'event_scores.thresholds_nine': ('ValueError',
        "event_scores: 1 to 8 thresholds per variable, '2t' has 9"),
    'event_scores.thresholds_unknown': ('ValueError',
        "event_scores: thresholds name the variable 'msl', which pred and truth do not both hold as a surface or atmospheric variable"),
    'event_scores.longitudes': ('ValueError',
        'event_scores: the grid has 4097 longitudes; 1 to 4096 are supported'),
    'event_scores.scales_not_sequence': ('ValueError',
        'event_scores: scales must be a sequence of odd window sizes'),
    'event_scores.scales_fraction': ('ValueError',
        'event_scores: scales must be whole numbers, got 2.5'),
    'event_scores.scales_bool': ('ValueError',
        'event_scores: scales must be whole numbers, got True'),
    'event_scores.scales_even': ('ValueError',
        'event_scores: scales must be odd (a window has a centre point), got 4'),
    'event_scores.scales_range': ('ValueError',
        'event_scores: scales must be within 1..63, got 65'),
    'event_scores.scales_wider': ('ValueError',
        "event_scores: scales must not be wider than the grid's 8 longitudes, got 9"),
    'event_scores.scales_twice': ('ValueError',
        'event_scores: scales must be distinct, 3 is given twice'),
    'event_scores.scales_nine': ('ValueError',
        'event_scores: at most 8 scales can be taken at a time (1 included), got 10'),
    'probability_scores.truth_band': ('ValueError',
        'probability_scores: truth is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'probability_scores.truth_not_batch': ('TypeError',
        'probability_scores: truth must be a Batch, got int'),
    'probability_scores.member_not_batch': ('TypeError',
        'probability_scores: members[1] must be a Batch, got str'),
    'probability_scores.one_member': ('ValueError',
        'probability_scores: members must hold 2 to 64 batches, got 1'),
    'probability_scores.65_members': ('ValueError',
        'probability_scores: members must hold 2 to 64 batches, got 65'),
    'probability_scores.member_band': ('ValueError',
        'ensemble_probability_scores: members[1] is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'probability_scores.member_matrices': ('ValueError',
        'ensemble_probability_scores: members[0] has matrices for latitudes / longitudes; vector coordinates are needed'),
    'probability_scores.truth_matrices': ('ValueError',
        'probability_scores: truth has matrices for latitudes / longitudes; vector coordinates are needed'),
    'probability_scores.lat_length': ('ValueError',
        'ensemble_probability_scores: members[0] and truth differ in lat: 5 against 7 values'),
    'probability_scores.lat_length_crop_hint': ('ValueError',
        "ensemble_probability_scores: members[0] and truth differ in lat: 5 against 6 values; members[0] was cropped to the model's patch size: use truth.crop(model.patch_size)"),
    'probability_scores.lat_values': ('ValueError',
        'ensemble_probability_scores: members[1] and truth differ in lat (same length, different values)'),
    'probability_scores.lon_length': ('ValueError',
        'ensemble_probability_scores: members[0] and truth differ in lon: 8 against 9 values'),
    'probability_scores.lon_values': ('ValueError',
        'ensemble_probability_scores: members[0] and truth differ in lon (same length, different values)'),
    'probability_scores.levels': ('ValueError',
        'ensemble_probability_scores: members[0] and truth differ in atmos_levels: (500, 850) against (500, 700)'),
    'probability_scores.one_batch_band': ('ValueError',
        'ensemble_probability_scores: members is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'probability_scores.one_batch_lat_crop_hint': ('ValueError',
        "ensemble_probability_scores: members and truth differ in lat: 5 against 6 values; members was cropped to the model's patch size: use truth.crop(model.patch_size)"),
    'probability_scores.one_batch_lon_values': ('ValueError',
        'ensemble_probability_scores: members and truth differ in lon (same length, different values)'),
    'probability_scores.one_batch_levels': ('ValueError',
        'ensemble_probability_scores: members and truth differ in atmos_levels: (500, 850) against (500, 700)'),
    'probability_scores.both_groups': ('ValueError',
        "probability_scores: '2t' is both a surface and an atmospheric variable"),
    'probability_scores.truth_rank': ('ValueError',
        "probability_scores: truth.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'probability_scores.member_grid': ('ValueError',
        "probability_scores: members[1].surf_vars['2t'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'probability_scores.one_batch_grid': ('ValueError',
        "probability_scores: members.surf_vars['2t'] has shape (3, 2, 4, 8), which does not fit a 5 x 8 grid"),
    'probability_scores.one_batch_truth_batch': ('ValueError',
        "probability_scores: members is ONE Batch (its batch elements are the members), so truth must have batch size 1, got 2 for '2t'; pass a sequence of Batches to score a batch of ensembles"),
    'probability_scores.one_batch_shape': ('ValueError',
        "probability_scores: members and truth differ in shape for 'z': (3, 3, 5, 8) against (1, 2, 5, 8)"),
    'probability_scores.batch_size': ('ValueError',
        "probability_scores: members[1] and truth differ in batch size for '2t': (2, 5, 8) against (1, 5, 8)"),
    'probability_scores.shape': ('ValueError',
        "probability_scores: members[1] and truth differ in shape for 'z': (1, 3, 5, 8) against (1, 2, 5, 8)"),
    'probability_scores.one_batch_one_member': ('ValueError',
        'probability_scores: members is ONE Batch, whose batch size is the number of members: it must be 2 to 64, got [1]'),
    'probability_scores.one_batch_65_members': ('ValueError',
        'probability_scores: members is ONE Batch, whose batch size is the number of members: it must be 2 to 64, got [65]'),
    'probability_scores.one_batch_sizes_differ': ('ValueError',
        'probability_scores: members is ONE Batch, whose batch size is the number of members: it must be 2 to 64, got [3, 4]'),
    'probability_scores.devices': ('ValueError',
        "probability_scores: the fields of members and truth are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'probability_scores.one_batch_devices': ('ValueError',
        "probability_scores: the fields of members and truth are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'probability_scores.thresholds_not_mapping': ('ValueError',
        'probability_scores: thresholds must be a non-empty mapping from variable name to values'),
    'probability_scores.thresholds_empty': ('ValueError',
        'probability_scores: thresholds must be a non-empty mapping from variable name to values'),
    'probability_scores.thresholds_not_numbers': ('ValueError',
        "probability_scores: the thresholds of '2t' must be numbers"),
    'probability_scores.thresholds_surface_2d': ('ValueError',
        "probability_scores: the thresholds of '2t' have shape (2, 2); a sequence is needed"),
    'probability_scores.thresholds_levels': ('ValueError',
        "probability_scores: the thresholds of 'z' have shape (3, 2); a (C, T) array needs C = 2 levels"),
    'probability_scores.thresholds_3d': ('ValueError',
        "probability_scores: the thresholds of 'z' have shape (2, 2, 2); a sequence or a (2, T) array is needed"),
    'probability_scores.thresholds_scalar': ('ValueError',
        "probability_scores: the thresholds of '2t' have shape (); a sequence is needed"),
    'probability_scores.thresholds_none': ('ValueError',
        "probability_scores: 1 to 8 thresholds per variable, '2t' has 0"),
    'probability_scores.thresholds_nine': ('ValueError',
        "probability_scores: 1 to 8 thresholds per variable, '2t' has 9"),
    'probability_scores.thresholds_unknown': ('ValueError',
        "probability_scores: thresholds name the variable 'msl', which members and truth do not all hold as a surface or atmospheric variable"),
    'probability_scores.thresholds_unknown_one_batch': ('ValueError',
        "probability_scores: thresholds name the variable 'msl', which members and truth do not all hold as a surface or atmospheric variable"),
    'spectra.pred_band': ('ValueError',
        'scores: pred is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'spectra.truth_band': ('ValueError',
        'scores: truth is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'spectra.pred_matrices': ('ValueError',
        'scores: pred has matrices for latitudes / longitudes; vector coordinates are needed'),
    'spectra.truth_matrices': ('ValueError',
        'scores: truth has matrices for latitudes / longitudes; vector coordinates are needed'),
    'spectra.lat_length': ('ValueError',
        'scores: pred and truth differ in lat: 5 against 7 values'),
    'spectra.lat_length_crop_hint': ('ValueError',
        "scores: pred and truth differ in lat: 5 against 6 values; the prediction was cropped to the model's patch size: use truth.crop(model.patch_size)"),
    'spectra.lat_values': ('ValueError',
        'scores: pred and truth differ in lat (same length, different values)'),
    'spectra.lon_length': ('ValueError',
        'scores: pred and truth differ in lon: 8 against 9 values'),
    'spectra.lon_values': ('ValueError',
        'scores: pred and truth differ in lon (same length, different values)'),
    'spectra.levels': ('ValueError',
        'scores: pred and truth differ in atmos_levels: (500, 850) against (500, 700)'),
    'spectra.both_groups': ('ValueError',
        "spectra: '2t' is both a surface and an atmospheric variable"),
    'spectra.pred_rank': ('ValueError',
        "spectra: pred.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'spectra.truth_grid': ('ValueError',
        "spectra: truth.surf_vars['2t'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'spectra.batch_size': ('ValueError',
        "spectra: pred and truth differ in batch size for '2t': (1, 5, 8) against (2, 5, 8)"),
    'spectra.shape': ('ValueError',
        "spectra: pred and truth differ in shape for 'z': (1, 2, 5, 8) against (1, 3, 5, 8)"),
    'spectra.devices': ('ValueError',
        "spectra: the fields are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'spectra.no_common': ('ValueError',
        'spectra: pred and truth have no surface or atmospheric variable in common'),
    'spectra.no_variable': ('ValueError',
        'spectra: pred has no surface or atmospheric variable'),
    'spectra.alone_band': ('ValueError',
        'scores: pred is a latitude band (BandBatch); gather the forecast first, band scores are not supported'),
    'spectra.alone_matrices': ('ValueError',
        'scores: pred has matrices for latitudes / longitudes; vector coordinates are needed'),
    'spectra.alone_both_groups': ('ValueError',
        "spectra: '2t' is both a surface and an atmospheric variable"),
    'spectra.alone_rank': ('ValueError',
        "spectra: pred.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'spectra.alone_devices': ('ValueError',
        "spectra: the fields are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'spectra.bands_not_pairs': ('ValueError',
        'spectra: bands must be a sequence of (south, north) pairs in degrees'),
    'spectra.bands_none': ('ValueError',
        'spectra: 1 to 8 bands can be taken at a time, got 0'),
    'spectra.bands_nine': ('ValueError',
        'spectra: 1 to 8 bands can be taken at a time, got 9'),
    'spectra.bands_order': ('ValueError',
        'spectra: a band needs -90 <= south <= north <= 90, got (10.0, -10.0)'),
    'spectra.one_longitude': ('ValueError',
        'spectra: the grid has 1 longitudes; 2 to 4096 are supported'),
    'spectra.longitudes': ('ValueError',
        'spectra: the grid has 4097 longitudes; 2 to 4096 are supported'),
    'spectra.longitudes_regional': ('ValueError',
        'spectra: the longitudes must be equally spaced and cover the full circle (a zonal spectrum of a regional or irregular grid is not defined)'),
    'FieldStats.thresholds_not_mapping': ('ValueError',
        'FieldStats: thresholds must be a mapping from variable name to values'),
    'FieldStats.derived_unknown': ('ValueError',
        "FieldStats: derived offers ['10ws', 'ws'], got 'vo'"),
    'FieldStats.over': ('ValueError',
        "FieldStats: over must be None or 'batch', got 'time'"),
    'FieldStats.batch_band': ('ValueError',
        'FieldStats: batch is a latitude band (BandBatch); gather the forecast first, band statistics are not supported'),
    'FieldStats.minus_band': ('ValueError',
        'FieldStats: minus is a latitude band (BandBatch); gather the forecast first, band statistics are not supported'),
    'FieldStats.batch_not_batch': ('TypeError',
        'FieldStats: batch must be a Batch, got int'),
    'FieldStats.minus_not_batch': ('TypeError',
        'FieldStats: minus must be a Batch, got int'),
    'FieldStats.batch_matrices': ('ValueError',
        'FieldStats: batch has matrices for latitudes / longitudes; vector coordinates are needed'),
    'FieldStats.minus_matrices': ('ValueError',
        'FieldStats: minus has matrices for latitudes / longitudes; vector coordinates are needed'),
    'FieldStats.minus_lat_length': ('ValueError',
        'FieldStats: batch and minus differ in lat: 5 against 7 values'),
    'FieldStats.minus_lat_crop_hint': ('ValueError',
        "FieldStats: batch and minus differ in lat: 5 against 6 values; batch was cropped to the model's patch size: use minus.crop(model.patch_size)"),
    'FieldStats.minus_lat_values': ('ValueError',
        'FieldStats: batch and minus differ in lat (same length, different values)'),
    'FieldStats.minus_lon_length': ('ValueError',
        'FieldStats: batch and minus differ in lon: 8 against 9 values'),
    'FieldStats.minus_lon_values': ('ValueError',
        'FieldStats: batch and minus differ in lon (same length, different values)'),
    'FieldStats.minus_levels': ('ValueError',
        'FieldStats: batch and minus differ in atmos_levels: (500, 850) against (500, 700)'),
    'FieldStats.batch_rank': ('ValueError',
        "FieldStats: batch.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'FieldStats.minus_grid': ('ValueError',
        "FieldStats: minus.surf_vars['2t'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'FieldStats.holds_derived': ('ValueError',
        "FieldStats: batch holds '10ws', which is also a derived variable"),
    'FieldStats.reference_of_derived': ('ValueError',
        "FieldStats: with minus=, the reference of the derived variable '10ws' is minus.surf_vars['10ws'], which is missing"),
    'FieldStats.derived_components': ('ValueError',
        "FieldStats: the derived variable 'ws' needs 'u' and 'v' in batch.atmos_vars"),
    'FieldStats.both_groups': ('ValueError',
        "FieldStats: '2t' is both a surface and an atmospheric variable"),
    'FieldStats.no_variable': ('ValueError',
        'FieldStats: batch has no surface or atmospheric variable'),
    'FieldStats.batch_sizes': ('ValueError',
        'FieldStats: the variables of batch differ in batch size: [2, 3]'),
    'FieldStats.over_batch_one': ('ValueError',
        "FieldStats: with over='batch' the batch size is the number of samples: it must be 2 to 64, got 1"),
    'FieldStats.over_batch_65': ('ValueError',
        "FieldStats: with over='batch' the batch size is the number of samples: it must be 2 to 64, got 65"),
    'FieldStats.minus_lacks': ('ValueError',
        "FieldStats: minus has no variable '2t'"),
    'FieldStats.minus_batch_size': ('ValueError',
        "FieldStats: batch and minus differ in batch size for '2t': (2, 5, 8) against (1, 5, 8)"),
    'FieldStats.minus_shape': ('ValueError',
        "FieldStats: batch and minus differ in shape for 'z': (1, 2, 5, 8) against (1, 3, 5, 8)"),
    'FieldStats.minus_over_batch': ('ValueError',
        "FieldStats: batch and minus differ in batch size for '2t': (1, 5, 8) against (3, 5, 8)"),
    'FieldStats.devices': ('ValueError',
        "FieldStats: the fields are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'FieldStats.thresholds_not_numbers': ('ValueError',
        "FieldStats: the thresholds of '2t' must be numbers"),
    'FieldStats.thresholds_surface_2d': ('ValueError',
        "FieldStats: the thresholds of '2t' have shape (2, 2); a sequence is needed"),
    'FieldStats.thresholds_levels': ('ValueError',
        "FieldStats: the thresholds of 'z' have shape (3, 2); a (C, T) array needs C = 2 levels"),
    'FieldStats.thresholds_3d': ('ValueError',
        "FieldStats: the thresholds of 'z' have shape (2, 2, 2); a sequence or a (2, T) array is needed"),
    'FieldStats.thresholds_none': ('ValueError',
        "FieldStats: 1 to 8 thresholds per variable, '2t' has 0"),
    'FieldStats.thresholds_nine': ('ValueError',
        "FieldStats: 1 to 8 thresholds per variable, '2t' has 9"),
    'FieldStats.thresholds_unknown': ('ValueError',
        "FieldStats: thresholds name the variable 'msl', which the batch does not hold as a surface, atmospheric or derived variable"),
    'FieldStats.later_lat_length': ('ValueError',
        'FieldStats: batch and the first update differ in lat: 6 against 5 values'),
    'FieldStats.later_lat_values': ('ValueError',
        'FieldStats: batch and the first update differ in lat (same length, different values)'),
    'FieldStats.later_lon_length': ('ValueError',
        'FieldStats: batch and the first update differ in lon: 9 against 8 values'),
    'FieldStats.later_lon_values': ('ValueError',
        'FieldStats: batch and the first update differ in lon (same length, different values)'),
    'FieldStats.later_levels': ('ValueError',
        'FieldStats: batch and the first update differ in atmos_levels: (500, 700) against (500, 850)'),
    'FieldStats.later_variables': ('ValueError',
        "FieldStats: batch holds the variables ['msl', 'z'], the first update held ['2t', 'z']"),
    'FieldStats.later_batch_size': ('ValueError',
        "FieldStats: batch and the first update differ in batch size for '2t': (2,) against (1,)"),
    'FieldStats.later_shape': ('ValueError',
        "FieldStats: batch and the first update differ in shape for 'z': (1, 3) against (1, 2)"),
    'FieldStats.no_update': ('ValueError',
        'FieldStats: no update yet'),
    'FieldStats.no_thresholds': ('ValueError',
        'FieldStats: no thresholds were given'),
    'FieldStats.no_thresholds_fraction': ('ValueError',
        'FieldStats: no thresholds were given'),
    'FieldStats.as_batch': ('ValueError',
        "FieldStats: as_batch offers ('mean', 'std', 'var', 'rms', 'min', 'max'), got 'median'"),
    'diagnostics.band': ('ValueError',
        'diagnostics: batch is a latitude band (BandBatch); gather the forecast first, band diagnostics are not supported'),
    'diagnostics.not_batch': ('TypeError',
        'diagnostics: batch must be a Batch, got int'),
    'diagnostics.matrices': ('ValueError',
        'diagnostics: batch has matrices for latitudes / longitudes; vector coordinates are needed'),
    'diagnostics.unknown': ('ValueError',
        "diagnostics: which offers ['10d', '10vo', '10ws', 'd', 'ivt', 'ivtu', 'ivtv', 'tcwv', 'vo', 'ws'], got 'pv'"),
    'diagnostics.nothing': ('ValueError',
        "diagnostics: which names no field; it offers ['10d', '10vo', '10ws', 'd', 'ivt', 'ivtu', 'ivtv', 'tcwv', 'vo', 'ws']"),
    'diagnostics.one_latitude': ('ValueError',
        'diagnostics: the grid has 1 latitudes and 8 longitudes; at least 2 of each are needed'),
    'diagnostics.longitudes': ('ValueError',
        'diagnostics: the longitudes must be equally spaced'),
    'diagnostics.already_held': ('ValueError',
        "diagnostics: batch.atmos_vars already holds 'ws'"),
    'diagnostics.component_missing': ('ValueError',
        "diagnostics: '10vo' needs '10v' in batch.surf_vars, which is missing"),
    'diagnostics.rank': ('ValueError',
        "diagnostics: batch.atmos_vars['u'] has shape (1, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'diagnostics.grid': ('ValueError',
        "diagnostics: batch.surf_vars['10v'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'diagnostics.batch_sizes': ('ValueError',
        'diagnostics: the variables of batch differ in batch size or levels: [(1, 2), (2, 2)]'),
    'diagnostics.level_counts': ('ValueError',
        'diagnostics: the variables of batch differ in batch size or levels: [(1, 2), (1, 3)]'),
    'diagnostics.metadata_levels': ('ValueError',
        "diagnostics: batch.atmos_vars['q'] has 2 levels, the metadata names 3"),
    'diagnostics.one_level': ('ValueError',
        'diagnostics: a vertical integral takes 2 to 64 pressure levels, the batch has 1'),
    'diagnostics.levels_twice': ('ValueError',
        'diagnostics: a vertical integral needs distinct pressure levels, got (500, 500)'),
    'diagnostics.devices': ('ValueError',
        "diagnostics: the fields are on ['cpu', 'meta']; move the batch to the CPU or to one GPU first"),
}
DIGESTS = {
    'scores': 'aa222d66bb09044a6020cfb45d1c571974d2c8972feb3cf389364f4fedd74dc0',
    'scores.no_climatology': 'fa9e3226d3589370e825164ad28700cc42056c55d5e49228077a226d8c598c2c',
    'ensemble_scores': '6860101582517e07a17a3b2d007e9fa0a4432b893dc3906e24e3be3361a36c54',
    'ensemble_scores.one_batch': '234fbcdd809d013a35da812189ec29bd1680fb9d444820fc0b9bfef5420211f4',
    'event_scores': '7460c2cafc043c2f07a36f8cca6c0261c9a1f9442c81c529dda318ff68968f45',
    'probability_scores': '84a9083892fb59950408e689e60b5ec96272b0eab6971ebafe36457f750ed185',
    'spectra': '47d144fb09a0c111283b67760d235f3c63b7ebafebbdd98b65426a283361dcc0',
    'spectra.alone': '821b9560cb1e5e58d96544e314f7be5597fcde55bee6b58d8f063ee255749856',
    'FieldStats': '909025fb621e661b7834babd8ae5d4a184c21a9cf3e9e311890da7b00b24e09f',
    'diagnostics': '05b22b499b369bb2aee581e60858e7e6f728f9e6cff220346233d197553e20c8',
    'accessors': 'd837d732c3fbfa49a5d8e931d5555e3b3b50ff5ee22020a871c60634a5bd15ce',
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_message(case):
    assert case in MESSAGES, f"{case} has no recorded message: python tests/test_verification_messages.py"
    assert outcome(case) == MESSAGES[case]


def test_every_case_raises():
    assert set(MESSAGES) == set(CASES) and all(kind is not None for kind, _ in MESSAGES.values())


def test_host_numbers_keep_their_bits():
    got = {k: sha(v) for k, v in digest_results().items()}
    assert got == DIGESTS


def test_device_checks_keep_their_texts():
    """The float32 and row-major checks of the device branch, on CPU tensors standing in for one device: the literals are
    those of scores.py, ensemble.py, spectra.py, fieldstats.py and diagnostics.py before the checks were shared."""
    from aurora_amd import _fields

    f64, f32 = torch.zeros(1, 5, 8, dtype=torch.float64), torch.zeros(1, 5, 8)
    slanted = torch.zeros(1, 8, 5).transpose(-1, -2)                     # (1, 5, 8) with strides (40, 1, 5)
    name_less = lambda what, _: f"a variable of {what}"  # noqa: E731

    def text(fn, what, f, task=_fields.SCORES_TASK, **kw):
        with pytest.raises((TypeError, ValueError)) as err:
            _fields.check_planes(fn, [("pred", ["2t"], [f32]), (what, ["z"], [f])], 5, 8, task, **kw)
        return type(err.value).__name__, str(err.value)

    assert text("scores", "truth", f64) == ("TypeError", "scores: truth variable 'z' is torch.float64; the device path scores float32 fields "
                                            "(move the batches to the CPU to score other precisions)")
    assert text("scores", "climatology", slanted) == ("ValueError", "scores: the planes of climatology variable 'z' are not row-major contiguous; "
                                                      "call .contiguous() on it first")
    assert text("ensemble_scores", "members[2]", f64) == ("TypeError", "ensemble_scores: members[2] variable 'z' is torch.float64; the device path scores float32 "
                                                          "fields (move the batches to the CPU to score other precisions)")
    assert text("probability_scores", "members[2]", slanted) == ("ValueError", "probability_scores: the planes of members[2] variable 'z' are not row-major "
                                                                 "contiguous; call .contiguous() on it first")
    spectra_task = "transforms float32 fields (move the batches to the CPU for other precisions)"
    assert text("spectra", "truth", f64, spectra_task) == ("TypeError", "spectra: truth variable 'z' is torch.float64; the device path transforms float32 "
                                                           "fields (move the batches to the CPU for other precisions)")
    assert text("FieldStats", "minus", f64, _fields.TAKES_TASK, noun=name_less) == (
        "TypeError", "FieldStats: a variable of minus is torch.float64; the device path takes float32 fields "
        "(move the batches to the CPU for other precisions)")
    assert text("diagnostics", "batch", slanted, _fields.TAKES_TASK, noun=name_less) == (
        "ValueError", "diagnostics: the planes of a variable of batch are not row-major contiguous; call "
        ".contiguous() on it first")
    _fields.check_planes("scores", [("pred", ["2t"], [torch.zeros(5, 1).as_strided((1, 5, 1), (5, 1, 3))])], 5, 1,
                         _fields.SCORES_TASK)                                                         # one column: any stride
    assert _fields.place("scores", [("pred", ["2t"], [f64])], 5, 8) == "cpu"                          # the host takes any precision


def test_device_table_cache():
    """LRU beyond the limit; a table used during stream capture stays whatever comes later; a miss during capture raises the
    caller's message.  No GPU: the upload and the capture state are injected."""
    from aurora_amd._fields import DeviceTables

    state = {"capturing": False}
    uploads = []

    def upload(a, device):
        uploads.append(a)
        return ("table", a, device)

    tables = DeviceTables(limit=3, upload=upload, capturing=lambda: state["capturing"])
    get = lambda k: tables.get((k,), "dev", lambda: k, f"call once with {k}")  # noqa: E731
    for k in (0, 1, 2):
        get(k)
    assert get(0) == ("table", 0, "dev") and uploads == [0, 1, 2]          # a hit: nothing uploaded, 0 is the most recent
    get(3)                                                                  # beyond the limit: 1, the least recent, leaves
    assert uploads == [0, 1, 2, 3]
    get(0), get(2), get(3)
    assert uploads == [0, 1, 2, 3]
    get(1)
    assert uploads == [0, 1, 2, 3, 1]
    state["capturing"] = True
    pinned = get(2)                                                         # used by a captured graph from here on
    with pytest.raises(RuntimeError, match="^call once with 7$"):
        get(7)
    state["capturing"] = False
    for k in range(100, 140):
        get(k)
    n = len(uploads)
    assert get(2) is pinned and len(uploads) == n                           # never evicted
    get(0)
    assert len(uploads) == n + 1                                            # while 0, which no graph used, left long ago
    assert get(("another device",)) != get(2)


if __name__ == "__main__":
    print("MESSAGES = {")
    for case in CASES:
        kind, text = outcome(case)
        print(f"    {case!r}: ({kind!r},\n        {text!r}),")
    print("}")
    print("DIGESTS = {")
    for k, v in digest_results().items():
        print(f"    {k!r}: {sha(v)!r},")
    print("}")
