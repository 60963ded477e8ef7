"""The argument errors, the host numbers and the wrap decision of the object chain -- `objects`, `object_matches`,
`nearest_event`, `object_separations`, `smooth`, `conservative_regrid` -- and the coordinate refusals of `diagnostics`, pinned as
literals in the form of tests/test_verification_messages.py (no GPU needed).

`CASES` drives every `raise` of these entry points that the CPU can reach through the public functions, on grids of 5 x 8 and
smaller (a limit case takes the coordinates it needs and no fields); `MESSAGES` holds the exception type and the exact text each
case gave BEFORE the grid rule, the sphere arithmetic and the result base of these modules were shared, so a shared helper
cannot reword a module's message unnoticed.  `DIGESTS` holds the sha256 of the raw bytes of every result tensor of one fixed small
input per entry point on three grids: one that wraps (6 x 12, 30 degrees), a regional one (5 x 7) and one that wraps with
descending latitudes.  `FULL_CIRCLE` holds, for five longitude axes, whether the grid counts as covering the full circle; the
entry points are probed through what they return, so nothing here imports a private helper.  To record again after a deliberate
change:

    python tests/test_object_chain_messages.py"""
import dataclasses
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from aurora_amd import (Batch, Metadata, conservative_regrid, diagnostics, nearest_event, object_matches, object_separations,  # noqa: E402
                        objects, smooth)
from aurora_amd.batch import derive_metadata  # noqa: E402
from tests.test_verification_messages import TIME, WIND, band, fill, holed, matrices, mk, sha, with_var  # noqa: E402

f64 = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
THR = {"2t": [280.0, 290.0], "z": [285.0]}


def obj(seed=0, thr=THR, **kw):
    return objects(mk(seed=seed, **kw), thr)


def moved(b: Batch, lat=None, lon=None) -> Batch:
    """The same fields under other coordinates, which `Metadata` itself would refuse (it takes descending latitudes and ascending
    longitudes only): what a batch carries after `derive_metadata`, and all that these entry points see."""
    md = b.metadata
    return dataclasses.replace(b, metadata=derive_metadata(md, lat=md.lat if lat is None else lat, lon=md.lon if lon is None else lon))


def only_coords(lat, lon) -> Batch:
    """A batch without fields: for the limits that are checked on the coordinates alone."""
    return moved(Batch({}, {}, {}, Metadata(f64(10.0, -10), f64(0.0, 180), TIME, (500, 850))), lat, lon)


def remade(o, **kw):
    """A hand-made `Objects`: the result of `objects` with some of its fields replaced."""
    return dataclasses.replace(o, **kw)


def on_meta(o):
    return remade(o, labels_table=o.labels_table.to("meta"))


def one_on_meta(b: Batch) -> Batch:
    return with_var(b, "surf_vars", "2t", b.surf_vars["2t"].to("meta"))


def static(b: Batch, shape) -> Batch:
    return dataclasses.replace(b, static_vars={"lsm": fill(shape, 9)})


def arange(n, step, first=0.0):
    return first + torch.arange(n, dtype=torch.float64) * step


def pair_cases(fn, call):
    """The five checks of a pair of `Objects` and the type check before them; `call(a, b)`."""
    out = {
        "a_not_objects": lambda: call(3, obj()),
        "b_not_objects": lambda: call(obj(), "x"),
        "layout": lambda: call(obj(), obj(thr={"2t": [280.0]})),
        "thresholds": lambda: call(obj(), obj(thr={"2t": [280.0], "z": [285.0]})),
        "grid": lambda: call(obj(), obj(n_lon=7)),
        "device": lambda: call(obj(), on_meta(obj(seed=1))),
        "lat_values": lambda: call(obj(), objects(moved(mk(seed=1), lat=torch.linspace(70, -70, 5, dtype=torch.float64)), THR)),
        "lon_values": lambda: call(obj(), objects(moved(mk(seed=1), lon=arange(8, 45.0, 1.0)), THR)),
    }
    return {f"{fn}.{k}": v for k, v in out.items()}


def threshold_cases(fn, call):
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


IRREGULAR = f64(0.0, 10, 20, 30, 40, 50, 60, 75)
LAT_BENT = f64(40.0, 20, 30, 0, -20)
LAT_FAR = f64(95.0, 60, 30, 0, -30)
CR = conservative_regrid
LAT3, LON4 = f64(-40.0, 0, 40), f64(0.0, 90, 180, 270)

CASES = {
    "objects.not_batch": lambda: objects(3, THR),
    "objects.band": lambda: objects(band(mk()), THR),
    "objects.matrices": lambda: objects(matrices(mk()), THR),
    "objects.connectivity": lambda: objects(mk(), THR, connectivity=6),
    "objects.connectivity_bool": lambda: objects(mk(), THR, connectivity=True),
    "objects.wrap": lambda: objects(mk(), THR, wrap="yes"),
    "objects.max_objects_zero": lambda: objects(mk(), THR, max_objects=0),
    "objects.max_objects_fraction": lambda: objects(mk(), THR, max_objects=2.5),
    "objects.max_objects_bool": lambda: objects(mk(), THR, max_objects=True),
    "objects.longitudes": lambda: objects(only_coords(f64(10.0, -10), arange(4097, 360.0 / 4097)), THR),
    "objects.no_longitude": lambda: objects(only_coords(f64(10.0, -10), f64()), THR),
    "objects.no_latitude": lambda: objects(only_coords(f64(), arange(8, 45.0)), THR),
    "objects.points": lambda: objects(only_coords(torch.linspace(80, -80, 2 ** 19, dtype=torch.float64), arange(4096, 360.0 / 4096)), THR),
    **threshold_cases("objects", lambda thr: objects(mk(), thr)),
    "objects.both_groups": lambda: objects(with_var(mk(), "atmos_vars", "2t", fill((1, 2, 2, 5, 8), 3)), THR),
    "objects.rank": lambda: objects(with_var(mk(), "surf_vars", "2t", fill((1, 2, 2, 5, 8), 3)), THR),
    "objects.grid": lambda: objects(with_var(mk(), "surf_vars", "2t", fill((1, 2, 5, 7), 3)), THR),
    "objects.devices": lambda: objects(one_on_meta(mk()), THR),
    "objects.latitude_range": lambda: objects(moved(mk(), lat=LAT_FAR), THR),
    "objects.latitude_nan": lambda: objects(moved(mk(), lat=f64(40.0, 20, float("nan"), 0, -20)), THR),
    "objects.mask_unknown": lambda: obj().mask("msl", 1),

    **pair_cases("object_matches", object_matches),
    "object_matches.max_pairs_zero": lambda: object_matches(obj(), obj(seed=1), max_pairs=0),
    "object_matches.max_pairs_many": lambda: object_matches(obj(), obj(seed=1), max_pairs=8193),
    "object_matches.max_pairs_fraction": lambda: object_matches(obj(), obj(seed=1), max_pairs=2.5),
    "object_matches.max_pairs_bool": lambda: object_matches(obj(), obj(seed=1), max_pairs=True),

    "nearest_event.not_objects": lambda: nearest_event(mk()),
    "nearest_event.max_km_zero": lambda: nearest_event(obj(), 0.0),
    "nearest_event.max_km_nan": lambda: nearest_event(obj(), float("nan")),
    "nearest_event.max_km_bool": lambda: nearest_event(obj(), True),
    "nearest_event.max_km_text": lambda: nearest_event(obj(), "300"),
    "nearest_event.latitude_range": lambda: nearest_event(remade(obj(), lat=LAT_FAR)),
    "nearest_event.latitude_nan": lambda: nearest_event(remade(obj(), lat=f64(40.0, 20, float("nan"), 0, -20))),
    "nearest_event.latitudes_bent": lambda: nearest_event(objects(moved(mk(), lat=LAT_BENT), THR)),
    "nearest_event.latitudes_twice": lambda: nearest_event(objects(moved(mk(), lat=f64(40.0, 20, 20, 0, -20)), THR)),
    "nearest_event.longitudes": lambda: nearest_event(remade(obj(n_lat=2), lon=arange(4097, 360.0 / 4097),
                                                             labels_table=torch.zeros(3, 2, 2, 4097, dtype=torch.int32))),
    "nearest_event.spacing_regional": lambda: nearest_event(objects(moved(mk(), lon=IRREGULAR), THR)),
    "nearest_event.spacing_wrapping": lambda: nearest_event(objects(moved(mk(), lon=arange(8, 10.0)), THR, wrap=True)),
    "nearest_event.spacing_one_value": lambda: nearest_event(objects(moved(mk(), lon=torch.full((8,), 20.0, dtype=torch.float64)), THR)),
    "nearest_event.spacing_nan": lambda: nearest_event(objects(moved(mk(), lon=f64(0.0, 10, 20, float("nan"), 40, 50, 60, 70)), THR)),

    **pair_cases("object_separations", object_separations),
    "object_separations.max_km": lambda: object_separations(obj(), obj(seed=1), max_km=-1.0),
    "object_separations.latitudes_bent": lambda: object_separations(*(objects(moved(mk(seed=s), lat=LAT_BENT), THR) for s in (0, 1))),

    "smooth.not_batch": lambda: smooth(3, 100.0),
    "smooth.band": lambda: smooth(band(mk()), 100.0),
    "smooth.matrices": lambda: smooth(matrices(mk()), 100.0),
    "smooth.radius_text": lambda: smooth(mk(), "wide"),
    "smooth.radius_none": lambda: smooth(mk(), None),
    "smooth.radius_zero": lambda: smooth(mk(), 0.0),
    "smooth.radius_infinite": lambda: smooth(mk(), float("inf")),
    "smooth.min_valid_range": lambda: smooth(mk(), 100.0, min_valid=1.5),
    "smooth.min_valid_bool": lambda: smooth(mk(), 100.0, min_valid=True),
    "smooth.min_valid_text": lambda: smooth(mk(), 100.0, min_valid="half"),
    "smooth.no_latitude": lambda: smooth(only_coords(f64(), arange(8, 45.0)), 100.0),
    "smooth.no_longitude": lambda: smooth(only_coords(f64(10.0, -10), f64()), 100.0),
    "smooth.latitude_range": lambda: smooth(moved(mk(), lat=LAT_FAR), 100.0),
    "smooth.latitude_nan": lambda: smooth(moved(mk(), lat=f64(40.0, 20, float("nan"), 0, -20)), 100.0),
    "smooth.latitudes_bent": lambda: smooth(moved(mk(), lat=LAT_BENT), 100.0),
    "smooth.latitudes_twice": lambda: smooth(moved(mk(), lat=f64(40.0, 20, 20, 0, -20)), 100.0),
    "smooth.spacing": lambda: smooth(moved(mk(), lon=IRREGULAR), 100.0),
    "smooth.spacing_descending": lambda: smooth(moved(mk(), lon=arange(8, -10.0, 100.0)), 100.0),
    "smooth.spacing_one_value": lambda: smooth(moved(mk(), lon=torch.full((8,), 20.0, dtype=torch.float64)), 100.0),
    "smooth.spacing_nan": lambda: smooth(moved(mk(), lon=f64(0.0, 10, 20, float("nan"), 40, 50, 60, 70)), 100.0),
    "smooth.both_groups": lambda: smooth(with_var(mk(), "atmos_vars", "2t", fill((1, 2, 2, 5, 8), 3)), 100.0),
    "smooth.rank": lambda: smooth(with_var(mk(), "surf_vars", "2t", fill((1, 2, 2, 5, 8), 3)), 100.0),
    "smooth.grid": lambda: smooth(with_var(mk(), "surf_vars", "2t", fill((1, 2, 5, 7), 3)), 100.0),
    "smooth.only_unknown": lambda: smooth(mk(), 100.0, only=("2t", "msl")),
    "smooth.no_variable": lambda: smooth(mk(surf=(), atmos=()), 100.0),
    "smooth.devices": lambda: smooth(one_on_meta(mk()), 100.0),
    "smooth.rows": lambda: smooth(moved(mk(n_lat=300, n_lon=2, atmos=()), lat=torch.linspace(60, -60, 300, dtype=torch.float64)), 6000.0),

    "conservative_regrid.not_batch": lambda: CR(3, 45.0),
    "conservative_regrid.band": lambda: CR(band(mk()), 45.0),
    "conservative_regrid.matrices": lambda: CR(matrices(mk()), 45.0),
    "conservative_regrid.res_and_lat": lambda: CR(mk(), 45.0, lat=LAT3),
    "conservative_regrid.no_target": lambda: CR(mk()),
    "conservative_regrid.lat_alone": lambda: CR(mk(), lat=LAT3),
    "conservative_regrid.min_valid_text": lambda: CR(mk(), 45.0, min_valid="half"),
    "conservative_regrid.min_valid_zero": lambda: CR(mk(), 45.0, min_valid=0.0),
    "conservative_regrid.res_range": lambda: CR(mk(), 120.0),
    "conservative_regrid.res_text": lambda: CR(mk(), "coarse"),
    "conservative_regrid.lat_tensor_matrix": lambda: CR(mk(), lat=torch.zeros(2, 2, dtype=torch.float64), lon=LON4),
    "conservative_regrid.lon_array_matrix": lambda: CR(mk(), lat=LAT3, lon=np.zeros((2, 2))),
    "conservative_regrid.source_one_latitude": lambda: CR(mk(n_lat=1), lat=LAT3, lon=LON4),
    "conservative_regrid.source_latitude_range": lambda: CR(moved(mk(), lat=LAT_FAR), lat=LAT3, lon=LON4),
    "conservative_regrid.source_latitudes_bent": lambda: CR(moved(mk(), lat=LAT_BENT), lat=LAT3, lon=LON4),
    "conservative_regrid.source_one_longitude": lambda: CR(mk(n_lon=1), lat=LAT3, lon=LON4),
    "conservative_regrid.source_longitude_range": lambda: CR(moved(mk(), lon=arange(8, 45.0, 45.0)), lat=LAT3, lon=LON4),
    "conservative_regrid.source_longitudes_descending": lambda: CR(moved(mk(), lon=arange(8, -10.0, 100.0)), lat=LAT3, lon=LON4),
    "conservative_regrid.target_one_latitude": lambda: CR(mk(), lat=f64(10.0), lon=LON4),
    "conservative_regrid.target_latitude_range": lambda: CR(mk(), lat=f64(-91.0, 0, 40), lon=LON4),
    "conservative_regrid.target_latitude_nan": lambda: CR(mk(), lat=f64(-40.0, float("nan"), 40), lon=LON4),
    "conservative_regrid.target_latitudes_bent": lambda: CR(mk(), lat=f64(-40.0, 40, 0), lon=LON4),
    "conservative_regrid.target_one_longitude": lambda: CR(mk(), lat=LAT3, lon=f64(10.0)),
    "conservative_regrid.target_longitude_range": lambda: CR(mk(), lat=LAT3, lon=f64(-10.0, 90, 180, 270)),
    "conservative_regrid.target_longitudes_twice": lambda: CR(mk(), lat=LAT3, lon=f64(0.0, 90, 90, 270)),
    "conservative_regrid.row_taps": lambda: CR(only_coords(torch.linspace(80, -80, 140, dtype=torch.float64), arange(8, 45.0)), lat=f64(40.0, -40), lon=LON4),
    "conservative_regrid.column_taps": lambda: CR(only_coords(f64(10.0, -10), arange(140, 360.0 / 140)), lat=f64(10.0, -10), lon=f64(0.0, 180)),
    "conservative_regrid.static_shape": lambda: CR(static(mk(), (5, 7)), 45.0),
    "conservative_regrid.rank": lambda: CR(with_var(mk(), "surf_vars", "2t", fill((1, 2, 2, 5, 8), 3)), 45.0),
    "conservative_regrid.devices": lambda: CR(one_on_meta(mk()), 45.0),

    "diagnostics.latitudes_bent": lambda: diagnostics(moved(mk(**WIND), lat=LAT_BENT), "ws"),
    "diagnostics.latitudes_twice": lambda: diagnostics(moved(mk(**WIND), lat=f64(40.0, 20, 20, 0, -20)), "ws"),
    "diagnostics.latitude_nan": lambda: diagnostics(moved(mk(**WIND), lat=f64(40.0, 20, float("nan"), 0, -20)), "ws"),
    "diagnostics.one_longitude": lambda: diagnostics(mk(n_lon=1, **WIND), "ws"),
    "diagnostics.spacing_regional": lambda: diagnostics(moved(mk(**WIND), lon=f64(100.0, 110, 120, 130, 140, 150, 160, 171)), "ws"),
    "diagnostics.spacing_descending": lambda: diagnostics(moved(mk(**WIND), lon=arange(8, -10.0, 100.0)), "ws"),
    "diagnostics.spacing_one_value": lambda: diagnostics(moved(mk(**WIND), lon=torch.full((8,), 20.0, dtype=torch.float64)), "ws"),
    "diagnostics.spacing_nan": lambda: diagnostics(moved(mk(**WIND), lon=f64(0.0, 10, 20, float("nan"), 40, 50, 60, 70)), "ws"),
}


def outcome(case):
    try:
        CASES[case]()
    except Exception as err:  # noqa: BLE001
        return type(err).__name__, str(err)
    return None, None


# ---- one fixed small input per entry point on three grids -----------------------------------------------------------------
GRIDS = {"wrap": (torch.linspace(-75, 75, 6, dtype=torch.float64), arange(12, 30.0)),
         "regional": (torch.linspace(-40, 40, 5, dtype=torch.float64), arange(7, 5.0, 10.0)),
         "descending": (torch.linspace(75, -75, 6, dtype=torch.float64), arange(12, 30.0))}
TARGETS = {"wrap": ((f64(-60.0, 0, 60), arange(6, 60.0, 15.0)), (f64(40.0, 10, -20), f64(40.0, 70, 100, 130))),
           "regional": ((f64(-30.0, 0, 30), f64(15.0, 25, 35)), (f64(35.0, 5), f64(8.0, 12, 16, 20))),
           "descending": ((f64(-60.0, 0, 60), arange(6, 60.0, 15.0)), (f64(40.0, 10, -20), f64(40.0, 70, 100, 130)))}
DIGEST_THR = {"ivt": [285.0, 295.0], "z": [[280.0, 290.0], [285.0, 299.0]]}
OBJECT_PROPERTIES = ("labels", "count", "table", "truncated", "thresholds", "points", "area", "centroid_row", "centroid_col",
                     "centroid_lat", "centroid_lon", "peak", "peak_row", "peak_col", "peak_lat", "peak_lon", "bbox")
MATCH_PROPERTIES = ("pairs", "count", "overflow", "truncated", "intersection", "iou", "fraction_of_a", "fraction_of_b", "distance_km",
                    "best_b", "best_b_fraction", "best_a", "best_a_fraction")
NEAREST_PROPERTIES = ("index", "key", "label", "distance_km")
SEPARATION_PROPERTIES = ("table", "hausdorff_bits", "distance_km", "nearest_b", "a_lat", "a_lon", "b_lat", "b_lon", "hausdorff_km")


def tensors(d) -> list[torch.Tensor]:
    """The tensors of a (nested) dict by variable, in the order of the names."""
    return [t for k in sorted(d) for t in (tensors(d[k]) if isinstance(d[k], dict) else [d[k]])]


def every(result, names) -> list[torch.Tensor]:
    return [t for name in names for t in tensors(getattr(result, name))]


def fields_of(b: Batch) -> list[torch.Tensor]:
    return [*tensors(b.surf_vars), *tensors(b.static_vars), *tensors(b.atmos_vars), b.metadata.lat, b.metadata.lon]


def digest_results(kind: str) -> dict[str, list[torch.Tensor]]:
    lat, lon = GRIDS[kind]
    on = dict(n_lat=lat.shape[0], n_lon=lon.shape[0], B=2)
    grid = lambda b: moved(b, lat, lon)  # noqa: E731
    fa, fb = (grid(holed(mk(surf=("ivt", "msl"), atmos=("z",), seed=s, **on), s)) for s in (3, 4))
    a = objects(fa, DIGEST_THR, max_objects=8)
    b = objects(fb, DIGEST_THR, connectivity=4, max_objects=6)
    low = objects(fa, {"msl": [282.0]}, below=True, wrap=(kind == "regional"), max_objects=3)
    m, few = object_matches(a, b), object_matches(a, b, max_pairs=2)
    n, near = nearest_event(b), nearest_event(b, 2500.0)
    s, close = object_separations(a, b), object_separations(a, b, 2500.0)
    back = s.cpu()
    assert back.b is back.nearest.objects
    shape = (lat.shape[0], lon.shape[0])
    whole = grid(static(holed(mk(surf=("2t",), atmos=("z",), seed=6, **on), 5), shape))
    (lat_c, lon_c), (lat_r, lon_r) = TARGETS[kind]
    out = {
        "objects": every(a, OBJECT_PROPERTIES) + every(b, OBJECT_PROPERTIES) + every(low, OBJECT_PROPERTIES)
        + [a.mask("ivt", 1), a.lat, a.lon, torch.tensor([a.wrap, b.wrap, low.wrap])] + every(a.cpu(), OBJECT_PROPERTIES),
        "object_matches": every(m, MATCH_PROPERTIES) + every(few, MATCH_PROPERTIES)
        + tensors(m.matched_a()) + tensors(m.matched_b(0.25)) + tensors(m.summary()) + tensors(m.summary(0.5)) + tensors(few.summary())
        + every(m.cpu(), MATCH_PROPERTIES),
        "nearest_event": every(n, NEAREST_PROPERTIES) + every(near, NEAREST_PROPERTIES) + every(near.cpu(), NEAREST_PROPERTIES),
        "object_separations": every(s, SEPARATION_PROPERTIES) + every(close, SEPARATION_PROPERTIES) + tensors(s.matched(3000.0))
        + tensors(close.matched(0.0)) + every(close.nearest, NEAREST_PROPERTIES) + every(back, SEPARATION_PROPERTIES),
        "smooth.one_row": fields_of(smooth(whole, 1000.0)),
        "smooth.rows": fields_of(smooth(whole, 4000.0, min_valid=0.25, keep_mask=False)),
        "smooth.only": fields_of(smooth(whole, 4000.0, only="z")),
        "conservative_regrid.coarser": fields_of(conservative_regrid(whole, lat=lat_c, lon=lon_c)),
        "conservative_regrid.regional": fields_of(conservative_regrid(whole, lat=lat_r, lon=lon_r, min_valid=0.9)),
        "diagnostics": fields_of(diagnostics(grid(holed(mk(seed=5, **WIND, **on), 2)),
                                             ("ws", "vo", "d", "10ws", "10vo", "10d", "tcwv", "ivtu", "ivtv", "ivt"))),
    }
    if kind != "regional":
        out["conservative_regrid.res"] = fields_of(conservative_regrid(whole, 60.0))
    return {f"{kind}.{k}": v for k, v in out.items()}


# ---- the wrap decision -------------------------------------------------------------------------------------------------------
AXES = {"circle_8": arange(8, 45.0), "shifted_8": arange(8, 45.0, 0.25 * 45.0), "regional_7": arange(7, 5.0, 10.0),
        "single": f64(20.0), "circle_4097": arange(4097, 360.0 / 4097)}


def seen_by(entry: str, lon: torch.Tensor):
    """Whether `entry` took the grid of `lon` as wrapping, read off what it returns: a field that is 1 in the last column and 0
    elsewhere reaches column 0 only across the seam."""
    W = lon.shape[0]
    step = 360.0 / W if W == 1 else float(lon[1] - lon[0])
    last = torch.zeros(1, 1, 2, W)
    last[..., -1] = 1.0
    md = derive_metadata(Metadata(f64(10.0, -10), f64(0.0, 180), TIME, (500, 850)), lon=lon)
    if entry == "objects":
        return objects(Batch({"2t": last}, {}, {}, md), {"2t": [0.5]}).wrap
    if entry == "diagnostics":                            # du/dlon in column 0: centred across the seam, or one-sided
        out = diagnostics(Batch({"10u": last, "10v": torch.zeros_like(last)}, {}, {}, md), "10d")
        return bool((out.surf_vars["10d"][..., 0] != 0).all())
    if entry == "smooth":                                 # a disc of 1.5 columns at the equator
        out = smooth(Batch({"2t": last[..., :1, :]}, {}, {}, derive_metadata(md, lat=f64(0.0))), 1.5 * step * 111.2)
        return bool((out.surf_vars["2t"][..., 0] > 0).all())
    if entry == "conservative_regrid":                    # the target cell of longitude 0 spans two columns to either side: covered on a full circle only
        out = conservative_regrid(Batch({"2t": torch.ones(1, 1, 2, W)}, {}, {}, md), lat=f64(10.0, -10), lon=f64(0.0, 4.0 * step), min_valid=0.99)
        return bool(torch.isfinite(out.surf_vars["2t"][..., 0]).all())
    raise KeyError(entry)


def wrap_results() -> dict[str, dict[str, object]]:
    """axis -> entry point -> True / False, or the type of the exception where the entry point refuses the axis."""
    out = {}
    for axis, lon in AXES.items():
        out[axis] = {}
        for entry in ("objects", "diagnostics", "smooth", "conservative_regrid"):
            if (entry, axis) == ("smooth", "single"):     # one column: nothing to reach
                continue
            try:
                out[axis][entry] = seen_by(entry, lon)
            except ValueError:
                out[axis][entry] = "ValueError"
    return out


MESSAGES = {
    'objects.not_batch': ('TypeError',
        'objects: batch must be a Batch, got int'),
    'objects.band': ('ValueError',
        'objects: batch is a latitude band (BandBatch); gather the forecast first, band objects are not supported'),
    'objects.matrices': ('ValueError',
        'objects: batch has matrices for latitudes / longitudes; vector coordinates are needed'),
    'objects.connectivity': ('ValueError',
        'objects: connectivity must be 4 or 8, got 6'),
    'objects.connectivity_bool': ('ValueError',
        'objects: connectivity must be 4 or 8, got True'),
    'objects.wrap': ('ValueError',
        "objects: wrap must be None, True or False, got 'yes'"),
    'objects.max_objects_zero': ('ValueError',
        'objects: max_objects must be a whole number of at least 1, got 0'),
    'objects.max_objects_fraction': ('ValueError',
        'objects: max_objects must be a whole number of at least 1, got 2.5'),
    'objects.max_objects_bool': ('ValueError',
        'objects: max_objects must be a whole number of at least 1, got True'),
    'objects.longitudes': ('ValueError',
        'objects: the grid has 4097 longitudes; 1 to 4096 are supported'),
    'objects.no_longitude': ('ValueError',
        'objects: the grid has 0 longitudes; 1 to 4096 are supported'),
    'objects.no_latitude': ('ValueError',
        'objects: the grid has 0 x 8 points; 1 to 2^31 - 2 fit an int32 label map'),
    'objects.points': ('ValueError',
        'objects: the grid has 524288 x 4096 points; 1 to 2^31 - 2 fit an int32 label map'),
    'objects.thresholds_not_mapping': ('ValueError',
        'objects: thresholds must be a non-empty mapping from variable name to values'),
    'objects.thresholds_empty': ('ValueError',
        'objects: thresholds must be a non-empty mapping from variable name to values'),
    'objects.thresholds_not_numbers': ('ValueError',
        "objects: the thresholds of '2t' must be numbers"),
    'objects.thresholds_surface_2d': ('ValueError',
        "objects: the thresholds of '2t' have shape (2, 2); a sequence is needed"),
    'objects.thresholds_levels': ('ValueError',
        "objects: the thresholds of 'z' have shape (3, 2); a (C, T) array needs C = 2 levels"),
    'objects.thresholds_3d': ('ValueError',
        "objects: the thresholds of 'z' have shape (2, 2, 2); a sequence or a (2, T) array is needed"),
    'objects.thresholds_scalar': ('ValueError',
        "objects: the thresholds of '2t' have shape (); a sequence is needed"),
    'objects.thresholds_none': ('ValueError',
        "objects: 1 to 8 thresholds per variable, '2t' has 0"),
    'objects.thresholds_nine': ('ValueError',
        "objects: 1 to 8 thresholds per variable, '2t' has 9"),
    'objects.thresholds_unknown': ('ValueError',
        "objects: thresholds name the variable 'msl', which batch does not hold as a surface or atmospheric variable"),
    'objects.both_groups': ('ValueError',
        "objects: '2t' is both a surface and an atmospheric variable"),
    'objects.rank': ('ValueError',
        "objects: pred.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'objects.grid': ('ValueError',
        "objects: pred.surf_vars['2t'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'objects.devices': ('ValueError',
        "objects: the fields are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"),
    'objects.latitude_range': ('ValueError',
        'scores: latitudes must be in the range [-90, 90]'),
    'objects.latitude_nan': ('ValueError',
        'scores: latitudes must be in the range [-90, 90]'),
    'objects.mask_unknown': ('KeyError',
        '"objects: no variable \'msl\'; the variables are (\'2t\', \'z\')"'),
    'object_matches.a_not_objects': ('TypeError',
        'object_matches: a must be an Objects (the result of aurora_amd.objects), got int'),
    'object_matches.b_not_objects': ('TypeError',
        'object_matches: b must be an Objects (the result of aurora_amd.objects), got str'),
    'object_matches.layout': ('ValueError',
        "object_matches: a and b differ in layout (variable, first plane, shape): (('2t', 0, (1,)), ('z', 1, (1, 2))) against (('2t', 0, (1,)),)"),
    'object_matches.thresholds': ('ValueError',
        'object_matches: a and b differ in the number of thresholds: 2 against 1'),
    'object_matches.grid': ('ValueError',
        'object_matches: a and b differ in grid: 5 x 8 against 5 x 7 points; regrid first'),
    'object_matches.device': ('ValueError',
        'object_matches: a is on cpu and b on meta; move both to the CPU (.cpu()) or label both on one GPU'),
    'object_matches.lat_values': ('ValueError',
        'object_matches: a and b differ in lat (same length, different values); regrid first'),
    'object_matches.lon_values': ('ValueError',
        'object_matches: a and b differ in lon (same length, different values); regrid first'),
    'object_matches.max_pairs_zero': ('ValueError',
        'object_matches: max_pairs must be a whole number from 1 to 8192, got 0'),
    'object_matches.max_pairs_many': ('ValueError',
        'object_matches: max_pairs must be a whole number from 1 to 8192, got 8193'),
    'object_matches.max_pairs_fraction': ('ValueError',
        'object_matches: max_pairs must be a whole number from 1 to 8192, got 2.5'),
    'object_matches.max_pairs_bool': ('ValueError',
        'object_matches: max_pairs must be a whole number from 1 to 8192, got True'),
    'nearest_event.not_objects': ('TypeError',
        'nearest_event: o must be an Objects (the result of aurora_amd.objects), got Batch'),
    'nearest_event.max_km_zero': ('ValueError',
        'nearest_event: max_km must be None or a positive finite number of kilometres, got 0.0'),
    'nearest_event.max_km_nan': ('ValueError',
        'nearest_event: max_km must be None or a positive finite number of kilometres, got nan'),
    'nearest_event.max_km_bool': ('ValueError',
        'nearest_event: max_km must be None or a positive finite number of kilometres, got True'),
    'nearest_event.max_km_text': ('ValueError',
        "nearest_event: max_km must be None or a positive finite number of kilometres, got '300'"),
    'nearest_event.latitude_range': ('ValueError',
        'nearest_event: latitudes must be in the range [-90, 90]'),
    'nearest_event.latitude_nan': ('ValueError',
        'nearest_event: latitudes must be in the range [-90, 90]'),
    'nearest_event.latitudes_bent': ('ValueError',
        'nearest_event: the latitudes must be strictly monotone (the row walk relies on rows farther away in index being farther away in latitude)'),
    'nearest_event.latitudes_twice': ('ValueError',
        'nearest_event: the latitudes must be strictly monotone (the row walk relies on rows farther away in index being farther away in latitude)'),
    'nearest_event.longitudes': ('ValueError',
        'nearest_event: the grid has 4097 longitudes; 1 to 4096 are supported'),
    'nearest_event.spacing_regional': ('ValueError',
        'nearest_event: the longitudes must be equally spaced (the nearest event of a row is found by its column gap)'),
    'nearest_event.spacing_wrapping': ('ValueError',
        'nearest_event: the longitudes must be equally spaced and cover the full circle on a wrapping grid'),
    'nearest_event.spacing_one_value': ('ValueError',
        'nearest_event: the longitudes must be equally spaced (the nearest event of a row is found by its column gap)'),
    'nearest_event.spacing_nan': ('ValueError',
        'nearest_event: the longitudes must be equally spaced (the nearest event of a row is found by its column gap)'),
    'object_separations.a_not_objects': ('TypeError',
        'object_separations: a must be an Objects (the result of aurora_amd.objects), got int'),
    'object_separations.b_not_objects': ('TypeError',
        'object_separations: b must be an Objects (the result of aurora_amd.objects), got str'),
    'object_separations.layout': ('ValueError',
        "object_separations: a and b differ in layout (variable, first plane, shape): (('2t', 0, (1,)), ('z', 1, (1, 2))) against (('2t', 0, (1,)),)"),
    'object_separations.thresholds': ('ValueError',
        'object_separations: a and b differ in the number of thresholds: 2 against 1'),
    'object_separations.grid': ('ValueError',
        'object_separations: a and b differ in grid: 5 x 8 against 5 x 7 points; regrid first'),
    'object_separations.device': ('ValueError',
        'object_separations: a is on cpu and b on meta; move both to the CPU (.cpu()) or label both on one GPU'),
    'object_separations.lat_values': ('ValueError',
        'object_separations: a and b differ in lat (same length, different values); regrid first'),
    'object_separations.lon_values': ('ValueError',
        'object_separations: a and b differ in lon (same length, different values); regrid first'),
    'object_separations.max_km': ('ValueError',
        'nearest_event: max_km must be None or a positive finite number of kilometres, got -1.0'),
    'object_separations.latitudes_bent': ('ValueError',
        'nearest_event: the latitudes must be strictly monotone (the row walk relies on rows farther away in index being farther away in latitude)'),
    'smooth.not_batch': ('TypeError',
        'smooth: batch must be a Batch, got int'),
    'smooth.band': ('ValueError',
        'smooth: batch is a latitude band (BandBatch); gather the forecast first, band fields are not supported'),
    'smooth.matrices': ('ValueError',
        'smooth: batch has matrices for latitudes / longitudes; vector coordinates are needed'),
    'smooth.radius_text': ('ValueError',
        "smooth: radius_km must be a finite number above 0, got 'wide'"),
    'smooth.radius_none': ('ValueError',
        'smooth: radius_km must be a finite number above 0, got None'),
    'smooth.radius_zero': ('ValueError',
        'smooth: radius_km must be a finite number above 0, got 0.0'),
    'smooth.radius_infinite': ('ValueError',
        'smooth: radius_km must be a finite number above 0, got inf'),
    'smooth.min_valid_range': ('ValueError',
        'smooth: min_valid must be a number in [0, 1], got 1.5'),
    'smooth.min_valid_bool': ('ValueError',
        'smooth: min_valid must be a number in [0, 1], got True'),
    'smooth.min_valid_text': ('ValueError',
        "smooth: min_valid must be a number in [0, 1], got 'half'"),
    'smooth.no_latitude': ('ValueError',
        'smooth: the grid has 0 latitudes and 8 longitudes; at least 1 of each is needed'),
    'smooth.no_longitude': ('ValueError',
        'smooth: the grid has 2 latitudes and 0 longitudes; at least 1 of each is needed'),
    'smooth.latitude_range': ('ValueError',
        'smooth: latitudes must be in the range [-90, 90]'),
    'smooth.latitude_nan': ('ValueError',
        'smooth: latitudes must be in the range [-90, 90]'),
    'smooth.latitudes_bent': ('ValueError',
        'smooth: the latitudes must be strictly monotonic'),
    'smooth.latitudes_twice': ('ValueError',
        'smooth: the latitudes must be strictly monotonic'),
    'smooth.spacing': ('ValueError',
        'smooth: the longitudes must be equally spaced'),
    'smooth.spacing_descending': ('ValueError',
        'smooth: the longitudes must be equally spaced'),
    'smooth.spacing_one_value': ('ValueError',
        'smooth: the longitudes must be equally spaced'),
    'smooth.spacing_nan': ('ValueError',
        'smooth: the longitudes must be equally spaced'),
    'smooth.both_groups': ('ValueError',
        "smooth: '2t' is both a surface and an atmospheric variable"),
    'smooth.rank': ('ValueError',
        "smooth: batch.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'smooth.grid': ('ValueError',
        "smooth: batch.surf_vars['2t'] has shape (1, 2, 5, 7), which does not fit a 5 x 8 grid"),
    'smooth.only_unknown': ('ValueError',
        "smooth: only names the variable 'msl', which batch does not hold as a surface or atmospheric variable"),
    'smooth.no_variable': ('ValueError',
        'smooth: batch holds no surface or atmospheric variable to smooth'),
    'smooth.devices': ('ValueError',
        "smooth: the fields are on ['cpu', 'meta']; move the batch to the CPU or to one GPU first"),
    'smooth.rows': ('ValueError',
        'smooth: a radius of 6000 km spans 269 latitude rows of this grid; at most 255 are supported, which allows any radius below 5712.426 km'),
    'conservative_regrid.not_batch': ('TypeError',
        'conservative_regrid: batch must be a Batch, got int'),
    'conservative_regrid.band': ('ValueError',
        'conservative_regrid: batch is a latitude band (BandBatch); gather the forecast first, band regrids are not supported'),
    'conservative_regrid.matrices': ('ValueError',
        'conservative_regrid: batch has matrices for latitudes / longitudes; vector coordinates are needed'),
    'conservative_regrid.res_and_lat': ('ValueError',
        'conservative_regrid: give either res or lat / lon, not both'),
    'conservative_regrid.no_target': ('ValueError',
        'conservative_regrid: give the target grid: res, or both lat and lon'),
    'conservative_regrid.lat_alone': ('ValueError',
        'conservative_regrid: give the target grid: res, or both lat and lon'),
    'conservative_regrid.min_valid_text': ('ValueError',
        "conservative_regrid: min_valid must be a number in (0, 1], got 'half'"),
    'conservative_regrid.min_valid_zero': ('ValueError',
        'conservative_regrid: min_valid must be in (0, 1], got 0.0'),
    'conservative_regrid.res_range': ('ValueError',
        'conservative_regrid: res must be a spacing in degrees in (0, 90], got 120.0'),
    'conservative_regrid.res_text': ('ValueError',
        "conservative_regrid: res must be a spacing in degrees in (0, 90], got 'coarse'"),
    'conservative_regrid.lat_tensor_matrix': ('ValueError',
        'conservative_regrid: lat must be a vector, got shape (2, 2)'),
    'conservative_regrid.lon_array_matrix': ('ValueError',
        'conservative_regrid: lon must be a vector, got shape (2, 2)'),
    'conservative_regrid.source_one_latitude': ('ValueError',
        'conservative_regrid: the latitudes of the batch must be a vector of at least 2 values'),
    'conservative_regrid.source_latitude_range': ('ValueError',
        'conservative_regrid: the latitudes of the batch must be in the range [-90, 90]'),
    'conservative_regrid.source_latitudes_bent': ('ValueError',
        'conservative_regrid: the latitudes of the batch must be strictly monotonic'),
    'conservative_regrid.source_one_longitude': ('ValueError',
        'conservative_regrid: the longitudes of the batch must be a vector of at least 2 values'),
    'conservative_regrid.source_longitude_range': ('ValueError',
        'conservative_regrid: the longitudes of the batch must be in the range [0, 360)'),
    'conservative_regrid.source_longitudes_descending': ('ValueError',
        'conservative_regrid: the longitudes of the batch must be strictly increasing'),
    'conservative_regrid.target_one_latitude': ('ValueError',
        'conservative_regrid: the latitudes of the target must be a vector of at least 2 values'),
    'conservative_regrid.target_latitude_range': ('ValueError',
        'conservative_regrid: the latitudes of the target must be in the range [-90, 90]'),
    'conservative_regrid.target_latitude_nan': ('ValueError',
        'conservative_regrid: the latitudes of the target must be in the range [-90, 90]'),
    'conservative_regrid.target_latitudes_bent': ('ValueError',
        'conservative_regrid: the latitudes of the target must be strictly monotonic'),
    'conservative_regrid.target_one_longitude': ('ValueError',
        'conservative_regrid: the longitudes of the target must be a vector of at least 2 values'),
    'conservative_regrid.target_longitude_range': ('ValueError',
        'conservative_regrid: the longitudes of the target must be in the range [0, 360)'),
    'conservative_regrid.target_longitudes_twice': ('ValueError',
        'conservative_regrid: the longitudes of the target must be strictly increasing'),
    'conservative_regrid.row_taps': ('ValueError',
        'conservative_regrid: a target cell overlaps 70 source rows; at most 64 are supported'),
    'conservative_regrid.column_taps': ('ValueError',
        'conservative_regrid: a target cell overlaps 71 source columns; at most 64 are supported'),
    'conservative_regrid.static_shape': ('ValueError',
        "conservative_regrid: batch.static_vars['lsm'] has shape (5, 7), which does not fit a 5 x 8 grid"),
    'conservative_regrid.rank': ('ValueError',
        "conservative_regrid: batch.surf_vars['2t'] has shape (1, 2, 2, 5, 8), which does not fit a 5 x 8 grid"),
    'conservative_regrid.devices': ('ValueError',
        "conservative_regrid: the fields and coordinates are on ['cpu', 'meta']; move the whole batch to the CPU or to one GPU first"),
    'diagnostics.latitudes_bent': ('ValueError',
        'diagnostics: the latitudes must be strictly monotonic'),
    'diagnostics.latitudes_twice': ('ValueError',
        'diagnostics: the latitudes must be strictly monotonic'),
    'diagnostics.latitude_nan': ('ValueError',
        'diagnostics: the latitudes must be strictly monotonic'),
    'diagnostics.one_longitude': ('ValueError',
        'diagnostics: the grid has 5 latitudes and 1 longitudes; at least 2 of each are needed'),
    'diagnostics.spacing_regional': ('ValueError',
        'diagnostics: the longitudes must be equally spaced'),
    'diagnostics.spacing_descending': ('ValueError',
        'diagnostics: the longitudes must be equally spaced'),
    'diagnostics.spacing_one_value': ('ValueError',
        'diagnostics: the longitudes must be equally spaced'),
    'diagnostics.spacing_nan': ('ValueError',
        'diagnostics: the longitudes must be equally spaced'),
}
DIGESTS = {
    'wrap.objects': 'ded234f5be281a28c7ba596466e046e9b282fe1c4d43828b843e7ca183b66bad',
    'wrap.object_matches': '31c9ae80a65a7d76d1a9aee580367b4bd91f049c4c5fb9acac3b90bb4eaf6061',
    'wrap.nearest_event': '8732c2b11b17bb1edc687ec70459245137d15ce8c2d82646bffae1efd1235803',
    'wrap.object_separations': '83981cc7cdf62b74b992e1b6a71b01958ba07abe139000c08d1dd10462690e12',
    'wrap.smooth.one_row': '9df2c37c18cb821aadb1dd664f4b83081cc3fdded0c1e56af39816b2a7647f2a',
    'wrap.smooth.rows': '8e0ab9bfd270092dab789caf41d232250f7d1f2b0641505b78555a46bc02f413',
    'wrap.smooth.only': 'f090056578e537847d26017244f5c0b5874f912b83dfbd7e7d9b409508854557',
    'wrap.conservative_regrid.coarser': 'a0c4682a3de00d73477e868ae1deb615c72b59dc13f60cbe8561dd81e4474f64',
    'wrap.conservative_regrid.regional': '77676087021a990fad6d317c9daa0c081fcaf032a41992b4f08a15f4c1cd3d22',
    'wrap.diagnostics': '23076f02af8ccb5184508080445f9cb56f0ab24091c61b16f485f979e79f5779',
    'wrap.conservative_regrid.res': 'f525f92260379a969a55727dbc3ffe201212b0455cdaf908617837e5652d23b9',
    'regional.objects': 'c144bb40308ba469a966c94194f53de9561630974249aa89b3f58c5cfcb57f73',
    'regional.object_matches': '2099766c668f1705526a54d3b39a1a38ea847ecf2259295a4a979ae4927283be',
    'regional.nearest_event': 'ebbb955fb14c62684022eb72a61114087ac541b85b25f7c7dfc8eded1cc124be',
    'regional.object_separations': '48c69cd044176b354458381d33a19bbd42dd411a60ad37af0546d0b7f8ca80a5',
    'regional.smooth.one_row': 'ff45bb583ac7b17f1aa198383eb2e679d3d100157a8942cc23946500374c19aa',
    'regional.smooth.rows': 'b0615b1ff2016eee5413d759b84b2e729e15670bf716cca0390325e7298fc374',
    'regional.smooth.only': '68d2330dab58b0e41ea59d89345b9af39dee89dab758ec95975d9e0d73e9dbe1',
    'regional.conservative_regrid.coarser': 'a0996cb4169e0982eb515c5d3e3b1fd8a90f9d5c06c037078e0f2c5736df31e2',
    'regional.conservative_regrid.regional': '50e3d100a3d21955e4f1dd04fc526456a755d8a7716ec94988414342188769e7',
    'regional.diagnostics': '1943d913facca4b2b9b3681d5073033f1a850551842a84437730b0b25de11177',
    'descending.objects': 'd69c5d884100aed5a22550d6dced8b883e0e4aa2819b696cd4f03bb349a1c32c',
    'descending.object_matches': '31c9ae80a65a7d76d1a9aee580367b4bd91f049c4c5fb9acac3b90bb4eaf6061',
    'descending.nearest_event': '8732c2b11b17bb1edc687ec70459245137d15ce8c2d82646bffae1efd1235803',
    'descending.object_separations': 'ccb6740bd4914d9f6bb7ca5136c976e72a0996f7aac5b84c72e89afab35c3cc2',
    'descending.smooth.one_row': 'd51800c1600de2dc20d130710f6b87181982fd81d8c59094574ac9f2bf3ea940',
    'descending.smooth.rows': '964134e1d3326df5b7a78ab6f1ac702fdb65abfca2997eab34c7b5b8b6d9ae0f',
    'descending.smooth.only': '870c69ccbabd14bad337a2ab3d6b6ae157a64c52e1cdad235f5b64f40254b81d',
    'descending.conservative_regrid.coarser': '71e40c4ec318da219b970c490e53931f2ceb01e591a49b8486d85cd0adad5f43',
    'descending.conservative_regrid.regional': '4fbc314032296f447df596e643590b15cff5389ae77f08ef01fc2ac780162564',
    'descending.diagnostics': 'f0112bcc27e684e5f1390fb2db35938c33efdec1add79de8387c4a97ec022df5',
    'descending.conservative_regrid.res': '20be9ddace59b64cfd8610cb01f8809e41e06e503d567f4d9a0784d936ef846e',
}
FULL_CIRCLE = {"circle_8": True, "shifted_8": True, "regional_7": False, "single": False, "circle_4097": False}
REFUSED = {("objects", "circle_4097"), ("diagnostics", "single"), ("conservative_regrid", "single")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_message(case):
    assert case in MESSAGES, f"{case} has no recorded message: python tests/test_object_chain_messages.py"
    assert outcome(case) == MESSAGES[case]


def test_every_case_raises():
    assert set(MESSAGES) == set(CASES) and all(kind is not None for kind, _ in MESSAGES.values())


@pytest.mark.parametrize("kind", sorted(GRIDS))
def test_host_numbers_keep_their_bits(kind):
    got = {k: sha(v) for k, v in digest_results(kind).items()}
    assert got == {k: v for k, v in DIGESTS.items() if k.startswith(kind + ".")}


def test_wrap_follows_the_full_circle():
    """Every entry point takes a grid as wrapping exactly where its longitudes count as a full circle -- 2 to 4096 equally spaced
    values at a step of 360 / n -- or refuses the axis.  4097 longitudes around the circle are NOT one: `objects` refuses them,
    the others take the grid as regional."""
    for axis, by_entry in wrap_results().items():
        for entry, seen in by_entry.items():
            assert seen == ("ValueError" if (entry, axis) in REFUSED else FULL_CIRCLE[axis]), (axis, entry, seen)


if __name__ == "__main__":
    print("MESSAGES = {")
    for case in CASES:
        kind, text = outcome(case)
        print(f"    {case!r}: ({kind!r},\n        {text!r}),")
    print("}")
    print("DIGESTS = {")
    for kind in GRIDS:
        for k, v in digest_results(kind).items():
            print(f"    {k!r}: {sha(v)!r},")
    print("}")
    print("wrap:", wrap_results())
