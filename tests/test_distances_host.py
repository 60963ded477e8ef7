"""`aurora_amd.nearest_event` and `aurora_amd.object_separations` on the CPU against yardsticks written here: a plain-Python brute
force of THE RULE (aurora_amd/distances.py) -- every point against every row candidate, the key by Python floats, which round
every operation on its own -- and a dict-and-loop evaluation of the separations.  index, key and the integer tables are compared
exactly.  tests/test_gpu_distances.py compares the kernels with the CPU path on inputs made here."""
import ctypes
import dataclasses
import importlib
import math
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import nearest_event, object_matches, object_separations, objects
from aurora_amd.diagnostics import EARTH_RADIUS
from aurora_amd.object_matches import haversine_km
from tests.test_object_matches_host import objects_of
from tests.test_objects_host import HAND, batch_of, patterns

mod = importlib.import_module("aurora_amd.distances")
ROOT = Path(__file__).resolve().parents[1]
INF_BITS = 0x7FF0000000000000


# ---- grids -----------------------------------------------------------------------------------------------------------------
def lats(H, kind="poles"):
    """poles: 90 .. -90 descending (rows at both poles); up: -80 .. 80 ascending; one row: 37.5 degrees."""
    if H == 1:
        return np.array([37.5])
    return np.linspace(90, -90, H) if kind == "poles" else np.linspace(-80, 80, H)


def lons(W, wrap):
    return np.linspace(0, 360, W + 1)[:-1] if wrap else 10.0 + 0.5 * np.arange(W)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def brute(labels, lat, lon, wrap, max_km=None):
    """(index, key) of one label map by THE RULE, in plain Python; the tables in numpy, as the rule says."""
    H, W = labels.shape
    s = np.sin(np.deg2rad(lat)).tolist()
    c = np.maximum(np.cos(np.deg2rad(lat)), 0.0).tolist()
    step = 0.0 if W == 1 else (360.0 / W if wrap else (lon[-1] - lon[0]) / (W - 1))
    cd = np.cos(np.deg2rad(np.arange(W) * step)).tolist()
    cd[0] = 1.0
    key_max = math.inf if max_km is None else float(1.0 - np.cos(min(max_km * 1000.0 / EARTH_RADIUS, math.pi)))
    gap = lambda j, e: min(abs(j - e), W - abs(j - e)) if wrap else abs(j - e)  # noqa: E731
    cand = []
    for k in range(H):
        events = [e for e in range(W) if labels[k, e] > 0]
        cand.append([min(events, key=lambda e: (gap(j, e), e)) for j in range(W)] if events else None)
    index, key = np.full((H, W), -1, np.int32), np.full((H, W), np.inf)
    for i in range(H):
        for j in range(W):
            best = (math.inf, -1)
            for k in range(H):
                if cand[k] is None:
                    continue
                e = cand[k][j]
                m1 = s[i] * s[k]
                m2 = c[i] * c[k]
                m3 = m2 * cd[gap(j, e)]
                a = m1 + m3
                v = max(1.0 - a, 0.0)
                if k == i and e == j:
                    v = 0.0
                if v <= key_max and (v, k * W + e) < best:
                    best = (v, k * W + e)
            index[i, j], key[i, j] = best[1], best[0]
    return index, key


def assert_rule(labels, lat, lon, wrap, max_km=None):
    labels = np.asarray(labels, dtype=np.int32)
    got = mod.nearest_of(labels, *mod.tables_of(lat, lon, wrap), wrap, mod.key_max_of(max_km))
    want = brute(labels, lat, lon, wrap, max_km)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    return got


def sprinkle(H, W, density=0.03, seed=0):
    """Labels -1 .. 3, positive at about `density` of the points."""
    g = np.random.default_rng(seed + 31 * H + W)
    return np.where(g.random((H, W)) < density, g.integers(1, 4, (H, W)), g.integers(-1, 1, (H, W))).astype(np.int32)


# ---- nearest_event against the brute force --------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (1, 2, 63, 64, 65, 129))
@pytest.mark.parametrize("H", (1, 2, 24))
def test_widths_and_heights_equal_the_brute_force(H, W):
    labels = sprinkle(H, W)
    assert_rule(labels, lats(H), lons(W, True), True)                               # wrapping, descending, pole rows
    assert_rule(labels, lats(H, "up"), lons(W, False), False)                       # regional, ascending


def test_empty_full_and_one_event():
    lat, lon = lats(6), lons(70, True)
    index, key = assert_rule(np.zeros((6, 70)), lat, lon, True)
    assert (index == -1).all() and np.isinf(key).all()
    index, key = assert_rule(np.ones((6, 70)), lat, lon, True)
    assert np.array_equal(index, np.arange(6 * 70).reshape(6, 70)) and not key.any()   # every point its own, key exactly 0
    for at in ((0, 0), (23, 129), (11, 64)):                                        # corners: the longest walks
        one = np.zeros((24, 130), np.int32)
        one[at] = 7
        for wrap in (True, False):
            index, _ = assert_rule(one, lats(24), lons(130, wrap), wrap)
            assert (index == at[0] * 130 + at[1]).all()


def test_events_only_in_the_pole_rows():
    labels = np.zeros((24, 65), np.int32)
    labels[0, [3, 40]], labels[23, 17] = 1, 2
    index, key = assert_rule(labels, lats(24), lons(65, True), True)
    assert set(np.unique(index)) <= {3, 40, 23 * 65 + 17}
    assert_rule(labels, lats(24)[::-1].copy(), lons(65, False), False)              # ascending with pole rows


def test_ties_go_to_the_smaller_column_and_the_smaller_flat_index():
    lat, lon = np.array([20.0, 10.0, 0.0, -10.0, -20.0]), lons(12, True)
    seam = np.zeros((5, 12), np.int32)
    seam[2, [2, 10]] = 1                                                            # two columns east and two west of column 0
    index, key = assert_rule(seam, lat, lon, True)
    assert index[2, 0] == 2 * 12 + 2 and index[2, 6] == 2 * 12 + 2 and index[2, 11] == 2 * 12 + 10
    assert assert_rule(seam, lat, lons(12, False), False)[0][2, 0] == 2 * 12 + 2    # without the seam column 2 is simply nearer
    opposite = np.zeros((5, 12), np.int32)
    opposite[1, 9] = 1                                                              # six columns from column 3 either way: one event
    assert assert_rule(opposite, lat, lon, True)[0][1, 3] == 12 + 9
    north_south = np.zeros((5, 12), np.int32)
    north_south[[0, 4], 3] = 1
    index, key = assert_rule(north_south, lat, lon, True)
    s, c, _ = mod.tables_of(lat, lon, True)
    assert mod._keys(s[2], c[2], s[0], c[0], 1.0) == mod._keys(s[2], c[2], s[4], c[4], 1.0)   # twenty degrees north and south
    assert index[2, 3] == 3 and index[3, 3] == 4 * 12 + 3 and index[1, 3] == 3      # equal keys: the smaller flat index, row 0


def test_max_km_cuts_some_all_and_none():
    labels = np.zeros((24, 130), np.int32)
    labels[5, 20], labels[18, 100] = 1, 2
    lat, lon = lats(24, "up"), lons(130, True)
    free = assert_rule(labels, lat, lon, True)
    some = assert_rule(labels, lat, lon, True, max_km=2500.0)
    assert (some[0] >= 0).any() and (some[0] < 0).any()
    reached = some[0] >= 0
    assert np.array_equal(some[0][reached], free[0][reached]) and np.array_equal(some[1][reached], free[1][reached])
    assert (free[1][~reached] > mod.key_max_of(2500.0)).all()
    nothing = assert_rule(labels, lat, lon, True, max_km=1e-3)
    assert (nothing[0] >= 0).sum() == 2 and nothing[1][5, 20] == 0                  # an event always reaches itself
    everything = assert_rule(labels, lat, lon, True, max_km=30000.0)                # more than half the circumference
    assert np.array_equal(everything[0], free[0]) and mod.key_max_of(30000.0) == 2.0


# ---- the front end ---------------------------------------------------------------------------------------------------------
def objects_on(labels, lat, lon, wrap, max_objects=64):
    """CPU `Objects` around (n, T, H, W) label maps on the given grid."""
    o = objects_of(labels, max_objects=max_objects, lat=lat)
    return dataclasses.replace(o, lon=torch.from_numpy(np.array(lon, dtype=np.float64)), wrap=wrap)


def test_nearest_event_of_objects_labels_and_distances():
    labels = np.stack([sprinkle(24, 130, 0.02, seed=s) for s in range(4)]).reshape(2, 2, 24, 130)
    for wrap in (True, False):
        lat, lon = lats(24, "up"), (lons(130, True) if wrap else 10.0 + 2.5 * np.arange(130))
        o = objects_on(labels, lat, lon, wrap)
        n = nearest_event(o)
        assert n.index["x"].shape == (2, 2, 24, 130) and n.index["x"].dtype == torch.int32 and n.key["x"].dtype == torch.float64
        for at in np.ndindex(2, 2):
            want = brute(labels[at], lat, lon, wrap)
            assert np.array_equal(n.index["x"][at].numpy(), want[0]) and np.array_equal(n.key["x"][at].numpy(), want[1])
        index = n.index["x"].numpy().astype(np.int64)
        assert np.array_equal(n.label["x"].numpy(), np.take_along_axis(labels.reshape(2, 2, -1), index.reshape(2, 2, -1), -1).reshape(labels.shape))
        # distance_km is 2 R asin(sqrt(key / 2)) and haversine_km another formula for the same angle t.  A key is off by at most
        # 4e-15 (five roundings, 3.9e-16; the sine and cosine tables, 1.3e-15; the cosine of the longitude gap, whose argument
        # reaches 2 pi, 2.2e-15), d(distance) / d(key) = R / sin t, and the haversine's h has the same conditioning with an error of
        # a few 1e-16.  On these grids two different points are at least 40 km apart (2.5 degrees of longitude at 80 degrees
        # north) and every nearest event is far from the antipode, so sin t >= 6.2e-3 -- asserted below -- and the two differ by
        # at most 6371 km x 5e-15 / 6.2e-3 = 5e-9 km, plus a few ulps of the polynomials: far inside 1e-6 km + 1e-9 relative.
        rows, cols = np.divmod(index, 130)
        here_lat, here_lon = np.broadcast_to(lat[:, None], labels.shape), np.broadcast_to(lon[None], labels.shape)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))  # noqa: E731
        want = haversine_km(t(here_lat), t(here_lon), t(lat[rows]), t(lon[cols])).numpy()
        got = n.distance_km["x"].numpy()
        apart = got > 0
        assert np.sin(want[apart] * 1000.0 / EARTH_RADIUS).min() >= 6.2e-3 and want[apart].min() >= 40.0
        print("distance_km against haversine_km: largest difference", np.abs(got - want).max(), "km")
        assert np.all(np.abs(got - want) <= 1e-6 + 1e-9 * want)
        assert np.array_equal(got == 0, labels > 0) and (got[labels > 0] == 0).all()   # exactly 0 on events, and only there
    none = nearest_event(objects_on(np.zeros((1, 1, 5, 7), np.int32), lats(5), lons(7, True), True))
    assert torch.isnan(none.distance_km["x"]).all() and not none.label["x"].any() and (none.index["x"] == -1).all()
    bounded = nearest_event(o, max_km=800.0)
    far = bounded.index["x"] < 0
    assert far.any() and torch.isnan(bounded.distance_km["x"][far]).all() and (bounded.distance_km["x"][~far] <= 800.0).all()
    assert bounded.cpu().max_km == 800.0 and (n.distance_km["x"][far] > 800.0).all()


@pytest.mark.parametrize("name", ("seam", "band", "comb", "serpentine", "rings", "special", "hand"))
def test_patterns_through_objects_equal_the_brute_force(name):
    plane = np.asarray(patterns()[name], dtype=np.float32)
    o = objects(batch_of(plane[None]), {"x": [0.5]}, wrap=True, max_objects=64)
    n = nearest_event(o)
    want = brute(o.labels["x"][0, 0].numpy(), o.lat.numpy(), o.lon.numpy(), True)
    assert np.array_equal(n.index["x"][0, 0].numpy(), want[0]) and np.array_equal(n.key["x"][0, 0].numpy(), want[1])


# ---- object_separations against a dict and a loop --------------------------------------------------------------------------------
def separations_yardstick(la, key, index, count, max_objects):
    least = {}
    hausdorff = 0
    bits = key.view(np.int64)
    H, W = la.shape
    for i in range(H):
        for j in range(W):
            k = int(la[i, j])
            if k <= 0:
                continue
            hausdorff = max(hausdorff, int(bits[i, j]))
            if k <= max_objects:
                entry = (int(bits[i, j]), i * W + j, int(index[i, j]))
                least[k] = min(least.get(k, entry), entry)
    rows = np.zeros((max_objects, 3), dtype=np.int64)
    for r in range(min(count, max_objects)):
        b, p, q = least.get(r + 1, (INF_BITS, -1, -1))
        rows[r] = [b, p, q] if b != INF_BITS else [INF_BITS, -1, -1]
    return rows, hausdorff


def assert_separations(s):
    la, key, index = s.a.labels_table.numpy(), s.nearest.key_table.numpy(), s.nearest.index_table.numpy()
    assert s.table_table.dtype == torch.int64 and s.hausdorff_table.dtype == torch.int64
    assert tuple(s.table_table.shape) == (*la.shape[:2], s.a.max_objects, 3) and tuple(s.hausdorff_table.shape) == la.shape[:2]
    for at in np.ndindex(*la.shape[:2]):
        rows, hausdorff = separations_yardstick(la[at], key[at], index[at], int(s.a.count_table[at]), s.a.max_objects)
        assert np.array_equal(s.table_table[at].numpy(), rows), (at, s.table_table[at].numpy()[:8], rows[:8])
        assert int(s.hausdorff_table[at]) == hausdorff


@pytest.mark.parametrize("name", ("seam", "band", "comb", "serpentine", "rings", "special", "hand"))
def test_patterns_shifted_equal_the_loop_and_touching_is_overlapping(name):
    plane = np.asarray(patterns()[name], dtype=np.float32)
    lat = np.linspace(80, -80, plane.shape[0])                                    # no row at a pole: every overlap has an area
    a = objects(batch_of(plane[None], lat=lat), {"x": [0.5, 1.5]}, wrap=True, max_objects=64)
    b = objects(batch_of(np.roll(plane, 2, axis=1)[None], lat=lat), {"x": [0.5, 1.5]}, wrap=True, max_objects=64)
    for max_km in (None, 900.0):
        s = object_separations(a, b, max_km)
        assert_separations(s)
        assert torch.equal(s.matched(0.0)["x"], object_matches(a, b, max_pairs=512).matched_a()["x"])


def test_separations_ties_truncation_and_finalisation():
    lat, lon = np.linspace(40, -40, 9), lons(12, True)
    la, lb = np.zeros((1, 1, 9, 12), np.int32), np.zeros((1, 1, 9, 12), np.int32)
    la[0, 0, 2, [3, 7]] = 1                                                        # both two columns from b's object 2: a tie on a_point
    la[0, 0, 6, 0:2] = 2
    la[0, 0, 0, 1] = 5                                                             # no row with max_objects = 4; 3 and 4 have no point
    lb[0, 0, 2, 5], lb[0, 0, 6, 1], lb[0, 0, 0, 0] = 2, 1, 9                       # 9: no row in b, an event all the same
    a, b = objects_on(la, lat, lon, True, max_objects=4), objects_on(lb, lat, lon, True, max_objects=4)
    s = object_separations(a, b)
    assert_separations(s)
    t = s.table["x"][0, 0]
    assert t[0, 1:].tolist() == [2 * 12 + 3, 2 * 12 + 5] and t[1].tolist() == [0, 6 * 12 + 1, 6 * 12 + 1]
    assert t[2].tolist() == [INF_BITS, -1, -1] and t[3].tolist() == [INF_BITS, -1, -1]   # numbers without points, below count = 5
    assert s.nearest_b["x"][0, 0].tolist() == [2, 1, 0, 0] and s.distance_km["x"][0, 0, 1] == 0
    assert s.matched(0.0)["x"][0, 0].tolist() == [False, True, False, False] and s.matched(1e5)["x"][0, 0].tolist() == [True, True, False, False]
    assert s.a_lat["x"][0, 0, 0] == 20 and s.a_lon["x"][0, 0, 0] == 90 and s.b_lon["x"][0, 0, 0] == 150 and torch.isnan(s.b_lat["x"][0, 0, 2])
    assert torch.isinf(s.distance_km["x"][0, 0, 2]) and s.cpu().table["x"].shape == (1, 1, 4, 3)
    # the point of object 5 is nearest to b's 9 next to it: neither has a row, and it counts in the Hausdorff cell
    assert int(s.nearest.index["x"][0, 0, 0, 1]) == 0 and int(s.hausdorff_bits["x"][0, 0]) == int(s.nearest.key_table[0, 0].view(torch.int64)[la[0, 0] > 0].max())
    # rows past count are zero, and NaN / 0 when finalised
    few = object_separations(objects_on(np.where(la == 5, 0, la), lat, lon, True, max_objects=4), b)
    assert_separations(few)
    assert not few.table["x"][0, 0, 2:].any() and torch.isnan(few.distance_km["x"][0, 0, 2:]).all()
    # nothing in reach: +inf in the table and in the Hausdorff cell; no event in a: the bits of 0
    near = object_separations(a, b, max_km=100.0)
    assert_separations(near)
    assert near.table["x"][0, 0, 0].tolist() == [INF_BITS, -1, -1] and int(near.hausdorff_bits["x"][0, 0]) == INF_BITS
    assert torch.isinf(near.hausdorff_km["x"]).all() and near.table["x"][0, 0, 1, 0] == 0
    empty = object_separations(objects_on(np.zeros_like(la), lat, lon, True), b)
    assert int(empty.hausdorff_bits["x"][0, 0]) == 0 and float(empty.hausdorff_km["x"][0, 0]) == 0 and not empty.table["x"].any()


def test_symmetric_hausdorff_along_a_meridian():
    lat, lon = np.linspace(40, -40, 9), lons(12, True)                             # rows ten degrees apart
    la, lb = np.zeros((1, 1, 9, 12), np.int32), np.zeros((1, 1, 9, 12), np.int32)
    la[0, 0, [1, 3], 5], lb[0, 0, 4, 5] = 1, 1
    a, b = objects_on(la, lat, lon, True), objects_on(lb, lat, lon, True)
    ab, ba = object_separations(a, b), object_separations(b, a)
    step = math.radians(10.0) * EARTH_RADIUS / 1000.0
    # three rows from (1, 5) to (4, 5) one way, one row from (4, 5) to (3, 5) the other; sin t >= 0.17, so by the bound above
    # the kilometres are good to 1e-9
    assert abs(float(ab.hausdorff_km["x"][0, 0]) - 3 * step) <= 1e-6 and abs(float(ba.hausdorff_km["x"][0, 0]) - step) <= 1e-6
    symmetric = torch.maximum(ab.hausdorff_km["x"], ba.hausdorff_km["x"])
    assert abs(float(symmetric[0, 0]) - 3 * step) <= 1e-6
    assert abs(float(ab.distance_km["x"][0, 0, 0]) - step) <= 1e-6 and ab.table["x"][0, 0, 0, 1:].tolist() == [3 * 12 + 5, 4 * 12 + 5]


def test_atmospheric_variables_come_back_in_the_layout_of_objects():
    g = np.random.default_rng(5)
    surf, atmos = g.random((2, 7, 10)).astype(np.float32), g.random((2, 3, 7, 10)).astype(np.float32)
    thr = {"a": np.array([[0.6, 0.9], [0.7, 0.95], [0.8, np.nan]]), "x": [0.85]}
    a = objects(batch_of(surf, atmos), thr, wrap=True, max_objects=32)
    b = objects(batch_of(np.roll(surf, 3, axis=-1), np.roll(atmos, 2, axis=-2)), thr, wrap=True, max_objects=16)
    s = object_separations(a, b)
    assert s.table["a"].shape == (2, 3, 2, 32, 3) and s.table["x"].shape == (2, 2, 32, 3) and s.hausdorff_km["a"].shape == (2, 3, 2)
    assert s.nearest.index["a"].shape == (2, 3, 2, 7, 10) and s.distance_km["x"].shape == (2, 2, 32) and s.matched(500.0)["a"].shape == (2, 3, 2, 32)
    assert_separations(s)
    assert not s.table["x"][:, 1].any() and (s.nearest.index["a"][:, 2, 1] == -1).all()   # the padded threshold: NaN, no events


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refused_inputs_say_why():
    a = objects(batch_of(HAND[None]), {"x": [0.5]}, wrap=False)
    with pytest.raises(TypeError, match="nearest_event: o must be an Objects"):
        nearest_event(a.labels_table)
    uneven = a.lon.clone()
    uneven[5] += 0.01
    with pytest.raises(ValueError, match="nearest_event: the longitudes must be equally spaced"):
        nearest_event(dataclasses.replace(a, lon=uneven))
    with pytest.raises(ValueError, match="nearest_event: the longitudes must be equally spaced and cover the full circle"):
        nearest_event(dataclasses.replace(a, lon=a.lon * 0.5, wrap=True))
    folded = a.lat.clone()
    folded[4] = folded[2]
    with pytest.raises(ValueError, match="nearest_event: the latitudes must be strictly monotone"):
        nearest_event(dataclasses.replace(a, lat=folded))
    for bad in (0, -5.0, float("inf"), float("nan"), True, "300"):
        with pytest.raises(ValueError, match="nearest_event: max_km must be None or a positive finite number"):
            nearest_event(a, max_km=bad)
        with pytest.raises(ValueError, match="nearest_event: max_km must be None or a positive finite number"):
            object_separations(a, a, max_km=bad)
    with pytest.raises(TypeError, match="object_separations: b must be an Objects .* got Tensor"):
        object_separations(a, a.labels_table)
    with pytest.raises(ValueError, match="object_separations: a and b differ in the number of thresholds: 1 against 2"):
        object_separations(a, objects(batch_of(HAND[None]), {"x": [0.5, 0.7]}, wrap=False))
    with pytest.raises(ValueError, match="object_separations: a and b differ in grid: 9 x 12 against 9 x 11 points"):
        object_separations(a, objects(batch_of(HAND[None, :, :11]), {"x": [0.5]}, wrap=False))
    with pytest.raises(ValueError, match="object_separations: a and b differ in lat"):
        object_separations(a, objects(batch_of(HAND[None], lat=np.linspace(80, -80, 9)), {"x": [0.5]}, wrap=False))
    with pytest.raises(ValueError, match="object_separations: a and b differ in lon"):
        object_separations(a, dataclasses.replace(a, lon=a.lon + 1.0))
    with pytest.raises(ValueError, match="object_separations: a and b differ in layout"):
        object_separations(a, dataclasses.replace(a, layout=(("y", 0, (1,)),)))
    with pytest.raises(ValueError, match="object_separations: a is on cpu and b on meta; move both"):
        object_separations(a, dataclasses.replace(a, labels_table=a.labels_table.to("meta")))
    other = objects(batch_of(HAND[None]), {"x": [0.25]}, wrap=True, connectivity=4, max_objects=16)   # what may differ does
    assert object_separations(a, other).table["x"].shape == (1, 1, 4096, 3)


def test_the_c_entry_points_refuse_before_any_launch():
    from aurora_amd.engine import lib

    raw, header = lib.load(), (lib.library_path().parents[2] / "include" / "aurora_hip.h").read_text()
    for name in ("aurora_hip_nearest_event", "aurora_hip_nearest_event_workspace_bytes", "aurora_hip_object_separations"):
        assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    assert "nearest_event.hip" in __import__("aurora_amd.build", fromlist=["SOURCES"]).SOURCES
    assert aurora_amd.nearest_event is mod.nearest_event and aurora_amd.object_separations is mod.object_separations
    assert {"nearest_event", "NearestEvent", "object_separations", "ObjectSeparations"} <= set(aurora_amd.__all__)
    assert "2^-46" in header and mod.MARGIN == 2.0 ** -46
    assert "70368744177664.0" in (ROOT / "aurora_amd" / "csrc" / "nearest_event_search.h").read_text() and 2 ** 46 == 70368744177664
    up8 = lambda b: (b + 7) // 8 * 8  # noqa: E731
    for n, H, W in ((1, 1, 1), (3, 9, 13), (17, 721, 1440), (2, 5, 4096)):
        assert raw.aurora_hip_nearest_event_workspace_bytes(n, H, W) == up8(2 * n * H * W) + up8(4 * n * H) + 8 * n
    assert raw.aurora_hip_nearest_event_workspace_bytes(1, 9, 4097) == 0 and raw.aurora_hip_nearest_event_workspace_bytes(-1, 9, 12) == 0
    err = lambda: raw.aurora_hip_last_error()  # noqa: E731
    need = raw.aurora_hip_nearest_event_workspace_bytes(6, 9, 12)
    args = lambda **kw: tuple({**dict(labels=16, n_items=6, n_lat=9, n_lon=12, tables=16, wrap=1, key_max=math.inf, index=16, key=16,  # noqa: E731
                                     ws=16, ws_size=need, stream=None), **kw}.values())
    for kw, text in ((dict(ws_size=need - 8), b"workspace"), (dict(n_lon=4097), b"4096 longitudes"), (dict(wrap=2), b"wrap"),
                     (dict(key_max=-1.0), b"key_max"), (dict(key_max=math.nan), b"key_max"), (dict(n_lat=0), b"bad sizes"),
                     (dict(n_lat=600000, n_lon=4096), b"2^31 - 2"), (dict(labels=None), b"null"), (dict(tables=None), b"null"),
                     (dict(key=None), b"null"), (dict(ws=None), b"null"), (dict(ws=20), b"aligned"), (dict(key=20), b"aligned")):
        assert raw.aurora_hip_nearest_event(*args(**kw)) == -1 and text in err(), (kw, err())
    assert raw.aurora_hip_nearest_event(*args(n_items=0, labels=None)) == 0        # no items: nothing to do
    args = lambda **kw: tuple({**dict(la=16, key=16, index=16, count=16, n_items=6, n_lat=9, n_lon=12, max_objects=4, table=16,  # noqa: E731
                                     hausdorff=16, stream=None), **kw}.values())
    for kw, text in ((dict(max_objects=0), b"max_objects"), (dict(n_items=-1), b"bad sizes"), (dict(la=None), b"null"),
                     (dict(count=None), b"null"), (dict(table=None), b"null"), (dict(key=12), b"aligned"), (dict(index=18), b"aligned")):
        assert raw.aurora_hip_object_separations(*args(**kw)) == -1 and text in err(), (kw, err())
    assert raw.aurora_hip_object_separations(*args(n_items=0, table=None)) == 0
    assert isinstance(ctypes.c_size_t(need).value, int)


def test_the_search_runs_on_the_host_against_a_brute_force(tmp_path):
    compiler = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert compiler, "no host C++ compiler (c++, g++, clang++ or $CXX) to build tools/probes/nearest_event_host.cpp with"
    exe = tmp_path / "nearest_event_host"
    built = subprocess.run([compiler, "-std=c++17", "-O1", str(ROOT / "tools" / "probes" / "nearest_event_host.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0 and " 0 mismatches" in ran.stdout, ran.stdout + ran.stderr
