"""`aurora_amd.closed_contours` on the host: the numpy path of THE RULE (aurora_amd/contours.py) against a plain-Python
breadth-first fill over the members that `disc_table` names -- every byte of the table, no tolerance anywhere -- hand-drawn 24 x 48
planes with the answer written down, the exact properties (monotone in delta, padding, truncation, empty planes), the finalised
tensors, the refusals, and the C entry's argument checks (no GPU needed).

One hand-drawn case is held to THE RULE where the list that asked for it says otherwise: "a ring of +Inf: closed".  By PASSABLE a
point that is not finite is passable, so the fill walks through a ring of +Inf as it does through a NaN, and the contour is open
where the field beyond the ring is passable; `test_hand_drawn` asserts that, and that the ring closes (with its eight points
inside F) once the field beyond it holds the contour."""
import collections
import dataclasses
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch
from aurora_amd.objects import Result
from tests.test_extrema_host import GRIDS, members_of, planes_for, table_of
from tests.test_smooth_host import batch_of, full_lon
from tests.verification_inputs import red_noise

mod = importlib.import_module("aurora_amd.contours")
extrema_mod = importlib.import_module("aurora_amd.extrema")
extrema, closed_contours = extrema_mod.extrema, mod.closed_contours

BRUTE_GRIDS = ("regional 17 x 39", "19 x 40 ascending", "polar disc covers the circle")
DELTAS = (40.0, 250.0, 1500.0)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the brute force ------------------------------------------------------------------------------------------------------
def neighbours(k, c, H, W, connectivity, wrap):
    """NEIGHBOURS of THE RULE in plain Python."""
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    for dk, dc in steps:
        kk, cc = k + dk, c + dc
        if not 0 <= kk < H:
            continue
        if wrap:
            yield kk, cc % W
        elif 0 <= cc < W:
            yield kk, cc


def brute(x, p0, inside, delta, is_max, connectivity, wrap):
    """(points, exits) of one candidate of one plane at one delta: a breadth-first fill over the members."""
    H, W = x.shape
    inside = set(inside)
    start = divmod(p0, W)
    v0, d = float(x[start]), float(np.float32(delta))

    def passable(q):
        v = float(x[q])
        return not math.isfinite(v) or ((v0 - v) if is_max else (v - v0)) < d

    F, queue = {start}, collections.deque([start])
    while queue:
        q = queue.popleft()
        for nb in neighbours(*q, H, W, connectivity, wrap):
            if nb in inside and nb not in F and passable(nb):
                F.add(nb)
                queue.append(nb)
    exits = 0
    for k, c in F:
        on_edge = not wrap and (k in (0, H - 1) or c in (0, W - 1))
        exits += on_edge or any(nb not in inside and passable(nb) for nb in neighbours(k, c, H, W, connectivity, wrap))
    return len(F), exits


def brute_table(x, e_table, e_count, members, deltas, is_max, connectivity, wrap):
    """(T, max_points, 2) int32 of one plane."""
    W = x.shape[1]
    out = np.zeros((len(deltas), e_table.shape[0], 2), dtype=np.int32)
    for s in range(min(int(e_count), e_table.shape[0])):
        p0 = int(e_table[s, 0])
        for t, d in enumerate(deltas):
            if not np.isnan(d):
                out[t, s] = brute(x, p0, members[divmod(p0, W)], d, is_max, connectivity, wrap)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(planes, lat, lon, wrap, radius, members) of a grid of GRIDS; shared, never modified."""
    lat, lon, wrap, radius = GRIDS[name]
    H, W = len(lat), len(lon)
    x = planes_for(H, W, 5 * H + W)
    x.setflags(write=False)
    return x, lat, lon, wrap, radius, members_of(table_of(lat, lon, wrap, radius), H, W, wrap)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("kind", ["min", "max"])
@pytest.mark.parametrize("name", BRUTE_GRIDS)
def test_numpy_path_equals_the_brute_force(name, kind, connectivity):
    x, lat, lon, wrap, radius, members = case(name)
    e = extrema(batch_of(np.array(x), lat, lon), radius * 0.6, kind=kind, max_points=64)
    c = closed_contours(e, {"x": DELTAS}, radius, connectivity=connectivity)
    table = c.table["x"].numpy()
    assert table.dtype == np.int32 and table.shape == (7, 3, 64, 2) and c.wrap == wrap and c.kind == kind
    rows, count = e.table["x"].numpy(), e.count["x"].numpy()
    closed = open_ = 0
    for p in range(7):
        want = brute_table(x[p], rows[p], count[p], members, DELTAS, kind == "max", connectivity, wrap)
        assert same(table[p], want), f"plane {p}"
        live = min(int(count[p]), 64)
        closed += int((want[:, :live, 1] == 0).sum())
        open_ += int((want[:, :live, 1] > 0).sum())
        assert (want[:, :live, 0] >= 1).all()                                       # the candidate itself
    assert closed > 0 and open_ > 0                                                  # both outcomes occur
    assert count[4] == 0 and not table[4].any()                                      # the all-NaN plane: no candidate
    # MONOTONE: closed at a delta implies closed at every smaller one; the fill only shrinks as delta falls
    live = torch.arange(64) < e.count["x"][:, None]
    is_closed = c.closed["x"].numpy()
    assert same(is_closed, ((table[..., 1] == 0) & live.numpy()[:, None, :]))
    assert not (is_closed[:, 1:] & ~is_closed[:, :-1]).any()
    assert (table[:, 1:, :, 0] >= table[:, :-1, :, 0]).all()


# ---- hand-drawn planes ------------------------------------------------------------------------------------------------------
LAT24, LON48, R_HAND = np.linspace(86.25, -86.25, 24), full_lon(48), 2600.0         # 7.5 degrees: three points are 2502 km
REG_LAT, REG_LON, R_REG = np.linspace(60.0, 2.5, 24), 10.0 + 2.5 * np.arange(48), 900.0
LOW, FIELD, WALL, DELTA = 90.0, 100.0, 110.0, 20.0                                   # the wall is EXACTLY delta above the low
BOX = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
SNAKE = ([(12, 21), (12, 22), (11, 22)] + [(10, c) for c in (22, 21, 20, 19, 18)] + [(11, 18), (12, 18), (13, 18)]
         + [(14, c) for c in (18, 19, 20, 21, 22)])                                  # a corridor from (12, 20): 16 points and the low
OPEN = "open"
WHOLE_KM = 19800.0                                                                   # 178.06 degrees


def ringed(at, H=24, W=48, wrap=True, field=FIELD, wall=WALL, change=None):
    """A plane of `field` with a low at `at` and a wall on its eight neighbours; change: {offset: value} of ring points."""
    x = np.full((H, W), field, dtype=np.float32)
    x[at] = LOW
    for (dk, dc) in BOX:
        k, c = at[0] + dk, at[1] + dc
        if 0 <= k < H and (wrap or 0 <= c < W):
            x[k, c % W] = (change or {}).get((dk, dc), wall)
    return x


def snake(opening=None):
    x = np.full((24, 48), WALL, dtype=np.float32)
    for q in SNAKE:
        x[q] = 95.0
    x[12, 20] = LOW
    if opening:
        x[opening] = FIELD
    return x


def plateau():
    x = np.full((24, 48), FIELD, dtype=np.float32)
    x[10:15, 18:23] = WALL
    x[11:14, 19:22] = LOW
    return x


# name -> (plane, regional?, the candidate, {connectivity: (points, exits) or OPEN})
HAND = {
    "ring": (ringed((12, 20)), False, (12, 20), {4: (1, 0), 8: (1, 0)}),
    "ring, one point lowered": (ringed((12, 20), change={(0, 1): FIELD}), False, (12, 20), {4: OPEN, 8: OPEN}),
    "ring, a diagonal gap": (ringed((12, 20), change={(-1, -1): FIELD}), False, (12, 20), {4: (1, 0), 8: OPEN}),
    "ring, a NaN in it": (ringed((12, 20), change={(0, 1): np.nan}), False, (12, 20), {4: OPEN, 8: OPEN}),
    "ring of +Inf": (ringed((12, 20), wall=np.inf), False, (12, 20), {4: OPEN, 8: OPEN}),          # (see the module's text)
    "ring of +Inf in a high field": (ringed((12, 20), field=WALL, wall=np.inf), False, (12, 20), {4: (9, 0), 8: (9, 0)}),
    "seam, column 0": (ringed((12, 0)), False, (12, 0), {4: (1, 0), 8: (1, 0)}),
    "seam, column W - 1": (ringed((12, 47)), False, (12, 47), {4: (1, 0), 8: (1, 0)}),
    "seam, column 0, opened across it": (ringed((12, 0), change={(0, -1): FIELD}), False, (12, 0), {4: OPEN, 8: OPEN}),
    "seam, column W - 1, opened across it": (ringed((12, 47), change={(1, 1): FIELD}), False, (12, 47), {4: (1, 0), 8: OPEN}),
    "row 0 of a wrapping grid": (ringed((0, 20)), False, (0, 20), {4: (1, 0), 8: (1, 0)}),          # the wall
    "row 0 of a regional grid": (ringed((0, 20), wrap=False), True, (0, 20), {4: (1, 1), 8: (1, 1)}),   # an exit
    "column 0 of a regional grid": (ringed((12, 0), wrap=False), True, (12, 0), {4: (1, 1), 8: (1, 1)}),
    "inside a regional grid": (ringed((12, 20), wrap=False), True, (12, 20), {4: (1, 0), 8: (1, 0)}),
    "serpentine": (snake(), False, (12, 20), {4: (17, 0), 8: (17, 0)}),
    "serpentine, open at its end": (snake((15, 22)), False, (12, 20), {4: (17, 1), 8: (17, 2)}),
    "plateau": (plateau(), False, (11, 19), {4: (9, 0), 8: (9, 0)}),
}


def hand_grid(regional):
    return (REG_LAT, REG_LON, R_REG) if regional else (LAT24, LON48, R_HAND)


def check_hand(name, connectivity, c, e) -> None:
    """The row of the hand-drawn candidate in a result `c` of the extrema `e` (host tensors) has the answer written down."""
    x, regional, at, want = HAND[name]
    rows, count = e.table["x"][0].numpy(), int(e.count["x"][0])
    found = np.flatnonzero(rows[:count, 0] == at[0] * 48 + at[1])
    assert found.size == 1, f"{name}: the low is not a candidate"
    points, exits = c.table["x"][0, 0, found[0]].numpy()
    is_closed = bool(c.closed["x"][0, 0, found[0]])
    if want[connectivity] == OPEN:
        assert exits >= 1 and points > 1 and not is_closed, (name, connectivity, points, exits)
    else:
        assert (points, exits) == want[connectivity] and is_closed == (exits == 0), (name, connectivity, points, exits)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(HAND))
def test_hand_drawn(name, connectivity):
    x, regional, at, _ = HAND[name]
    lat, lon, radius = hand_grid(regional)
    e = extrema(batch_of(x[None], lat, lon), radius, max_points=256)
    assert e.wrap == (not regional)
    c = closed_contours(e, [DELTA], radius, connectivity=connectivity)
    check_hand(name, connectivity, c, e)
    members = members_of(table_of(lat, lon, not regional, radius), 24, 48, not regional)
    want = brute_table(x, e.table["x"][0].numpy(), e.count["x"][0], members, [DELTA], False, connectivity, not regional)
    assert same(c.table["x"][0].numpy(), want)
    if name.startswith("serpentine"):                                                # what the written answer relies on
        assert all(q in members[12, 20] for q in SNAKE) and (15, 22) not in members[12, 20]
    if name == "plateau":                                                            # one candidate, the plateau inside F
        at_plateau = [p for p in e.table["x"][0, :int(e.count["x"][0]), 0].tolist() if x.reshape(-1)[p] == LOW]
        assert at_plateau == [11 * 48 + 19]


def test_constant_plane_whose_disc_is_the_whole_grid():
    x = np.full((1, 24, 48), 287.125, dtype=np.float32)
    lat = np.linspace(85.0, -87.5, 24)                           # no point has its antipode on the grid: the farthest is 177.5 degrees
    e = extrema(batch_of(x, lat, LON48), WHOLE_KM)
    assert int(e.count["x"]) == 1
    for connectivity in (4, 8):
        c = closed_contours(e, [0.5, 3.0], WHOLE_KM, connectivity=connectivity)
        assert c.table["x"][0, :, 0].tolist() == [[24 * 48, 0]] * 2 and bool(c.closed["x"][0, :, 0].all())
        assert not c.table["x"][0, :, 1:].any() and c.depth["x"][0, 0] == 3.0


# ---- further checks -----------------------------------------------------------------------------------------------------------
def two_variable_batch():
    x = red_noise((2, 2, 19, 40), 11)
    b = batch_of(x[0], GRIDS["19 x 40"][0], GRIDS["19 x 40"][1])
    return Batch({"x": b.surf_vars["x"], "y": batch_of(x[1], GRIDS["19 x 40"][0], GRIDS["19 x 40"][1]).surf_vars["x"]}, {}, {},
                 b.metadata)


def test_padded_deltas_give_zero_rows_and_only_named_variables_are_tested():
    b = two_variable_batch()
    e = extrema(b, 1234.5, max_points=32)
    c = closed_contours(e, {"y": [50.0], "x": [50.0, 300.0, 900.0]}, 2000.0)
    assert list(c.table) == ["x", "y"] and c.table["y"].shape == (2, 3, 32, 2)
    assert not c.table["y"][:, 1:].any() and c.table["y"][:, 0, 0, 0].min() >= 1
    assert torch.isnan(c.deltas["y"][:, 1:]).all() and c.deltas["x"].tolist() == [[50.0, 300.0, 900.0]] * 2
    assert not c.closed["y"][:, 1:].any() and not c.count_closed["y"][:, 1:].any()
    only = closed_contours(e, {"y": [50.0]}, 2000.0)
    assert list(only.table) == ["y"] and torch.equal(only.table["y"], c.table["y"][:, :1])
    assert same(only.value["y"].numpy(), e.value["y"].numpy()) and torch.equal(only.row["y"], e.row["y"])
    one = closed_contours(e, [50.0, 300.0, 900.0], 2000.0)                            # one sequence stands for every variable
    assert list(one.table) == ["x", "y"] and torch.equal(one.table["x"], c.table["x"])
    rounded = closed_contours(e, {"y": [50.0 + 1e-9]}, 2000.0)                        # float32, once
    assert rounded.deltas["y"].dtype == torch.float32 and torch.equal(rounded.table["y"], only.table["y"])


def test_max_points_below_count_tests_the_first_rows():
    x, lat, lon, wrap, radius, _ = case("19 x 40 ascending")
    b = batch_of(np.array(x), lat, lon)
    whole, cut = extrema(b, 700.0, max_points=256), extrema(b, 700.0, max_points=3)
    assert int(whole.count["x"][0]) > 3 and cut.truncated["x"][0]
    a, c = closed_contours(whole, [250.0], radius), closed_contours(cut, [250.0], radius)
    assert c.table["x"].shape == (7, 1, 3, 2) and c.max_points == 3
    assert torch.equal(c.table["x"], a.table["x"][:, :, :3])
    assert not c.table["x"][4].any() and bool(c.table["x"][0, 0, :, 0].all())          # the all-NaN plane; three live rows


def test_finalised_tensors():
    from tests.verification_inputs import red_noise_batch

    b = red_noise_batch(19, 40, seed=3)
    e = extrema(b, 1234.5, kind="max", max_points=48)
    c = closed_contours(e, {"z": [30.0, 200.0, 2000.0], "msl": [100.0]}, 2500.0, connectivity=4)
    assert isinstance(c, aurora_amd.ClosedContours) and isinstance(c, Result) and c.kind == "max" and c.connectivity == 4
    assert c.radius_km == 2500.0 and list(c.table) == ["msl", "z"]
    assert c.table["z"].shape == (2, 3, 3, 48, 2) and c.table["msl"].shape == (2, 3, 48, 2) and c.table["z"].dtype == torch.int32
    assert c.points["z"].shape == c.exits["z"].shape == c.closed["z"].shape == (2, 3, 3, 48) and c.closed["z"].dtype == torch.bool
    assert c.depth["z"].shape == (2, 3, 48) and c.depth["z"].dtype == torch.float32 and c.count_closed["z"].shape == (2, 3, 3)
    table, count = c.table["z"], e.count["z"]
    live = torch.arange(48) < count[..., None]
    assert torch.equal(c.points["z"], table[..., 0]) and torch.equal(c.exits["z"], table[..., 1])
    assert torch.equal(c.closed["z"], live[:, :, None, :] & (table[..., 1] == 0))
    assert torch.equal(c.count_closed["z"], c.closed["z"].sum(-1)) and bool(c.closed["z"].any()) and not bool(c.closed["z"].all())
    deltas = torch.tensor([30.0, 200.0, 2000.0])
    depth = (c.closed["z"] * deltas[:, None]).amax(dim=-2)
    assert torch.equal(c.depth["z"][live], depth[live]) and torch.isnan(c.depth["z"][~live]).all() and bool((~live).any())
    assert set(c.depth["z"][live].tolist()) <= {0.0, 30.0, 200.0, 2000.0}
    for name in ("value", "lat", "lon", "row", "col"):
        assert same(getattr(c, name)["z"].numpy(), getattr(e, name)["z"].numpy())      # passed through, bit for bit
    assert (c.row["z"][~live] == -1).all() and torch.isnan(c.lat["z"][~live]).all()
    assert not c.closed["msl"][:, 1:].any() and torch.isnan(c.deltas["msl"][:, 1:]).all()       # padded to T = 3
    host = c.cpu()
    assert isinstance(host, aurora_amd.ClosedContours) and torch.equal(host.table["z"], c.table["z"])
    alone = closed_contours(extrema(Batch({}, {}, {"z": b.atmos_vars["z"][1:, :, 1:]}, b.metadata), 1234.5, kind="max", max_points=48),
                            {"z": [30.0, 200.0, 2000.0]}, 2500.0, connectivity=4)
    assert torch.equal(alone.table["z"], c.table["z"][1:, 1:])     # a plane does not depend on its neighbours in the call


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    x = red_noise((1, 19, 40), 9)
    b = batch_of(x, GRIDS["19 x 40"][0], full_lon(40))
    e = extrema(b, 1234.5)
    with pytest.raises(TypeError, match="closed_contours: e must be an Extrema, got Batch"):
        closed_contours(b, [1.0], 500.0)
    mixed = dataclasses.replace(e, table_table=e.table_table.to("meta"))
    with pytest.raises(ValueError, match=r"closed_contours: the tables of e and the fields of e.source are on \['cpu', 'meta'\]; "
                                         "move the Extrema and its source batch to the CPU or to one GPU first"):
        closed_contours(mixed, [1.0], 500.0)
    for delta in ([0.0], [-1.0, 2.0], [float("nan")], [float("inf")], [1.0, float("nan")], [1e-60]):
        with pytest.raises(ValueError, match=r"closed_contours: the deltas of 'x' must be finite and above 0 \(as float32\)"):
            closed_contours(e, delta, 500.0)
    for delta in ([2.0, 1.0], [1.0, 1.0], [1.0, 1.0 + 1e-12]):
        with pytest.raises(ValueError, match="closed_contours: the deltas of 'x' must be strictly ascending"):
            closed_contours(e, {"x": delta}, 500.0)
    with pytest.raises(ValueError, match="closed_contours: 1 to 8 deltas per variable, 'x' has 9"):
        closed_contours(e, [float(v) for v in range(1, 10)], 500.0)
    with pytest.raises(ValueError, match="closed_contours: 1 to 8 deltas per variable, 'x' has 0"):
        closed_contours(e, {"x": []}, 500.0)
    assert closed_contours(e, [float(v) for v in range(1, 9)], 500.0).table["x"].shape == (1, 8, 4096, 2)
    with pytest.raises(ValueError, match="closed_contours: delta names the variable 'y', which e does not hold"):
        closed_contours(e, {"y": [1.0]}, 500.0)
    with pytest.raises(ValueError, match="closed_contours: delta must be a non-empty mapping"):
        closed_contours(e, {}, 500.0)
    for connectivity in (6, 0, True, "8"):
        with pytest.raises(ValueError, match="closed_contours: connectivity must be 4 or 8"):
            closed_contours(e, [1.0], 500.0, connectivity=connectivity)
    for radius in (0.0, -5.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="closed_contours: radius_km must be a finite number above 0"):
            closed_contours(e, [1.0], radius)


def polar_cap():
    """120 rows within 2 degrees of the pole and 4096 longitudes: at 250 km every window is 122 rows of the whole circle."""
    lat = np.linspace(90.0, 88.0, 120)
    return batch_of(np.zeros((1, 120, 4096), dtype=np.float32), lat, full_lon(4096)), lat


def test_a_window_beyond_the_lds_budget_is_refused_on_the_cpu_too():
    b, lat = polar_cap()
    e = extrema(b, 3.0)
    with pytest.raises(ValueError, match=r"closed_contours: a radius of 250 km gives windows of 122 rows x 64 words of 64 columns on "
                                         r"this grid, 187392 bytes of LDS in three bitmaps; the budget is 159744 bytes, which allows "
                                         r"54 words at this many rows, and 120 target rows \(0 to 119\) exceed it"):
        closed_contours(e, [1.0], 250.0)
    table = table_of(lat, full_lon(4096), True, 250.0)
    assert mod.window_words(table, 4096, True).tolist() == [64] * 120 and table[2].shape[1] == 120
    assert mod.LDS_BUDGET == 156 * 1024
    # what the budget admits: 721 x 1440 at 1000 km, and (by arithmetic alone) 1801 x 3600 at 600 km
    quarter = table_of(np.linspace(90, -90, 721), full_lon(1440), True, 1000.0)
    assert quarter[2].shape[1] + 2 == 73 and int(mod.window_words(quarter, 1440, True).max()) == 23
    assert mod._check_budget(quarter, 1440, True, 1000.0) == 23 and 24 * 73 * 23 <= mod.LDS_BUDGET
    assert 24 * (2 * 53 + 1 + 2) * 57 <= mod.LDS_BUDGET


def test_window_words():
    lat, lon, wrap, radius = GRIDS["33 x 70"]
    table = table_of(lat, lon, wrap, radius)
    widest = mod._widest(table)
    assert widest.min() >= 0
    words = mod.window_words(table, 70, True)
    assert words.tolist() == [2 if 2 * n + 1 >= 70 or 2 * n + 3 > 64 else 1 for n in widest.tolist()] and set(words.tolist()) == {1, 2}
    lat, lon, wrap, radius = GRIDS["regional 17 x 39"]
    assert mod.window_words(table_of(lat, lon, wrap, radius), 39, False).tolist() == [1] * 17
    assert mod.window_words(table_of(lat, lon, wrap, 5000.0), 39, False).tolist() == [1] * 17     # at most W + 2 columns


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_the_c_entry_point_refuses_before_any_launch():
    from aurora_amd.engine import lib

    raw, header = lib.load(), (lib.library_path().parents[2] / "include" / "aurora_hip.h").read_text()
    name = "aurora_hip_closed_contours"
    assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    assert "contours.hip" in importlib.import_module("aurora_amd.build").SOURCES
    assert aurora_amd.closed_contours is mod.closed_contours and aurora_amd.ClosedContours is mod.ClosedContours
    assert "closed_contours" in aurora_amd.__all__ and "ClosedContours" in aurora_amd.__all__
    assert lib.CONTOUR_LDS_BUDGET == mod.LDS_BUDGET and lib.contour_lds_bytes(120, 64) == 187392
    err = lambda: raw.aurora_hip_last_error()  # noqa: E731
    args = lambda **kw: tuple({**dict(planes=16, table=16, count=16, delta=16, out=16, n_planes=3, n_lat=9, n_lon=12,  # noqa: E731
                                     n_deltas=2, max_points=64, row_lo=16, row_count=16, half=16, max_rows=3, max_words=1, wrap=1,
                                     is_max=0, connectivity=8, stream=None), **kw}.values())
    for kw, text in ((dict(max_rows=256), b"255 source rows"), (dict(max_rows=0), b"source rows"), (dict(wrap=2), b"flags"),
                     (dict(is_max=-1), b"flags"), (dict(max_points=0), b"max_points"), (dict(max_points=65537), b"max_points"),
                     (dict(n_deltas=0), b"1 to 8 deltas"), (dict(n_deltas=9), b"1 to 8 deltas"), (dict(connectivity=6), b"connectivity"),
                     (dict(max_words=0), b"words per window row"), (dict(max_words=66), b"words per window row"),
                     (dict(n_lon=4097), b"4097 longitudes; 1 to 4096 are supported"), (dict(n_lat=600000, n_lon=4096), b"too large"),
                     (dict(half=None), b"null"), (dict(out=None), b"null"), (dict(count=None), b"null"), (dict(delta=None), b"null"),
                     (dict(table=20), b"aligned"), (dict(out=18), b"aligned"), (dict(n_lon=0), b"bad sizes"),
                     (dict(n_planes=-1), b"bad sizes"),
                     # the LDS budget: 24 (max_rows + 2) max_words <= 159744, the windows that the host refuses
                     (dict(max_rows=120, max_words=64), b"windows of 122 rows x 64 words of 64 columns need 187392 bytes of LDS in "
                                                        b"three bitmaps; the budget is 159744 bytes"),
                     (dict(max_rows=255, max_words=26), b"budget is 159744 bytes"), (dict(max_rows=101, max_words=65), b"budget")):
        assert raw.aurora_hip_closed_contours(*args(**kw)) == -1 and text in err(), (kw, err())
    assert raw.aurora_hip_closed_contours(*args(n_planes=0)) == 0
    assert raw.aurora_hip_closed_contours(*args(n_planes=0, max_rows=255, max_words=25)) == 0       # 24 x 257 x 25 = 154200
    assert raw.aurora_hip_closed_contours(*args(n_planes=0, max_rows=71, max_words=23)) == 0        # 721 x 1440 at 1000 km
    assert raw.aurora_hip_closed_contours(*args(n_planes=0, max_rows=107, max_words=57)) == 0       # 1801 x 3600 at 600 km
