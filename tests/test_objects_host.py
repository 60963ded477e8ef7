"""`aurora_amd.objects` on the CPU against a yardstick written here: a breadth-first flood fill in plain Python over the event
mask with the neighbour rule of THE RULE (aurora_amd/objects.py), objects numbered by first point, the table by explicit loops.
Independent of scipy and of the module; every comparison is exact.  tests/test_gpu_objects.py compares the kernel with the CPU
path on the patterns made here."""
import ctypes
import importlib
import struct
from collections import deque
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, objects
from aurora_amd._fields import latitude_weights
from tests.verification_inputs import red_noise

mod = importlib.import_module("aurora_amd.objects")       # (the package's attribute of this name is the function)


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def key_of(v: float, idx: int, below: bool) -> int:
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    k = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
    if below:
        k = ~k & 0xffffffff
    return (k << 32) | (0xffffffff - idx)


def yardstick(values, thr, below=False, connectivity=8, wrap=False, max_objects=4096, lat=None):
    """(labels, count, table) of one float32 plane and one threshold, in plain Python."""
    v = np.asarray(values, dtype=np.float32)
    H, W = v.shape
    unit = [int(round(float(w) * 2.0 ** 32)) for w in latitude_weights(lat_of(H) if lat is None else lat)]
    event = [[bool(np.isfinite(v[i, j]) and (v[i, j] <= thr if below else v[i, j] >= thr)) for j in range(W)] for i in range(H)]
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    labels = np.zeros((H, W), dtype=np.int32)
    table = np.zeros((max_objects, 10), dtype=np.int64)
    count = 0
    for i in range(H):
        for j in range(W):
            if not event[i][j] or labels[i, j]:
                continue
            count += 1
            labels[i, j] = count
            queue, members = deque([(i, j)]), []
            while queue:
                a, b = queue.popleft()
                members.append((a, b))
                for da, db in steps:
                    c, d = a + da, b + db
                    if not 0 <= c < H:
                        continue
                    if not 0 <= d < W:
                        if not wrap:
                            continue
                        d %= W
                    if event[c][d] and not labels[c, d]:
                        labels[c, d] = count
                        queue.append((c, d))
            if count <= max_objects:
                offs = []
                for a, b in members:
                    d = b - j
                    if wrap:
                        d = d + W if d < -(W // 2) else (d - W if d >= W - W // 2 else d)
                    offs.append(d)
                peak = max(key_of(float(v[a, b]), a * W + b, below) for a, b in members)
                table[count - 1] = [len(members), sum(unit[a] for a, _ in members), i * W + j, min(a for a, _ in members),
                                    max(a for a, _ in members), sum(a for a, _ in members), min(offs), max(offs), sum(offs),
                                    peak - (1 << 64) if peak >= 1 << 63 else peak]
    return labels, count, table


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def lat_of(H):
    return np.linspace(90, -90, H) if H > 1 else np.zeros(1)


def batch_of(planes, atmos=None, lat=None) -> Batch:
    """planes: (B, H, W) values of the surface variable "x"; atmos: (B, C, H, W) of the atmospheric variable "a"."""
    planes = np.asarray(planes)
    B, H, W = planes.shape
    md = Metadata(lat=torch.as_tensor(lat_of(H) if lat is None else lat, dtype=torch.float64),
                  lon=torch.linspace(0, 360, W + 1, dtype=torch.float64)[:-1], time=tuple(datetime(2023, 1, 1, 6) for _ in range(B)),
                  atmos_levels=tuple(range(100, 100 + (0 if atmos is None else np.asarray(atmos).shape[1]))))
    a = {} if atmos is None else {"a": torch.as_tensor(np.asarray(atmos))[:, None]}
    return Batch({"x": torch.as_tensor(planes)[:, None]}, {}, a, md)


def draw(*rows) -> np.ndarray:
    """A float32 plane from rows of text: '#' is 1, anything else 0."""
    return np.array([[1.0 if c == "#" else 0.0 for c in r] for r in rows], dtype=np.float32)


def serpentine(H=33, W=70) -> np.ndarray:
    p = np.zeros((H, W), dtype=np.float32)
    p[::2] = 1
    for i in range(1, H, 2):
        p[i, W - 1 if i % 4 == 1 else 0] = 1
    return p


def rings(n=21) -> np.ndarray:
    i, j = np.indices((n, n))
    return (np.maximum(abs(i - n // 2), abs(j - n // 2)) % 2 == 0).astype(np.float32)


def comb(H=9, W=13) -> np.ndarray:
    p = np.zeros((H, W), dtype=np.float32)
    p[:, ::2] = 1
    p[-1] = 1
    return p


def checkerboard(H, W) -> np.ndarray:
    i, j = np.indices((H, W))
    return ((i + j) % 2).astype(np.float32)


HAND = draw("##....#....#",
            "#..##.#....#",
            "....#..##...",
            ".#......#..#",
            "#.#........#",
            ".........#..",
            "###.....#.#.",
            "..#......#..",
            "#.#.#......#")
# 8-connected, no wrap, numbered by first point
HAND_LABELS = np.array([[1, 1, 0, 0, 0, 0, 2, 0, 0, 0, 0, 3],
                        [1, 0, 0, 4, 4, 0, 2, 0, 0, 0, 0, 3],
                        [0, 0, 0, 0, 4, 0, 0, 2, 2, 0, 0, 0],
                        [0, 5, 0, 0, 0, 0, 0, 0, 2, 0, 0, 6],
                        [5, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 6],
                        [0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 0, 0],
                        [8, 8, 8, 0, 0, 0, 0, 0, 7, 0, 7, 0],
                        [0, 0, 8, 0, 0, 0, 0, 0, 0, 7, 0, 0],
                        [9, 0, 8, 0, 10, 0, 0, 0, 0, 0, 0, 11]], dtype=np.int32)

SEAM = draw("............",
            "##........##",
            "#..........#",
            "............",
            "#...........",
            "...........#",
            "............",
            "############")
U_SHAPE = draw("#.....#", "#.....#", "#.....#", "#######")
DIAGONAL = np.eye(8, dtype=np.float32)


def patterns() -> dict:
    """name -> float32 plane with events at >= 0.5: what this file and the GPU file label."""
    special = HAND.copy()
    special[0, 3], special[2, 0], special[5, 5], special[8, 7] = np.nan, np.inf, -np.inf, np.nan
    ties = np.zeros((6, 9), dtype=np.float32)
    ties[1:3, 1:4] = 2.0                            # a plateau: the peak is its first point
    ties[4, 5:8] = [1.0, 3.0, 3.0]
    ties[0, 8] = -0.0
    return {"hand": HAND, "seam": SEAM, "band": draw("......", "######", "......", "##..##"), "u": U_SHAPE, "comb": comb(),
            "diagonal": DIAGONAL, "checkerboard_even": checkerboard(6, 8), "checkerboard_odd": checkerboard(5, 7),
            "serpentine": serpentine(), "rings": rings(), "special": special, "ties": ties, "one_row": draw("##.#..##"),
            "one_column": draw("#", "#", ".", "#"), "two_columns": draw("#.", ".#", "..", "##", ".."), "full": np.ones((3, 5), np.float32),
            "empty": np.zeros((3, 5), np.float32)}


def run(plane, thr=(0.5,), **kw):
    o = objects(batch_of(np.asarray(plane)[None]), {"x": list(thr)}, **kw)
    return o, o.labels["x"][0].numpy(), o.count["x"][0].numpy(), o.table["x"][0].numpy()


def assert_matches_yardstick(plane, thr=(0.5,), **kw):
    o, labels, count, table = run(plane, thr, **kw)
    for t, value in enumerate(thr):
        want = yardstick(plane, np.float32(value), below=kw.get("below", False), connectivity=kw.get("connectivity", 8),
                         wrap=o.wrap, max_objects=kw.get("max_objects", 4096))
        assert np.array_equal(labels[t], want[0]), (t, labels[t], want[0])
        assert count[t] == want[1]
        assert np.array_equal(table[t], want[2]), (t, table[t][:want[1]], want[2][:want[1]])
    return o, labels, count, table


# ---- labels, counts and tables -------------------------------------------------------------------------------------------------
def test_the_hand_drawn_plane_has_the_labels_written_here():
    _, labels, count, _ = assert_matches_yardstick(HAND, connectivity=8, wrap=False)
    assert np.array_equal(labels[0], HAND_LABELS) and count[0] == 11
    _, wrapped, count, _ = assert_matches_yardstick(HAND, connectivity=8, wrap=True)
    # across the seam: 3 joins 1 (rows 0 and 1), 6 joins 5 (row 4), 11 joins 9 (row 8): three objects fewer
    assert count[0] == 8 and wrapped[0][0, 11] == 1 and wrapped[0][3, 11] == wrapped[0][4, 0] and wrapped[0][8, 11] == wrapped[0][8, 0]
    _, four, count, _ = assert_matches_yardstick(HAND, connectivity=4, wrap=False)
    assert count[0] == 17                                                         # counted by hand


@pytest.mark.parametrize("name", sorted(patterns()))
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("wrap", (False, True))
def test_every_pattern_equals_the_flood_fill(name, connectivity, wrap):
    assert_matches_yardstick(patterns()[name], connectivity=connectivity, wrap=wrap, max_objects=64)


def test_seam_band_and_split():
    _, labels, count, _ = run(SEAM, wrap=True)
    assert count[0] == 3 and labels[0][1, 0] == labels[0][1, 11] == labels[0][2, 11] == 1
    assert labels[0][4, 0] == labels[0][5, 11] == 2                               # diagonal across the seam (8-connected)
    assert run(SEAM, wrap=False)[2][0] == 5 and run(SEAM, wrap=True, connectivity=4)[2][0] == 4
    band = patterns()["band"]
    assert run(band, wrap=True)[2][0] == 2 and run(band, wrap=False)[2][0] == 3   # the band is one either way, row 3 splits
    # wrap=None: the rule of diagnostics -- these longitudes cover the full circle
    assert run(SEAM)[0].wrap is True and run(SEAM)[2][0] == 3


def test_connectivity_on_a_diagonal_and_a_checkerboard():
    assert run(DIAGONAL, connectivity=4, wrap=False)[2][0] == 8 and run(DIAGONAL, connectivity=8, wrap=False)[2][0] == 1
    even = checkerboard(6, 8)
    assert run(even, connectivity=4, wrap=True)[2][0] == even.sum()                 # every event its own object
    assert run(even, connectivity=8, wrap=True)[2][0] == 1 and run(even, connectivity=8, wrap=False)[2][0] == 1


def test_u_comb_serpentine_and_rings():
    assert run(U_SHAPE, wrap=False)[2][0] == 1 and run(U_SHAPE[:-1], wrap=False)[2][0] == 2
    assert run(comb(), connectivity=4, wrap=False)[2][0] == 1 and run(comb()[:-1], connectivity=4, wrap=False)[2][0] == 7
    _, labels, count, table = run(serpentine(), connectivity=4, wrap=False)
    assert count[0] == 1 and table[0][0, 0] == serpentine().sum() and table[0][0, 2] == 0
    assert run(rings(), connectivity=8, wrap=False)[2][0] == 6 and run(rings(), connectivity=4, wrap=False)[2][0] == 6


def test_nan_inf_and_a_nan_threshold_are_background():
    special = patterns()["special"]
    _, labels, count, _ = assert_matches_yardstick(special, thr=(0.5, float("nan")), wrap=False)
    assert labels[0][0, 3] == labels[0][2, 0] == labels[0][5, 5] == 0 and count[1] == 0 and not labels[1].any()
    _, labels, _, _ = assert_matches_yardstick(special, below=True, wrap=False)    # <= 0.5: -inf is not finite either
    assert labels[0][5, 5] == 0 and labels[0][2, 0] == 0 and labels[0][0, 2] > 0


def test_below_and_peak_ties():
    ties = patterns()["ties"]
    o, _, count, _ = assert_matches_yardstick(ties, wrap=False)
    assert count[0] == 2
    assert o.peak["x"][0, 0, :2].tolist() == [2.0, 3.0]
    assert (o.peak_row["x"][0, 0, :2].tolist(), o.peak_col["x"][0, 0, :2].tolist()) == ([1, 4], [1, 6])   # the smallest index wins
    o, _, count, _ = assert_matches_yardstick(ties, thr=(0.0,), below=True, wrap=False)
    k = int(o.labels["x"][0, 0, 0, 8]) - 1                                         # the object that holds -0 among +0
    assert o.peak["x"][0, 0, k] == 0 and np.signbit(o.peak["x"][0, 0, k].item())   # -0 sorts below +0
    assert (int(o.peak_row["x"][0, 0, k]), int(o.peak_col["x"][0, 0, k])) == (0, 8)


def test_max_objects_truncates_the_table_alone():
    o, labels, count, table = assert_matches_yardstick(HAND, wrap=False, max_objects=4)
    assert count[0] == 11 and labels[0].max() == 11 and bool(o.truncated["x"][0, 0])
    assert table.shape == (1, 4, 10) and (table[0][:, 0] > 0).all()
    assert np.array_equal(table[0], run(HAND, wrap=False)[3][0][:4])
    assert not bool(run(HAND, wrap=False, max_objects=11)[0].truncated["x"][0, 0])


@pytest.mark.parametrize("shape", [(1, 9), (7, 1), (5, 2), (1, 1)])
def test_extreme_shapes(shape):
    g = np.random.default_rng(shape[0] * 10 + shape[1])
    plane = (g.random(shape) < 0.6).astype(np.float32)
    for wrap in (False, True):
        for connectivity in (4, 8):
            assert_matches_yardstick(plane, wrap=wrap, connectivity=connectivity)


def test_levels_thresholds_per_level_and_batch():
    g = np.random.default_rng(5)
    surf, atmos = g.random((2, 7, 10)).astype(np.float32), g.random((2, 3, 7, 10)).astype(np.float32)
    thr = np.array([[0.3, 0.6], [0.5, 0.9], [0.7, np.nan]])
    o = objects(batch_of(surf, atmos), {"a": thr, "x": [0.4]}, wrap=True)
    assert o.labels["a"].shape == (2, 3, 2, 7, 10) and o.labels["x"].shape == (2, 2, 7, 10) and o.count["a"].shape == (2, 3, 2)
    assert o.table["a"].shape == (2, 3, 2, 4096, 10) and o.points["a"].shape == (2, 3, 2, 4096) and o.bbox["x"].shape == (2, 2, 4096, 4)
    for b in range(2):
        for c in range(3):
            for t in range(2):
                want = yardstick(atmos[b, c], np.float32(thr[c, t]), wrap=True)
                assert np.array_equal(o.labels["a"][b, c, t].numpy(), want[0]) and o.count["a"][b, c, t] == want[1]
                assert np.array_equal(o.table["a"][b, c, t].numpy(), want[2])
        want = yardstick(surf[b], np.float32(0.4), wrap=True)
        assert np.array_equal(o.labels["x"][b, 0].numpy(), want[0]) and np.array_equal(o.table["x"][b, 0].numpy(), want[2])
        assert o.count["x"][b, 1] == 0                                             # the padded threshold: NaN
    assert torch.equal(o.mask("a", 2), o.labels["a"] == 2)
    # the last history entry is the one labelled; float64 fields are rounded to float32 first
    b64 = batch_of(surf.astype(np.float64))
    assert torch.equal(objects(b64, {"x": [0.4]}, wrap=True).labels["x"], o.labels["x"][:, :1])


def test_scipy_agrees_where_the_grid_does_not_wrap():
    ndimage = pytest.importorskip("scipy.ndimage")
    plane = red_noise((40, 96), seed=3)[None]
    thr = np.quantile(plane, [0.5, 0.9]).astype(np.float32)
    for connectivity, structure in ((8, np.ones((3, 3))), (4, None)):
        o = objects(batch_of(plane), {"x": thr}, wrap=False, connectivity=connectivity)
        for t in range(2):
            want, n = ndimage.label(plane[0] >= thr[t], structure=structure)
            assert np.array_equal(o.labels["x"][0, t].numpy(), want) and o.count["x"][0, t] == n
        assert_matches_yardstick(plane[0], thr=thr, wrap=False, connectivity=connectivity, max_objects=16)


# ---- finalisation ----------------------------------------------------------------------------------------------------------------
def test_centroid_area_peak_and_bbox_of_rectangles():
    plane = np.zeros((9, 12), dtype=np.float32)
    plane[2:5, 3:8] = 1.0                                                          # rows 2..4, columns 3..7
    plane[3, 6] = 4.0
    plane[6:8, 10:] = 1.0                                                          # rows 6..7, columns 10, 11, 0, 1
    plane[6:8, :2] = 1.0
    plane[7, 0] = 5.0
    o = objects(batch_of(plane[None]), {"x": [0.5]}, wrap=True)
    f = lambda d: d["x"][0, 0]                                                     # noqa: E731
    assert f(o.count) == 2 and f(o.points)[:3].tolist() == [15, 8, -1]
    assert f(o.centroid_row)[:2].tolist() == [3.0, 6.5] and f(o.centroid_col)[:2].tolist() == [5.0, 11.5]
    lat, lon = lat_of(9), np.arange(12) * 30.0
    assert f(o.centroid_lat)[0] == lat[3] and f(o.centroid_lat)[1] == lat[6] + 0.5 * (lat[7] - lat[6])
    assert f(o.centroid_lon)[0] == lon[5] and f(o.centroid_lon)[1] == lon[11] + 0.5 * (360.0 - lon[11])   # across the seam
    assert f(o.peak)[:2].tolist() == [4.0, 5.0] and f(o.peak_row)[:2].tolist() == [3, 7] and f(o.peak_col)[:2].tolist() == [6, 0]
    assert f(o.peak_lat)[:2].tolist() == [lat[3], lat[7]] and f(o.peak_lon)[:2].tolist() == [lon[6], lon[0]]
    assert f(o.bbox)[:3].tolist() == [[2, 4, 3, 7], [6, 7, 10, 1], [-1, -1, -1, -1]]
    assert torch.isnan(f(o.area)[2:]).all() and torch.isnan(f(o.peak)[2:]).all() and (f(o.peak_row)[2:] == -1).all()
    w = latitude_weights(lat)
    want = np.array([5 * w[2:5].sum(), 4 * w[6:8].sum()])
    assert np.all(np.abs(f(o.area)[:2].numpy() - want) <= np.array([15, 8]) * 2.0 ** -33 + 1e-12)
    assert o.cpu().table["x"] is not None and o.thresholds["x"].shape == (1, 1)


def test_area_equals_points_on_an_equatorial_row():
    row = draw("##.###..#.##")
    o = objects(batch_of(row[None]), {"x": [0.5]}, wrap=False)
    n = int(o.count["x"][0, 0])
    points, area = o.points["x"][0, 0, :n].numpy(), o.area["x"][0, 0, :n].numpy()
    assert points.tolist() == [2, 3, 1, 2] and np.all(np.abs(area - points) <= points * 2.0 ** -33)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_inputs_say_why():
    b = batch_of(HAND[None])
    with pytest.raises(TypeError, match="objects: batch must be a Batch"):
        objects({"x": HAND}, {"x": [1.0]})
    with pytest.raises(ValueError, match="objects: thresholds must be a non-empty mapping"):
        objects(b, {})
    with pytest.raises(ValueError, match="objects: thresholds name the variable 'y'"):
        objects(b, {"y": [1.0]})
    with pytest.raises(ValueError, match="objects: 1 to 8 thresholds per variable"):
        objects(b, {"x": list(range(9))})
    with pytest.raises(ValueError, match="objects: connectivity must be 4 or 8"):
        objects(b, {"x": [1.0]}, connectivity=6)
    with pytest.raises(ValueError, match="objects: max_objects must be a whole number of at least 1"):
        objects(b, {"x": [1.0]}, max_objects=0)
    with pytest.raises(ValueError, match="objects: wrap must be None, True or False"):
        objects(b, {"x": [1.0]}, wrap="yes")
    matrix = Batch(b.surf_vars, {}, {}, Metadata(lat=b.metadata.lat[:, None].expand(9, 12), lon=b.metadata.lon[None].expand(9, 12), time=b.metadata.time, atmos_levels=()))
    with pytest.raises(ValueError, match="objects: batch has matrices for latitudes / longitudes"):
        objects(matrix, {"x": [1.0]})


def test_the_c_entry_point_refuses_before_any_launch():
    from aurora_amd.engine import lib

    raw, header = lib.load(), (lib.library_path().parents[2] / "include" / "aurora_hip.h").read_text()
    for name in ("aurora_hip_objects", "aurora_hip_objects_workspace_bytes"):
        assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    assert "objects.hip" in __import__("aurora_amd.build", fromlist=["SOURCES"]).SOURCES
    assert aurora_amd.objects is mod.objects and "objects" in aurora_amd.__all__ and "Objects" in aurora_amd.__all__
    err = lambda: raw.aurora_hip_last_error()  # noqa: E731
    need = raw.aurora_hip_objects_workspace_bytes(2, 9, 12, 3)
    assert need == (2 * 3 * (9 * 12 + 9) * 4 + 7) // 8 * 8
    assert raw.aurora_hip_objects_workspace_bytes(1, 9, 4097, 1) == 0 and raw.aurora_hip_objects_workspace_bytes(1, 600000, 4096, 1) == 0
    args = lambda **kw: tuple({**dict(planes=16, n_planes=2, n_lat=9, n_lon=12, thr=16, T=3, unit=16, below=0, conn=8, wrap=1,  # noqa: E731
                                     max_objects=4, labels=16, count=16, table=16, ws=16, ws_size=need, stream=None), **kw}.values())
    for kw, text in ((dict(ws_size=need - 8), b"workspace"), (dict(n_lon=4097), b"4096 longitudes"), (dict(conn=6), b"connectivity"),
                     (dict(below=2), b"flags"), (dict(wrap=-1), b"flags"), (dict(T=9), b"thresholds"), (dict(max_objects=0), b"max_objects"),
                     (dict(n_lat=600000, n_lon=4096), b"2^31 - 2"), (dict(table=None), b"null"), (dict(ws=20), b"aligned")):
        assert raw.aurora_hip_objects(*args(**kw)) == -1 and text in err(), (kw, err())
    assert isinstance(ctypes.c_size_t(need).value, int)
