"""aurora_amd.link_extrema and aurora_amd.tracks on the host: the numpy path equals a plain-Python double loop over live rows by
THE RULE of aurora_amd/links.py in every byte (the loop rounds each operation on its own with Python floats), hand-made tables
with their answers written down, the numbering of tracks, and the refusals."""
import dataclasses
import importlib
import math

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import distances, extrema
from aurora_amd._sphere import EARTH_RADIUS
from aurora_amd.objects import Result
from tests import links_inputs as li
from tests.test_smooth_host import batch_of, full_lon
from tests.verification_inputs import red_noise

mod = importlib.import_module("aurora_amd.links")
link_extrema, tracks = aurora_amd.link_extrema, aurora_amd.tracks


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def keep_dict(rows):
    return None if rows is None else {"x": torch.tensor([rows], dtype=torch.bool)}


def run_case(c):
    return link_extrema(c["a"], c["b"], c["max_km"], keep_a=keep_dict(c["keep_a"]), keep_b=keep_dict(c["keep_b"]))


# ---- the numpy path against the double loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [True, False])
def test_numpy_path_equals_the_double_loop(wrap):
    lat, lon, _ = li.grid(wrap)
    rng = np.random.default_rng(11 + wrap)
    sizes = [(5, 9), (40, 31), (1, 60), (64, 64), (0, 7), (90, 3)]
    ma, mb = 64, 50                                              # (90 > 64: a truncated table; 0: an empty one)
    a = li.make([li.random_points(rng, 19, 36, n) for n, _ in sizes], lat, lon, wrap, ma)
    b = li.make([li.random_points(rng, 19, 36, n) for _, n in sizes], lat, lon, wrap, mb)
    keep_a, keep_b = rng.random((len(sizes), ma)) < 0.7, rng.random((len(sizes), mb)) < 0.7
    for max_km in (800.0, 2500.0, 30000.0):
        for ka, kb in ((None, None), (keep_a, keep_b)):
            got = link_extrema(a, b, max_km, keep_a=None if ka is None else {"x": torch.from_numpy(ka)},
                               keep_b=None if kb is None else {"x": torch.from_numpy(kb)})
            forward, backward = li.brute(a, b, max_km, ka, kb)
            assert same(got.forward_table.numpy(), forward) and same(got.backward_table.numpy(), backward)
            assert (forward[..., 1] >= 0).any() and (forward[..., 1] < 0).any()
            # a mutual pair carries the same key bits on both sides (the key is symmetric bit for bit)
            nxt = got.next["x"].numpy()
            p, r = np.nonzero(nxt >= 0)
            assert p.size and (forward[p, r, 0] == backward[p, nxt[p, r], 0]).all()
            assert (backward[p, nxt[p, r], 1] == r).all()


def test_blocks_of_the_key_matrix_change_nothing(monkeypatch):
    lat, lon, wrap = li.grid(True)
    rng = np.random.default_rng(3)
    a = li.make([li.random_points(rng, 19, 36, 200)], lat, lon, wrap, 256)
    b = li.make([li.random_points(rng, 19, 36, 300)], lat, lon, wrap, 300)
    whole = link_extrema(a, b, 2000.0)
    monkeypatch.setattr(mod, "_BLOCK_BYTES", 8 * 300 * 7)        # 7 rows of a at a time
    blocked = link_extrema(a, b, 2000.0)
    assert same(whole.forward_table.numpy(), blocked.forward_table.numpy())
    assert same(whole.backward_table.numpy(), blocked.backward_table.numpy())


def test_the_key_is_symmetric_bit_for_bit():
    rng = np.random.default_rng(5)
    for wrap in (True, False):
        lat, lon, _ = li.grid(wrap)
        s, c, cd = distances.tables_of(lat, lon, wrap)
        for fa, fb in rng.integers(0, 19 * 36, size=(4000, 2)):
            k1, k2 = li.key_of(int(fa), int(fb), s, c, cd, 36, wrap), li.key_of(int(fb), int(fa), s, c, cd, 36, wrap)
            assert li.bits_of(k1) == li.bits_of(k2)


# ---- hand-made tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(li.hand_made()))
def test_hand_made_tables(name):
    c = li.hand_made()[name]
    got = run_case(c)
    for what in ("next", "prev", "nearest_next", "nearest_prev"):
        assert getattr(got, what)["x"][0].tolist() == c[what], what
    forward, backward = li.brute(c["a"], c["b"], c["max_km"], None if c["keep_a"] is None else np.array([c["keep_a"]]),
                                 None if c["keep_b"] is None else np.array([c["keep_b"]]))
    assert same(got.forward_table.numpy(), forward) and same(got.backward_table.numpy(), backward)
    none = got.forward["x"][0][:, 1] < 0
    assert (got.forward["x"][0][none, 0] == li.INF_BITS).all()   # not live, or nothing in reach: the bits of +inf and -1


def test_hand_made_answers_in_kilometres_and_flags():
    got = run_case(li.hand_made()["across the seam"])
    step_km = EARTH_RADIUS / 1000.0 * math.radians(10.0)           # 10 degrees of the equator: 1111.99 km
    assert got.distance_km["x"][0, 0].item() == pytest.approx(step_km, rel=1e-12)
    assert torch.isnan(got.distance_km["x"][0, 1:]).all()
    tri = run_case(li.hand_made()["triangle"])
    assert tri.ends["x"][0].tolist() == [True, False, False, False] and tri.starts["x"][0].tolist() == [False] * 4
    assert tri.live_a["x"][0].tolist() == [True, True, False, False] and tri.live_b["x"][0].tolist() == [True, False, False, False]
    assert torch.isnan(tri.distance_km["x"][0, 0]) and tri.distance_km["x"][0, 1].item() == pytest.approx(step_km, rel=1e-12)
    pole = run_case(li.hand_made()["pole row"])
    assert pole.forward["x"][0, :2].tolist() == [[0, 0], [0, 0]] and pole.distance_km["x"][0, 0].item() == 0.0
    assert isinstance(got, Result) and got.cpu().forward_table is not None


@pytest.mark.parametrize("name", li.EXACT)
def test_exact_keys(name):
    """The same flat index on both sides has key 0 exactly; key == key_max is kept and the next larger key ignored: the cases and
    their written answers are `links_inputs.exact_cases`."""
    c = li.exact_cases()[name]
    got = link_extrema(c["a"], c["b"], c["max_km"])
    assert got.forward["x"][0].tolist() == c["forward"] and got.backward["x"][0].tolist() == c["backward"]
    mutual = [q if q >= 0 and c["backward"][q][1] == p else -1 for p, (_, q) in enumerate(c["forward"])]
    assert got.next["x"][0].tolist() == mutual


def test_exact_cases_decide_something():
    cases = li.exact_cases()
    assert sorted(cases) == list(li.EXACT)
    at, above = cases["key at key_max"], cases["key above key_max"]
    key = np.int64(at["forward"][0][0]).view(np.float64)
    assert distances.key_max_of(at["max_km"]) == key > distances.key_max_of(above["max_km"])
    assert at["forward"][0][1] == 0 and above["forward"][0][1] == -1


def test_atmospheric_layout_and_keep_by_name():
    lat, lon, wrap = li.grid(True)
    rng = np.random.default_rng(8)
    a = li.make([li.random_points(rng, 19, 36, 6) for _ in range(8)], lat, lon, wrap, 8)
    b = li.make([li.random_points(rng, 19, 36, 5) for _ in range(8)], lat, lon, wrap, 7)
    layout = (("t", 0, (2, 3)), ("msl", 6, (2,)))
    a, b = dataclasses.replace(a, layout=layout), dataclasses.replace(b, layout=layout)
    keep = rng.random((2, 3, 8)) < 0.5
    got = link_extrema(a, b, 4000.0, keep_a={"t": torch.from_numpy(keep)})
    assert got.forward["t"].shape == (2, 3, 8, 2) and got.backward["msl"].shape == (2, 7, 2) and got.next["t"].shape == (2, 3, 8)
    full = np.ones((8, 8), dtype=bool)
    full[:6] = keep.reshape(6, 8)
    forward, backward = li.brute(a, b, 4000.0, full, None)
    assert same(got.forward_table.numpy(), forward) and same(got.backward_table.numpy(), backward)


# ---- tracks --------------------------------------------------------------------------------------------------------------------
def five_steps(device="cpu"):
    """Track 0 dies after step 2, track 1 lasts throughout, track 2 is born at step 2; a column a step, tables in ascending flat
    index, M = 4."""
    lat, lon, wrap = li.grid(True)
    steps = [[(4, 20), (9, 2)], [(4, 21), (9, 3)], [(4, 22), (9, 4), (14, 30)], [(9, 5), (14, 31)], [(9, 6), (14, 32)]]
    return [li.make([pts], lat, lon, wrap, 4, device=device) for pts in steps]


FIVE_IDS = [[0, 1, -1, -1], [0, 1, -1, -1], [0, 1, 2, -1], [1, 2, -1, -1], [1, 2, -1, -1]]
FIVE_LENGTH = [[3, 5, 0, 0], [3, 5, 0, 0], [3, 5, 3, 0], [5, 3, 0, 0], [5, 3, 0, 0]]
FIVE_FIRST = [[0, 0, -1, -1], [0, 0, -1, -1], [0, 0, 2, -1], [0, 2, -1, -1], [0, 2, -1, -1]]


def test_five_steps_with_a_birth_and_a_death():
    t = tracks(five_steps(), 1500.0)
    assert t.track_id["x"].dtype == torch.int32 and t.track_id["x"].shape == (5, 1, 4)
    assert t.track_id["x"][:, 0].tolist() == FIVE_IDS and t.n_tracks["x"].tolist() == [3]
    assert t.length["x"][:, 0].tolist() == FIVE_LENGTH and t.first_step["x"][:, 0].tolist() == FIVE_FIRST
    assert len(t.links) == 4 and t.links[2].ends["x"][0].tolist() == [True, False, False, False]      # the death of track 0
    assert t.links[1].starts["x"][0].tolist() == [False, False, True, False]                          # the birth of track 2
    assert t.row["x"][2, 0].tolist() == [4, 9, 14, -1] and t.col["x"][4, 0].tolist() == [6, 32, -1, -1]
    out = t.cpu().tracks_of("x")
    assert [o["step"].tolist() for o in out] == [[0, 1, 2], [0, 1, 2, 3, 4], [2, 3, 4]]
    assert [o["row"].tolist() for o in out] == [[0, 0, 0], [1, 1, 1, 0, 0], [2, 1, 1]]
    assert [o["lat"].tolist() for o in out] == [[50.0] * 3, [0.0] * 5, [-50.0] * 3]
    assert [o["lon"].tolist() for o in out] == [[200.0, 210.0, 220.0], [20.0, 30.0, 40.0, 50.0, 60.0], [300.0, 310.0, 320.0]]
    assert all(o["value"].dtype == np.float32 and np.isfinite(o["value"]).all() for o in out)
    step_km = EARTH_RADIUS / 1000.0 * math.radians(10.0)
    assert np.isnan(out[1]["distance_km"][0]) and out[1]["distance_km"][1:] == pytest.approx([step_km] * 4, rel=1e-12)
    angle = math.acos(math.sin(math.radians(50)) ** 2 + math.cos(math.radians(50)) ** 2 * math.cos(math.radians(10)))
    assert np.isnan(out[0]["distance_km"][0]) and out[0]["distance_km"][1:] == pytest.approx([EARTH_RADIUS / 1000.0 * angle] * 2, rel=1e-9)
    assert [o["step"].tolist() for o in t.tracks_of("x", min_length=4)] == [[0, 1, 2, 3, 4]]
    with pytest.raises(ValueError, match="tracks_of: no variable 'y'"):
        t.tracks_of("y")
    with pytest.raises(ValueError, match="surface variable and has no level"):
        t.tracks_of("x", c=1)
    with pytest.raises(ValueError, match=r"has the planes \(1,\), got \(3,\)"):
        t.tracks_of("x", b=3)


def test_cpu_moves_every_step_once():
    t = tracks(five_steps(), 1500.0)
    moved = t.cpu()
    assert len(moved.steps) == 5 and len(moved.links) == 4
    for k, l in enumerate(moved.links):                                       # the links share the steps: one host copy each
        assert l.a is moved.steps[k] and l.b is moved.steps[k + 1]
    assert moved.links[0].b is moved.links[1].a
    assert moved.track_id["x"][:, 0].tolist() == FIVE_IDS and moved.links[2].ends["x"][0].tolist() == [True, False, False, False]


def test_keep_takes_a_node_out_of_its_track():
    keep = [None, None, {"x": torch.tensor([[True, False, True, True]])}, None, None]     # step 2 loses the node of track 1
    t = tracks(five_steps(), 1500.0, keep=keep)
    assert t.track_id["x"][:, 0].tolist() == [[0, 1, -1, -1], [0, 1, -1, -1], [0, -1, 2, -1], [3, 2, -1, -1], [3, 2, -1, -1]]
    assert t.n_tracks["x"].tolist() == [4]
    assert t.length["x"][:, 0].tolist() == [[3, 2, 0, 0], [3, 2, 0, 0], [3, 0, 3, 0], [2, 3, 0, 0], [2, 3, 0, 0]]


def test_a_field_moved_two_columns_a_step_keeps_every_track():
    lat, lon = np.linspace(90, -90, 33), full_lon(140)            # two columns: 572 km on the equator, under half the 1234.5 km
    x = red_noise((2, 33, 140), 21)                               # that separate two extrema, so the moved point is the nearest
    steps = [extrema(batch_of(np.roll(x, 2 * t, axis=-1), lat, lon), 1234.5, max_points=64) for t in range(5)]
    count = steps[0].count["x"]
    assert all(torch.equal(e.count["x"], count) for e in steps) and 3 < int(count.min()) and int(count.max()) <= 64
    t = tracks(steps, 700.0)
    assert torch.equal(t.n_tracks["x"], count)
    live = t.track_id["x"] >= 0
    assert (t.length["x"][live] == 5).all() and (t.first_step["x"][live] == 0).all() and (t.length["x"][~live] == 0).all()
    for b in range(2):
        for o in t.cpu().tracks_of("x", b=b):
            moved = (o["lon"][1:] - o["lon"][:-1]) % 360.0
            assert o["step"].tolist() == [0, 1, 2, 3, 4] and np.allclose(moved, 2 * 360.0 / 140) and len(set(o["lat"])) == 1
            assert len(set(o["value"].tolist())) == 1


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_of_link_extrema():
    lat, lon, wrap = li.grid(True)
    pts = [[(9, 10)]]
    a = li.make(pts, lat, lon, wrap, 4)
    ok = lambda **kw: li.make(pts, **{**dict(lat=lat, lon=lon, wrap=wrap, max_points=4), **kw})  # noqa: E731
    with pytest.raises(TypeError, match="link_extrema: b must be an Extrema"):
        link_extrema(a, "b", 100.0)
    with pytest.raises(ValueError, match="link_extrema: a and b differ in layout"):
        link_extrema(a, ok(name="y"), 100.0)
    with pytest.raises(ValueError, match="link_extrema: a and b differ in layout"):
        link_extrema(a, li.make(pts * 2, lat, lon, wrap, 4), 100.0)
    with pytest.raises(ValueError, match="link_extrema: a and b differ in kind: 'min' against 'max'"):
        link_extrema(a, ok(kind="max"), 100.0)
    with pytest.raises(ValueError, match="link_extrema: a and b differ in wrap: True against False"):
        link_extrema(a, ok(lon=li.LON_REGIONAL, wrap=False), 100.0)
    with pytest.raises(ValueError, match=r"link_extrema: a and b differ in grid: 19 x 36 against 19 x 72 points; regrid first"):
        link_extrema(a, ok(lon=full_lon(72)), 100.0)
    with pytest.raises(ValueError, match="link_extrema: a and b differ in grid_lat"):
        link_extrema(a, ok(lat=li.LAT19[::-1].copy()), 100.0)
    with pytest.raises(ValueError, match="link_extrema: a and b differ in grid_lon"):
        link_extrema(dataclasses.replace(a, wrap=False), ok(lon=li.LON_REGIONAL, wrap=False), 100.0)
    with pytest.raises(ValueError, match="link_extrema: a is on cpu and b on meta"):
        link_extrema(a, dataclasses.replace(a, table_table=a.table_table.to("meta")), 100.0)
    for bad in (None, 0.0, -3.0, float("nan"), float("inf"), "far", True):
        with pytest.raises(ValueError, match="link_extrema: max_km"):
            link_extrema(a, a, bad)
    with pytest.raises(TypeError, match="link_extrema: keep_a must be None or a dict"):
        link_extrema(a, a, 100.0, keep_a=torch.ones(1, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="link_extrema: keep_b names the variable 'y'"):
        link_extrema(a, a, 100.0, keep_b={"y": torch.ones(1, 4, dtype=torch.bool)})
    with pytest.raises(TypeError, match=r"link_extrema: keep_a\['x'\] must be a bool tensor, got torch.int64"):
        link_extrema(a, a, 100.0, keep_a={"x": torch.ones(1, 4, dtype=torch.int64)})
    with pytest.raises(ValueError, match=r"link_extrema: keep_a\['x'\] has shape \(1, 5\), not \(1, 4\)"):
        link_extrema(a, a, 100.0, keep_a={"x": torch.ones(1, 5, dtype=torch.bool)})
    with pytest.raises(ValueError, match=r"link_extrema: keep_a\['x'\] is on meta and the tables on cpu"):
        link_extrema(a, a, 100.0, keep_a={"x": torch.ones(1, 4, dtype=torch.bool, device="meta")})
    bent = li.LAT19.copy()
    bent[3], bent[4] = bent[4], bent[3]                                       # a grid that the distance tables refuse
    with pytest.raises(ValueError, match="^link_extrema: the latitudes must be strictly monotone"):
        link_extrema(ok(lat=bent), ok(lat=bent), 100.0)
    wide = ok(lat=np.zeros(1), lon=full_lon(4100))
    with pytest.raises(ValueError, match="^link_extrema: the grid has 4100 longitudes; 1 to 4096 are supported"):
        link_extrema(wide, wide, 100.0)
    different = link_extrema(a, ok(max_points=9, radius_km=77.0), 100.0)      # radius_km and max_points may differ
    assert different.forward["x"].shape == (1, 4, 2) and different.backward["x"].shape == (1, 9, 2)


def test_refusals_of_tracks():
    lat, lon, wrap = li.grid(True)
    a = li.make([[(9, 10)]], lat, lon, wrap, 4)
    with pytest.raises(TypeError, match="tracks: steps must be a sequence of Extrema"):
        tracks(a, 100.0)
    with pytest.raises(ValueError, match="tracks: 2 to 256 steps are linked, got 1"):
        tracks([a], 100.0)
    with pytest.raises(ValueError, match="tracks: 2 to 256 steps are linked, got 257"):
        tracks([a] * 257, 100.0)
    with pytest.raises(TypeError, match=r"tracks: steps\[1\] must be an Extrema"):
        tracks([a, None], 100.0)
    with pytest.raises(ValueError, match=r"tracks: steps\[0\] and steps\[2\] differ in max_points: 4 against 5"):
        tracks([a, a, li.make([[(9, 10)]], lat, lon, wrap, 5)], 100.0)
    with pytest.raises(ValueError, match=r"tracks: steps\[0\] and steps\[1\] differ in kind"):
        tracks([a, dataclasses.replace(a, kind="max")], 100.0)
    with pytest.raises(ValueError, match="tracks: keep holds 1 entries for 2 steps"):
        tracks([a, a], 100.0, keep=[None])
    with pytest.raises(TypeError, match="tracks: keep must be None or a sequence"):
        tracks([a, a], 100.0, keep={"x": None})
    with pytest.raises(ValueError, match="link_extrema: max_km"):
        tracks([a, a], None)
    t = tracks([a, a], 100.0)
    with pytest.raises(ValueError, match="tracks_of: the result is on a device"):
        dataclasses.replace(t, track_id_table=t.track_id_table.to("meta")).tracks_of("x")


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_the_c_entry_point_refuses_before_any_launch():
    from aurora_amd.engine import lib

    raw, header = lib.load(), (lib.library_path().parents[2] / "include" / "aurora_hip.h").read_text()
    name = "aurora_hip_link_extrema"
    assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    assert "links.hip" in importlib.import_module("aurora_amd.build").SOURCES
    assert aurora_amd.link_extrema is mod.link_extrema and aurora_amd.tracks is mod.tracks
    assert {"link_extrema", "Links", "tracks", "Tracks"} <= set(aurora_amd.__all__)
    err = lambda: raw.aurora_hip_last_error()  # noqa: E731
    big = 1 << 30                                                 # (addresses far apart: nothing is dereferenced before a launch)
    args = lambda **kw: tuple({**dict(table_a=big, count_a=2 * big, keep_a=None, ma=64, table_b=3 * big, count_b=4 * big,  # noqa: E731
                                     keep_b=None, mb=32, n_planes=3, tables=5 * big, n_lat=9, n_lon=12, wrap=1, key_max=0.5,
                                     forward=6 * big, backward=7 * big, stream=None), **kw}.values())
    for kw, text in ((dict(n_lon=4097), b"4097 longitudes; 1 to 4096 are supported"), (dict(n_lat=600000, n_lon=4096), b"too large"),
                     (dict(n_lon=0), b"bad sizes"), (dict(n_planes=-1), b"bad sizes"), (dict(ma=0), b"max_points"),
                     (dict(mb=65537), b"max_points"), (dict(wrap=2), b"wrap"), (dict(key_max=-1.0), b"key_max"),
                     (dict(key_max=float("nan")), b"key_max"), (dict(table_a=None), b"null"), (dict(count_b=None), b"null"),
                     (dict(tables=None), b"null"), (dict(backward=None), b"null"), (dict(table_b=3 * big + 4), b"aligned"),
                     (dict(count_a=2 * big + 2), b"aligned"), (dict(forward=6 * big + 4), b"aligned"),
                     (dict(backward=6 * big + 16), b"overlap"), (dict(forward=big + 8), b"overlap"),
                     (dict(keep_b=7 * big + 95), b"overlap"), (dict(backward=5 * big + 8 * 29), b"overlap")):
        assert raw.aurora_hip_link_extrema(*args(**kw)) == -1 and text in err(), (kw, err())
    assert raw.aurora_hip_link_extrema(*args(n_planes=0)) == 0
