"""aurora_amd.link_extrema and aurora_amd.tracks on the device: forward and backward EQUAL the numpy path's in every byte and every
finalised tensor has the same bits (THE RULE of aurora_amd/links.py; nothing here has a tolerance), at live counts on either side
of every thread-chunk (256) and LDS-tile (1024) boundary, on hand-made tables, on the real smooth -> extrema chain, independent of
the other planes of a call, repeatable, inside guard regions, replayed from a graph; and what the binding refuses."""
import dataclasses
import functools
import importlib

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import extrema, smooth
from aurora_amd.engine import lib
from tests import links_inputs as li
from tests.device_buffers import same_bits
from tests.test_links_host import FIVE_IDS, five_steps, keep_dict
from tests.test_smooth_host import batch_of, full_lon
from tests.verification_inputs import DEV, carve, red_noise

pytestmark = pytest.mark.gpu

mod = importlib.import_module("aurora_amd.links")
link_extrema, tracks = aurora_amd.link_extrema, aurora_amd.tracks
FINAL = ("next", "prev", "nearest_next", "nearest_prev", "distance_km", "ends", "starts", "live_a", "live_b")
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1500)      # the tile is 1024 rows, a chunk 256
GRIDS = {"40 x 257 wrapping": (np.linspace(88, -88, 40), full_lon(257), True),
         "33 x 64 regional": (np.linspace(70, -10, 33), -20.0 + 1.25 * np.arange(64), False)}


def bits(t):
    return t.to(torch.int32) if t.dtype == torch.bool else t


def to_device(e):
    moved = {f: getattr(e, f).to(DEV) for f in ("index_table", "filtered_table", "table_table", "count_table", "grid_lat", "grid_lon")}
    return dataclasses.replace(e, **moved)


def on_device(keep):
    return None if keep is None else {k: v.to(DEV) for k, v in keep.items()}


def same_links(dev, host):
    assert dev.forward_table.is_cuda and dev.backward_table.is_cuda
    d = dev.cpu()
    assert same_bits(d.forward_table, host.forward_table), "forward differs from the numpy path's"
    assert same_bits(d.backward_table, host.backward_table), "backward differs from the numpy path's"
    for name in FINAL:
        for k, v in getattr(host, name).items():
            assert same_bits(bits(getattr(dev, name)[k].cpu()), bits(v)), f"{name} differs"


def check(a, b, max_km, keep_a=None, keep_b=None):
    """The device's links of two host `Extrema`, after they were held to the numpy path's."""
    host = link_extrema(a, b, max_km, keep_a=keep_a, keep_b=keep_b)
    dev = link_extrema(to_device(a), to_device(b), max_km, keep_a=on_device(keep_a), keep_b=on_device(keep_b))
    same_links(dev, host)
    return dev, host


@functools.lru_cache(maxsize=None)
def counted(name, shift):
    """A plane per entry of COUNTS: that many live rows in a, the count `shift` places on in b; Ma = 1536, Mb = 1500."""
    lat, lon, wrap = GRIDS[name]
    rng = np.random.default_rng(len(name) + shift)
    H, W = len(lat), len(lon)
    a = li.make([li.random_points(rng, H, W, n) for n in COUNTS], lat, lon, wrap, 1536)
    b = li.make([li.random_points(rng, H, W, COUNTS[(i + shift) % len(COUNTS)]) for i in range(len(COUNTS))], lat, lon, wrap, 1500)
    return a, b


# ---- every chunk and tile boundary ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 5, 8])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_counts_across_chunks_and_tiles(name, shift):
    a, b = counted(name, shift)
    max_km = 900.0 if GRIDS[name][2] else 150.0
    _, host = check(a, b, max_km)
    nxt = host.next["x"]
    assert (nxt >= 0).any(dim=-1).sum() >= 8 and (host.ends["x"]).any()      # links and ends: the case decides something


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_keep_masks_on_the_device(name):
    a, b = counted(name, 5)
    rng = np.random.default_rng(77)
    keep_a = {"x": torch.from_numpy(rng.random((len(COUNTS), 1536)) < 0.6)}
    keep_b = {"x": torch.from_numpy(rng.random((len(COUNTS), 1500)) < 0.6)}
    _, host = check(a, b, 2000.0, keep_a, keep_b)
    _, free = check(a, b, 2000.0, None, keep_b)
    assert not same_bits(host.forward_table, free.forward_table)


def test_4096_by_4096_on_one_plane():
    lat, lon, wrap = GRIDS["40 x 257 wrapping"]
    rng = np.random.default_rng(4096)
    a = li.make([li.random_points(rng, 40, 257, 4096)], lat, lon, wrap, 4096)
    b = li.make([li.random_points(rng, 40, 257, 4096)], lat, lon, wrap, 4096)
    _, host = check(a, b, 400.0)
    assert (host.next["x"] >= 0).sum() > 1000


@pytest.mark.parametrize("name", sorted(li.hand_made()))
def test_hand_made_tables_on_the_device(name):
    c = li.hand_made()[name]
    dev, _ = check(c["a"], c["b"], c["max_km"], keep_dict(c["keep_a"]), keep_dict(c["keep_b"]))
    for what in ("next", "prev", "nearest_next", "nearest_prev"):
        assert getattr(dev, what)["x"][0].tolist() == c[what], what


@pytest.mark.parametrize("name", li.EXACT)
def test_exact_keys_on_the_device(name):
    """key == key_max is kept (key_max travels by value to the kernel's <=), the next smaller key_max loses the pair, and one and
    the same grid point has key 0 on a row where the formula alone has not: the written answers of `links_inputs.exact_cases`."""
    c = li.exact_cases()[name]
    dev, _ = check(c["a"], c["b"], c["max_km"])
    assert dev.forward["x"][0].tolist() == c["forward"] and dev.backward["x"][0].tolist() == c["backward"]


# ---- the real chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,planes", [(181, 360, 3), (721, 1440, 1)])
def test_the_real_chain(H, W, planes):
    lat, lon = np.linspace(90, -90, H), full_lon(W)
    x = red_noise((planes, H, W), 5 + H)
    steps = []
    for moved in (x, np.roll(x, 3, axis=-1)):                               # the field, and the field moved 3 columns east
        b = batch_of(moved, lat, lon)
        b = aurora_amd.Batch({k: carve(v) for k, v in b.surf_vars.items()}, {}, {}, b.metadata)
        steps.append(extrema(smooth(b, 100.0), 300.0, max_points=4096))
    a, b = steps
    dev = link_extrema(a, b, 500.0)
    host = link_extrema(a.cpu(), b.cpu(), 500.0)                              # (the device's extrema are the numpy path's: test_gpu_extrema)
    same_links(dev, host)
    count = host.a.count["x"]
    assert int(count.min()) > 20 and not host.a.truncated["x"].any()
    linked = (host.next["x"] >= 0).sum(dim=-1)
    assert (linked > count // 2).all()                                        # most lows find themselves 3 columns on
    t = tracks([a, b], 500.0)
    th = tracks([a.cpu(), b.cpu()], 500.0)
    assert same_bits(t.track_id_table.cpu(), th.track_id_table) and same_bits(t.n_tracks_table.cpu(), th.n_tracks_table)


# ---- independence, repeatability, guards, graphs -----------------------------------------------------------------------------
def planes_of(e, rows):
    return dataclasses.replace(e, table_table=e.table_table[rows].contiguous(), count_table=e.count_table[rows].contiguous(),
                               layout=(("x", 0, (len(rows),)),))


def test_a_plane_alone_among_three_and_as_the_last_of_seven():
    a, b = counted("40 x 257 wrapping", 5)
    a, b = to_device(a), to_device(b)
    p = 8                                                                     # 1023 rows against 2
    q = 10                                                                    # 1025 rows against 64
    for plane in (p, q):
        alone = link_extrema(planes_of(a, [plane]), planes_of(b, [plane]), 900.0)
        three = link_extrema(planes_of(a, [0, plane, 3]), planes_of(b, [0, plane, 3]), 900.0)
        seven = link_extrema(planes_of(a, [1, 2, 3, 4, 5, 6, plane]), planes_of(b, [1, 2, 3, 4, 5, 6, plane]), 900.0)
        for name in ("forward_table", "backward_table"):
            assert same_bits(getattr(alone, name)[0], getattr(three, name)[1])
            assert same_bits(getattr(alone, name)[0], getattr(seven, name)[6])


def test_two_calls_give_the_same_bytes():
    a, b = counted("33 x 64 regional", 8)
    a, b = to_device(a), to_device(b)
    one, two = link_extrema(a, b, 150.0), link_extrema(a, b, 150.0)
    assert same_bits(one.forward_table, two.forward_table) and same_bits(one.backward_table, two.backward_table)


def binding_args(a, b):
    grid = mod.types.SimpleNamespace(lat=a.grid_lat, lon=a.grid_lon, wrap=a.wrap)
    tables = mod.distances._device_tables(grid, a.table_table.device)
    return (a.table_table, a.count_table, None, b.table_table, b.count_table, None, tables, a.grid_lat.shape[0], a.grid_lon.shape[0],
            bool(a.wrap))


def test_guards_around_the_outputs():
    a, b = counted("40 x 257 wrapping", 1)
    a, b = to_device(a), to_device(b)
    want = link_extrema(a, b, 900.0)
    n, guard = len(COUNTS), 512
    sizes = (n * 1536 * 2, n * 1500 * 2)
    bufs = [torch.full((guard + size + guard,), -7, dtype=torch.int64, device=DEV) for size in sizes]
    out = (bufs[0][guard:guard + sizes[0]].view(n, 1536, 2), bufs[1][guard:guard + sizes[1]].view(n, 1500, 2))
    got = lib.link_extrema_tables(*binding_args(a, b), mod.distances.key_max_of(900.0), out=out)
    assert got[0] is out[0] and same_bits(out[0], want.forward_table) and same_bits(out[1], want.backward_table)
    for buf, size in zip(bufs, sizes):
        assert (buf[:guard] == -7).all() and (buf[guard + size:] == -7).all()
    assert (out[0] != -7).all() and (out[1] != -7).all()                     # every row of both is written


def test_capture_in_a_hip_graph():
    a, b = counted("33 x 64 regional", 1)
    other_a, other_b = counted("33 x 64 regional", 5)
    want = link_extrema(other_a, other_b, 150.0)                              # on the host
    a, b = to_device(a), to_device(b)
    a = dataclasses.replace(a, table_table=a.table_table.clone(), count_table=a.count_table.clone())
    b = dataclasses.replace(b, table_table=b.table_table.clone(), count_table=b.count_table.clone(),
                            grid_lat=a.grid_lat, grid_lon=a.grid_lon)     # one coordinate tensor per grid, as `extrema` hands out
    link_extrema(a, b, 150.0)                                                 # the eager call: (s, c, cd) uploaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = link_extrema(a, b, 150.0)
        nxt = out.next["x"]
    for e, o in ((a, other_a), (b, other_b)):
        e.table_table.copy_(o.table_table)
        e.count_table.copy_(o.count_table)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out.forward_table.cpu(), want.forward_table) and same_bits(out.backward_table.cpu(), want.backward_table)
    assert same_bits(nxt.cpu(), want.next["x"])
    with pytest.MonkeyPatch.context() as mp:                                 # a cold call during capture is refused
        mp.setattr(mod.distances._fields, "tables", mod.distances._fields.DeviceTables(capturing=lambda: True))
        with pytest.raises(RuntimeError, match="nearest_event: call once on this grid before capturing a graph"):
            link_extrema(a, b, 150.0)


# ---- tracks --------------------------------------------------------------------------------------------------------------------
def test_tracks_over_five_steps_equal_the_hosts():
    host, dev = tracks(five_steps(), 1500.0), tracks(five_steps(DEV), 1500.0)
    assert dev.track_id_table.is_cuda and dev.track_id["x"][:, 0].tolist() == FIVE_IDS
    lat, lon, wrap = GRIDS["40 x 257 wrapping"]
    rng = np.random.default_rng(55)
    first = [np.array(li.random_points(rng, 40, 257, n)) for n in (300, 40, 1)]
    steps = []
    for t in range(5):                                                        # 2 columns east a step; every third point dies at step 2,
        pts = [np.sort(np.concatenate([(f // 257) * 257 + (f % 257 + 2 * t) % 257, [7 * 257 + 11] * (t >= 3)])) for f in first]
        pts = [p[(np.arange(p.size) % 3 != 0) | (t < 2)].astype(int).tolist() for p in pts]     # one is born at step 3
        steps.append(li.make(pts, lat, lon, wrap, 320))
    keep = [None, {"x": torch.from_numpy(rng.random((3, 320)) < 0.8)}, None, None, {}]
    h = tracks(steps, 600.0, keep=keep)
    d = tracks([to_device(e) for e in steps], 600.0, keep=[on_device(k) for k in keep])
    assert int(h.n_tracks["x"][0]) > 300 and (h.length["x"] == 5).any() and (h.length["x"] == 2).any()
    for got, want in ((dev, host), (d, h)):
        for name in ("track_id_table", "n_tracks_table", "length_table", "first_step_table"):
            assert same_bits(getattr(got, name).cpu(), getattr(want, name)), name
        for name in ("value", "lat", "lon", "row", "col"):
            assert same_bits(getattr(got, name)["x"].cpu(), getattr(want, name)["x"]), name
        for lg, lw in zip(got.links, want.links):
            same_links(lg, lw)
        moved = got.cpu()
        assert all(l.a is moved.steps[k] and l.b is moved.steps[k + 1] for k, l in enumerate(moved.links))     # one host copy a step
        assert [o["row"].tolist() for o in moved.tracks_of("x")] == [o["row"].tolist() for o in want.tracks_of("x")]


# ---- what the binding refuses, and in which words -------------------------------------------------------------------------------
def _operands(**kw):
    i64, i32 = (lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)), (lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV))
    args = dict(table_a=i64(2, 8, 2), count_a=i32(2), keep_a=None, table_b=i64(2, 6, 2), count_b=i32(2), keep_b=None,
                tables=torch.zeros(2 * 3 + 5, dtype=torch.float64, device=DEV), n_lat=3, n_lon=5, wrap=True, key_max=0.5)
    out = kw.pop("out", None)
    args.update(kw)
    return lambda: lib.link_extrema_tables(*args.values(), out=out)


_I64 = lambda *s, device=DEV: torch.zeros(*s, dtype=torch.int64, device=device)  # noqa: E731
_TABLE = "(n_planes, max_points, 2) int64 tensor"
_FLAT = lambda: _I64(64)  # noqa: E731

# name -> (the operands that differ, made when the case runs; the whole message)
CASES = {
    "table_a int32": (lambda: dict(table_a=torch.zeros(2, 8, 2, dtype=torch.int32, device=DEV)),
                      f"link_extrema_tables: table_a must be a contiguous {_TABLE} on the device"),
    "table_a on the host": (lambda: dict(table_a=_I64(2, 8, 2, device="cpu")),
                            f"link_extrema_tables: table_a must be a contiguous {_TABLE} on the device"),
    "table_b strided": (lambda: dict(table_b=_I64(2, 6, 4)[..., ::2]),
                        f"link_extrema_tables: table_b must be a contiguous {_TABLE} on the device of table_a"),
    "table_b planes": (lambda: dict(table_b=_I64(3, 6, 2)), "link_extrema_tables: table_b has shape (3, 6, 2), not (2, 1..65536, 2)"),
    "table_a columns": (lambda: dict(table_a=_I64(2, 8, 3)), "link_extrema_tables: table_a has shape (2, 8, 3), not (2, 1..65536, 2)"),
    "count_a int64": (lambda: dict(count_a=_I64(2)),
                      "link_extrema_tables: count_a must be a contiguous (n_planes,) int32 vector on the device of table_a"),
    "count_b length": (lambda: dict(count_b=torch.zeros(3, dtype=torch.int32, device=DEV)),
                       "link_extrema_tables: count_b must be a contiguous (n_planes,) int32 vector on the device of table_a"),
    "keep_a uint8": (lambda: dict(keep_a=torch.ones(2, 8, dtype=torch.uint8, device=DEV)),
                     "link_extrema_tables: keep_a must be a contiguous (n_planes, max_points) bool matrix on the device of table_a"),
    "keep_b shape": (lambda: dict(keep_b=torch.ones(2, 8, dtype=torch.bool, device=DEV)),
                     "link_extrema_tables: keep_b must be a contiguous (n_planes, max_points) bool matrix on the device of table_a"),
    "tables length": (lambda: dict(tables=torch.zeros(12, dtype=torch.float64, device=DEV)),
                      "link_extrema_tables: tables must be a contiguous (2 n_lat + n_lon,) fp64 vector on the device of table_a"),
    "n_lon": (lambda: dict(n_lon=4097, tables=torch.zeros(6 + 4097, dtype=torch.float64, device=DEV)),
              "link_extrema_tables: n_lat must be at least 1 and n_lon in 1..4096, got 3 and 4097"),
    "forward shape": (lambda: dict(out=(_I64(2, 6, 2), _I64(2, 6, 2))),
                      "link_extrema_tables: forward must be a contiguous torch.int64 tensor of shape (2, 8, 2) on the device of table_a"),
    "backward dtype": (lambda: dict(out=(_I64(2, 8, 2), torch.zeros(2, 6, 2, dtype=torch.int32, device=DEV))),
                       "link_extrema_tables: backward must be a contiguous torch.int64 tensor of shape (2, 6, 2) on the device of table_a"),
    "outputs overlap": (lambda: (lambda flat: dict(out=(flat[:32].view(2, 8, 2), flat[24:48].view(2, 6, 2))))(_FLAT()),
                        "link_extrema_tables: forward and backward must not overlap each other or an input"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_binding_refusals(name):
    kw, message = CASES[name]
    with pytest.raises(AssertionError) as info:
        _operands(**kw())()
    assert str(info.value) == message


def test_binding_refuses_an_output_that_is_an_input():
    table_a = torch.zeros(2, 8, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(AssertionError, match="link_extrema_tables: forward and backward must not overlap each other or an input"):
        _operands(table_a=table_a, out=(table_a, torch.zeros(2, 6, 2, dtype=torch.int64, device=DEV)))()
    forward, backward = _operands()()                                         # and the same operands, unchanged, are taken
    assert forward.shape == (2, 8, 2) and backward.shape == (2, 6, 2)
