"""aurora_hip_extrema (aurora_amd/csrc/extrema.hip) through `aurora_amd.extrema` on the device: every byte of index, filtered,
table and count equals the numpy path's (which tests/test_extrema_host.py holds to a brute force) -- no tolerance anywhere --
at every width and height at which the kernel takes another path, on regional, ascending and polar grids; the bytes are
repeatable, independent of the other planes of a call and of plane alignment, replayed from a graph, and nothing is written
outside the outputs and the workspace."""
import functools
import importlib

import numpy as np
import pytest
import torch

from aurora_amd import Batch, _fields, smooth
from aurora_amd.engine import lib
from tests.device_buffers import same_bits
from tests.test_extrema_host import GRIDS, planes_for
from tests.test_smooth_host import batch_of, field, full_lon
from tests.verification_inputs import DEV, carve, red_noise

pytestmark = pytest.mark.gpu

mod = importlib.import_module("aurora_amd.extrema")
smooth_mod = importlib.import_module("aurora_amd.smooth")
extrema = mod.extrema
TABLES = ("index_table", "filtered_table", "table_table", "count_table")


def lat_of(H, ascending=False):
    lat = np.linspace(90, -90, H) if H > 1 else np.zeros(1)
    return lat[::-1].copy() if ascending else lat


def on_device(b: Batch, offset_floats=0) -> Batch:
    return Batch({k: carve(v, offset_floats) for k, v in b.surf_vars.items()}, {}, {}, b.metadata)


def same_result(dev, host) -> None:
    """Every table of a device result (moved to the host) has the bytes of the numpy path's."""
    for name in TABLES:
        d, h = getattr(dev, name), getattr(host, name)
        assert not h.is_cuda and same_bits(d.cpu(), h), f"{name} differs from the numpy path's"


def check(x, lat, lon, radius, offset_floats=0, **kw):
    """The device's result for the planes x (n, H, W), after it was held to the numpy path's."""
    b = batch_of(np.array(x), lat, lon)
    host = extrema(b, radius, **kw)
    dev = extrema(on_device(b, offset_floats), radius, **kw)
    assert dev.index_table.is_cuda and dev.index_table.shape == x.shape and dev.grid_lat.is_cuda
    same_result(dev, host)
    assert same_bits(dev.is_extremum["x"].cpu().to(torch.int32), host.is_extremum["x"].to(torch.int32))
    for name in ("value", "lat", "lon", "row", "col"):                      # finalised in torch: the same bits on either device
        assert same_bits(getattr(dev, name)["x"].cpu(), getattr(host, name)["x"])
    return dev


def scattered(shape, seed):
    """Three red-noise planes with NaN and infinities scattered over the second and third."""
    H, W = shape
    x = red_noise((3, H, W), seed)
    if H * W > 6:
        g = np.random.default_rng(seed)
        x[1][g.random((H, W)) < 0.1] = np.nan
        x[2, H // 2, W // 2], x[2, 0, W - 1] = np.inf, -np.inf
        x[2][g.random((H, W)) < 0.02] = np.inf
    return x


# ---- shapes and heights -----------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 2), (5, 3), (9, 63), (16, 64), (17, 65), (33, 255), (40, 256), (7, 257)]


@pytest.mark.parametrize("kind", ["min", "max"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_against_numpy(H, W, kind):
    x = scattered((H, W), 10 + W)
    lon = full_lon(W) if W > 1 else np.array([12.0])
    check(x, lat_of(H), lon, 1234.5, kind=kind)
    if W in (64, 256):
        check(x, lat_of(H), lon, 1234.5, offset_floats=1, kind=kind)        # planes that are not 16-byte aligned


def test_every_height():
    for H in range(1, 41):                                                  # the last row block holds 1 to 4 rows
        check(scattered((H, 24), 100 + H), lat_of(H), full_lon(24), 1500.0, offset_floats=H % 2, kind=("min", "max")[H % 2])
        check(scattered((H, 24), 100 + H)[:1], lat_of(H), full_lon(24), 1500.0, kind=("max", "min")[H % 2])


@pytest.mark.parametrize("kind", ["min", "max"])
@pytest.mark.parametrize("name", ["regional 17 x 39", "19 x 40 ascending", "polar disc covers the circle"])
def test_grids(name, kind):
    lat, lon, wrap, radius = GRIDS[name]
    dev = check(planes_for(len(lat), len(lon), 21), lat, lon, radius, kind=kind, max_points=len(lat) * len(lon))
    assert dev.wrap == wrap and int(dev.count["x"][5]) == 1                 # the constant plane


# ---- large planes -------------------------------------------------------------------------------------------------------------
def test_one_degree_grid_at_500_km():
    x = red_noise((2, 181, 360), 31)
    x[0, 60:64, 100:130] = np.nan
    check(x, lat_of(181), full_lon(360), 500.0, kind="min")
    check(x[1:], lat_of(181), full_lon(360), 500.0, kind="max")


def test_quarter_degree_plane_at_300_km():
    x = red_noise((1, 721, 1440), 32)                                       # six columns a thread; whole-row windows near the poles
    x[0, 300:303, 700:760], x[0, 0, 5], x[0, 720, :] = np.nan, np.inf, np.nan
    dev = check(x, lat_of(721), full_lon(1440), 300.0, kind="min")
    assert 1 <= int(dev.count["x"]) <= 4096


def test_the_widest_row():
    x = red_noise((2, 12, 4096), 33)                                        # sixteen columns a thread, 64 KiB of LDS
    x[1, 5, 4000:4096], x[1, 6, 0] = np.nan, -np.inf
    check(x, lat_of(12), full_lon(4096), 2500.0, kind="max")
    check(x[:1], lat_of(12), full_lon(4096), 1900.0, kind="min", offset_floats=3)


# ---- bytes and placement -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seven():
    """The seven 33 x 70 planes of the host tests (NaN, infinities, a NaN row, all NaN, constant, signed zeros); never modified."""
    return planes_for(33, 70, 40)


def device_result(x, offset_floats=0, **kw):
    return extrema(on_device(batch_of(np.array(x), lat_of(33), full_lon(70)), offset_floats), 1234.5, **kw)


def test_same_bytes_twice_and_wherever_a_plane_sits():
    x = seven()
    a, b = device_result(x), device_result(x)
    for name in TABLES:
        assert same_bits(getattr(a, name), getattr(b, name))
    last = x[6:7]
    alone = device_result(last)
    among = device_result(np.concatenate([x[0:1], last, x[3:4]]))
    unaligned = device_result(x, 1)
    for name in TABLES:
        assert same_bits(getattr(alone, name)[0], getattr(among, name)[1]) and same_bits(getattr(alone, name)[0], getattr(a, name)[6])
        assert same_bits(getattr(unaligned, name), getattr(a, name))


def rows_of(radius=1234.5):
    table = smooth_mod.disc_table(lat_of(33), float(np.deg2rad(360.0 / 70)), 70, True, radius)
    return torch.from_numpy(smooth_mod._packed(table)).to(DEV)


def test_guards_around_outputs_and_workspace():
    x = seven()
    rows, fields = rows_of(), [carve(x)]
    whole = lib.extrema_planes(fields, rows, True, False, 4096)
    assert [tuple(t.shape) for t in whole] == [(7, 33, 70), (7, 33, 70), (7, 4096, 2), (7,)]
    need = lib.extrema_workspace_bytes(7, 33, 70)
    assert need == 16 * 7 * 33                                               # per row, not per point
    guard, n = 512, 7 * 33 * 70
    i_buf = torch.full((guard + n + guard,), -7, dtype=torch.int32, device=DEV)
    f_buf = torch.full((guard + n + guard,), float("nan"), device=DEV)
    t_buf = torch.full((guard + 7 * 4096 * 2 + guard,), -7, dtype=torch.int64, device=DEV)
    c_buf = torch.full((guard + 7 + guard,), -7, dtype=torch.int32, device=DEV)
    ws_buf = torch.full((guard + need + guard,), 0xAB, dtype=torch.uint8, device=DEV)
    out = (i_buf[guard:guard + n].view(7, 33, 70), f_buf[guard:guard + n].view(7, 33, 70),
           t_buf[guard:guard + 7 * 4096 * 2].view(7, 4096, 2), c_buf[guard:guard + 7])
    lib.extrema_planes(fields, rows, True, False, 4096, out=out, workspace=ws_buf[guard:guard + need])
    for got, want in zip(out, whole):
        assert same_bits(got, want)
    for buf, size in ((i_buf, n), (t_buf, 7 * 4096 * 2), (c_buf, 7)):
        assert (buf[:guard] == -7).all() and (buf[guard + size:] == -7).all()
    assert torch.isnan(f_buf[:guard]).all() and torch.isnan(f_buf[guard + n:]).all()
    assert (ws_buf[:guard] == 0xAB).all() and (ws_buf[guard + need:] == 0xAB).all()
    public = device_result(x)
    for got, name in zip(whole, TABLES):                                     # and the public function gives these bytes
        assert same_bits(got, getattr(public, name))
    with pytest.raises(ValueError, match="extrema: the workspace has"):
        lib.extrema_planes(fields, rows, True, False, 4096, workspace=ws_buf[:need - 8])


def test_truncation():
    x = seven()
    host = extrema(batch_of(np.array(x), lat_of(33), full_lon(70)), 1234.5, max_points=3)
    count = host.count["x"].numpy()
    assert count[0] > 3 and host.truncated["x"][0]
    same_result(device_result(x, max_points=3), host)
    guard = 64                                                               # nothing past a short table is written
    t_buf = torch.full((guard + 7 * 3 * 2 + guard,), -7, dtype=torch.int64, device=DEV)
    out = (torch.empty((7, 33, 70), dtype=torch.int32, device=DEV), torch.empty((7, 33, 70), device=DEV),
           t_buf[guard:guard + 42].view(7, 3, 2), torch.empty((7,), dtype=torch.int32, device=DEV))
    lib.extrema_planes([carve(x)], rows_of(), True, False, 3, out=out)
    assert same_bits(out[2].cpu(), host.table_table) and same_bits(out[3].cpu(), host.count_table)
    assert (t_buf[:guard] == -7).all() and (t_buf[guard + 42:] == -7).all()


def test_capture_in_a_hip_graph():
    x = seven()
    b = on_device(batch_of(np.array(x[:3]), lat_of(33), full_lon(70)))
    other = field((3, 33, 70), 43)
    want = device_result(other, kind="max")
    extrema(b, 1234.5, kind="max")                                           # the eager call: tables uploaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = extrema(b, 1234.5, kind="max")
    b.surf_vars["x"][:, -1].copy_(torch.from_numpy(other))
    graph.replay()
    torch.cuda.synchronize()
    for name in TABLES:
        assert same_bits(getattr(out, name), getattr(want, name))
    with pytest.MonkeyPatch.context() as mp:                                 # a cold call during capture is refused
        mp.setattr(mod._fields, "tables", _fields.DeviceTables(capturing=lambda: True))
        with pytest.raises(RuntimeError, match="extrema: call once .* before capturing a graph"):
            extrema(b, 987.0)


def test_smooth_then_extrema_uploads_the_disc_table_once():
    b = on_device(batch_of(np.array(seven()[:2]), lat_of(33), full_lon(70)))
    smooth(b, 777.0)
    with pytest.MonkeyPatch.context() as mp:                                 # a hit in the table cache never packs the table
        mp.setattr(mod, "_packed", lambda table: pytest.fail("the disc table that smooth uploaded was packed and uploaded again"))
        extrema(b, 777.0)


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def test_lows_of_a_smoothed_field():
    lat, lon = lat_of(33), full_lon(70)
    x = red_noise((2, 33, 70), 44, amp=3000.0) + field((2, 33, 70), 45, mean=0.0, amp=300.0)
    b = batch_of(x.astype(np.float32), lat, lon)
    s_host, s_dev = smooth(b, 300.0), smooth(on_device(b), 300.0)
    assert same_bits(s_dev.surf_vars["x"].cpu(), s_host.surf_vars["x"])      # on this grid the smoothed planes are bit-equal
    e_host, e_dev = extrema(s_host, 500.0, kind="min"), extrema(s_dev, 500.0, kind="min")
    assert e_dev.table["x"].is_cuda and int(e_host.count["x"].min()) >= 1
    same_result(e_dev, e_host)
