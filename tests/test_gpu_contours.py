"""aurora_hip_closed_contours (aurora_amd/csrc/contours.hip) through `aurora_amd.closed_contours` on the device: every byte of the
table equals the numpy path's (which tests/test_contours_host.py holds to a brute force) and the finalised tensors have the same
bits -- no tolerance anywhere -- at every width at which a window gains a word or becomes the whole circle, at every height, on
regional, ascending and polar grids and on the hand-drawn planes; the bytes are repeatable, independent of the other planes of a
call and of plane alignment, replayed from a graph, and nothing is written outside the output."""
import functools
import importlib

import numpy as np
import pytest
import torch

from aurora_amd import Batch, _fields, smooth
from aurora_amd.engine import lib
from tests.device_buffers import same_bits
from tests.test_contours_host import DELTA, HAND, check_hand, hand_grid
from tests.test_extrema_host import GRIDS, planes_for
from tests.test_gpu_extrema import lat_of, on_device, scattered
from tests.test_smooth_host import batch_of, field, full_lon
from tests.verification_inputs import DEV, carve, red_noise

pytestmark = pytest.mark.gpu

mod = importlib.import_module("aurora_amd.contours")
extrema_mod = importlib.import_module("aurora_amd.extrema")
smooth_mod = importlib.import_module("aurora_amd.smooth")
extrema, closed_contours = extrema_mod.extrema, mod.closed_contours
FINAL = ("points", "exits", "depth", "count_closed", "value", "lat", "lon", "row", "col")
EIGHT = [20.0, 60.0, 150.0, 400.0, 800.0, 1500.0, 4000.0, 1e6]


def same_result(dev, host) -> None:
    """The table of a device result (moved to the host) has the bytes of the numpy path's, the finalised tensors the same bits."""
    assert dev.table_table.is_cuda and not host.table_table.is_cuda and dev.table_table.dtype == torch.int32
    assert same_bits(dev.table_table.cpu(), host.table_table), "the table differs from the numpy path's"
    for name in FINAL:
        for k, h in getattr(host, name).items():
            assert same_bits(getattr(dev, name)[k].cpu(), h), f"{name} differs from the numpy path's"
    for k, h in host.closed.items():
        assert torch.equal(dev.closed[k].cpu(), h)


def check(x, lat, lon, radius_e, delta, radius_c, offset_floats=0, connectivity=8, **kw):
    """The device's result for the planes x (n, H, W), after it was held to the numpy path's; and the host's."""
    b = batch_of(np.array(x), lat, lon)
    e_host = extrema(b, radius_e, **kw)
    e_dev = extrema(on_device(b, offset_floats), radius_e, **kw)
    assert same_bits(e_dev.table_table.cpu(), e_host.table_table)
    host = closed_contours(e_host, delta, radius_c, connectivity=connectivity)
    dev = closed_contours(e_dev, delta, radius_c, connectivity=connectivity)
    same_result(dev, host)
    return dev, host


# ---- shapes and heights -----------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 2), (5, 3), (9, 63), (16, 64), (17, 65), (7, 127), (7, 128), (7, 129), (33, 255), (40, 256), (7, 257)]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("kind", ["min", "max"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_against_numpy(H, W, kind, connectivity):
    x = scattered((H, W), 10 + W)
    lon = full_lon(W) if W > 1 else np.array([12.0])
    # 2300 km: the windows of the first and last rows are the whole circle, those at the equator narrow
    table = smooth_mod.disc_table(lat_of(H), 2 * np.pi / W, W, W > 1, 2300.0)
    if H >= 7 and W >= 63:
        words = mod.window_words(table, W, True)
        assert words[0] == (W + 63) // 64 and 2 * mod._widest(table)[H // 2] + 3 < W
    for delta in ([250.0], EIGHT):
        check(x, lat_of(H), lon, 1234.5, delta, 2300.0, kind=kind, connectivity=connectivity, max_points=128)
    if W in (64, 256):
        check(x, lat_of(H), lon, 1234.5, EIGHT, 2300.0, offset_floats=1, kind=kind, connectivity=connectivity, max_points=128)


def test_every_height():
    for H in range(1, 41):
        check(scattered((H, 24), 100 + H), lat_of(H), full_lon(24), 1500.0, [100.0, 600.0], 2500.0, offset_floats=H % 2,
              kind=("min", "max")[H % 2], connectivity=(4, 8)[H // 2 % 2], max_points=64)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(HAND))
def test_hand_drawn_planes_through_the_device(name, connectivity):
    x, regional, at, _ = HAND[name]
    lat, lon, radius = hand_grid(regional)
    dev, host = check(x[None], lat, lon, radius, [DELTA], radius, connectivity=connectivity, max_points=256)
    check_hand(name, connectivity, dev.cpu(), extrema(batch_of(x[None], lat, lon), radius, max_points=256))


def test_constant_plane_whose_disc_is_the_whole_grid():
    x = np.full((1, 24, 48), 287.125, dtype=np.float32)
    dev, _ = check(x, np.linspace(85.0, -87.5, 24), full_lon(48), 19800.0, [0.5, 3.0], 19800.0)
    assert dev.table["x"][0, :, 0].tolist() == [[24 * 48, 0]] * 2


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("kind", ["min", "max"])
@pytest.mark.parametrize("name", ["regional 17 x 39", "19 x 40 ascending", "polar disc covers the circle"])
def test_grids(name, kind, connectivity):
    lat, lon, wrap, radius = GRIDS[name]
    dev, _ = check(planes_for(len(lat), len(lon), 21), lat, lon, radius * 0.6, [40.0, 250.0, 1500.0], radius, kind=kind,
                   connectivity=connectivity, max_points=len(lat) * len(lon))
    assert dev.wrap == wrap and not dev.table["x"][4].any()                 # the all-NaN plane


# ---- large planes -------------------------------------------------------------------------------------------------------------
def test_one_degree_pair_at_500_km():
    # (the seed and the deltas were chosen on the CPU with the numpy path: both outcomes occur among the candidates)
    x = red_noise((2, 181, 360), 31, amp=3000.0) + field((2, 181, 360), 45, mean=0.0, amp=30.0)
    x = x.astype(np.float32)
    x[0, 60:64, 100:130] = np.nan
    dev, host = check(x, lat_of(181), full_lon(360), 500.0, [60.0, 100.0, 150.0], 500.0, kind="min", max_points=1024)
    live = torch.arange(1024) < host.count["x"][:, None]
    closed = host.closed["x"]
    assert int(live.sum()) >= 20
    for t in range(3):                                                      # a condition on the input, not a tolerance
        assert bool(closed[:, t].any()) and bool((~closed[:, t] & live).any()), f"delta {t}: one outcome only"


def test_quarter_degree_plane_at_300_km():
    x = red_noise((1, 721, 1440), 32)                                       # whole-circle windows of 23 words near the poles
    x[0, 300:303, 700:760], x[0, 0, 5], x[0, 720, :] = np.nan, np.inf, np.nan
    x[0, 400:420, 200:230] = np.nan                                         # NaN blocks: open water for the fill
    dev, host = check(x, lat_of(721), full_lon(1440), 300.0, [100.0, 400.0], 300.0, kind="min", max_points=512)
    assert int(host.count["x"]) >= 100 and bool(host.closed["x"].any()) and not bool(host.closed["x"].all())


# ---- bytes and placement -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seven():
    """The seven 33 x 70 planes of the host tests (NaN, infinities, a NaN row, all NaN, constant, signed zeros); never modified."""
    return planes_for(33, 70, 40)


def device_result(x, offset_floats=0, delta=(40.0, 250.0, 1500.0), radius=2000.0, **kw):
    e = extrema(on_device(batch_of(np.array(x), lat_of(33), full_lon(70)), offset_floats), 1234.5, max_points=256)
    return closed_contours(e, list(delta), radius, **kw)


def test_same_bytes_twice_and_wherever_a_plane_sits():
    x = seven()
    a, b = device_result(x), device_result(x)
    assert same_bits(a.table_table, b.table_table) and bool(a.table_table.any())
    last = x[6:7]
    alone = device_result(last)
    among = device_result(np.concatenate([x[0:1], last, x[3:4]]))
    unaligned = device_result(x, 1)
    assert same_bits(alone.table_table[0], among.table_table[1]) and same_bits(alone.table_table[0], a.table_table[6])
    assert same_bits(unaligned.table_table, a.table_table)


def rows_of(radius=2000.0):
    table = smooth_mod.disc_table(lat_of(33), float(np.deg2rad(360.0 / 70)), 70, True, radius)
    return torch.from_numpy(smooth_mod._packed(table)).to(DEV), int(mod.window_words(table, 70, True).max())


def test_guards_around_the_output():
    x = seven()
    fields = [carve(x)]
    e = extrema(on_device(batch_of(np.array(x), lat_of(33), full_lon(70))), 1234.5, max_points=256)
    rows, max_words = rows_of()
    deltas = torch.tensor([[40.0, 250.0, float("nan")]] * 7, device=DEV)
    whole = lib.closed_contours_planes(fields, e.table_table, e.count_table, deltas, rows, max_words, True, False, 8)
    assert tuple(whole.shape) == (7, 3, 256, 2) and whole.dtype == torch.int32
    assert not whole[:, 2].any() and bool(whole[:, :2].any())               # the padded delta: zero rows
    guard, n = 512, 7 * 3 * 256 * 2
    buf = torch.full((guard + n + guard,), -7, dtype=torch.int32, device=DEV)
    out = buf[guard:guard + n].view(7, 3, 256, 2)
    lib.closed_contours_planes(fields, e.table_table, e.count_table, deltas, rows, max_words, True, False, 8, out=out)
    assert same_bits(out, whole) and (buf[:guard] == -7).all() and (buf[guard + n:] == -7).all()
    public = device_result(x, delta=(40.0, 250.0))
    assert same_bits(public.table_table, whole[:, :2].contiguous())          # and the public function gives these bytes
    # the binding's own checks, and the library's refusal of an over-budget window before any launch
    with pytest.raises(AssertionError, match="closed_contours_planes: 7 planes but deltas for 6"):
        lib.closed_contours_planes(fields, e.table_table, e.count_table, deltas[:6].contiguous(), rows, max_words, True)
    with pytest.raises(AssertionError, match="closed_contours_planes: table has shape"):
        lib.closed_contours_planes(fields, e.table_table[:6].contiguous(), e.count_table, deltas, rows, max_words, True)
    before = out.clone()
    with pytest.raises(ValueError, match="closed_contours: connectivity must be 4 or 8, got 6"):
        lib.closed_contours_planes(fields, e.table_table, e.count_table, deltas, rows, max_words, True, False, 6, out=out)
    with pytest.raises(ValueError, match=r"closed_contours: windows of \d+ rows x 65 words of 64 columns need \d+ bytes of LDS"):
        lib.closed_contours_planes(fields, e.table_table, e.count_table, deltas, rows.repeat(16)[:33 * 130].contiguous(), 65, True,
                                   out=out)
    torch.cuda.synchronize()
    assert same_bits(out, before)


def test_capture_in_a_hip_graph():
    x = seven()
    b = on_device(batch_of(np.array(x[:3]), lat_of(33), full_lon(70)))
    other = red_noise((3, 33, 70), 43)
    e = extrema(b, 1234.5, max_points=256)
    closed_contours(e, [40.0, 250.0], 2000.0)                               # the eager call: tables uploaded, the LDS limit raised
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e_out = extrema(b, 1234.5, max_points=256)
        out = closed_contours(e_out, [40.0, 250.0], 2000.0)
    b.surf_vars["x"][:, -1].copy_(torch.from_numpy(other))
    graph.replay()
    torch.cuda.synchronize()
    want = device_result(other, delta=(40.0, 250.0))
    assert same_bits(out.table_table, want.table_table) and bool(out.table_table.any())
    with pytest.MonkeyPatch.context() as mp:                                 # a cold call during capture is refused
        mp.setattr(mod._fields, "tables", _fields.DeviceTables(capturing=lambda: True))
        with pytest.raises(RuntimeError, match="closed_contours: call once .* before capturing a graph"):
            closed_contours(e, [40.0, 250.0], 987.0)


def test_smooth_then_contours_uploads_the_disc_table_once():
    b = on_device(batch_of(np.array(seven()[:2]), lat_of(33), full_lon(70)))
    e = extrema(smooth(b, 777.0), 1234.5)
    with pytest.MonkeyPatch.context() as mp:                                 # a hit in the table cache never packs the table
        mp.setattr(mod, "_packed", lambda table: pytest.fail("the disc table that smooth uploaded was packed and uploaded again"))
        closed_contours(e, [100.0], 777.0)


def test_mixed_devices_are_refused():
    b = batch_of(np.array(seven()[:1]), lat_of(33), full_lon(70))
    e = extrema(on_device(b), 1234.5)
    with pytest.raises(ValueError, match="closed_contours: the tables of e and the fields of e.source are on"):
        closed_contours(e.cpu(), [100.0], 2000.0)
