"""aurora_hip_smooth (aurora_amd/csrc/smooth.hip) through `aurora_amd.smooth` on the device: against the dense haversine
yardstick of tests/smooth_reference.py within the bound derived there, against the numpy path within twice that bound, and
the bytes: repeatable, independent of the other planes of a call and of how the binding divides them, replayed from a graph,
with the NaN footprint of the numpy path and nothing written outside the outputs and the workspace."""
import functools
import importlib

import numpy as np
import pytest
import torch

from aurora_amd import Batch, _fields, objects
from aurora_amd.engine import lib
from tests import smooth_reference as ref
from tests.device_buffers import same_bits
from tests.test_smooth_host import LAT19, batch_of, field, full_lon
from tests.verification_inputs import DEV, carve, red_noise

pytestmark = pytest.mark.gpu

mod = importlib.import_module("aurora_amd.smooth")
smooth = mod.smooth


def lat_of(H, ascending=False):
    lat = np.linspace(90, -90, H) if H > 1 else np.zeros(1)
    return lat[::-1].copy() if ascending else lat


def on_device(b: Batch, offset_floats=0) -> Batch:
    return Batch({k: carve(v, offset_floats) for k, v in b.surf_vars.items()}, {}, {}, b.metadata)


def both(x, lat, lon, radius, offset_floats=0, **kw):
    """(the device's result, the numpy path's) for the planes x (n, H, W)."""
    b = batch_of(x, lat, lon)
    host = smooth(b, radius, **kw).surf_vars["x"][:, 0].numpy()
    got = smooth(on_device(b, offset_floats), radius, **kw).surf_vars["x"]
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (x.shape[0], 1, *x.shape[1:])
    return got[:, 0].cpu().numpy(), host


def check(x, lat, lon, dlam, radius, rows=None, offset_floats=0, **kw):
    dev, host = both(x, lat, lon, radius, offset_floats, **kw)
    y, _, bound, margin = ref.dense(x, lat, dlam, radius, rows)
    assert margin > 1e-6, f"a point pair lies {margin} km from the radius"
    sel = slice(None) if rows is None else rows
    d, h = dev[:, sel], host[:, sel]
    assert np.array_equal(np.isnan(dev), np.isnan(host)), "the NaN footprint differs from the numpy path's"
    ok = np.isfinite(y) & np.isfinite(d)
    allowed = ref.allowed(y, bound)
    err_y, err_h = np.abs(d - y)[ok], np.abs(d - h)[ok]
    if not ok.any():                                                         # (two rows are two poles: no weight anywhere)
        assert np.isnan(y).all()
        return dev
    print(f"{x.shape} radius {radius}: margin {margin:.3g} km; device - yardstick up to {err_y.max():.3g} "
          f"({(err_y / allowed[ok]).max():.3g} of allowed); device - numpy up to {err_h.max():.3g}; fp64 bound up to {bound[ok].max():.3g}")
    assert np.all(err_y <= allowed[ok]) and np.all(err_h <= 2.0 * allowed[ok])
    if kw.get("min_valid") == 0.0 and not kw.get("keep_mask", True):
        assert np.array_equal(np.isnan(d), np.isnan(y))
    return dev


# ---- agreement -------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 2), (5, 3), (9, 63), (16, 64), (17, 65), (33, 255), (40, 256), (7, 257)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_widths_against_yardstick_and_numpy(H, W):
    x = field((3, H, W), 10 + W)
    if H * W > 6:
        g = np.random.default_rng(W)
        x[1][g.random((H, W)) < 0.1] = np.nan
        x[2, H // 2, W // 2] = np.inf
    lon = full_lon(W) if W > 1 else np.array([12.0])
    dlam = 2 * np.pi / W if W > 1 else 0.0
    check(x, lat_of(H), lon, dlam, 1234.5, min_valid=0.0, keep_mask=False)
    if W in (64, 256):
        check(x, lat_of(H), lon, dlam, 1234.5, offset_floats=1)          # the four-byte loads of the same values


def test_every_height():
    for H in range(1, 41):
        x = field((2, H, 24), 100 + H)
        check(x, lat_of(H), full_lon(24), 2 * np.pi / 24, 1500.0, offset_floats=H % 2, min_valid=0.0, keep_mask=False)


@pytest.mark.parametrize("what", ["regional", "ascending", "polar disc covers the circle"])
def test_grids(what):
    if what == "regional":
        lat, W = np.linspace(60, 20, 17), 39
        x = field((2, 17, W), 21)
        x[1, 4, 0] = np.nan
        for min_valid in (0.0, 0.5, 1.0):
            check(x, lat, 10.0 + 2.5 * np.arange(W), np.deg2rad(2.5), 700.0, min_valid=min_valid)
    elif what == "ascending":
        check(field((2, 19, 40), 22), LAT19[::-1].copy(), full_lon(40), 2 * np.pi / 40, 1234.5)
    else:
        check(field((2, 19, 40), 23), LAT19, full_lon(40), 2 * np.pi / 40, 2500.0, min_valid=1.0)


def test_one_degree_grid_at_500_km():
    x = red_noise((1, 181, 360), 31)
    x[0, 60:64, 100:130] = np.nan
    check(x, lat_of(181), full_lon(360), 2 * np.pi / 360, 500.0)


def test_quarter_degree_plane_at_100_km():
    x = red_noise((1, 721, 1440), 32)                                       # six prefix chunks a row: the carry
    rows = np.array([0, 1, 2, 5, 50, 180, 360, 361, 540, 700, 719, 720])    # the yardstick is dense in these target rows
    check(x, lat_of(721), full_lon(1440), 2 * np.pi / 1440, 100.0, rows=rows)


# ---- bytes and placement -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seven():
    """Seven 33 x 70 planes with NaN and infinities scattered, a NaN row and an all-NaN plane; shared, never modified."""
    x = field((7, 33, 70), 40)
    g = np.random.default_rng(41)
    x[1][g.random((33, 70)) < 0.3] = np.nan
    x[2, 5, 6], x[2, 20, 69] = np.inf, -np.inf
    x[3, 16] = np.nan
    x[4] = np.nan
    return x


def device_result(x, **kw):
    return smooth(on_device(batch_of(x, lat_of(33), full_lon(70))), 1234.5, **kw).surf_vars["x"][:, 0]


def test_same_bytes_twice_and_wherever_a_plane_sits():
    x = seven()
    a, b = device_result(x), device_result(x)
    assert same_bits(a, b)
    last = x[6:7]
    alone = device_result(last)
    among = device_result(np.concatenate([x[0:1], last, x[3:4]]))
    assert same_bits(alone[0], among[1]) and same_bits(alone[0], a[6])
    unaligned = smooth(on_device(batch_of(x, lat_of(33), full_lon(70)), 1), 1234.5).surf_vars["x"][:, 0]
    assert same_bits(unaligned, a)                                           # the quad rule: the same association either way


@pytest.mark.parametrize("keep_mask", [True, False])
def test_nan_footprint_is_the_numpy_path_s(keep_mask):
    x = seven()
    for min_valid in (0.0, 0.5, 1.0):
        host = smooth(batch_of(x, lat_of(33), full_lon(70)), 1234.5, min_valid=min_valid, keep_mask=keep_mask).surf_vars["x"][:, 0].numpy()
        dev = device_result(x, min_valid=min_valid, keep_mask=keep_mask).cpu().numpy()
        assert np.array_equal(np.isnan(dev), np.isnan(host))
        if keep_mask:
            assert np.isnan(dev[~np.isfinite(x)]).all()


def tables(dev=DEV):
    lat = lat_of(33)
    table = mod.disc_table(lat, 2 * np.pi / 70, 70, True, 1234.5)
    return torch.from_numpy(mod._packed(table)).to(dev), torch.from_numpy(table[3]).to(dev)


def test_small_workspace_cap_and_guards():
    x = seven()
    rows, w = tables()
    fields = [carve(x)]
    whole = lib.smooth_planes(fields, rows, w, True)
    assert whole.shape == (7, 33, 70)
    one = lib.smooth_workspace_bytes(1, 33, 70)
    assert one == (33 * 71 * 12 + 7) // 8 * 8 and lib.smooth_workspace_bytes(7, 33, 70) == (7 * 33 * 71 * 12 + 7) // 8 * 8
    # outputs and workspace inside NaN / 0xAB guards; two planes in flight: four chunks
    guard, n_out = 512, 7 * 33 * 70
    out_buf = torch.full((guard + n_out + guard,), float("nan"), device=DEV)
    ws_buf = torch.full((guard + 2 * one + guard,), 0xAB, dtype=torch.uint8, device=DEV)
    out = out_buf[guard:guard + n_out].view(7, 33, 70)
    lib.smooth_planes(fields, rows, w, True, out=out, workspace=ws_buf[guard:guard + 2 * one])
    assert same_bits(out, whole)
    assert torch.isnan(out_buf[:guard]).all() and torch.isnan(out_buf[guard + n_out:]).all()
    assert (ws_buf[:guard] == 0xAB).all() and (ws_buf[guard + 2 * one:] == 0xAB).all()
    capped = lib.smooth_planes(fields, rows, w, True, workspace_cap=1)       # a plane at a time: seven chunks
    assert same_bits(capped, whole)
    assert same_bits(whole, device_result(x))                             # and the public function gives these bytes
    with pytest.raises(AssertionError, match="smooth_planes: the workspace has"):
        lib.smooth_planes(fields, rows, w, True, workspace=ws_buf[:one - 8])


def test_capture_in_a_hip_graph():
    x = seven()
    b = on_device(batch_of(x[:3], lat_of(33), full_lon(70)))
    other = field((3, 33, 70), 43)
    want = device_result(other)
    smooth(b, 1234.5)                                                        # the eager call: tables uploaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = smooth(b, 1234.5)
    b.surf_vars["x"][:, -1].copy_(torch.from_numpy(other))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out.surf_vars["x"][:, 0], want)
    with pytest.MonkeyPatch.context() as mp:                                 # a cold call during capture is refused
        mp.setattr(mod._fields, "tables", _fields.DeviceTables(capturing=lambda: True))
        with pytest.raises(RuntimeError, match="smooth: call once .* before capturing a graph"):
            smooth(b, 987.0)


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def test_objects_of_a_smoothed_field():
    lat, lon = lat_of(33), full_lon(70)
    x = red_noise((2, 33, 70), 44, amp=3000.0) + field((2, 33, 70), 45, mean=0.0, amp=300.0)
    b = batch_of(x.astype(np.float32), lat, lon)
    host = smooth(b, 1234.5)
    dev = smooth(on_device(b), 1234.5)
    s = host.surf_vars["x"][:, 0].numpy()
    thr = float(np.quantile(s[np.isfinite(s)], 0.8))
    o_host, o_dev = objects(host, {"x": [thr]}), objects(dev, {"x": [thr]})
    assert o_dev.labels["x"].is_cuda
    y, _, bound, _ = ref.dense(x.astype(np.float32), lat, 2 * np.pi / 70, 1234.5)
    excluded = ~(np.abs(s - np.float32(thr)) > 2.0 * ref.allowed(y, bound)) & np.isfinite(s)
    share = excluded.mean()
    print(f"objects(smooth): {excluded.sum()} of {excluded.size} points ({100 * share:.3g} %) lie within the bound of the threshold")
    assert share <= 0.01
    l_host, l_dev = o_host.labels["x"][:, 0].numpy(), o_dev.labels["x"][:, 0].cpu().numpy()
    assert l_host.max() >= 1
    assert np.array_equal((l_host > 0)[~excluded], (l_dev > 0)[~excluded])
    if np.array_equal(l_host > 0, l_dev > 0):                                # the same events: the same objects and numbers
        assert np.array_equal(l_host, l_dev)
    else:                                                                    # events differ at excluded points only
        assert excluded.any()
