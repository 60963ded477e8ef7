"""`aurora_amd.extrema` on the host: the numpy path of THE RULE (aurora_amd/extrema.py) against a plain-Python brute force over
the members that `disc_table` names -- every byte of index, filtered, table and count, no tolerance anywhere -- the exact
properties (a constant plane, signed zeros, discs of one point), truncation, the finalised tensors, the refusals, and the C
entry's argument checks (no GPU needed)."""
import functools
import importlib

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, _sphere
from aurora_amd.batch import BandBatch, derive_metadata
from aurora_amd.objects import Result, value_keys
from tests.test_smooth_host import LAT19, batch_of, full_lon
from tests.verification_inputs import red_noise

mod = importlib.import_module("aurora_amd.extrema")
smooth_mod = importlib.import_module("aurora_amd.smooth")
extrema = mod.extrema

LAT33 = np.linspace(90, -90, 33)
# name -> (latitudes, longitudes, wrap, radius in km)
GRIDS = {
    "33 x 70": (LAT33, full_lon(70), True, 1234.5),
    "19 x 40": (LAT19, full_lon(40), True, 1234.5),
    "19 x 40 ascending": (LAT19[::-1].copy(), full_lon(40), True, 1234.5),
    "polar disc covers the circle": (LAT19, full_lon(40), True, 2500.0),
    "regional 17 x 39": (np.linspace(60, 20, 17), 10.0 + 2.5 * np.arange(39), False, 700.0),
}


def planes_for(H, W, seed):
    """Seven planes: red noise, with NaN scattered, with infinities, with a NaN row, all NaN, constant, and zeros of both signs."""
    x = red_noise((7, H, W), seed)
    g = np.random.default_rng(seed + 1)
    x[1][g.random((H, W)) < 0.3] = np.nan
    x[2, H // 3, W // 5], x[2, H // 2, W - 1], x[2, 0, 0] = np.inf, -np.inf, np.inf
    x[3, H // 2] = np.nan
    x[4] = np.nan
    x[5] = np.float32(287.125)
    x[6] = np.where(g.random((H, W)) < 0.1, np.float32(-0.0), np.float32(0.0))
    return x


def table_of(lat, lon, wrap, radius):
    step, wraps = _sphere.regular_grid("extrema", np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64), least=1,
                                       in_range=True)
    assert wraps == wrap
    return smooth_mod.disc_table(lat, float(np.deg2rad(step)), len(lon), wrap, radius)


def members_of(table, H, W, wrap):
    """THE RULE's MEMBERSHIP in plain Python: (i, j) -> the list of the (k, c) inside the disc."""
    row_lo, row_count, half, _ = table
    out = {}
    for i in range(H):
        for j in range(W):
            inside = set()
            for r in range(int(row_count[i])):
                k, n = int(row_lo[i]) + r, int(half[i, r])
                if k == i:
                    n = max(n, 0)
                for d in range(-n, n + 1):
                    c = j + d
                    if wrap:
                        inside.add((k, c % W))
                    elif 0 <= c < W:
                        inside.add((k, c))
            out[i, j] = sorted(inside)
    return out


def key_of(bits: int) -> int:
    return (~bits & 0xffffffff) if bits & 0x80000000 else (bits | 0x80000000)


def brute(x, members, is_max, max_points):
    """(index, filtered, table, count) of one plane, a loop over every member of every disc."""
    H, W = x.shape
    bits = x.view(np.uint32)
    finite = np.isfinite(x)
    index = np.full((H, W), -1, dtype=np.int32)
    filtered = np.full((H, W), np.float32("nan"), dtype=np.float32)
    for (i, j), inside in members.items():
        best = None
        for k, c in inside:
            if not finite[k, c]:
                continue
            key = key_of(int(bits[k, c]))
            comp = ((key ^ 0xffffffff if is_max else key) << 32) | (k * W + c)
            best = comp if best is None or comp < best else best
        if best is not None:
            index[i, j] = best & 0xffffffff
            filtered[i, j] = x.reshape(-1)[best & 0xffffffff]
    own = [p for p in range(H * W) if index.reshape(-1)[p] == p]
    table = np.zeros((max_points, 2), dtype=np.int64)
    for row, p in enumerate(own[:max_points]):
        table[row] = p, key_of(int(bits.reshape(-1)[p]))
    return index, filtered, table, len(own)


@functools.lru_cache(maxsize=None)
def case(name):
    """(planes, lat, lon, wrap, radius, members) of a grid of GRIDS; shared, never modified."""
    lat, lon, wrap, radius = GRIDS[name]
    H, W = len(lat), len(lon)
    x = planes_for(H, W, 7 * H + W)
    x.setflags(write=False)
    return x, lat, lon, wrap, radius, members_of(table_of(lat, lon, wrap, radius), H, W, wrap)


def run(x, lat, lon, radius, **kw):
    return extrema(batch_of(np.array(x), lat, lon), radius, **kw)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the brute force ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["min", "max"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_numpy_path_equals_the_brute_force(name, kind):
    x, lat, lon, wrap, radius, members = case(name)
    H, W = x.shape[-2:]
    e = run(x, lat, lon, radius, kind=kind, max_points=H * W)
    index, filtered, table, count = (e.index["x"].numpy(), e.filtered["x"].numpy(), e.table["x"].numpy(), e.count["x"].numpy())
    assert index.dtype == np.int32 and filtered.dtype == np.float32 and table.dtype == np.int64 and count.dtype == np.int32
    assert e.wrap == wrap
    for p in range(x.shape[0]):
        want = brute(x[p], members, kind == "max", H * W)
        assert same(index[p], want[0]), f"plane {p}: index"
        assert same(filtered[p], want[1]), f"plane {p}: filtered bits"
        assert same(table[p], want[2]) and count[p] == want[3], f"plane {p}: table and count"
        # the minimum / maximum filter over the valid members
        clean = np.where(np.isfinite(x[p]), x[p], np.float32("nan"))
        fold = np.nanmax if kind == "max" else np.nanmin
        for (i, j), inside in members.items():
            v = clean[tuple(np.array(inside).T)]
            if np.isnan(v).all():
                assert index[p, i, j] == -1 and np.isnan(filtered[p, i, j])
            else:
                assert filtered[p, i, j] == fold(v) and x[p].reshape(-1)[index[p, i, j]] == filtered[p, i, j]
    assert count[4] == 0 and (index[4] == -1).all() and np.isnan(filtered[4]).all()         # the all-NaN plane
    assert count[5] == 1 and table[5, 0, 0] == 0 and not table[5, 1:].any()                  # the constant plane: flat index 0
    assert np.isfinite(filtered[3, x.shape[1] // 2]).all()                                   # a NaN row is filled from its neighbours
    zeros = filtered[6].view(np.uint32)                                                     # -0 is below +0
    minus = x[6].view(np.uint32) != 0
    has_minus = np.array([[any(minus[k, c] for k, c in members[i, j]) for j in range(W)] for i in range(H)])
    has_plus = np.array([[any(not minus[k, c] for k, c in members[i, j]) for j in range(W)] for i in range(H)])
    want_minus = ~has_plus if kind == "max" else has_minus
    assert np.array_equal(zeros != 0, want_minus) and set(np.unique(zeros)) <= {0, 0x80000000}
    assert has_minus.any() and (~has_minus).any()


def test_is_extremum_and_invalid_points():
    x, lat, lon, _, radius, _ = case("33 x 70")
    e = run(x, lat, lon, radius)
    index, is_ext = e.index["x"].numpy(), e.is_extremum["x"].numpy()
    assert is_ext.dtype == np.bool_ and is_ext.shape == x.shape
    assert np.array_equal(is_ext, index == np.arange(33 * 70).reshape(33, 70))
    assert not is_ext[~np.isfinite(x)].any()                                                 # NaN and +-Inf are never extrema
    assert np.array_equal(is_ext.reshape(7, -1).sum(axis=1), e.count["x"].numpy())
    picked = np.where(index >= 0, index, 0)
    assert np.isfinite(np.take_along_axis(x.reshape(7, -1), picked.reshape(7, -1), axis=1).reshape(x.shape)[index >= 0]).all()


# ---- exact properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["min", "max"])
def test_discs_of_one_point_return_the_input(kind):
    lat, W = np.linspace(40, -40, 17), 72                      # 5 degrees of latitude and of longitude: 556 km and more than 425 km
    x = red_noise((2, 17, W), 3)
    x[1, 4, 7], x[1, 9, 0], x[1, 2, 3] = np.nan, np.inf, -np.inf
    table = smooth_mod.disc_table(lat, 2 * np.pi / W, W, True, 100.0)
    assert table[1].max() == 1 and table[2].max() == 0
    e = run(x, lat, full_lon(W), 100.0, kind=kind, max_points=17 * W)
    valid = np.isfinite(x)
    f = e.filtered["x"].numpy()
    assert np.array_equal(f.view(np.uint32)[valid], x.view(np.uint32)[valid]) and np.isnan(f[~valid]).all()
    assert np.array_equal(e.is_extremum["x"].numpy(), valid)
    assert np.array_equal(e.count["x"].numpy(), valid.reshape(2, -1).sum(axis=1))
    assert np.array_equal(e.index["x"].numpy()[~valid], np.full((~valid).sum(), -1))


@pytest.mark.parametrize("kind", ["min", "max"])
def test_single_row_and_single_column(kind):
    row = red_noise((2, 1, 40), 7)
    row[1, 0, 5] = np.nan
    lat, lon = np.zeros(1), full_lon(40)
    e = extrema(batch_of(row, lat, lon, T=1), 1234.5, kind=kind)
    members = members_of(table_of(lat, lon, True, 1234.5), 1, 40, True)
    col = red_noise((2, 19, 1), 8)
    col[0, 3, 0] = np.inf
    e_col = extrema(batch_of(col, LAT19, [12.0]), 1234.5, kind=kind)
    assert e_col.wrap is False
    members_col = members_of(table_of(LAT19, np.array([12.0]), False, 1234.5), 19, 1, False)
    for got, x, m in ((e, row, members), (e_col, col, members_col)):
        for p in range(2):
            want = brute(x[p], m, kind == "max", 4096)
            assert same(got.index["x"][p].numpy(), want[0]) and same(got.filtered["x"][p].numpy(), want[1])
            assert same(got.table["x"][p].numpy(), want[2]) and int(got.count["x"][p]) == want[3]


def test_max_points_truncates_the_table_not_the_count():
    x, lat, lon, _, radius, _ = case("33 x 70")
    whole = run(x, lat, lon, radius, max_points=33 * 70)
    count = whole.count["x"].numpy()
    assert count[0] > 3 and count[1] > 3
    cut = run(x, lat, lon, radius, max_points=3)
    assert cut.table["x"].shape == (7, 3, 2) and cut.max_points == 3
    assert np.array_equal(cut.count["x"].numpy(), count)                                     # the true number
    assert np.array_equal(cut.truncated["x"].numpy(), count > 3) and not whole.truncated["x"].any()
    assert np.array_equal(cut.table["x"].numpy(), whole.table["x"].numpy()[:, :3])           # the first rows, zero for a short plane
    assert not cut.table["x"].numpy()[5, 1:].any() and not whole.table["x"].numpy()[0, count[0]:].any()
    assert same(cut.index["x"].numpy(), whole.index["x"].numpy())
    for name in ("value", "lat", "lon"):                                                     # finalised: the rows of the table only
        assert not torch.isnan(getattr(cut, name)["x"][0]).any() and torch.isnan(getattr(cut, name)["x"][5, 1:]).all()


def test_finalised_tensors_and_as_batch():
    from datetime import datetime

    from aurora_amd import Metadata

    md = Metadata(lat=torch.linspace(90, -90, 19, dtype=torch.float64), lon=torch.as_tensor(full_lon(40)),
                  time=(datetime(2023, 1, 1, 6),) * 2, atmos_levels=(500, 850))
    g = torch.Generator().manual_seed(0)
    b = Batch({"2t": torch.randn(2, 2, 19, 40, generator=g), "msl": torch.randn(2, 2, 19, 40, generator=g, dtype=torch.float64)},
              {"lsm": torch.randn(19, 40, generator=g)}, {"z": torch.randn(2, 2, 2, 19, 40, generator=g)}, md)
    e = extrema(b, 1234.5, kind="max", max_points=256)
    assert isinstance(e, aurora_amd.Extrema) and isinstance(e, Result) and e.kind == "max" and e.radius_km == 1234.5
    assert list(e.index) == ["2t", "msl", "z"]
    assert e.index["2t"].shape == (2, 19, 40) and e.filtered["z"].shape == (2, 2, 19, 40) and e.is_extremum["z"].shape == (2, 2, 19, 40)
    assert e.table["msl"].shape == (2, 256, 2) and e.table["z"].shape == (2, 2, 256, 2) and e.count["z"].shape == (2, 2)
    assert e.count["z"].dtype == torch.int32 and e.truncated["z"].dtype == torch.bool
    # the finalised tensors, from the table and the coordinates
    z = b.atmos_vars["z"][:, -1].numpy()
    for name in ("value", "lat", "lon", "row", "col"):
        assert getattr(e, name)["z"].shape == (2, 2, 256)
    n = int(e.count["z"][1, 0])
    assert 1 <= n < 256
    at = e.table["z"][1, 0, :n, 0].numpy()
    assert np.array_equal(at, np.flatnonzero(e.is_extremum["z"][1, 0].numpy()))
    assert np.array_equal(e.table["z"][1, 0, :n, 1].numpy(), value_keys(z[1, 0].reshape(-1)[at], False).astype(np.int64))
    assert e.value["z"].dtype == torch.float32 and e.row["z"].dtype == torch.int64 and e.lat["z"].dtype == torch.float64
    assert np.array_equal(e.value["z"][1, 0, :n].numpy().view(np.uint32), z[1, 0].reshape(-1)[at].view(np.uint32))
    assert np.array_equal(e.row["z"][1, 0, :n].numpy(), at // 40) and np.array_equal(e.col["z"][1, 0, :n].numpy(), at % 40)
    assert np.array_equal(e.lat["z"][1, 0, :n].numpy(), md.lat.numpy()[at // 40])
    assert np.array_equal(e.lon["z"][1, 0, :n].numpy(), md.lon.numpy()[at % 40])
    assert torch.isnan(e.value["z"][1, 0, n:]).all() and (e.row["z"][1, 0, n:] == -1).all() and (e.col["z"][1, 0, n:] == -1).all()
    assert torch.isnan(e.lat["z"][1, 0, n:]).all() and torch.isnan(e.lon["z"][1, 0, n:]).all()
    # msl is float64: rounded to float32 once
    msl = b.surf_vars["msl"][:, -1].numpy().astype(np.float32)
    picked = e.index["msl"].numpy().reshape(2, -1)
    assert np.array_equal(e.filtered["msl"].numpy().reshape(2, -1), np.take_along_axis(msl.reshape(2, -1), picked, axis=1))
    # as_batch: the layout of `smooth`
    out = e.as_batch()
    assert list(out.surf_vars) == ["2t", "msl"] and list(out.atmos_vars) == ["z"] and out.metadata is md
    assert out.surf_vars["2t"].shape == (2, 1, 19, 40) and out.atmos_vars["z"].shape == (2, 1, 2, 19, 40)
    assert all(v.dtype == torch.float32 for v in (*out.surf_vars.values(), *out.atmos_vars.values()))
    assert out.static_vars["lsm"] is b.static_vars["lsm"]
    assert torch.equal(out.atmos_vars["z"][:, 0], e.filtered["z"])
    assert aurora_amd.objects(out, {"z": [0.5]}).count["z"].shape == (2, 2, 1)               # the chain takes it
    only = extrema(b, 1234.5, kind="max", only=["z"], max_points=256)
    assert list(only.index) == ["z"] and torch.equal(only.table["z"], e.table["z"]) and not only.as_batch().surf_vars
    alone = extrema(Batch({}, {}, {"z": b.atmos_vars["z"][1:, :, 1:]}, md), 1234.5, kind="max", max_points=256)
    assert torch.equal(alone.index["z"], e.index["z"][1:, 1:])     # a plane does not depend on its neighbours in the call
    host = e.cpu()
    assert isinstance(host, aurora_amd.Extrema) and torch.equal(host.table["z"], e.table["z"]) and host.kind == "max"


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    x = red_noise((1, 19, 40), 9)
    b = batch_of(x, LAT19, full_lon(40))
    for radius in (0.0, -5.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="extrema: radius_km must be a finite number above 0"):
            extrema(b, radius)
    for kind in ("low", "MIN", None, 0):
        with pytest.raises(ValueError, match="extrema: kind must be 'min' or 'max'"):
            extrema(b, 300.0, kind=kind)
    for max_points in (0, -1, 65537, 2.5, None, True):
        with pytest.raises(ValueError, match=r"extrema: max_points must be a whole number in 1\.\.65536"):
            extrema(b, 300.0, max_points=max_points)
    assert extrema(b, 300.0, max_points=65536).table["x"].shape == (1, 65536, 2)
    with pytest.raises(TypeError, match="extrema: batch must be a Batch, got dict"):
        extrema({}, 300.0)
    with pytest.raises(ValueError, match="extrema: only names the variable 'y'"):
        extrema(b, 300.0, only=["y"])
    band = BandBatch(b.surf_vars, {}, {}, b.metadata, full_patch_rows=4, band=(0, 4))
    with pytest.raises(ValueError, match=r"extrema: batch is a latitude band \(BandBatch\)"):
        extrema(band, 300.0)
    md = b.metadata
    matrix = Batch(b.surf_vars, {}, {}, derive_metadata(md, lat=md.lat[:, None].expand(19, 40), lon=md.lon[None].expand(19, 40)))
    with pytest.raises(ValueError, match="extrema: batch has matrices for latitudes / longitudes"):
        extrema(matrix, 300.0)
    mixed = Batch({"x": b.surf_vars["x"], "y": torch.empty(1, 2, 19, 40, device="meta")}, {}, {}, md)
    with pytest.raises(ValueError, match=r"extrema: the fields are on \['cpu', 'meta'\]; move the batch to the CPU or to one GPU first"):
        extrema(mixed, 300.0)
    with pytest.raises(ValueError, match="extrema: the latitudes must be strictly monotonic"):
        extrema(batch_of(x, np.r_[LAT19[:-1], LAT19[-2]], full_lon(40)), 300.0)
    with pytest.raises(ValueError, match=r"extrema: batch.surf_vars\['x'\] has shape"):
        extrema(batch_of(x[:, :18], LAT19, full_lon(40)), 300.0)


def test_too_many_rows_and_too_many_longitudes():
    lat = np.linspace(89.875, -89.875, 720)
    b = batch_of(np.zeros((1, 720, 4), dtype=np.float32), lat, full_lon(4))
    with pytest.raises(ValueError, match=r"smooth: a radius of 4000 km spans \d+ latitude rows of this grid; at most 255"):
        extrema(b, 4000.0)                                      # the refusal of `disc_table`, unchanged
    wide = batch_of(np.zeros((1, 2, 4097), dtype=np.float32), [1.0, -1.0], 0.01 * np.arange(4097))
    with pytest.raises(ValueError, match="extrema: the grid has 4097 longitudes; 1 to 4096 are supported"):
        extrema(wide, 300.0)
    edge = extrema(batch_of(np.zeros((1, 2, 4096), dtype=np.float32), [1.0, -1.0], 0.01 * np.arange(4096)), 300.0)
    assert edge.index["x"].shape == (1, 2, 4096) and int(edge.count["x"]) == 1


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_the_c_entry_point_refuses_before_any_launch():
    from aurora_amd.engine import lib

    raw, header = lib.load(), (lib.library_path().parents[2] / "include" / "aurora_hip.h").read_text()
    for name in ("aurora_hip_extrema", "aurora_hip_extrema_workspace_bytes"):
        assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    assert "extrema.hip" in importlib.import_module("aurora_amd.build").SOURCES
    assert aurora_amd.extrema is mod.extrema and aurora_amd.Extrema is mod.Extrema
    assert "extrema" in aurora_amd.__all__ and "Extrema" in aurora_amd.__all__
    # the workspace: 16 bytes per row of every plane -- not plane-sized
    need = raw.aurora_hip_extrema_workspace_bytes(3, 9, 12)
    assert need == 16 * 3 * 9 and raw.aurora_hip_extrema_workspace_bytes(1, 1, 2) == 16
    assert raw.aurora_hip_extrema_workspace_bytes(69, 721, 1440) == 16 * 69 * 721 == lib.extrema_workspace_bytes(69, 721, 1440)
    assert raw.aurora_hip_extrema_workspace_bytes(2, 5, 4096) == 160 and raw.aurora_hip_extrema_workspace_bytes(2, 5, 4097) == 0
    assert raw.aurora_hip_extrema_workspace_bytes(0, 9, 12) == 0 and raw.aurora_hip_extrema_workspace_bytes(1, 600000, 4096) == 0
    err = lambda: raw.aurora_hip_last_error()  # noqa: E731
    args = lambda **kw: tuple({**dict(planes=16, index=16, filtered=16, table=16, count=16, n_planes=3, n_lat=9, n_lon=12,  # noqa: E731
                                     row_lo=16, row_count=16, half=16, max_rows=3, wrap=1, is_max=0, max_points=64, ws=16,
                                     ws_size=need, stream=None), **kw}.values())
    for kw, text in ((dict(ws_size=need - 8), b"workspace"), (dict(max_rows=256), b"255 source rows"), (dict(max_rows=0), b"source rows"),
                     (dict(wrap=2), b"flags"), (dict(is_max=-1), b"flags"), (dict(max_points=0), b"max_points"),
                     (dict(max_points=65537), b"max_points"), (dict(n_lon=4097), b"4097 longitudes; 1 to 4096 are supported"),
                     (dict(n_lat=600000, n_lon=4096), b"too large"), (dict(half=None), b"null"), (dict(index=None), b"null"),
                     (dict(count=None), b"null"), (dict(filtered=18), b"aligned"), (dict(table=20), b"aligned"), (dict(ws=20), b"aligned"),
                     (dict(n_lon=0), b"bad sizes"), (dict(n_planes=-1), b"bad sizes")):
        assert raw.aurora_hip_extrema(*args(**kw)) == -1 and text in err(), (kw, err())
    assert raw.aurora_hip_extrema(*args(n_planes=0)) == 0
