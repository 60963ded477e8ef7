"""`aurora_amd.smooth` on the host: the numpy path of THE RULE (aurora_amd/smooth.py) against the dense haversine yardstick of
tests/smooth_reference.py within the bound derived there, the disc table against a brute force of its own, the exact
properties, validity and coverage, the refusals, and the C entry's argument checks (no GPU needed)."""
import importlib
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata
from aurora_amd.batch import BandBatch, derive_metadata
from tests import smooth_reference as ref

mod = importlib.import_module("aurora_amd.smooth")
smooth = mod.smooth

LAT19 = np.linspace(90, -90, 19)
RADII = (300.0, 1234.5, 2500.0)            # margins to the nearest point pair on the 19 x 40 grid: 42, 14.3 and 9.5 km


def full_lon(W):
    return np.arange(W) * (360.0 / W)


def batch_of(x, lat, lon, name="x", T=2):
    """One surface variable `name` whose last history entry is x (B, H, W); the entry before is garbage that must not be read."""
    x = torch.as_tensor(np.asarray(x))
    hist = torch.stack([torch.full_like(x, 7e9)] * (T - 1) + [x], dim=1)
    lat, lon = torch.as_tensor(np.asarray(lat, dtype=np.float64)), torch.as_tensor(np.asarray(lon, dtype=np.float64))
    md = Metadata(lat=torch.linspace(1, -1, len(lat), dtype=torch.float64), lon=torch.linspace(0, 1, len(lon), dtype=torch.float64),
                  time=tuple(datetime(2023, 1, 1, 6) for _ in range(x.shape[0])), atmos_levels=())
    md = derive_metadata(md, lat=lat, lon=lon)                   # (the constructor takes descending latitudes only)
    return Batch({name: hist}, {"lsm": torch.zeros(x.shape[-2:])}, {}, md)


def field(shape, seed, mean=1e5, amp=1e3):
    return (mean + amp * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def run(x, lat, lon, radius, **kw):
    return smooth(batch_of(x, lat, lon), radius, **kw).surf_vars["x"][:, 0].numpy()


def check_against_yardstick(out, x, lat, dlam, radius, rows=None, factor=1.0):
    y, den, bound, margin = ref.dense(x, lat, dlam, radius, rows)
    assert margin > 1e-6, f"a point pair lies {margin} km from the radius: the yardstick and the table may disagree"
    got = out if rows is None else out[:, rows]
    assert np.array_equal(np.isnan(got), np.isnan(y)), "the NaN footprint differs from the yardstick's"
    err, allowed = np.abs(got - y), factor * ref.allowed(y, bound)
    ok = np.isfinite(y)
    print(f"radius {radius}: margin {margin:.3g} km, max error {err[ok].max():.3g}, worst error / allowed {(err[ok] / allowed[ok]).max():.3g}, "
          f"fp64 bound up to {bound[ok].max():.3g}")
    assert np.all(err[ok] <= allowed[ok])


# ---- the dense yardstick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("ascending", [False, True])
def test_numpy_path_against_the_dense_yardstick(radius, ascending):
    lat = LAT19[::-1].copy() if ascending else LAT19
    x = field((2, 19, 40), 1)
    x[0, 3, 5], x[1, 10, 39], x[1, 10, 0] = np.nan, np.inf, -np.inf
    out = run(x, lat, full_lon(40), radius, min_valid=0.0, keep_mask=False)
    assert out.dtype == np.float32
    check_against_yardstick(out, x, lat, 2 * np.pi / 40, radius)


@pytest.mark.parametrize("W", [39, 40])
def test_regional_grid_against_the_dense_yardstick(W):
    lat, lon = np.linspace(60, 20, 17), 10.0 + 2.5 * np.arange(W)
    x = field((1, 17, W), 2)
    out = run(x, lat, lon, 700.0, min_valid=0.0)
    check_against_yardstick(out, x, lat, np.deg2rad(2.5), 700.0)


# ---- the table ------------------------------------------------------------------------------------------------------------
def brute_half(lat, dlam, W, wrap, radius):
    """n(i, k) from the yardstick's haversine per row pair: the largest gap whose point is inside, -1 for none."""
    phi = np.deg2rad(lat)
    gaps = np.arange((W // 2 if wrap else W - 1) + 1)
    out = {}
    for i in range(len(lat)):
        for k in range(len(lat)):
            d = ref.haversine_km(phi[i], phi[k], gaps * dlam)
            assert np.abs(d - radius).min() > 1e-6
            inside = np.nonzero(d <= radius)[0]
            out[i, k] = int(inside.max()) if inside.size else -1
    return out


@pytest.mark.parametrize("lat,W,wrap,radius", [
    (LAT19, 40, True, 300.0), (LAT19, 40, True, 1234.5), (LAT19, 40, True, 2500.0), (LAT19[::-1].copy(), 40, True, 1234.5),
    (LAT19, 41, True, 2500.0), (LAT19, 6, True, 5000.0), (LAT19, 7, True, 5000.0), (np.linspace(60, 20, 17), 39, False, 700.0)])
def test_table_against_brute_force(lat, W, wrap, radius):
    dlam = 2 * np.pi / W if wrap else np.deg2rad(2.5)
    row_lo, row_count, half, w = mod.disc_table(lat, dlam, W, wrap, radius)
    assert half.dtype == row_lo.dtype == row_count.dtype == np.int32 and w.dtype == np.float64
    want = brute_half(lat, dlam, W, wrap, radius)
    H = len(lat)
    for i in range(H):
        rows = range(row_lo[i], row_lo[i] + row_count[i])
        for k in range(H):
            n = half[i, k - row_lo[i]] if k in rows else -1
            assert n == want[i, k], (i, k, n, want[i, k])
        assert np.all(half[i, row_count[i]:] == -1)
    poles = np.abs(lat) >= 90 - 1e-9
    assert np.all(w[poles] == 0.0) and np.all(w[~poles] > 0)
    if wrap and poles.any():                                  # at a pole the disc is the whole circle of every row it reaches
        for i in np.nonzero(poles)[0]:
            reached = half[i, :row_count[i]]
            assert np.all(reached[reached >= 0] == W // 2)
    if wrap and radius == 5000.0:                             # even and odd W at n = floor(W / 2)
        assert half.max() == W // 2 and mod._window(W // 2, W, True)[3] == W


# ---- exact properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
def test_constant_plane_comes_back_bit_equal(radius):
    c = np.full((1, 19, 40), np.float32(287.123))
    out = run(c, LAT19, full_lon(40), radius, min_valid=1.0)
    inner = np.abs(LAT19) < 90                                # (a pole row alone carries no weight)
    assert np.array_equal(out[:, inner].view(np.uint32), c[:, inner].view(np.uint32))


def test_rows_that_hold_only_the_point_itself_return_the_input():
    lat, W = np.linspace(80, -80, 17), 72                     # 10 degrees of latitude, 5 of longitude
    x = field((2, 17, W), 3, mean=-3.0, amp=50.0)
    table = mod.disc_table(lat, 2 * np.pi / W, W, True, 250.0)
    alone = [i for i in range(17) if sum(n >= 0 for n in table[2][i, :table[1][i]]) == 1 and table[2][i].max() == 0]
    wide = [i for i in range(17) if table[2][i].max() > 0]
    assert alone and wide, "the grid must have rows of both kinds (near the poles a small radius spans many columns)"
    out = run(x, lat, full_lon(W), 250.0)
    assert np.array_equal(out[:, alone].view(np.uint32), x[:, alone].view(np.uint32))
    assert not np.array_equal(out[:, wide], x[:, wide])


# ---- validity, coverage, layout -------------------------------------------------------------------------------------------
def test_validity_and_min_valid_and_keep_mask():
    x = field((3, 19, 40), 4)
    g = np.random.default_rng(5)
    x[0][g.random((19, 40)) < 0.2] = np.nan
    x[0, 4, 7], x[0, 12, 1] = np.inf, -np.inf
    x[1, 9] = np.nan                                          # a NaN row
    x[2] = np.nan                                             # an all-NaN plane
    lon = full_lon(40)
    loose = run(x, LAT19, lon, 1234.5, min_valid=0.0, keep_mask=False)
    check_against_yardstick(loose, x, LAT19, 2 * np.pi / 40, 1234.5)
    assert np.isnan(loose[2]).all() and np.isfinite(loose[1, 9]).all() and np.isfinite(loose[0, 4, 7])
    kept = run(x, LAT19, lon, 1234.5, min_valid=0.0, keep_mask=True)
    assert np.array_equal(np.isnan(kept), np.isnan(loose) | ~np.isfinite(x))
    same = np.isfinite(kept)
    assert np.array_equal(kept[same], loose[same])
    # coverage: the weighted share of valid members, from the yardstick's den and the same sum over a plane of ones
    _, den, _, _ = ref.dense(x, LAT19, 2 * np.pi / 40, 1234.5)
    _, full, _, _ = ref.dense(np.ones_like(x), LAT19, 2 * np.pi / 40, 1234.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = den / full
    for min_valid in (0.5, 1.0):
        got = run(x, LAT19, lon, 1234.5, min_valid=min_valid, keep_mask=False)
        clear = np.abs(share - min_valid) > 1e-12             # (min_valid = 1: share == 1 exactly where every member is valid)
        want_nan = ~(full > 0) | (share < min_valid)
        if min_valid == 1.0:
            clear, want_nan = np.ones_like(clear), ~(full > 0) | (den != full)
        assert np.array_equal(np.isnan(got)[clear], want_nan[clear])
        assert np.array_equal(got[~np.isnan(got)], loose[~np.isnan(got)])
    assert np.isnan(run(x, LAT19, lon, 1234.5, min_valid=1.0, keep_mask=False)[1, 8:11]).all()


def test_regional_overhang_counts_as_invalid():
    lat, W = np.linspace(60, 20, 17), 39
    lon = 10.0 + 2.5 * np.arange(W)
    x = field((1, 17, W), 6)
    strict = run(x, lat, lon, 700.0, min_valid=1.0)
    assert np.isnan(strict[:, :, 0]).all() and np.isnan(strict[:, :, -1]).all() and np.isfinite(strict[:, :, W // 2]).all()
    loose = run(x, lat, lon, 700.0, min_valid=0.0)
    assert np.isfinite(loose).all()
    half = run(x, lat, lon, 700.0, min_valid=0.5)
    assert np.isfinite(half[:, 8, 0]).all()                   # at the edge a little more than half of the disc is on the grid


def test_single_row_and_single_column():
    x = field((2, 1, 40), 7)
    out = smooth(batch_of(x, [0.0], full_lon(40), T=1), 1234.5).surf_vars["x"][:, 0].numpy()
    check_against_yardstick(out, x, np.zeros(1), 2 * np.pi / 40, 1234.5)
    col = field((2, 19, 1), 8)
    out = smooth(batch_of(col, LAT19, [12.0]), 1234.5, min_valid=0.0).surf_vars["x"][:, 0].numpy()
    check_against_yardstick(out, col, LAT19, 0.0, 1234.5)


def test_returned_batch():
    g = torch.Generator().manual_seed(0)
    md = Metadata(lat=torch.linspace(90, -90, 19, dtype=torch.float64), lon=torch.as_tensor(full_lon(40)),
                  time=(datetime(2023, 1, 1, 6),) * 2, atmos_levels=(500, 850))
    b = Batch({"2t": torch.randn(2, 2, 19, 40, generator=g), "msl": torch.randn(2, 2, 19, 40, generator=g, dtype=torch.float64)},
              {"lsm": torch.randn(19, 40, generator=g)}, {"z": torch.randn(2, 2, 2, 19, 40, generator=g)}, md)
    out = smooth(b, 1234.5)
    assert list(out.surf_vars) == ["2t", "msl"] and list(out.atmos_vars) == ["z"] and out.metadata is md
    assert out.surf_vars["2t"].shape == (2, 1, 19, 40) and out.atmos_vars["z"].shape == (2, 1, 2, 19, 40)
    assert all(v.dtype == torch.float32 for v in (*out.surf_vars.values(), *out.atmos_vars.values()))
    assert out.static_vars["lsm"] is b.static_vars["lsm"]
    only = smooth(b, 1234.5, only=["z"])
    assert not only.surf_vars and torch.equal(only.atmos_vars["z"], out.atmos_vars["z"])
    alone = smooth(Batch({}, {}, {"z": b.atmos_vars["z"][1:, :, 1:]}, md), 1234.5).atmos_vars["z"]
    assert torch.equal(alone, out.atmos_vars["z"][1:, :, 1:])       # a plane does not depend on its neighbours in the call


def test_refusals():
    x = field((1, 19, 40), 9)
    b = batch_of(x, LAT19, full_lon(40))
    for radius in (0.0, -5.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="smooth: radius_km must be a finite number above 0"):
            smooth(b, radius)
    for min_valid in (-0.1, 1.5, float("nan"), None, True):
        with pytest.raises(ValueError, match=r"smooth: min_valid must be a number in \[0, 1\]"):
            smooth(b, 300.0, min_valid=min_valid)
    with pytest.raises(TypeError, match="smooth: batch must be a Batch, got dict"):
        smooth({}, 300.0)
    with pytest.raises(ValueError, match="smooth: only names the variable 'y'"):
        smooth(b, 300.0, only=["y"])
    band = BandBatch(b.surf_vars, {}, {}, b.metadata, full_patch_rows=4, band=(0, 4))
    with pytest.raises(ValueError, match=r"smooth: batch is a latitude band \(BandBatch\)"):
        smooth(band, 300.0)
    md = b.metadata
    matrix = Batch(b.surf_vars, {}, {}, derive_metadata(md, lat=md.lat[:, None].expand(19, 40), lon=md.lon[None].expand(19, 40)))
    with pytest.raises(ValueError, match="smooth: batch has matrices for latitudes / longitudes"):
        smooth(matrix, 300.0)
    mixed = Batch({"x": b.surf_vars["x"], "y": torch.empty(1, 2, 19, 40, device="meta")}, {}, {}, md)
    with pytest.raises(ValueError, match=r"smooth: the fields are on \['cpu', 'meta'\]; move the batch to the CPU or to one GPU first"):
        smooth(mixed, 300.0)
    with pytest.raises(ValueError, match="smooth: the latitudes must be strictly monotonic"):
        smooth(batch_of(x, np.r_[LAT19[:-1], LAT19[-2]], full_lon(40)), 300.0)
    lon = full_lon(40).copy()
    lon[3] += 1.0
    with pytest.raises(ValueError, match="smooth: the longitudes must be equally spaced"):
        smooth(batch_of(x, LAT19, lon), 300.0)
    with pytest.raises(ValueError, match=r"smooth: batch.surf_vars\['x'\] has shape"):
        smooth(batch_of(x[:, :18], LAT19, full_lon(40)), 300.0)


def test_too_many_rows_names_the_largest_radius():
    lat = np.linspace(89.875, -89.875, 720)
    b = batch_of(np.zeros((1, 720, 4), dtype=np.float32), lat, full_lon(4))
    step_km = np.deg2rad(0.25) * mod.EARTH_RADIUS_KM
    with pytest.raises(ValueError, match=r"smooth: a radius of 4000 km spans \d+ latitude rows of this grid; at most 255") as e:
        smooth(b, 4000.0)
    limit = float(str(e.value).rsplit("below ", 1)[1].split(" km")[0])
    assert abs(limit - 128 * step_km) < 1e-2                  # 127 rows on either side and the row itself: 255
    assert mod.disc_table(lat, 2 * np.pi / 4, 4, True, limit - 0.01)[1].max() == 255
    with pytest.raises(ValueError, match="at most 255"):
        smooth(b, limit + 0.01)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_the_c_entry_point_refuses_before_any_launch():
    from aurora_amd.engine import lib

    raw, header = lib.load(), (lib.library_path().parents[2] / "include" / "aurora_hip.h").read_text()
    for name in ("aurora_hip_smooth", "aurora_hip_smooth_workspace_bytes"):
        assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    assert "smooth.hip" in importlib.import_module("aurora_amd.build").SOURCES
    assert aurora_amd.smooth is mod.smooth and "smooth" in aurora_amd.__all__
    need = raw.aurora_hip_smooth_workspace_bytes(3, 9, 12)
    assert need == (3 * 9 * 13 * 12 + 7) // 8 * 8 and raw.aurora_hip_smooth_workspace_bytes(1, 1, 2) == 40
    assert raw.aurora_hip_smooth_workspace_bytes(0, 9, 12) == 0 and raw.aurora_hip_smooth_workspace_bytes(1, 600000, 4096) == 0
    err = lambda: raw.aurora_hip_last_error()  # noqa: E731
    args = lambda **kw: tuple({**dict(planes=16, out=16, n_planes=3, n_lat=9, n_lon=12, row_lo=16, row_count=16, half=16,  # noqa: E731
                                     max_rows=3, w=16, wrap=1, min_valid=0.5, keep_mask=1, ws=16, ws_size=need, stream=None), **kw}.values())
    for kw, text in ((dict(ws_size=need - 8), b"workspace"), (dict(max_rows=256), b"255 source rows"), (dict(max_rows=0), b"source rows"),
                     (dict(wrap=2), b"flags"), (dict(keep_mask=-1), b"flags"), (dict(min_valid=1.5), b"min_valid"),
                     (dict(min_valid=float("nan")), b"min_valid"), (dict(n_lat=600000, n_lon=4096), b"too large"),
                     (dict(half=None), b"null"), (dict(out=None), b"null"), (dict(out=18), b"aligned"), (dict(ws=20), b"aligned"), (dict(n_lon=0), b"bad sizes")):
        assert raw.aurora_hip_smooth(*args(**kw)) == -1 and text in err(), (kw, err())
    assert raw.aurora_hip_smooth(*args(n_planes=0)) == 0
