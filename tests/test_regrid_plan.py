"""The interpolation tables of `Batch.regrid`'s device path (aurora_hip_regrid_plan, host arithmetic, no GPU).

Applied in numpy -- fp64, the four corners summed in the kernel's order, rounded to fp32 -- the tables must give what the
host path (`aurora_amd.batch._interpolate`, SciPy's RegularGridInterpolator) gives: NaN for NaN, and within 1 fp32 ulp
elsewhere (where linear extrapolation cancels, 1e-9 x the plane's max |value| absolute).  Also: the argument errors of
the plan and of aurora_hip_regrid, which are raised before any launch."""
import numpy as np
import pytest
import torch

from aurora_amd.batch import _interpolate
from aurora_amd.engine import lib


def target_grid(res):
    n_lat, n_lon = round(180 / res) + 1, round(360 / res)
    return np.linspace(90, -90, n_lat), np.linspace(0, 360, n_lon, endpoint=False)


def apply_tables(fields, tables):
    """fields (..., h, w) -> (..., n_rows, n_cols) float32 through the plan's tables, in the kernel's arithmetic."""
    rows, row_w, cols, col_w = tables
    f = np.asarray(fields, dtype=np.float64)
    ay0, ay1 = (1.0 - row_w)[:, None], row_w[:, None]
    bx0, bx1 = 1.0 - col_w, col_w
    s0, s1 = f[..., rows[:, 0], :], f[..., rows[:, 1], :]
    v00, v01, v10, v11 = s0[..., cols[:, 0]], s0[..., cols[:, 1]], s1[..., cols[:, 0]], s1[..., cols[:, 1]]
    with np.errstate(invalid="ignore"):
        out = v00 * ay0 * bx0 + v01 * ay0 * bx1 + v10 * ay1 * bx0 + v11 * ay1 * bx1
    return out.astype(np.float32)


def assert_matches_host(mine, host, what=""):
    """NaN for NaN; else within 1 fp32 ulp of the host value, or 1e-9 x the plane's max |host| where extrapolation cancels."""
    mine, host = np.asarray(mine, dtype=np.float32), np.asarray(host, dtype=np.float32)
    assert mine.shape == host.shape, what
    np.testing.assert_array_equal(np.isnan(mine), np.isnan(host), err_msg=f"{what}: NaN footprint")
    planes_h = host.reshape(-1, *host.shape[-2:]).astype(np.float64)
    planes_m = mine.reshape(-1, *mine.shape[-2:]).astype(np.float64)
    for p, (m, h) in enumerate(zip(planes_m, planes_h)):
        ok = ~np.isnan(h)
        if not ok.any():
            continue
        err = np.abs(m[ok] - h[ok])
        bound = np.maximum(np.spacing(np.abs(h[ok]).astype(np.float32)).astype(np.float64), 1e-9 * np.abs(h[ok]).max())
        worst = int(np.argmax(err - bound))
        assert (err <= bound).all(), f"{what} plane {p}: |{m[ok][worst]} - {h[ok][worst]}| > {bound[worst]}"


def check_grid(lat, lon, fields, res=None, targets=None):
    lat_new, lon_new = targets if targets is not None else target_grid(res)
    tables = lib.regrid_plan(lat, lon, lat_new, lon_new)
    host = _interpolate(torch.from_numpy(fields), torch.from_numpy(np.asarray(lat)), torch.from_numpy(np.asarray(lon)),
                        torch.from_numpy(lat_new), torch.from_numpy(lon_new)).numpy()
    mine = apply_tables(fields, tables)
    assert_matches_host(mine, host, f"{len(lat)}x{len(lon)} -> {len(lat_new)}x{len(lon_new)}")
    return mine, host


def rand(*shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_same_resolution_is_the_identity():
    lat, lon = np.linspace(90, -90, 37), np.linspace(0, 360, 72, endpoint=False)
    f = rand(3, 37, 72)
    mine, _ = check_grid(lat, lon, f, res=5.0)
    np.testing.assert_array_equal(mine, f)


def test_seeded_batch_to_7p5_degrees():
    """The setup of tests/golden/batch_methods.npz: a 17 x 32 grid with float32 coordinates."""
    lat = torch.linspace(90, -90, 17, dtype=torch.float32).double().numpy()
    lon = torch.linspace(0, 360, 33, dtype=torch.float32)[:-1].double().numpy()
    check_grid(lat, lon, rand(4, 2, 17, 32, seed=7), res=7.5)


def test_source_without_the_south_pole_extrapolates():
    lat, lon = np.linspace(90, -90, 73)[:-1], np.linspace(0, 360, 144, endpoint=False)
    rows, row_w, _, _ = lib.regrid_plan(lat, lon, *target_grid(1.0))
    assert row_w[-1] < 0.0 and tuple(rows[-1]) == (71, 70)     # -90 lies below the last source row: t < 0
    check_grid(lat, lon, rand(2, 72, 144, seed=1), res=1.0)


def test_non_uniform_latitudes():
    g = np.random.default_rng(3)
    lat = np.sort(np.concatenate(([90.0, -90.0], g.uniform(-89.5, 89.5, 40))))[::-1].copy()
    lon = np.linspace(0, 360, 64, endpoint=False)
    check_grid(lat, lon, rand(3, 42, 64, seed=2), res=2.0)
    check_grid(lat[1:-1], lon, rand(3, 40, 64, seed=4), res=3.0)      # no pole at either end: both ends extrapolate


def test_last_longitude_close_to_360():
    lat = np.linspace(90, -90, 19)
    lon = np.concatenate((np.arange(0.0, 350.0, 10.0), [359.999]))
    _, _, cols, col_w = lib.regrid_plan(lat, lon, np.array([0.0]), np.array([0.0, 355.0, 359.9995]))
    assert tuple(cols[0]) == (0, 1) and col_w[0] == 0.0                   # on the node 0: the interval that starts there
    assert tuple(cols[1]) == (34, 35) and tuple(cols[2]) == (35, 0)       # between 359.999 and 360: wraps to column 0
    assert abs(col_w[2] - 0.5) < 1e-6
    check_grid(lat, lon, rand(2, 19, 36, seed=5), res=2.5)
    check_grid(lat, lon, rand(2, 19, 36, seed=6), targets=(np.array([90.0, 0.0]), np.array([0.0, 359.9995, 359.999])))


def test_nan_at_every_zero_weight_neighbour_of_an_on_node_target():
    """5 x 8 grid (45 degrees), targets on its own nodes: every single NaN cell gives the host path's NaN footprint."""
    lat, lon = np.linspace(90, -90, 5), np.linspace(0, 360, 8, endpoint=False)
    base = rand(5, 8, seed=8)
    for i in range(5):
        for j in range(8):
            f = base.copy()
            f[i, j] = np.nan
            check_grid(lat, lon, f[None], res=45.0)

    def nan_at(i, j):
        f = base.copy()
        f[i, j] = np.nan
        return apply_tables(f, lib.regrid_plan(lat, lon, *target_grid(45.0)))

    assert np.isnan(nan_at(2, 3)[2, 2])                  # lat 0 / lon 90 is NaN when (0, 135) is NaN
    assert np.isnan(nan_at(1, 5)[0, 5])                  # lat 90 is NaN when the 45-degree row is NaN
    assert np.isnan(nan_at(3, 0)[3, 7])                  # lon 315 is NaN when column 0 is NaN (wrap-around)
    assert not np.isnan(nan_at(3, 7)[3, 0])              # lon 0 is not NaN when column 7 is NaN


def test_plan_argument_errors():
    lat, lon = np.linspace(90, -90, 5), np.linspace(0, 360, 8, endpoint=False)
    tgt = target_grid(45.0)
    for bad_lat, bad_lon, msg in (
        (lat[[0, 2, 1, 3, 4]], lon, "latitudes must be finite and strictly monotone"),
        (np.array([90.0, 0.0, 0.0, -90.0]), lon, "strictly monotone"),
        (np.array([90.0, np.nan, -90.0]), lon, "strictly monotone"),
        (lat, lon[::-1].copy(), "longitudes must be finite, strictly increasing"),
        (lat, np.array([0.0, 90.0, 360.0]), "span less than 360"),
        (lat[:1], lon, "n >= 2"),
        (lat, lon[:1], "n >= 2"),
    ):
        with pytest.raises(ValueError, match=msg):
            lib.regrid_plan(bad_lat, bad_lon, *tgt)
    with pytest.raises(ValueError, match="target coordinates must be finite"):
        lib.regrid_plan(lat, lon, np.array([0.0, np.nan]), tgt[1])
    with pytest.raises(ValueError, match="empty target grid"):
        lib.regrid_plan(lat, lon, np.zeros(0), tgt[1])


def test_regrid_argument_errors_surface_without_a_gpu():
    L = lib.load()
    err = lambda: L.aurora_hip_last_error()  # noqa: E731
    p = 16   # a non-null dummy: every call below fails validation before anything is dereferenced or launched
    assert L.aurora_hip_regrid(None, lib.F32, p, 1, 4, 4, p, p, 2, p, p, 2, None) == -1 and b"null" in err()
    assert L.aurora_hip_regrid(p, lib.F32, p, 1, 4, 4, p, None, 2, p, p, 2, None) == -1 and b"null" in err()
    assert L.aurora_hip_regrid(p, lib.BF16, p, 1, 4, 4, p, p, 2, p, p, 2, None) == -1 and b"dtype" in err()
    assert L.aurora_hip_regrid(p, lib.F64, p, 0, 4, 4, p, p, 2, p, p, 2, None) == -1 and b"positive" in err()
    assert L.aurora_hip_regrid(p, lib.F32, p, 1, 4, 4, p, p, 0, p, p, 2, None) == -1 and b"positive" in err()
    assert L.aurora_hip_regrid(p, lib.F32, p, 1, 4, 4, p, p, 2, p, p, -3, None) == -1 and b"positive" in err()
