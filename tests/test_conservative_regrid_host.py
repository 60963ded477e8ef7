"""`aurora_amd.conservative_regrid` on the host: the numpy path against an independent dense evaluation, the exact
properties of the rule, NaN handling, errors and metadata.  No GPU.

THE YARDSTICK is written here from the cell model alone: edges computed by this file, dense overlap matrices
Wlat (n_out x n_in) in sin(lat) and Wlon (n_out x n_in) in degrees (the images of a full-circle source at -360, 0, +360
summed), and

    out = (Wlat @ (x . finite) @ Wlon^T) / (Wlat @ finite @ Wlon^T),    coverage = denominator / (A_i B_j).

The weights are fp64 numbers from the same elementary operations as the rule states (midpoints, sines, differences), so
both sides hold the same weights; the matrix products are taken in numpy's longdouble (64-bit significand on x86), so that
the yardstick's own rounding is a small part of the allowance below.

THE BOUND.  With u = 2^-53, r and c the numbers of row and column taps of a target point, w = a b >= 0: the module forms every
term of n = sum w x with two roundings of products and adds it into sums of r and of c terms, so every term carries at most
(r - 1 + 1) + (c - 1 + 1) = r + c roundings: |n^ - n| <= (r + c) u sum w|x| (to first order), likewise |d^ - d| <= (r + c) u d,
and the quotient rounds once more:

    |q^ - q| <= (2 (r + c) + 1) u sum w|x| / sum w  =  (r + c + 1/2) 2^-52 sum w|x| / sum w.

The check allows (r + c + 2) 2^-52 sum w|x| / sum w -- the remaining 1.5 units take the yardstick's extended-precision
products -- plus half an fp32 ulp of the result for the one rounding to float.  NaN must appear exactly where the yardstick's
coverage rule says so; the inputs keep every coverage more than 1e-9 away from min_valid (asserted)."""
import math

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, conservative_regrid
from aurora_amd import conservative as C
from aurora_amd.batch import BandBatch, derive_metadata
from tests.conservative_inputs import GLOBAL, GRIDS, batch, circle, every_field, field, lin, metadata, same_bits

WIDE = np.longdouble


# ---- the yardstick --------------------------------------------------------------------------------------------------------
def is_circle(lon) -> bool:
    n = len(lon)
    step = 360.0 / n
    return bool(np.all(np.abs(lon - lon[0] - np.arange(n) * step) <= 1e-6 * step))


def lat_edges(lat):
    """(lo, hi) per row in sin(lat)."""
    n = len(lat)
    lo, hi = np.empty(n), np.empty(n)
    for k in range(n):
        north = 0.5 * (lat[k - 1] + lat[k]) if k > 0 else lat[0] - 0.5 * (lat[1] - lat[0])
        south = 0.5 * (lat[k] + lat[k + 1]) if k < n - 1 else lat[-1] + 0.5 * (lat[-1] - lat[-2])
        m = []
        for e in (north, south):
            e = min(max(e, -90.0), 90.0)
            m.append(1.0 if e == 90.0 else -1.0 if e == -90.0 else float(np.sin(np.deg2rad(e))))
        lo[k], hi[k] = min(m), max(m)
    return lo, hi


def lon_edges(lon):
    n = len(lon)
    west, east = np.empty(n), np.empty(n)
    for k in range(n):
        west[k] = 0.5 * (lon[k - 1] + lon[k]) if k > 0 else lon[0] - 0.5 * (lon[1] - lon[0])
        east[k] = 0.5 * (lon[k] + lon[k + 1]) if k < n - 1 else lon[-1] + 0.5 * (lon[-1] - lon[-2])
    if is_circle(lon):
        west[0] = 0.5 * ((lon[-1] - 360.0) + lon[0])
        east[-1] = west[0] + 360.0
    return west, east


def dense(tl, th, sl, sh):
    return np.maximum(0.0, np.minimum(th[:, None], sh[None, :]) - np.maximum(tl[:, None], sl[None, :]))


def matrices(grid):
    slat, slon, dlat, dlon = grid
    Wlat = dense(*lat_edges(dlat), *lat_edges(slat))
    west, east = lon_edges(slon)
    if is_circle(slon):                                       # the three images of the source, edges shared across the seam
        n = len(slon)
        e = np.append(west, east[-1])
        u = np.concatenate([e[:-1] - 360.0, e[:-1], e + 360.0])
        W3 = dense(*lon_edges(dlon), u[:-1], u[1:])
        Wlon = W3[:, :n] + W3[:, n:2 * n] + W3[:, 2 * n:]
    else:
        Wlon = dense(*lon_edges(dlon), west, east)
    tl, th = lat_edges(dlat)
    west, east = lon_edges(dlon)
    return Wlat, Wlon, th - tl, east - west


def yardstick(x, grid, min_valid):
    """x: (..., n_lat, n_lon) -> (value (fp64, NaN by the coverage rule), allowed fp64 error, coverage)."""
    Wlat, Wlon, A, B = matrices(grid)
    fin = np.isfinite(x)
    xz = np.where(fin, x, 0.0).astype(WIDE)
    Wr, Wc = Wlat.astype(WIDE), Wlon.astype(WIDE).T
    num, den, mag = Wr @ xz @ Wc, Wr @ fin.astype(WIDE) @ Wc, Wr @ np.abs(xz) @ Wc
    cover = (den / (A[:, None] * B)).astype(np.float64)
    ok = (den > 0) & (cover >= min_valid)
    safe = np.where(ok, den, 1)
    taps = (Wlat > 0).sum(1)[:, None] + (Wlon > 0).sum(1)[None, :]
    allowed = ((taps + 2) * 2.0 ** -52 * (mag / safe)).astype(np.float64)
    return np.where(ok, (num / safe).astype(np.float64), np.nan), allowed, cover


def agrees(got: np.ndarray, x: np.ndarray, grid, min_valid: float) -> None:
    want, allowed, cover = yardstick(x, grid, min_valid)
    assert np.all(np.abs(cover - min_valid) > 1e-9), "an input with a coverage at min_valid: choose another"
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN where the coverage rule says otherwise"
    ok = ~np.isnan(want)
    half_ulp = 0.5 * np.spacing(np.abs(got[ok]))
    excess = np.abs(got[ok].astype(np.float64) - want[ok]) - (half_ulp.astype(np.float64) + allowed[ok])
    print(f"largest |difference| - allowance: {excess.max():.3e} (allowance {allowed[ok].max():.3e} + half an ulp)")
    assert np.all(excess <= 0)


def regridded(b: Batch, grid, **kw) -> Batch:
    return conservative_regrid(b, lat=grid[2], lon=grid[3], **kw)


# ---- against the yardstick ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_every_field_agrees_with_the_dense_evaluation(name):
    grid = GRIDS[name]
    b = batch(grid[0], grid[1], seed=1, B=2, T=2)
    out = regridded(b, grid)
    for (_, k, v), (_, _, o) in zip(every_field(b), every_field(out)):
        assert o.shape == (*v.shape[:-2], len(grid[2]), len(grid[3])) and o.dtype == torch.float32, k
        agrees(o.numpy(), v.numpy(), grid, 0.5)


def test_the_frame_of_an_overhanging_target_is_nan():
    grid = GRIDS["regional 13x13 -> overhanging 6x6"]
    out = regridded(batch(grid[0], grid[1], seed=2), grid).surf_vars["2t"][0, 0].numpy()
    frame = np.ones((6, 6), dtype=bool)
    frame[1:-1, 1:-1] = False
    assert np.array_equal(np.isnan(out), frame)
    loose = regridded(batch(grid[0], grid[1], seed=2), grid, min_valid=1e-6).surf_vars["2t"][0, 0].numpy()
    assert not np.isnan(loose).any() and np.array_equal(loose[1:-1, 1:-1], out[1:-1, 1:-1])


def test_a_finer_target_is_piecewise_constant():
    """Target cells that lie inside one source cell take its value (two equal roundings apart at the most: exactly)."""
    grid = GRIDS["finer 8x14 -> 19x36"]
    b = batch(grid[0], grid[1], seed=3)
    x, out = b.surf_vars["msl"][0, 0].numpy(), regridded(b, grid).surf_vars["msl"][0, 0].numpy()
    Wlat, Wlon, _, _ = matrices(grid)
    single = ((Wlat > 0).sum(1) == 1)[:, None] & ((Wlon > 0).sum(1) == 1)[None, :]
    assert single.sum() > 100
    src = x[np.argmax(Wlat, 1)][:, np.argmax(Wlon, 1)]
    assert np.array_equal(out[single], src[single])


def test_the_tables_of_a_tenth_degree_grid():
    p = C.plan(lin(90, -90, 1801), circle(3600), lin(90, -90, 721), circle(1440))
    for axis in (p.rows, p.cols):
        assert axis.count.min() >= 2 and axis.count.max() <= 4
        assert np.all(axis.w > 0) and axis.w.shape[0] == axis.count.sum()
        assert np.array_equal(axis.first[:, 1], np.concatenate([[0], np.cumsum(axis.count)[:-1]]))
        sums = np.add.reduceat(axis.w, axis.first[:, 1])
        assert np.all(np.abs(sums - axis.measure) <= 4 * np.spacing(axis.measure))
    assert p.rows.first[:, 0].min() == 0 and (p.rows.first[:, 0] + p.rows.count).max() == 1801
    assert np.all(np.diff(p.cols.first[:, 0]) >= 0) and np.all(np.diff(p.cols.first[:, 0] + p.cols.count) >= 0)
    assert p.cols.first[0, 0] == 3600 - 1 and p.cols.first[:, 0].max() < 3 * 3600       # the seam cell starts at the last column
    assert math.isclose(p.rows.measure.sum(), 2.0, rel_tol=1e-14) and math.isclose(p.cols.measure.sum(), 360.0, rel_tol=1e-14)


# ---- exact properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_target_equal_to_source_is_the_identity(name):
    slat, slon = GRIDS[name][:2]
    b = batch(slat, slon, seed=4, land=0.2)
    out = conservative_regrid(b, lat=slat, lon=slon)
    for (_, k, v), (_, _, o) in zip(every_field(b), every_field(out)):
        assert torch.isnan(v).any() and same_bits(o, v), k                                 # NaN for NaN, every other bit kept


@pytest.mark.parametrize("name", list(GRIDS))
def test_a_constant_comes_back_as_that_constant(name):
    grid = GRIDS[name]
    b = batch(grid[0], grid[1])
    c = np.float32(101325.7)
    b = Batch({"msl": torch.full_like(b.surf_vars["msl"], float(c))}, {}, {}, b.metadata)
    out = regridded(b, grid, min_valid=1e-6).surf_vars["msl"].numpy()
    assert np.all(out == c)


def test_an_integer_coarsening_in_longitude_is_the_mean_of_pairs():
    """36 -> 18 columns, the latitudes kept.  The values carry 16 significant bits, so the mean of a pair is a float and
    'rounded once' is free of ties: an fp32 tie would be decided by the last bit of the fp64 quotient."""
    lat, lon = lin(85, -85, 18), circle(36)
    target = 0.5 * (lon[0::2] + lon[1::2])
    x = field((18, 36), seed=5).view(np.uint32) & np.uint32(0xFFFFFF00)
    x = x.view(np.float32)
    b = Batch({"2t": torch.from_numpy(x.copy())[None, None]}, {}, {}, metadata(lat, lon))
    out = conservative_regrid(b, lat=lat, lon=target).surf_vars["2t"][0, 0].numpy()
    want = (0.5 * (x[:, 0::2].astype(np.float64) + x[:, 1::2].astype(np.float64))).astype(np.float32)
    assert np.array_equal(out, want)


def test_a_cell_across_the_seam_reads_the_last_columns_first():
    """The first target cell of 36 -> 14 columns spans the seam: its taps are columns 35, 0, 1 in that order, which the
    rule's own loop over them reproduces bit for bit."""
    grid = GRIDS["poles 19x36 -> 8x14"]
    p = C.plan(*grid)
    first, off = p.cols.first[0]
    cnt = p.cols.count[0]
    taps = [(first + t) % 36 for t in range(cnt)]
    assert taps == [35, 0, 1] and first == 35
    b = batch(grid[0], grid[1], seed=6)
    x = b.surf_vars["2t"][0, 0].numpy().astype(np.float64)
    out = regridded(b, grid).surf_vars["2t"][0, 0].numpy()

    def by_hand(order):
        vals = []
        for i in range(8):
            r0, ro = p.rows.first[i]
            cn, cd = np.zeros(36), np.zeros(36)
            for t in range(p.rows.count[i]):
                cn, cd = cn + p.rows.w[ro + t] * x[r0 + t], cd + p.rows.w[ro + t]
            n = d = 0.0
            for t in order:
                n, d = n + p.cols.w[off + t] * cn[taps[t]], d + p.cols.w[off + t] * cd[taps[t]]
            vals.append(np.float32(n / d))
        return np.array(vals)

    assert np.array_equal(out[:, 0], by_hand(range(cnt)))


@pytest.mark.parametrize("name", GLOBAL)
def test_the_global_integral_is_conserved(name):
    grid = GRIDS[name]
    b = batch(grid[0], grid[1], seed=7)
    x = b.surf_vars["2t"][0, 0].numpy().astype(np.float64)
    out = regridded(b, grid).surf_vars["2t"][0, 0].numpy()
    sl, sh = lat_edges(grid[0])
    west, east = lon_edges(grid[1])
    _, _, A, B = matrices(grid)
    area = A[:, None] * B
    source = float(np.sum((sh - sl)[:, None] * (east - west) * x))
    allowed = float(np.sum(area * 0.5 * np.spacing(np.abs(out)).astype(np.float64)))
    got = float(np.sum(area * out.astype(np.float64)))
    print(f"integral {got!r} against {source!r}: difference {abs(got - source):.3e}, summed half ulps {allowed:.3e}")
    assert abs(got - source) <= allowed


# ---- NaN handling -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_a_land_mask_drops_out_and_the_rest_is_renormalised(name):
    grid = GRIDS[name]
    b = batch(grid[0], grid[1], seed=8, land=0.3, T=1)
    for min_valid in (0.37, 0.83):                            # (equal taps make coverages of exactly 1/2, 3/4, ...: kept away from)
        out = regridded(b, grid, min_valid=min_valid)
        for (_, k, v), (_, _, o) in zip(every_field(b), every_field(out)):
            assert 0.2 < float(torch.isnan(v).float().mean()) < 0.4
            agrees(o.numpy(), v.numpy(), grid, min_valid)


def test_a_cell_with_one_finite_point():
    grid = GRIDS["poles 19x36 -> 8x14"]
    Wlat, Wlon, _, _ = matrices(grid)
    i, j = 3, 5
    rows, cols = np.nonzero(Wlat[i] > 0)[0], np.nonzero(Wlon[j] > 0)[0]
    x = field((19, 36), seed=9)
    x[np.ix_(rows, cols)] = np.nan
    x[rows[1], cols[1]] = np.float32(287.125)
    b = Batch({"2t": torch.from_numpy(x)[None, None]}, {}, {}, metadata(grid[0], grid[1]))
    assert regridded(b, grid, min_valid=1e-6).surf_vars["2t"][0, 0, i, j] == np.float32(287.125)
    assert torch.isnan(regridded(b, grid, min_valid=0.5).surf_vars["2t"][0, 0, i, j])


def test_an_infinity_is_treated_as_nan():
    grid = GRIDS["no poles 12x20 -> 7x12"]
    x = field((12, 20), seed=10)
    holes = np.random.default_rng(0).random((12, 20)) < 0.25
    a, b_ = x.copy(), x.copy()
    a[holes] = np.nan
    b_[holes] = np.where(np.arange(holes.sum()) % 2 == 0, np.inf, -np.inf).astype(np.float32)
    out = [regridded(Batch({"2t": torch.from_numpy(v)[None, None]}, {}, {}, metadata(grid[0], grid[1])), grid).surf_vars["2t"]
           for v in (a, b_)]
    assert same_bits(out[0], out[1]) and torch.isfinite(out[0]).any()


def test_a_plane_does_not_depend_on_the_other_planes():
    grid = GRIDS["poles 19x36 -> 8x14"]
    one, other = batch(grid[0], grid[1], seed=11, land=0.3), batch(grid[0], grid[1], seed=12, land=0.1)
    mixed = Batch({"2t": one.surf_vars["2t"], "msl": other.surf_vars["msl"]}, other.static_vars, other.atmos_vars, one.metadata)
    alone = Batch({"2t": one.surf_vars["2t"][:, -1:]}, {}, {}, one.metadata)
    want = regridded(one, grid).surf_vars["2t"]
    assert same_bits(regridded(mixed, grid).surf_vars["2t"], want)
    assert same_bits(regridded(alone, grid).surf_vars["2t"], want[:, -1:])


def test_precisions():
    """fp64 sources are read as they are; bf16 and fp16 are widened to fp32 first."""
    grid = GRIDS["no poles 12x20 -> 7x12"]
    b64 = batch(grid[0], grid[1], seed=13, dtype=torch.float64)
    v = b64.surf_vars["2t"].numpy()
    assert not np.array_equal(v, v.astype(np.float32))
    agrees(regridded(b64, grid).surf_vars["2t"].numpy(), v, grid, 0.5)
    for dt in (torch.bfloat16, torch.float16):
        low = batch(grid[0], grid[1], seed=13, dtype=dt)
        wide = Batch({k: f.float() for k, f in low.surf_vars.items()}, {k: f.float() for k, f in low.static_vars.items()},
                     {k: f.float() for k, f in low.atmos_vars.items()}, low.metadata)
        for (_, k, a), (_, _, w) in zip(every_field(regridded(low, grid)), every_field(regridded(wide, grid))):
            assert same_bits(a, w), (dt, k)


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_errors():
    grid = GRIDS["poles 19x36 -> 8x14"]
    slat, slon, dlat, dlon = grid
    b = batch(slat, slon)
    with pytest.raises(ValueError, match="conservative_regrid: give either res or lat / lon, not both"):
        conservative_regrid(b, 30.0, lat=dlat, lon=dlon)
    with pytest.raises(ValueError, match="not both"):
        conservative_regrid(b, 30.0, lon=dlon)
    with pytest.raises(ValueError, match="conservative_regrid: give the target grid"):
        conservative_regrid(b)
    with pytest.raises(ValueError, match="give the target grid"):
        conservative_regrid(b, lat=dlat)
    with pytest.raises(TypeError, match="batch must be a Batch"):
        conservative_regrid(b.surf_vars, 30.0)
    for bad in ([90.0, 10.0, 20.0, -90.0], [10.0, 10.0, 0.0]):
        with pytest.raises(ValueError, match="latitudes of the target must be strictly monotonic"):
            conservative_regrid(b, lat=np.array(bad), lon=dlon)
    with pytest.raises(ValueError, match=r"latitudes of the target must be in the range \[-90, 90\]"):
        conservative_regrid(b, lat=np.array([95.0, 0.0, -90.0]), lon=dlon)
    with pytest.raises(ValueError, match="latitudes of the batch must be strictly monotonic"):
        conservative_regrid(Batch(b.surf_vars, {}, {}, metadata(np.where(np.arange(19) == 4, 80.5, slat), slon)), lat=dlat, lon=dlon)
    for bad in ([-10.0, 0.0, 10.0], [0.0, 180.0, 360.0]):
        with pytest.raises(ValueError, match=r"longitudes of the target must be in the range \[0, 360\)"):
            conservative_regrid(b, lat=dlat, lon=np.array(bad))
    with pytest.raises(ValueError, match="longitudes of the target must be strictly increasing"):
        conservative_regrid(b, lat=dlat, lon=np.array([0.0, 20.0, 10.0]))
    with pytest.raises(ValueError, match="lat must be a vector"):
        conservative_regrid(b, lat=np.zeros((2, 2)), lon=dlon)
    for bad in (0.0, -0.5, 1.5, float("nan"), "half"):
        with pytest.raises(ValueError, match="min_valid must be"):
            conservative_regrid(b, lat=dlat, lon=dlon, min_valid=bad)
    # more than 64 taps: 200 source columns under one target cell
    fine = batch(lin(90, -90, 5), circle(200))
    with pytest.raises(ValueError, match="a target cell overlaps 10[01] source columns; at most 64"):
        conservative_regrid(fine, lat=lin(90, -90, 5), lon=circle(2))
    with pytest.raises(ValueError, match="a target cell overlaps [0-9]+ source rows; at most 64"):
        conservative_regrid(batch(lin(90, -90, 200), circle(4)), lat=lin(90, -90, 2), lon=circle(4))
    # a field whose shape does not match the grid
    wrong = Batch({"2t": b.surf_vars["2t"][..., :-1]}, {}, {}, b.metadata)
    with pytest.raises(ValueError, match=r"batch.surf_vars\['2t'\] has shape \(1, 2, 19, 35\), which does not fit a 19 x 36 grid"):
        conservative_regrid(wrong, lat=dlat, lon=dlon)
    with pytest.raises(ValueError, match=r"batch.static_vars\['lsm'\] has shape \(18, 36\)"):
        conservative_regrid(Batch({}, {"lsm": b.static_vars["lsm"][:-1]}, {}, b.metadata), lat=dlat, lon=dlon)
    # matrix coordinates
    lat2, lon2 = torch.from_numpy(slat)[:, None].expand(19, 36), torch.from_numpy(slon)[None].expand(19, 36)
    with pytest.raises(ValueError, match="conservative_regrid: batch has matrices for latitudes / longitudes"):
        conservative_regrid(Batch(b.surf_vars, {}, {}, derive_metadata(b.metadata, lat=lat2, lon=lon2)), lat=dlat, lon=dlon)
    band = BandBatch(b.surf_vars, b.static_vars, b.atmos_vars, b.metadata, full_patch_rows=4, band=(0, 2))
    with pytest.raises(ValueError, match=r"conservative_regrid: batch is a latitude band \(BandBatch\)"):
        conservative_regrid(band, lat=dlat, lon=dlon)


def test_the_c_entry_refuses_bad_arguments():
    """Through the library without a device: every refusal comes before any launch."""
    from aurora_amd.engine import lib

    L = lib.load()
    p = 0x1000                                                # a non-null pointer that is never followed
    good = dict(src=p, dtype=lib.F32, dst=p, n=3, n_lat=19, n_lon=36, rows=8, cols=14, t=[p] * 8, min_valid=0.5)

    def call(**kw):
        a = {**good, **kw}
        return L.aurora_hip_conservative_regrid(a["src"], a["dtype"], a["dst"], a["n"], a["n_lat"], a["n_lon"], a["rows"], a["cols"],
                                                *a["t"], a["min_valid"], None)

    for kw, text in (({"src": None}, b"null plane array"), ({"dst": None}, b"null plane array"),
                     *(({"t": [None if k == i else p for k in range(8)]}, b"null table pointer") for i in range(8)),
                     ({"dtype": lib.BF16}, b"source dtype must be AURORA_F32 or AURORA_F64"), ({"dtype": 7}, b"source dtype"),
                     ({"n": 0}, b"sizes must be positive"), ({"n_lat": 0}, b"sizes must be positive"),
                     ({"n_lon": -1}, b"sizes must be positive"), ({"rows": 0}, b"sizes must be positive"),
                     ({"cols": 0}, b"sizes must be positive"), ({"min_valid": 0.0}, b"min_valid must be in (0, 1]"),
                     ({"min_valid": 1.0000001}, b"min_valid"), ({"min_valid": float("nan")}, b"min_valid"),
                     ({"min_valid": -0.5}, b"min_valid")):
        assert call(**kw) == -1, kw
        assert text in L.aurora_hip_last_error(), (kw, L.aurora_hip_last_error())
    assert "aurora_hip_conservative_regrid" in lib.EXPORTED_SYMBOLS


# ---- metadata and the whole batch -----------------------------------------------------------------------------------------------
def test_metadata_static_variables_and_history():
    grid = GRIDS["poles 19x36 -> 8x14"]
    b = batch(grid[0], grid[1], seed=14, B=2, T=3)
    out = regridded(b, grid)
    md = out.metadata
    assert md.lat.dtype == md.lon.dtype == torch.float64 and md.lat.device.type == "cpu"
    assert np.array_equal(md.lat.numpy(), grid[2]) and np.array_equal(md.lon.numpy(), grid[3])
    assert md.time == b.metadata.time and md.atmos_levels == b.metadata.atmos_levels and md.rollout_step == 3
    assert out.static_vars["lsm"].shape == (8, 14) and out.surf_vars["2t"].shape == (2, 3, 8, 14)
    assert out.atmos_vars["z"].shape == (2, 3, 3, 8, 14)
    agrees(out.static_vars["lsm"].numpy(), b.static_vars["lsm"].numpy(), grid, 0.5)
    for t in range(3):                                        # every history entry, each as if it were alone
        alone = Batch({"2t": b.surf_vars["2t"][:, t:t + 1]}, {}, {}, b.metadata)
        assert same_bits(regridded(alone, grid).surf_vars["2t"][:, 0], out.surf_vars["2t"][:, t])
    lat_t, lon_t = torch.from_numpy(grid[2].copy()), torch.from_numpy(grid[3].copy())
    given = conservative_regrid(b, lat=lat_t, lon=lon_t)
    assert given.metadata.lat is lat_t and given.metadata.lon is lon_t and same_bits(given.surf_vars["msl"], out.surf_vars["msl"])


def test_res_is_the_grid_of_batch_regrid_and_the_result_is_a_batch_like_any_other(tmp_path):
    b = batch(lin(90, -90, 19), circle(36), seed=15)
    out = conservative_regrid(b, 30.0)
    bilinear = b.regrid(30.0)
    assert torch.equal(out.metadata.lat, bilinear.metadata.lat) and torch.equal(out.metadata.lon, bilinear.metadata.lon)
    assert out.surf_vars["2t"].shape == bilinear.surf_vars["2t"].shape == (1, 2, 7, 12)
    assert same_bits(out.surf_vars["2t"], conservative_regrid(b, lat=lin(90, -90, 7), lon=circle(12)).surf_vars["2t"])
    # the scorers, FieldStats, diagnostics, Batch.regrid and to_netcdf take it unchanged
    truth = conservative_regrid(batch(lin(90, -90, 19), circle(36), seed=16), 30.0)
    s = aurora_amd.scores(out, truth)
    assert all(np.isfinite(v.numpy()).all() for v in s.bias.values())
    acc = aurora_amd.FieldStats()
    acc.update(out)
    assert out.regrid(60.0).surf_vars["2t"].shape == (1, 2, 4, 6)
    out.to_netcdf(tmp_path / "coarse.nc")
    back = Batch.from_netcdf(tmp_path / "coarse.nc")
    assert same_bits(back.surf_vars["2t"], out.surf_vars["2t"])
    # the bias of the regridded field is the bias of the field: the area mean is kept (to the fp32 rounding of the outputs)
    x = b.surf_vars["2t"][0, -1].numpy().astype(np.float64)
    sl, sh = lat_edges(lin(90, -90, 19))
    mean_source = float(np.sum((sh - sl)[:, None] * x) / (36 * 2.0))
    tl, th = lat_edges(lin(90, -90, 7))
    mean_target = float(np.sum((th - tl)[:, None] * out.surf_vars["2t"][0, -1].numpy().astype(np.float64)) / (12 * 2.0))
    assert abs(mean_target - mean_source) <= 2.0 ** -24 * abs(mean_source)
