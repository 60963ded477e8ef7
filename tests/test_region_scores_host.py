"""`aurora_amd.region_scores` on the CPU against a numpy fp64 yardstick written here.

Yardstick: `yardstick_sums` loops over planes and regions, takes the membership of a point from its own reading of the rule
(closed latitude intervals; longitudes reduced mod 360, a box with west > east wraps; a bool mask), and forms ok.sum(),
(w * d).sum() and the rest over the member points.  It calls no code of `aurora_amd.regions`; a region is described to it
by a plain tuple (lat pairs, lon pairs, mask).  tests/test_gpu_region_scores.py compares the kernel with the same function.

Bound (derived in tests/test_gpu_scores.py, not tuned): a sum of N fp64 terms in any order is within N 2^-53 sum|term| of
the exact sum, and both sides carry that, so with N <= 721 x 1440 (2 N 2^-53 = 2.3e-10) the count is exact, S1, S3, S4, S6 and
S7 agree to 1e-9 relative, S2 to 1e-9 x S4 and S5 to 1e-9 x sum w |p' t'| (its absolute-value sum, which the yardstick forms);
finalised: rmse to 1e-9 relative, mae to 2e-9 relative, bias to 2e-9 x mae, acc to 3e-9 absolute."""
import functools

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, Region, Regions, region_scores, scores
from aurora_amd.batch import BandBatch
from aurora_amd.scores import Scores
from tests.verification_inputs import cos_weights, randn_batch, red_noise_batch

REL = 1e-9
GRIDS = ((33, 64), (33, 61), (5, 8))
KINDS = ("randn", "red_noise")
NAMES = ("global", "tropics", "extratropics", "europe", "land", "tropical land", "point")


# ---- the yardstick -----------------------------------------------------------------------------------------------------
def membership(lat, lon, spec) -> np.ndarray:
    """(n_lat, n_lon) bool of one region; spec = (lat pairs or None, lon pairs or None, bool mask or None)."""
    lats, lons, mask = spec
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    row = np.ones(lat.shape, dtype=bool) if lats is None else np.zeros(lat.shape, dtype=bool)
    for lo, hi in lats or ():
        row |= (lo <= lat) & (lat <= hi)
    col = np.ones(lon.shape, dtype=bool) if lons is None else np.zeros(lon.shape, dtype=bool)
    x = np.fmod(np.fmod(lon, 360.0) + 360.0, 360.0)
    for west, east in lons or ():
        west, east = (west % 360.0) % 360.0, (east % 360.0) % 360.0
        col |= ((west <= x) & (x <= east)) if west <= east else ((x >= west) | (x <= east))
    inside = row[:, None] & col[None, :]
    return inside if mask is None else inside & np.asarray(mask, dtype=bool)


def yardstick_sums(pred, truth, clim, w, lat, lon, specs, with_abs=False):
    """(n_planes, R, 8) sums of (n_planes, n_lat, n_lon) arrays: count, w, w d, w d^2, w |d|, w p' t', w p'^2, w t'^2 over
    the valid points of every region; fp64 throughout.  with_abs: also (n_planes, R) sums of w |p' t'|."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    out, abs5 = np.zeros((pred.shape[0], len(specs), 8)), np.zeros((pred.shape[0], len(specs)))
    W = np.repeat(np.asarray(w, dtype=np.float64)[:, None], pred.shape[2], axis=1)
    for k in range(pred.shape[0]):
        p, t = pred[k].astype(np.float64), truth[k].astype(np.float64)
        ok = np.isfinite(p) & np.isfinite(t)
        c = None
        if clim is not None:
            c = np.asarray(clim[k], dtype=np.float64)
            ok = ok & np.isfinite(c)
        for r, spec in enumerate(specs):
            m = ok & membership(lat, lon, spec)
            wm, d = W[m], p[m] - t[m]
            out[k, r, :5] = m.sum(), wm.sum(), (wm * d).sum(), (wm * d * d).sum(), (wm * np.abs(d)).sum()
            if c is not None:
                pa, ta = p[m] - c[m], t[m] - c[m]
                out[k, r, 5:] = (wm * pa * ta).sum(), (wm * pa * pa).sum(), (wm * ta * ta).sum()
                abs5[k, r] = (wm * np.abs(pa * ta)).sum()
    return (out, abs5) if with_abs else out


def brute_force_sums(p, t, c, w, lat, lon, spec) -> np.ndarray:
    """One plane, one region, a Python loop over the points."""
    lats, lons, mask = spec
    out = np.zeros(8)
    for i in range(p.shape[0]):
        for j in range(p.shape[1]):
            x = float(lon[j]) % 360.0
            in_row = lats is None or any(lo <= float(lat[i]) <= hi for lo, hi in lats)
            in_col = lons is None or any((a % 360.0 <= x <= b % 360.0) if a % 360.0 <= b % 360.0 else (x >= a % 360.0 or x <= b % 360.0)
                                         for a, b in lons)
            vals = [float(p[i, j]), float(t[i, j])] + ([float(c[i, j])] if c is not None else [])
            if not (in_row and in_col and (mask is None or mask[i, j]) and all(np.isfinite(v) for v in vals)):
                continue
            d = vals[0] - vals[1]
            out[:5] += (1, w[i], w[i] * d, w[i] * d * d, w[i] * abs(d))
            if c is not None:
                pa, ta = vals[0] - vals[2], vals[1] - vals[2]
                out[5:] += (w[i] * pa * ta, w[i] * pa * pa, w[i] * ta * ta)
    return out


def assert_sums_match(got: np.ndarray, want: np.ndarray, abs5, what: str):
    """got / want: (..., 8) sums, abs5: (...) sums of w |p' t'| (None: no climatology); the bound of the module's text."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[..., 0], want[..., 0]), (what, "count", got[..., 0], want[..., 0])
    for s in (1, 3, 4, 6, 7):
        assert (np.abs(got[..., s] - want[..., s]) <= REL * want[..., s]).all(), (what, s, got[..., s], want[..., s])
    assert (np.abs(got[..., 2] - want[..., 2]) <= REL * want[..., 4]).all(), (what, 2, got[..., 2], want[..., 2])
    if abs5 is None:
        assert (got[..., 5:] == 0).all(), (what, "no climatology")
    else:
        assert (np.abs(got[..., 5] - want[..., 5]) <= REL * abs5).all(), (what, 5, got[..., 5], want[..., 5])


def assert_scores_match(s, y: np.ndarray, what: str):
    """The finalised scores of a result (its (n_planes, R, 12) table) against the yardstick's (n_planes, R, 8) sums."""
    t = s.table.numpy()
    empty = y[..., 0] == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse, bias, mae = np.sqrt(y[..., 3] / y[..., 1]), y[..., 2] / y[..., 1], y[..., 4] / y[..., 1]
        den = np.sqrt(y[..., 6]) * np.sqrt(y[..., 7])
        acc = y[..., 5] / den
    for col in (8, 9, 10):
        assert np.array_equal(np.isnan(t[..., col]), empty), (what, col)
    k = ~empty
    assert (np.abs(t[..., 8][k] - rmse[k]) <= REL * rmse[k]).all(), (what, "rmse")
    assert (np.abs(t[..., 10][k] - mae[k]) <= 2 * REL * mae[k]).all(), (what, "mae")
    assert (np.abs(t[..., 9][k] - bias[k]) <= 2 * REL * mae[k]).all(), (what, "bias")
    if s.has_climatology:
        assert np.array_equal(np.isnan(t[..., 11]), ~(den > 0)), (what, "acc NaN")
        assert (np.abs(t[..., 11][den > 0] - acc[den > 0]) <= 3 * REL).all(), (what, "acc")
    else:
        assert np.isnan(t[..., 11]).all() and s.acc is None


# ---- inputs ------------------------------------------------------------------------------------------------------------
def specs_of(mask: np.ndarray) -> dict:
    """The six regions of the module's example and a one-point region, as the yardstick's tuples."""
    return {"global": (None, None, None), "tropics": (((-20, 20),), None, None),
            "extratropics": (((-90, -20), (20, 90)), None, None), "europe": (((35, 75),), ((-12.5, 42.5),), None),
            "land": (None, None, mask), "tropical land": (((-20, 20),), None, mask), "point": (((0, 0),), ((0, 0),), None)}


def regions_of(specs: dict, mask_as=torch.from_numpy) -> dict:
    """The same regions as `Region`s: a single pair is passed as a pair, a union as a list; the mask as a tensor."""
    one = lambda v: None if v is None else (v[0] if len(v) == 1 else list(v))  # noqa: E731
    return {k: Region(lat=one(la), lon=one(lo), mask=None if m is None else mask_as(m)) for k, (la, lo, m) in specs.items()}


@functools.lru_cache(maxsize=None)
def make_inputs(kind: str, n_lat: int, n_lon: int, seed: int = 0):
    """(pred, truth, clim, specs): batches of 2 surface variables and a three-level one, B = 2, two history entries; NaN and
    +-Inf sprinkled into each operand, one whole row of NaN in the truth; the mask is a seeded random field >= 0."""
    if kind == "randn":
        truth = randn_batch(n_lat, n_lon, seed=seed, offset=280.0, scale=15.0)
        clim = randn_batch(n_lat, n_lon, seed=seed + 2, offset=280.0, scale=5.0)
    else:
        truth, clim = red_noise_batch(n_lat, n_lon, seed=seed), red_noise_batch(n_lat, n_lon, seed=seed + 2)
    err = randn_batch(n_lat, n_lon, seed=seed + 1, offset=0.3, scale=1.5)
    pred = Batch({k: v + err.surf_vars[k] for k, v in truth.surf_vars.items()}, truth.static_vars,
                 {k: v + err.atmos_vars[k] for k, v in truth.atmos_vars.items()}, truth.metadata)
    mid = n_lat // 2
    pred.surf_vars["2t"][0, -1, 0, 0] = float("nan")
    pred.surf_vars["2t"][1, -1, mid, n_lon - 1] = float("inf")
    pred.atmos_vars["z"][0, -1, 1, mid, 0] = float("-inf")
    truth.surf_vars["msl"][0, -1, mid, 1] = float("nan")
    truth.surf_vars["2t"][0, -1, n_lat - 1, 2] = float("-inf")
    truth.atmos_vars["z"][1, -1, 2, mid] = float("nan")            # a whole row, on the equator
    clim.surf_vars["msl"][1, -1, mid - 1, 3] = float("inf")
    clim.atmos_vars["z"][0, -1, 0, 1, n_lon - 2] = float("nan")
    mask = np.random.default_rng(100 + seed).standard_normal((n_lat, n_lon)) >= 0
    return pred, truth, clim, specs_of(mask)


def stacked(b: Batch) -> np.ndarray:
    """(n_planes, n_lat, n_lon): the last history entry of every variable, in the order of the result's layout."""
    n_lat, n_lon = b.metadata.lat.shape[0], b.metadata.lon.shape[0]
    return np.concatenate([v[:, -1].reshape(-1, n_lat, n_lon).numpy() for v in (*b.surf_vars.values(), *b.atmos_vars.values())])


def coords(b: Batch):
    return b.metadata.lat.double().numpy(), b.metadata.lon.double().numpy()


def yardstick_of(pred, truth, clim, specs, with_abs=False):
    lat, lon = coords(pred)
    return yardstick_sums(stacked(pred), stacked(truth), None if clim is None else stacked(clim), cos_weights(lat), lat, lon,
                          list(specs.values()), with_abs)


def assert_not_trivial(pred: Batch, specs: dict):
    """Conditions on the INPUT, from the yardstick's membership alone."""
    lat, lon = coords(pred)
    inside = {k: membership(lat, lon, v) for k, v in specs.items()}
    assert inside["global"].all()
    for k, m in inside.items():
        if k != "global":
            assert 1 <= m.sum() < m.size, (k, m.sum())
    keys = list(inside)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(inside[a], inside[b]), (a, b)
    assert inside["point"].sum() == 1
    west, east = specs["europe"][1][0]
    assert west % 360.0 > east % 360.0                                            # europe wraps
    cols = inside["europe"].any(axis=0)
    assert cols[0] and not cols.all()
    if lat.shape[0] == 33:                                                        # (checked by hand for these grids)
        assert inside["tropics"].any(axis=1).sum() == 7 and inside["europe"].any(axis=1).sum() == 7
        assert cols.sum() == 10 and cols[lon.shape[0] // 2:].sum() == 2 and cols[-1] and cols[-2]


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_public_names():
    from aurora_amd import regions

    assert aurora_amd.region_scores is regions.region_scores and aurora_amd.Region is regions.Region
    assert aurora_amd.Regions is regions.Regions
    for name in ("region_scores", "Region", "Regions"):
        assert name in aurora_amd.__all__


def test_yardstick_equals_a_loop_over_the_points():
    pred, truth, clim, specs = make_inputs("randn", 5, 8)
    lat, lon = coords(pred)
    p, t, c, w = stacked(pred), stacked(truth), stacked(clim), cos_weights(lat)
    for cc in (None, c):
        y = yardstick_sums(p, t, cc, w, lat, lon, list(specs.values()))
        for k in (0, 3, 5):
            for r, spec in enumerate(specs.values()):
                b = brute_force_sums(p[k], t[k], None if cc is None else cc[k], w, lat, lon, spec)
                assert y[k, r, 0] == b[0]
                np.testing.assert_allclose(y[k, r], b, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("n_lat,n_lon", GRIDS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_inputs_are_not_trivial(kind, n_lat, n_lon):
    pred, truth, clim, specs = make_inputs(kind, n_lat, n_lon)
    assert_not_trivial(pred, specs)
    y = yardstick_of(pred, truth, clim, specs)
    n = n_lat * n_lon
    assert (y[:, 0, 0] <= n).all() and (y[:, 0, 0] < n).any() and (y[..., 0] >= 0).all()
    assert (y[:, NAMES.index("point"), 0] <= 1).all()


@pytest.mark.parametrize("with_clim", (False, True))
@pytest.mark.parametrize("n_lat,n_lon", GRIDS)
@pytest.mark.parametrize("kind", KINDS)
def test_cpu_path_equals_the_yardstick(kind, n_lat, n_lon, with_clim):
    pred, truth, clim, specs = make_inputs(kind, n_lat, n_lon)
    clim = clim if with_clim else None
    s = region_scores(pred, truth, regions_of(specs), climatology=clim)
    assert s.regions == NAMES and s.has_climatology == with_clim and list(s.rmse) == ["2t", "msl", "z"]
    assert s.rmse["2t"].shape == (2, 7) and s.rmse["z"].shape == (2, 3, 7) and s.rmse["z"].dtype == torch.float64
    assert s.sums["z"].shape == (2, 3, 7, 8) and s.count["2t"].dtype == torch.int64 and s.table.shape == (10, 7, 12)
    y, abs5 = yardstick_of(pred, truth, clim, specs, with_abs=True)
    assert_sums_match(s.table[..., :8].numpy(), y, abs5 if with_clim else None, f"{kind} {n_lat}x{n_lon}")
    assert_scores_match(s, y, f"{kind} {n_lat}x{n_lon}")
    assert np.array_equal(s.count["z"].numpy().reshape(-1, 7), y[4:, :, 0])
    assert torch.equal(s.bias["msl"], s.table[2:4, :, 9]) and torch.equal(s.mae["2t"], s.table[:2, :, 10])
    assert (s.acc is None) == (not with_clim)


@pytest.mark.parametrize("with_clim", (False, True))
def test_a_region_is_a_scores_object_and_global_equals_scores(with_clim):
    pred, truth, clim, specs = make_inputs("red_noise", 33, 64)
    clim = clim if with_clim else None
    s = region_scores(pred, truth, Regions(regions_of(specs)), climatology=clim)
    tropics, whole, ref = s["tropics"], s["global"], scores(pred, truth, clim)
    assert isinstance(tropics, Scores) and isinstance(whole, Scores) and tropics.has_climatology == with_clim
    assert tropics.layout == ref.layout and torch.equal(tropics.rmse["z"], s.rmse["z"][..., 1])
    assert torch.equal(whole.table[:, 0], ref.table[:, 0]) and (tropics.table[:, 0] < ref.table[:, 0]).all()
    y, abs5 = yardstick_of(pred, truth, clim, {"global": specs["global"]}, with_abs=True)
    for side in (whole, ref):                                                     # both within the bound of the yardstick
        assert_sums_match(side.table[:, None, :8].numpy(), y, abs5 if with_clim else None, "global")
    g, r = whole.table.numpy(), ref.table.numpy()
    assert (np.abs(g[:, 8] - r[:, 8]) <= REL * r[:, 8]).all() and (np.abs(g[:, 10] - r[:, 10]) <= 2 * REL * r[:, 10]).all()
    assert (np.abs(g[:, 9] - r[:, 9]) <= 2 * REL * r[:, 10]).all()
    if with_clim:
        assert (np.abs(g[:, 11] - r[:, 11]) <= 3 * REL).all()
    with pytest.raises(KeyError, match="no region 'mars'"):
        s["mars"]


def test_interval_ends_are_closed():
    """37 rows: a row lies exactly on 20 and one on -20; both are in the tropics AND in the extratropics."""
    truth = randn_batch(37, 16, seed=3)
    assert 20.0 in truth.metadata.lat.tolist() and -20.0 in truth.metadata.lat.tolist()
    i = truth.metadata.lat.tolist().index(20.0)

    def bump(v):
        v = v.clone()
        v[..., i, :] += 3.0
        return v

    pred = Batch({k: bump(v) for k, v in truth.surf_vars.items()}, {}, {k: bump(v) for k, v in truth.atmos_vars.items()}, truth.metadata)
    s = region_scores(pred, truth, {"tropics": Region(lat=(-20, 20)), "extratropics": Region(lat=[(-90, -20), (20, 90)]),
                                    "inner": Region(lat=(-19.999, 19.999))})
    assert (s.count["2t"] == torch.tensor([9 * 16, 30 * 16, 7 * 16])).all()        # 9 + 30 = 37 + the two shared rows
    assert (s.rmse["2t"][:, :2] > 0).all() and (s.rmse["z"][..., 2] == 0).all()


def test_longitudes_are_reduced_mod_360():
    pred, truth, clim, _ = make_inputs("randn", 33, 64)
    boxes = [(-12.5, 42.5), (347.5, 42.5), (347.5, 402.5), (-372.5, -317.5)]
    s = region_scores(pred, truth, {str(k): Region(lat=(35, 75), lon=b) for k, b in enumerate(boxes)}, climatology=clim)
    t = s.table.nan_to_num()
    for k in (1, 2, 3):
        assert torch.equal(t[:, 0], t[:, k]), boxes[k]
    assert (s.count["msl"][:, 0] == 7 * 10).all()
    # a box that does not wrap, and the union of its halves
    u = region_scores(pred, truth, {"box": Region(lon=(90, 270)), "halves": Region(lon=[(90, 180), (180, 270)]),
                                    "rest": Region(lon=(270.0001, 89.9999))})
    assert torch.equal(u.table[:, 0, :11], u.table[:, 1, :11]) and torch.isnan(u.table[..., 11]).all()   # (no climatology)
    assert torch.equal(u.count["2t"][:, 0] + u.count["2t"][:, 2], region_scores(pred, truth, {"all": Region()}).count["2t"][:, 0])


def test_an_empty_selection_raises():
    pred, truth, _, _ = make_inputs("randn", 33, 64)
    with pytest.raises(ValueError, match="region_scores: the latitudes .* of region 'gap' hold no row of the grid"):
        region_scores(pred, truth, {"all": Region(), "gap": Region(lat=(1, 2))})
    with pytest.raises(ValueError, match="region_scores: the longitudes .* of region 'gap' hold no column of the grid"):
        region_scores(pred, truth, {"gap": Region(lon=(1, 2))})
    with pytest.raises(ValueError, match="ascend"):
        Region(lat=(20, -20))
    with pytest.raises(ValueError, match="pair"):
        Region(lat=(1, 2, 3))


def test_an_all_false_mask_gives_count_zero_and_nan():
    pred, truth, clim, _ = make_inputs("randn", 33, 64)
    s = region_scores(pred, truth, {"none": Region(mask=np.zeros((33, 64), dtype=bool)), "all": Region()}, climatology=clim)
    assert (s.count["2t"][:, 0] == 0).all() and (s.count["z"][..., 0] == 0).all() and (s.table[:, 0, :8] == 0).all()
    for d in (s.rmse, s.bias, s.mae, s.acc):
        assert torch.isnan(d["z"][..., 0]).all() and not torch.isnan(d["z"][..., 1]).any()
    assert torch.isnan(s["none"].rmse["2t"]).all()


def test_mask_types():
    for bad in (torch.ones(33, 64), np.ones((33, 64), dtype=np.uint8), np.ones((33, 64)), [[True]], torch.ones(33, dtype=torch.bool)):
        with pytest.raises(TypeError, match="mask must be a bool tensor or numpy array of shape"):
            Region(mask=bad)
    pred, truth, _, specs = make_inputs("randn", 33, 64)
    mask = specs["land"][2]
    a = region_scores(pred, truth, {"land": Region(mask=mask)})
    b = region_scores(pred, truth, {"land": Region(mask=torch.from_numpy(mask))})
    assert torch.equal(a.table[..., :11], b.table[..., :11]) and (a.count["2t"] > 0).all()   # (column 11: acc, NaN here)


def test_the_number_of_regions():
    pred, truth, clim, specs = make_inputs("randn", 33, 64)
    one = regions_of(specs)
    many = lambda n: {f"{k} {i // 7}": v for i, (k, v) in zip(range(n), [kv for _ in range(5) for kv in one.items()])}  # noqa: E731
    with pytest.raises(ValueError, match="region_scores: 1 to 32 regions per call, got 33"):
        region_scores(pred, truth, many(33))
    with pytest.raises(ValueError, match="region_scores: 1 to 32 regions per call, got 0"):
        region_scores(pred, truth, {})
    with pytest.raises(TypeError, match="must be a Region"):
        region_scores(pred, truth, {"tropics": (-20, 20)})
    with pytest.raises(TypeError, match="strings"):
        region_scores(pred, truth, {1: Region()})
    base = region_scores(pred, truth, one, climatology=clim).table.nan_to_num()
    for n in (9, 32):
        s = region_scores(pred, truth, many(n), climatology=clim)
        assert len(s.regions) == n and s.table.shape == (10, n, 12) and s.rmse["z"].shape == (2, 3, n)
        for r in range(n):                                                        # the same region, wherever it stands
            assert torch.equal(s.table[:, r].nan_to_num(), base[:, r % 7]), (n, r)
        y, abs5 = yardstick_of(pred, truth, clim, {k: specs[k.rsplit(" ", 1)[0]] for k in s.regions}, with_abs=True)
        assert_sums_match(s.table[..., :8].numpy(), y, abs5, f"{n} regions")


def test_messages():
    pred, truth, clim, specs = make_inputs("randn", 33, 64)
    regs = {"tropics": Region(lat=(-20, 20))}
    meta = Batch({k: v.to("meta") for k, v in truth.surf_vars.items()}, {}, {k: v.to("meta") for k, v in truth.atmos_vars.items()},
                 truth.metadata)
    with pytest.raises(ValueError) as e:
        region_scores(pred, meta, regs)
    assert str(e.value) == "region_scores: the fields are on ['cpu', 'meta']; move the batches to the CPU or to one GPU first"
    band = BandBatch(truth.surf_vars, {}, truth.atmos_vars, truth.metadata, full_patch_rows=4, band=(0, 4))
    with pytest.raises(ValueError) as e:
        region_scores(pred, band, regs)
    assert str(e.value) == ("region_scores: truth is a latitude band (BandBatch); gather the forecast first, band scores are not "
                            "supported")
    md = truth.metadata
    lat2, lon2 = md.lat[:, None].expand(33, 64), md.lon[None, :].expand(33, 64)
    matrix = lambda b: Batch(b.surf_vars, {}, b.atmos_vars, Metadata(lat2, lon2, md.time, md.atmos_levels))  # noqa: E731
    with pytest.raises(ValueError, match="^region_scores: pred has matrices for latitudes / longitudes; vector coordinates are needed$"):
        region_scores(matrix(pred), matrix(truth), regs)
    with pytest.raises(ValueError) as e:
        region_scores(pred, truth, {"land": Region(mask=np.ones((33, 60), dtype=bool))})
    assert str(e.value) == "region_scores: the mask of region 'land' has shape (33, 60), which does not fit a 33 x 64 grid"
    with pytest.raises(ValueError) as e:
        region_scores(pred, truth, {"land": Region(mask=torch.ones(33, 64, dtype=torch.bool, device="meta"))})
    assert str(e.value) == ("region_scores: the mask of region 'land' is on meta but the fields are on cpu; move the mask to the "
                            "device of the fields or to the CPU first")
    with pytest.raises(ValueError, match=r"^region_scores: pred and truth differ in lat: .*truth\.crop\(model\.patch_size\)$"):
        region_scores(pred.crop(4), truth, regs)
    with pytest.raises(ValueError, match="^region_scores: the climatology has no surf variable 'msl'$"):
        region_scores(pred, truth, regs, climatology=Batch({"2t": clim.surf_vars["2t"]}, {}, clim.atmos_vars, md))
    with pytest.raises(ValueError, match="^region_scores: pred and truth have no surface or atmospheric variable in common$"):
        region_scores(Batch({"10u": pred.surf_vars["2t"]}, {}, {}, md), truth, regs)
    with pytest.raises(TypeError, match="Regions object or a dict"):
        region_scores(pred, truth, [Region()])


def test_history_only_the_last_entry_is_scored():
    pred, truth, _, specs = make_inputs("randn", 5, 8)
    moved = Batch({k: v.clone() for k, v in pred.surf_vars.items()}, {}, {k: v.clone() for k, v in pred.atmos_vars.items()}, pred.metadata)
    moved.surf_vars["2t"][:, 0] += 100.0
    moved.atmos_vars["z"][:, 0] = float("nan")
    regs = Regions(regions_of(specs))
    assert torch.equal(region_scores(moved, truth, regs).table.nan_to_num(), region_scores(pred, truth, regs).table.nan_to_num())


def test_scorecard_holds_the_published_boxes():
    from aurora_amd.regions import SCORECARD

    want = {"global": (None, None), "tropics": (((-20, 20),), None), "extratropics": (((-90, -20), (20, 90)), None),
            "n.hem": (((20, 90),), None), "s.hem": (((-90, -20),), None), "arctic": (((60, 90),), None),
            "antarctic": (((-90, -60),), None), "europe": (((35, 75),), ((-12.5, 42.5),)),
            "n.america": (((25, 60),), ((-120, -75),)), "n.atlantic": (((25, 65),), ((-70, -10),)),
            "n.pacific": (((25, 60),), ((145, -130),)), "e.asia": (((25, 60),), ((102.5, 150),)),
            "ausnz": (((-45, -12.5),), ((120, 175),))}
    assert list(SCORECARD) == list(want)
    for name, (lat, lon) in want.items():
        r = SCORECARD[name]
        assert isinstance(r, Region) and r.lat == lat and r.lon == lon and r.mask is None, name
    # every box holds points of a 33 x 64 grid, n.pacific wraps, and the thirteen go down as two launches
    pred, truth, _, _ = make_inputs("randn", 33, 64)
    s = region_scores(pred, truth, SCORECARD)
    assert s.regions == tuple(want) and (s.count["2t"] > 0).all()
    lat, lon = coords(pred)
    y = yardstick_of(pred, truth, None, {k: (la, lo, None) for k, (la, lo) in want.items()})
    assert_sums_match(s.table[..., :8].numpy(), y, None, "SCORECARD")
    pacific = membership(lat, lon, (*want["n.pacific"], None)).any(axis=0)
    assert pacific[32] and not pacific[0] and not pacific[-1] and 0 < pacific.sum() < 64


def test_device_path_argument_checks_need_no_kernel():
    """What `lib.region_sums` refuses is refused before any launch; the C entry point checks its arguments without a GPU."""
    from aurora_amd.engine import lib

    z, b = torch.zeros(1, 17, 32), torch.zeros(17, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="row_w"):
        lib.region_sums([z], [z], None, b, torch.zeros(32, dtype=torch.uint8), None, 1, torch.ones(17, dtype=torch.float64))
    assert {"aurora_hip_region_scores", "aurora_hip_region_scores_workspace_bytes"} <= set(lib.EXPORTED_SYMBOLS)
    ws = lib.region_scores_workspace_bytes
    assert ws(69, 721, 1440, 8) == 8 * ws(69, 721, 1440, 1) == 8 * lib.scores_workspace_bytes(69, 721, 1440)
    assert ws(69, 721, 1440, 8) == 69 * ws(1, 721, 1440, 8) and ws(1, 130, 1024, 1) == 4 * 64
    assert ws(69, 721, 1440, 0) == 0 and ws(69, 721, 1440, 9) == 0 and ws(0, 721, 1440, 8) == 0
    L = lib.load()
    assert L.aurora_hip_region_scores(None, None, None, 0, 17, 32, None, None, None, 3, None, None, None, None) == 0
    assert L.aurora_hip_region_scores(None, None, None, 4, 17, 32, None, None, None, 3, None, None, None, None) == -1
    assert b"null" in L.aurora_hip_last_error()
    assert L.aurora_hip_region_scores(None, None, None, 4, 17, 32, None, None, None, 9, None, None, None, None) == -1
    assert b"1 to 8 regions" in L.aurora_hip_last_error()
