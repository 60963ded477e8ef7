"""`aurora_amd.scores` on the host: closed forms, the latitude weights, NaN masks, argument errors and the C ABI of the
device path (no GPU needed).

The yardstick `yardstick_sums` is the table of include/aurora_hip.h written out in numpy fp64 here, independently of
`aurora_amd.scores._sums_host` (which is code under test); tests/test_gpu_scores.py compares the kernel with the same
function."""
import ctypes

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, scores
from aurora_amd.batch import BandBatch
from aurora_amd.scores import Scores, _sums_host, latitude_weights
from tests.verification_inputs import cos_weights, every, randn_batch, shifted

GRIDS = ((17, 32), (33, 64))


def yardstick_sums(p, t, c, w) -> np.ndarray:
    """The eight sums of ONE plane (n_lat, n_lon), straight from the table: count, w, w d, w d^2, w |d|, w p' t', w p'^2,
    w t'^2 over the points where every input present is finite; fp64 throughout."""
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    valid = np.isfinite(p) & np.isfinite(t)
    if c is not None:
        c = np.asarray(c, dtype=np.float64)
        valid &= np.isfinite(c)
    W = np.repeat(np.asarray(w, dtype=np.float64)[:, None], p.shape[1], axis=1)[valid]
    d = p[valid] - t[valid]
    out = [float(valid.sum()), W.sum(), (W * d).sum(), (W * d * d).sum(), (W * np.abs(d)).sum(), 0.0, 0.0, 0.0]
    if c is not None:
        pa, ta = p[valid] - c[valid], t[valid] - c[valid]
        out[5:] = [(W * pa * ta).sum(), (W * pa * pa).sum(), (W * ta * ta).sum()]
    return np.array(out)


def test_public_names():
    assert aurora_amd.scores is scores and aurora_amd.Scores is Scores
    assert "scores" in aurora_amd.__all__ and "Scores" in aurora_amd.__all__


@pytest.mark.parametrize("n_lat,n_lon", GRIDS)
@pytest.mark.parametrize("k", (2.5, -0.75))
def test_constant_offset_gives_bias_k_rmse_and_mae_abs_k(n_lat, n_lon, k):
    truth = randn_batch(n_lat, n_lon, offset=280.0, scale=10.0, dtype=torch.float64)
    s = scores(shifted(truth, lambda v: v + k), truth)
    assert isinstance(s, Scores) and s.acc is None
    assert s.rmse["2t"].shape == (2,) and s.rmse["z"].shape == (2, 3) and s.rmse["2t"].dtype == torch.float64
    assert set(s.rmse) == {"2t", "msl", "z"}                      # static variables are not scored
    np.testing.assert_allclose(every(s.bias), k, rtol=1e-12)
    np.testing.assert_allclose(every(s.rmse), abs(k), rtol=1e-12)
    np.testing.assert_allclose(every(s.mae), abs(k), rtol=1e-12)
    assert s.count["z"].dtype == torch.int64 and (every(s.count) == n_lat * n_lon).all()


@pytest.mark.parametrize("n_lat,n_lon", GRIDS)
def test_perfect_forecast_and_mirrored_anomaly(n_lat, n_lon):
    truth, clim = randn_batch(n_lat, n_lon, seed=1), randn_batch(n_lat, n_lon, seed=2)
    s = scores(truth, truth, clim)
    for d in (s.rmse, s.bias, s.mae):
        assert (every(d) == 0).all()
    np.testing.assert_allclose(every(s.acc), 1.0, rtol=1e-14)
    # p' = -t'  <=>  p = 2 c - t (exact in fp64 fields)
    t64, c64 = randn_batch(n_lat, n_lon, seed=1, dtype=torch.float64), randn_batch(n_lat, n_lon, seed=2, dtype=torch.float64)
    mirrored = Batch({k: 2 * c64.surf_vars[k] - v for k, v in t64.surf_vars.items()}, {},
                     {k: 2 * c64.atmos_vars[k] - v for k, v in t64.atmos_vars.items()}, t64.metadata)
    np.testing.assert_allclose(every(scores(mirrored, t64, c64).acc), -1.0, rtol=1e-14)


@pytest.mark.parametrize("n_lat,n_lon", GRIDS)
def test_an_error_on_one_row_weighs_as_that_row(n_lat, n_lon):
    truth = randn_batch(n_lat, n_lon, seed=3)
    w = cos_weights(np.linspace(90, -90, n_lat))
    e = 3.0
    for i in (0, 1, n_lat // 2, n_lat - 2):
        def bump(v, i=i):
            v[..., i, :] += e
            return v
        s = scores(shifted(truth, bump), truth)
        np.testing.assert_allclose(every(s.rmse) ** 2, w[i] * e * e / n_lat, rtol=1e-6, atol=1e-20)   # (fp32 fields: t + e rounds)
        np.testing.assert_allclose(every(s.bias), w[i] * e / n_lat, rtol=1e-6, atol=1e-20)


def test_history_only_the_last_entry_is_scored():
    truth = randn_batch(17, 32, seed=4)
    pred = shifted(truth, lambda v: v)
    pred.surf_vars["2t"][:, 0] += 100.0
    pred.atmos_vars["z"][:, 0] += 100.0
    assert (every(scores(pred, truth).rmse) == 0).all()


def test_only_common_variables_are_scored():
    truth = randn_batch(17, 32, seed=5)
    pred = Batch({"2t": truth.surf_vars["2t"] + 1, "10u": truth.surf_vars["msl"]}, {}, {"z": truth.atmos_vars["z"] + 1,
                 "q": truth.atmos_vars["z"]}, truth.metadata)
    s = scores(pred, truth)
    assert list(s.rmse) == ["2t", "z"]
    with pytest.raises(ValueError, match="in common"):
        scores(Batch({"10u": truth.surf_vars["2t"]}, {}, {}, truth.metadata), truth)


@pytest.mark.parametrize("n_lat", (17, 33, 721))
def test_weights(n_lat):
    lat = np.linspace(90, -90, n_lat)
    w = latitude_weights(lat)
    assert w.dtype == np.float64 and w.shape == (n_lat,)
    np.testing.assert_allclose(w, cos_weights(lat), rtol=1e-14, atol=1e-18)
    assert abs(w.mean() - 1) < 1e-14
    assert 0 <= w[0] < 1e-15 and 0 <= w[-1] < 1e-15 and (w[1:-1] > 0).all()
    np.testing.assert_allclose(w, w[::-1], rtol=1e-12, atol=1e-18)
    assert w.argmax() == n_lat // 2


def test_host_sums_equal_the_yardstick():
    n_lat, n_lon = 33, 61
    g = np.random.default_rng(6)
    p = (101325 + 300 * g.standard_normal((5, n_lat, n_lon))).astype(np.float32)
    t = (p + g.standard_normal(p.shape)).astype(np.float32)
    c = (101325 + 100 * g.standard_normal(p.shape)).astype(np.float32)
    p[1, 3, 4] = np.nan
    t[2, 5:9] = np.inf
    c[3, :, 7] = np.nan
    p[4] = np.nan
    w = cos_weights(np.linspace(90, -90, n_lat))
    for clim in (None, c):
        got = _sums_host(p, t, clim, w)
        want = np.stack([yardstick_sums(p[k], t[k], None if clim is None else clim[k], w) for k in range(5)])
        assert (got[:, 0] == want[:, 0]).all()
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        assert (got[4] == 0).all()


def test_nan_masks():
    n_lat, n_lon = 17, 32
    truth, clim = randn_batch(n_lat, n_lon, seed=7, offset=5.0), randn_batch(n_lat, n_lon, seed=8, offset=5.0)
    pred = shifted(truth, lambda v: v + 1.0)
    full = n_lat * n_lon
    base = scores(pred, truth, clim)

    # NaNs in pred only: 2t of batch element 0 loses 3 points; nothing else changes
    p = shifted(pred, lambda v: v)
    p.surf_vars["2t"][0, -1, 2, 3:6] = float("nan")
    p.surf_vars["2t"][0, 0] = float("nan")                        # (history entry 0 is not scored)
    s = scores(p, truth, clim)
    assert s.count["2t"].tolist() == [full - 3, full] and (every(s.count)[2:] == full).all()
    assert torch.equal(s.table[1:], base.table[1:])
    np.testing.assert_allclose(s.bias["2t"][0], 1.0, rtol=1e-6)

    # NaNs in truth only (a whole row of level 1, batch element 1) and in the climatology only (a column of msl)
    t = shifted(truth, lambda v: v)
    t.atmos_vars["z"][1, -1, 1, 4] = float("nan")
    c = shifted(clim, lambda v: v)
    c.surf_vars["msl"][0, -1, :, 9] = float("inf")
    s = scores(pred, t, c)
    assert s.count["z"].tolist() == [[full] * 3, [full, full - n_lon, full]]
    assert s.count["msl"].tolist() == [full - n_lat, full] and s.count["2t"].tolist() == [full, full]
    want = yardstick_sums(pred.atmos_vars["z"][1, -1, 1].numpy(), t.atmos_vars["z"][1, -1, 1].numpy(),
                          c.atmos_vars["z"][1, -1, 1].numpy(), cos_weights(np.linspace(90, -90, n_lat)))
    np.testing.assert_allclose(s.sums["z"][1, 1].numpy(), want, rtol=1e-12)
    # without the climatology its Inf masks nothing
    assert scores(pred, truth).count["msl"].tolist() == [full, full]

    # a whole-NaN plane: count 0, every score NaN, the other planes as before
    p = shifted(pred, lambda v: v)
    p.atmos_vars["z"][0, -1, 2] = float("nan")
    s = scores(p, truth, clim)
    assert s.count["z"].tolist() == [[full, full, 0], [full] * 3]
    assert (s.sums["z"][0, 2] == 0).all()
    for d in (s.rmse, s.bias, s.mae, s.acc):
        assert torch.isnan(d["z"][0, 2]) and not torch.isnan(d["z"][0, :2]).any() and not torch.isnan(d["2t"]).any()
    keep = torch.ones(s.table.shape[0], dtype=torch.bool)
    keep[4 + 2] = False                                            # planes: 2t x 2, msl x 2, then z (b, level)
    assert torch.equal(s.table[keep], base.table[keep])


def test_zero_anomaly_gives_nan_acc():
    truth = randn_batch(17, 32, seed=9)
    s = scores(truth, truth, truth)
    assert torch.isnan(s.acc["2t"]).all() and (s.rmse["2t"] == 0).all()


def test_cpu_returns_host_scores():
    truth = randn_batch(17, 32, seed=10)
    s = scores(shifted(truth, lambda v: v + 1), truth).cpu()
    assert isinstance(s, Scores) and s.rmse["2t"].device.type == "cpu"


def test_float64_fields_are_scored_on_the_host():
    truth = randn_batch(17, 32, seed=11, dtype=torch.float64, offset=1e5)
    s = scores(shifted(truth, lambda v: v + 1e-3), truth)
    np.testing.assert_allclose(every(s.bias), 1e-3, rtol=1e-6)    # an offset an fp32 field could not hold at 1e5


def test_argument_errors():
    truth = randn_batch(17, 32, seed=12)
    pred = shifted(truth, lambda v: v)
    md = truth.metadata

    def with_md(b, **kw):
        return Batch(b.surf_vars, b.static_vars, b.atmos_vars, Metadata(**{**dict(lat=md.lat, lon=md.lon, time=md.time,
                     atmos_levels=md.atmos_levels), **kw}))

    # the common case: a 721-row truth against a cropped 720-row prediction (here 17 against 16)
    cropped = pred.crop(4)
    assert cropped.spatial_shape == (16, 32)
    with pytest.raises(ValueError, match=r"lat.*truth\.crop\(model\.patch_size\)"):
        scores(cropped, truth)
    assert (every(scores(cropped, truth.crop(4)).rmse) == 0).all()
    with pytest.raises(ValueError, match="lon"):
        scores(pred, randn_batch(17, 16, seed=12))
    with pytest.raises(ValueError, match="lon"):
        scores(pred, with_md(truth, lon=md.lon + 0.5))
    with pytest.raises(ValueError, match="lat"):
        scores(pred, with_md(truth, lat=md.lat * 0.5))
    with pytest.raises(ValueError, match="atmos_levels"):
        scores(pred, with_md(truth, atmos_levels=(100, 500, 900)))
    with pytest.raises(ValueError, match="batch size"):
        scores(pred, randn_batch(17, 32, seed=12, B=3))
    with pytest.raises(ValueError, match="climatology.*atmos_levels"):
        scores(pred, truth, with_md(truth, atmos_levels=(1, 2, 3)))
    with pytest.raises(ValueError, match="climatology has no"):
        scores(pred, truth, Batch({"2t": truth.surf_vars["2t"]}, {}, {}, md))
    # matrix coordinates
    lat2, lon2 = md.lat[:, None].expand(17, 32), md.lon[None, :].expand(17, 32)
    with pytest.raises(ValueError, match="matrices"):
        scores(with_md(pred, lat=lat2, lon=lon2), with_md(truth, lat=lat2, lon=lon2))
    # latitude bands
    band = BandBatch(truth.surf_vars, {}, truth.atmos_vars, md, full_patch_rows=4, band=(0, 4))
    with pytest.raises(ValueError, match="BandBatch"):
        scores(band, truth)
    with pytest.raises(ValueError, match="BandBatch"):
        scores(pred, band)
    # latitudes outside [-90, 90] (Metadata refuses them at construction; a later edit is caught here)
    with pytest.raises(ValueError, match=r"\[-90, 90\]"):
        latitude_weights(np.linspace(95, -90, 17))
    bad = with_md(truth)
    bad.metadata.lat = md.lat * 1.1
    with pytest.raises(ValueError, match=r"\[-90, 90\]"):
        scores(bad, bad)


def test_device_path_argument_checks_need_no_kernel():
    """What `lib.scores_sums` refuses is refused before any launch."""
    from aurora_amd.engine import lib

    with pytest.raises(AssertionError, match="row_w"):
        lib.scores_sums([torch.zeros(1, 17, 32)], [torch.zeros(1, 17, 32)], None, torch.ones(17, dtype=torch.float64))


def test_library_exports_and_workspace_size():
    from aurora_amd.build import build_library
    from aurora_amd.engine import lib

    raw = ctypes.CDLL(str(build_library(force=False, verbose=False)))
    assert hasattr(raw, "aurora_hip_scores") and hasattr(raw, "aurora_hip_scores_workspace_bytes")
    assert {"aurora_hip_scores", "aurora_hip_scores_workspace_bytes"} <= set(lib.EXPORTED_SYMBOLS)
    ws = lib.scores_workspace_bytes
    for args in ((1, 1, 1), (4, 17, 32), (69, 721, 1440), (141, 1801, 3600)):
        assert ws(*args) > 0 and ws(*args) % 64 == 0, args          # whole partials of eight doubles
    sizes = (1, 2, 3, 17, 64, 720, 721, 1440, 3600)
    for a, b in zip(sizes, sizes[1:]):
        assert ws(a, 721, 1440) <= ws(b, 721, 1440) and ws(a, 721, 1440) * b == ws(b, 721, 1440) * a   # linear in planes
        assert ws(69, a, 1440) <= ws(69, b, 1440)
        assert ws(69, 721, a) <= ws(69, 721, b)
    assert ws(69, 721, 1440) < 721 * 1440 * 4                       # far below one plane
    assert ws(0, 721, 1440) == 0 and ws(69, 0, 1440) == 0 and ws(69, 721, -1) == 0
    # the row chunks of a plane do not depend on the number of planes
    assert ws(69, 721, 1440) == 69 * ws(1, 721, 1440)
    # argument errors surface without a GPU; an empty call is a no-op
    L = lib.load()
    assert L.aurora_hip_scores(None, None, None, 0, 17, 32, None, None, None, None) == 0
    assert L.aurora_hip_scores(None, None, None, 4, 17, 32, None, None, None, None) == -1
    assert b"null" in L.aurora_hip_last_error()
    assert L.aurora_hip_scores(None, None, None, 4, 0, 32, None, None, None, None) == -1
