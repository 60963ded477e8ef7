"""`aurora_amd.spectra` on the host: the definitions, Parseval, bands, invalid rows, argument errors and the C ABI of the
device path (no GPU needed).

The yardstick `yardstick_spectra` is the module text of aurora_amd/spectra.py written out in numpy fp64 here (np.fft.rfft,
explicit loops over rows and bands), independently of `aurora_amd.spectra._power_host` (code under test);
tests/test_gpu_spectra.py compares the kernel with the same function, under `spectra_bound` below."""
import ctypes
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, scores, spectra
from aurora_amd.batch import BandBatch
from aurora_amd.spectra import Spectra
from tests.verification_inputs import cos_weights, planes_of, red_noise, red_noise_batch

U = 2.0 ** -53


def ck(N: int) -> np.ndarray:
    c = np.full(N // 2 + 1, 2.0)
    c[0] = 1.0
    if N % 2 == 0:
        c[-1] = 1.0
    return c


def yardstick_spectra(p, t, lat, bands):
    """ONE plane (n_lat, N): power (1 or 3, n_bands, K) and rows (n_bands,), straight from the definitions, fp64."""
    p = np.asarray(p, dtype=np.float64)
    t = None if t is None else np.asarray(t, dtype=np.float64)
    n_lat, N = p.shape
    K = N // 2 + 1
    w = cos_weights(lat) if n_lat > 1 else np.ones(1)
    fields = [p] if t is None else [p, t, None]
    power = np.full((len(fields), len(bands), K), np.nan)
    rows = np.zeros(len(bands), dtype=np.int64)
    for b, (south, north) in enumerate(bands):
        acc, wsum = np.zeros((len(fields), K)), 0.0
        for i in range(n_lat):
            if not (south <= lat[i] <= north):
                continue
            if not (np.isfinite(p[i]).all() and (t is None or np.isfinite(t[i]).all())):
                continue
            rows[b] += 1
            wsum += w[i]
            for f, x in enumerate(fields):
                X = np.fft.rfft(p[i] - t[i] if x is None else x[i])
                acc[f] += w[i] * ck(N) * (X.real ** 2 + X.imag ** 2) / N ** 2
        if rows[b]:
            power[:, b] = acc / wsum
    return power, rows


def spectra_bound(p, t, lat, bands, want):
    """The bound of tests/test_gpu_spectra.py's text on |device - yardstick| for one plane: the shape of `want`."""
    p = np.asarray(p, dtype=np.float64)
    t = None if t is None else np.asarray(t, dtype=np.float64)
    n_lat, N = p.shape
    w = cos_weights(lat) if n_lat > 1 else np.ones(1)
    out = np.zeros_like(want)
    for b, (south, north) in enumerate(bands):
        acc, wsum = np.zeros(want.shape[::2]), 0.0
        for i in range(n_lat):
            if not (south <= lat[i] <= north) or not (np.isfinite(p[i]).all() and (t is None or np.isfinite(t[i]).all())):
                continue
            wsum += w[i]
            Ep = (N + 8) * U * np.abs(p[i]).sum()
            terms = [(np.abs(np.fft.rfft(p[i])), Ep)]
            if t is not None:
                Et = (N + 8) * U * np.abs(t[i]).sum()
                terms += [(np.abs(np.fft.rfft(t[i])), Et), (np.abs(np.fft.rfft(p[i] - t[i])), Ep + Et)]
            for f, (X, E) in enumerate(terms):
                acc[f] += w[i] * ck(N) * (2 * X * E + E * E) / N ** 2
        if wsum:
            out[:, b] = acc / wsum + (n_lat + 4) * U * want[:, b]
    return out


def assert_matches_yardstick(s: Spectra, pred: Batch, truth, bands, rel=1e-12):
    s = s.cpu()
    lat = pred.metadata.lat.double().cpu().numpy()
    tp = None if truth is None else {(k, idx): x for k, idx, x in planes_of(truth)}
    n = 0
    for k, idx, x in planes_of(pred):
        want, rows = yardstick_spectra(x, None if tp is None else tp[(k, idx)], lat, bands)
        got = [s.power[k][idx].numpy()] + ([] if tp is None else [s.truth_power[k][idx].numpy(), s.error_power[k][idx].numpy()])
        assert s.rows[k][idx].tolist() == rows.tolist(), (k, idx)
        for f, g in enumerate(got):
            assert g.shape == want[f].shape
            assert np.array_equal(np.isnan(g), np.isnan(want[f])), (k, idx, f)
            scale = np.nanmax(np.abs(want[f])) if np.isfinite(want[f]).any() else 0.0
            assert np.nanmax(np.abs(g - want[f]), initial=0.0) <= rel * scale, (k, idx, f)
        n += 1
    assert n == s.table.shape[0]


def test_public_names():
    assert aurora_amd.spectra is spectra and aurora_amd.Spectra is Spectra
    assert "spectra" in aurora_amd.__all__ and "Spectra" in aurora_amd.__all__


@pytest.mark.parametrize("N", (12, 45))
def test_the_yardstick_against_a_direct_long_double_transform(N):
    """The yardstick's own error is far inside the bound of the GPU test: an FFT's error grows like u log2(N) |x|, the
    bound like u (N + 8) sum|x|, so even at N = 12 (log2 N / (N + 8) = 0.18, times the FFT's small constant) it must stay under
    a tenth of it."""
    n_lat = 5
    lat = np.linspace(60, -60, n_lat)
    p, t = red_noise((n_lat, N), 1), red_noise((n_lat, N), 2)
    bands = ((-90, 90), (0, 90))
    want, _ = yardstick_spectra(p, t, lat, bands)
    n = np.arange(N, dtype=np.longdouble)
    k = np.arange(N // 2 + 1, dtype=np.longdouble)
    pi = np.longdouble("3.14159265358979323846264338327950288")
    ang = -2 * pi * np.outer(k, n) / N
    C, S = np.cos(ang), np.sin(ang)
    w = cos_weights(lat).astype(np.longdouble)
    exact = np.zeros(want.shape, dtype=np.longdouble)
    for b, (south, north) in enumerate(bands):
        m = (lat >= south) & (lat <= north)
        for f, x in enumerate((p.astype(np.longdouble), t.astype(np.longdouble), p.astype(np.longdouble) - t.astype(np.longdouble))):
            P = ((x @ C.T) ** 2 + (x @ S.T) ** 2) * ck(N) / np.longdouble(N) ** 2
            exact[f, b] = (w[m, None] * P[m]).sum(axis=0) / w[m].sum()
    bound = spectra_bound(p, t, lat, bands, want)
    assert (np.abs(want - exact) <= 0.1 * bound).all()


@pytest.mark.parametrize("n_lat,n_lon", [(17, 32), (9, 45), (33, 64)])
@pytest.mark.parametrize("with_truth", (False, True))
def test_cpu_spectra_equal_the_yardstick(n_lat, n_lon, with_truth):
    pred, truth = red_noise_batch(n_lat, n_lon, seed=1), red_noise_batch(n_lat, n_lon, seed=2)
    bands = ((-90, 90), (-30, 30), (20, 90))
    s = spectra(pred, truth if with_truth else None, bands=bands)
    K = n_lon // 2 + 1
    assert isinstance(s, Spectra) and s.power["2t"].shape == (2, 3, K) and s.power["z"].shape == (2, 3, 3, K)
    assert s.power["2t"].dtype == torch.float64 and s.rows["z"].dtype == torch.int64 and s.rows["z"].shape == (2, 3, 3)
    assert s.wavenumber.tolist() == list(range(K)) and set(s.power) == {"2t", "msl", "z"}
    assert (s.truth_power is None) == (not with_truth) and (s.error_power is None) == (not with_truth)
    assert (s.ratio is None) == (not with_truth)
    if with_truth:
        np.testing.assert_allclose(s.ratio["z"].numpy(), (s.power["z"] / s.truth_power["z"]).numpy(), rtol=1e-15)
    assert_matches_yardstick(s, pred, truth if with_truth else None, bands)
    assert spectra(pred).power["2t"].shape == (2, 1, K)                  # the default band: the whole sphere


@pytest.mark.parametrize("n_lon", (32, 45, 1440))
def test_parseval_and_the_error_spectrum_adds_up_to_rmse_squared(n_lon):
    n_lat = 17
    pred, truth = red_noise_batch(n_lat, n_lon, seed=3, mean=280.0), red_noise_batch(n_lat, n_lon, seed=4, mean=281.0)
    s = spectra(pred, truth)
    sc = scores(pred, truth)
    w = cos_weights(np.linspace(90, -90, n_lat))[:, None]
    for k, idx, x in planes_of(pred):
        x = x.astype(np.float64)
        np.testing.assert_allclose(s.power[k][idx][0].sum().item(), (w * x * x).sum() / (w.sum() * n_lon), rtol=1e-12)
        np.testing.assert_allclose(s.error_power[k][idx][0].sum().item(), sc.rmse[k][idx].item() ** 2, rtol=1e-12)


@pytest.mark.parametrize("n_lon", (32, 45))
def test_a_pure_cosine_has_one_bin(n_lon):
    n_lat = 5
    x = 3.0 * np.cos(2 * np.pi * 5 * np.arange(n_lon) / n_lon)
    f = torch.from_numpy(np.broadcast_to(x, (1, 1, n_lat, n_lon)).copy())
    md = Metadata(lat=torch.linspace(60, -60, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1, dtype=torch.float64)[:-1],
                  time=(datetime(2023, 1, 1, 6),), atmos_levels=())
    p = spectra(Batch({"2t": f}, {}, {}, md)).power["2t"][0, 0].numpy()
    np.testing.assert_allclose(p[5], 4.5, rtol=1e-12)                    # amplitude^2 / 2
    assert (np.delete(p, 5) < 1e-25).all()


def test_bands_an_empty_one_and_a_single_row():
    n_lat, n_lon = 17, 32
    pred = red_noise_batch(n_lat, n_lon, seed=5)
    lat = np.linspace(90, -90, n_lat)
    bands = ((-90, 90), (1.0, 2.0), (lat[3], lat[3]), (-90, 0), (0, 0), (-11.25, 33.75), (89, 90), (-90, -90))
    s = spectra(pred, bands=bands)
    assert s.rows["2t"][0].tolist() == [17, 0, 1, 9, 1, 5, 1, 1]
    assert torch.isnan(s.power["2t"][:, 1]).all() and not torch.isnan(s.power["2t"][:, [0, 2, 3, 4, 5, 6, 7]]).any()
    assert_matches_yardstick(s, pred, None, bands)
    x = pred.surf_vars["2t"][1, -1, 3].double().numpy()
    X = np.fft.rfft(x)
    np.testing.assert_allclose(s.power["2t"][1, 2].numpy(), ck(n_lon) * np.abs(X) ** 2 / n_lon ** 2, rtol=1e-12)


def test_invalid_rows_are_left_out_and_counted():
    n_lat, n_lon = 17, 32
    pred, truth = red_noise_batch(n_lat, n_lon, seed=6), red_noise_batch(n_lat, n_lon, seed=7)
    bands = ((-90, 90), (0, 90), (-90, -1), (1.0, 2.0))
    base = spectra(pred, truth, bands=bands)
    pred.surf_vars["2t"][0, -1, 2, 7] = float("nan")                     # northern rows of 2t, batch element 0
    truth.surf_vars["2t"][0, -1, 4, :3] = float("inf")
    pred.surf_vars["2t"][0, 0] = float("nan")                            # (history entry 0 is not taken)
    truth.atmos_vars["z"][1, -1, 1, 15] = float("-inf")                  # a southern row of one level
    s = spectra(pred, truth, bands=bands)
    assert s.rows["2t"].tolist() == [[15, 7, 8, 0], [17, 9, 8, 0]]      # every band but the empty one keeps > half its rows
    assert s.rows["z"][1].tolist() == [[17, 9, 8, 0], [16, 9, 7, 0], [17, 9, 8, 0]]
    assert s.rows["msl"].tolist() == base.rows["msl"].tolist()
    assert_matches_yardstick(s, pred, truth, bands)
    # the rows that were left out do not change the bands they are not in, nor any other plane
    assert torch.equal(s.table[0, :, 2], base.table[0, :, 2]) and torch.equal(s.table[1:4, :, :3], base.table[1:4, :, :3])
    assert not torch.equal(s.table[0, :, 1], base.table[0, :, 1])
    z11 = 4 + 3 + 1                                                      # planes: 2t x 2, msl x 2, then z (b, level)
    assert torch.equal(s.table[z11, :, 1], base.table[z11, :, 1]) and not torch.equal(s.table[z11, :, 2], base.table[z11, :, 2])
    # without the truth its Inf masks nothing
    assert spectra(pred, bands=bands).rows["2t"].tolist() == [[16, 8, 8, 0], [17, 9, 8, 0]]


def test_float64_fields_and_common_variables():
    pred = red_noise_batch(9, 16, seed=8, dtype=torch.float64)
    truth = red_noise_batch(9, 16, seed=9, dtype=torch.float64)
    del truth.surf_vars["msl"]
    s = spectra(pred, truth)
    assert list(s.power) == ["2t", "z"]
    assert_matches_yardstick(s, Batch({"2t": pred.surf_vars["2t"]}, {}, pred.atmos_vars, pred.metadata), truth, ((-90, 90),))
    assert s.cpu().power["2t"].device.type == "cpu"


def test_argument_errors():
    truth = red_noise_batch(17, 32, seed=10)
    pred = red_noise_batch(17, 32, seed=11)
    md = truth.metadata

    def with_md(b, **kw):
        return Batch(b.surf_vars, b.static_vars, b.atmos_vars, Metadata(**{**dict(lat=md.lat, lon=md.lon, time=md.time,
                     atmos_levels=md.atmos_levels), **kw}))

    # bands
    for bad in ((), tuple((-90, 90) for _ in range(9)), ((10, 5),), ((-91, 0),), ((0, 90.5),), ((float("nan"), 10),), (5,)):
        with pytest.raises(ValueError, match="band"):
            spectra(pred, bands=bad)
    # longitudes: regional, unequally spaced, too few
    with pytest.raises(ValueError, match="full circle"):
        spectra(with_md(pred, lon=md.lon * 0.5))
    lon = md.lon.clone()
    lon[5] += 0.01
    with pytest.raises(ValueError, match="equally spaced"):
        spectra(with_md(pred, lon=lon))
    one = Batch({"2t": pred.surf_vars["2t"][..., :1]}, {}, {}, Metadata(lat=md.lat, lon=md.lon[:1], time=md.time, atmos_levels=()))
    with pytest.raises(ValueError, match="longitudes"):
        spectra(one)
    n = 4098
    wide = Batch({"2t": torch.zeros(1, 1, 2, n)}, {}, {}, Metadata(lat=torch.tensor([10.0, -10.0], dtype=torch.float64),
                 lon=torch.linspace(0, 360, n + 1, dtype=torch.float64)[:-1], time=md.time[:1], atmos_levels=()))
    with pytest.raises(ValueError, match="4096"):
        spectra(wide)
    # the grid checks of scores
    with pytest.raises(ValueError, match=r"lat.*truth\.crop\(model\.patch_size\)"):
        spectra(pred.crop(4), truth)
    with pytest.raises(ValueError, match="lon"):
        spectra(pred, red_noise_batch(17, 16, seed=10))
    with pytest.raises(ValueError, match="atmos_levels"):
        spectra(pred, with_md(truth, atmos_levels=(100, 500, 900)))
    with pytest.raises(ValueError, match="batch size"):
        spectra(pred, red_noise_batch(17, 32, seed=10, B=3))
    with pytest.raises(ValueError, match="in common"):
        spectra(Batch({"10u": truth.surf_vars["2t"]}, {}, {}, md), truth)
    lat2, lon2 = md.lat[:, None].expand(17, 32), md.lon[None, :].expand(17, 32)
    with pytest.raises(ValueError, match="matrices"):
        spectra(with_md(pred, lat=lat2, lon=lon2))
    band = BandBatch(truth.surf_vars, {}, truth.atmos_vars, md, full_patch_rows=4, band=(0, 4))
    with pytest.raises(ValueError, match="BandBatch"):
        spectra(band)
    with pytest.raises(ValueError, match="BandBatch"):
        spectra(pred, band)


def test_device_path_argument_checks_need_no_kernel():
    from aurora_amd.engine import lib

    with pytest.raises(AssertionError, match="band_w"):
        lib.spectra_power([torch.zeros(1, 17, 32)], None, torch.ones(1, 17, dtype=torch.float64))


def test_library_exports_and_workspace_size():
    from aurora_amd.build import build_library
    from aurora_amd.engine import lib

    header = (build_library.__globals__["PKG"].parent / "include" / "aurora_hip.h").read_text()
    raw = ctypes.CDLL(str(build_library(force=False, verbose=False)))
    for name in ("aurora_hip_spectra", "aurora_hip_spectra_workspace_bytes"):
        assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    ws = lib.spectra_workspace_bytes
    # n_planes x ceil(n_lat / 32) x (F n_bands K + 2 n_bands) doubles, as the header states
    for n, n_lat, n_lon, nb, tr in ((1, 1, 2, 1, False), (4, 17, 32, 3, True), (69, 721, 1440, 1, True), (69, 721, 1440, 8, False),
                                    (2, 1801, 3600, 2, True), (1, 33, 4096, 8, True)):
        assert ws(n, n_lat, n_lon, nb, tr) == n * -(-n_lat // 32) * ((3 if tr else 1) * nb * (n_lon // 2 + 1) + 2 * nb) * 8
    assert ws(69, 721, 1440, 1, True) == 69 * ws(1, 721, 1440, 1, True)  # the tree of a plane does not depend on the others
    for args in ((0, 721, 1440, 1, 0), (1, 0, 1440, 1, 0), (1, 721, 1, 1, 0), (1, 721, 4097, 1, 0), (1, 721, 1440, 0, 0),
                 (1, 721, 1440, 9, 0)):
        assert ws(*args) == 0, args
    # argument errors surface without a GPU; an empty call is a no-op
    L = lib.load()
    assert L.aurora_hip_spectra(None, None, 0, 17, 32, 1, None, None, None, None, None, 0, None) == 0
    assert L.aurora_hip_spectra(None, None, 4, 17, 32, 1, None, None, None, None, None, 0, None) == -1
    assert b"null" in L.aurora_hip_last_error()
    assert L.aurora_hip_spectra(None, None, 4, 17, 1, 1, None, None, None, None, None, 0, None) == -1
    assert b"n_lon" in L.aurora_hip_last_error()
    assert L.aurora_hip_spectra(None, None, 4, 17, 32, 9, None, None, None, None, None, 0, None) == -1
    assert b"n_bands" in L.aurora_hip_last_error()
    assert L.aurora_hip_spectra(8, None, 4, 17, 32, 1, 8, 8, 8, 8, 8, 16, None) == -1
    assert b"workspace" in L.aurora_hip_last_error()
