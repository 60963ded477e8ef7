"""`aurora_amd.event_scores` on the host: the definitions, the identities of the contingency table and of the fractions skill
score, argument errors and the C ABI of the device path (no GPU needed).

The yardstick `yardstick_rowsums` is the module text of aurora_amd/events.py written out in plain numpy integers here (window
sums by explicit np.roll over the longitude offsets and zero-padded shifts over the latitude offsets), independently of
`aurora_amd.events._rowsums_host` (code under test, which uses running sums).  It is checked below against a brute-force loop
over every point and window offset and, where SciPy is installed, against scipy.ndimage.uniform_filter.  Everything is an
integer, so every comparison with it is exact; tests/test_gpu_event_scores.py compares the kernel with the same function.

The call needs no workspace (aurora_hip_event_scores_workspace_bytes is 0 for every argument), so "a workspace that is too
short" cannot be constructed; the C-ABI test asserts the 0 instead."""
import ctypes

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, event_scores
from aurora_amd.batch import BandBatch
from aurora_amd.events import EventScores
from aurora_amd.scores import latitude_weights
from tests.verification_inputs import planes_of, quantile_thresholds, red_noise, red_noise_batch


def yardstick_rowsums(p, t, thr, scales, below):
    """ONE plane (n_lat, n_lon) against T thresholds: rowsums (T, S, n_lat, 3) and valid (n_lat,), int64."""
    p, t = np.asarray(p, dtype=np.float32), np.asarray(t, dtype=np.float32)
    n_lat, n_lon = p.shape
    ok = np.isfinite(p) & np.isfinite(t)
    out = np.zeros((len(thr), len(scales), n_lat, 3), dtype=np.int64)
    for ti, th in enumerate(np.asarray(thr, dtype=np.float32)):
        with np.errstate(invalid="ignore"):
            f = (ok & ((p <= th) if below else (p >= th))).astype(np.int64)
            o = (ok & ((t <= th) if below else (t >= th))).astype(np.int64)
        if not f.any() and not o.any():                                 # no event anywhere: every sum stays 0
            continue
        for si, n in enumerate(scales):
            h = n // 2
            counts = []
            for x in (f, o):
                rows = np.zeros_like(x)
                for dj in range(-h, h + 1):
                    rows += np.roll(x, -dj, axis=1)                     # rows[i, j] += x[i, (j + dj) mod n_lon]
                c = np.zeros_like(x)
                for di in range(-h, h + 1):                             # c[i] += rows[i + di], zero outside the grid
                    lo, hi = max(0, -di), min(n_lat, n_lat - di)
                    if lo < hi:
                        c[lo:hi] += rows[lo + di:hi + di]
                counts.append(c)
            cf, co = counts
            out[ti, si, :, 0] = np.where(ok, (cf - co) ** 2, 0).sum(axis=1)
            out[ti, si, :, 1] = np.where(ok, cf ** 2, 0).sum(axis=1)
            out[ti, si, :, 2] = np.where(ok, co ** 2, 0).sum(axis=1)
    return out, ok.sum(axis=1).astype(np.int64)


def brute_rowsums(p, t, th, n, below):
    n_lat, n_lon = p.shape
    h = n // 2
    ok = np.isfinite(p) & np.isfinite(t)
    ev = lambda x, i, j: bool(ok[i, j] and (x[i, j] <= th if below else x[i, j] >= th))  # noqa: E731
    out = np.zeros((n_lat, 3), dtype=np.int64)
    for i in range(n_lat):
        for j in range(n_lon):
            if not ok[i, j]:
                continue
            cf = co = 0
            for di in range(-h, h + 1):
                for dj in range(-h, h + 1):
                    if 0 <= i + di < n_lat:
                        cf += ev(p, i + di, (j + dj) % n_lon)
                        co += ev(t, i + di, (j + dj) % n_lon)
            out[i] += ((cf - co) ** 2, cf ** 2, co ** 2)
    return out


def test_public_names():
    assert aurora_amd.event_scores is event_scores and aurora_amd.EventScores is EventScores
    assert "event_scores" in aurora_amd.__all__ and "EventScores" in aurora_amd.__all__


@pytest.mark.parametrize("n_lat,n_lon,scales", [(5, 7, (1, 3, 5, 7)), (4, 9, (1, 3, 5, 7)), (4, 9, (1, 9))])
@pytest.mark.parametrize("below", (False, True))
def test_the_yardstick_against_a_brute_force_loop(n_lat, n_lon, scales, below):
    p, t = red_noise((n_lat, n_lon), 1), red_noise((n_lat, n_lon), 2)
    p[1, 0], t[2, n_lon - 1], p[3, 3] = np.nan, np.inf, -np.inf
    thr = quantile_thresholds(t, extra=(np.nan,))[[0, 1, 3]]
    got, valid = yardstick_rowsums(p, t, thr, scales, below)
    assert valid.tolist() == (np.isfinite(p) & np.isfinite(t)).sum(axis=1).tolist() and valid.sum() == n_lat * n_lon - 3
    for ti, th in enumerate(thr):
        for si, n in enumerate(scales):
            assert np.array_equal(got[ti, si], brute_rowsums(p, t, th, n, below)), (ti, n)
    assert got[0].any() and not got[2].any()                            # the NaN threshold: no event


def test_the_yardstick_against_scipy_uniform_filter():
    ndimage = pytest.importorskip("scipy.ndimage")
    n_lat, n_lon = 9, 16
    p, t = red_noise((n_lat, n_lon), 3), red_noise((n_lat, n_lon), 4)
    thr = quantile_thresholds(t)[:2]
    scales = (1, 3, 5, 7)
    got, _ = yardstick_rowsums(p, t, thr, scales, False)
    for ti, th in enumerate(thr):
        for si, n in enumerate(scales):
            ff, fo = (ndimage.uniform_filter((x >= th).astype(np.float64), size=n, mode=("constant", "wrap")) for x in (p, t))
            for c, want in enumerate((((ff - fo) ** 2).sum(axis=1), (ff ** 2).sum(axis=1), (fo ** 2).sum(axis=1))):
                assert np.abs(got[ti, si, :, c] / float(n) ** 4 - want).max() <= 1e-12 * n_lon   # |d| <= 1e-12 per fraction


def thresholds_for(pred, truth):
    z = truth.atmos_vars["z"][:, -1].numpy()
    return {"2t": quantile_thresholds(truth.surf_vars["2t"][:, -1].numpy()),
            "z": np.stack([quantile_thresholds(z[:, c])[:2] for c in range(z.shape[1])])}


def assert_equals_yardstick(s: EventScores, pred, truth, thresholds, below=False):
    s = s.cpu()
    tp = {(k, idx): x for k, idx, x in planes_of(truth)}
    n = 0
    for k, idx, x in planes_of(pred):
        if k not in thresholds:
            continue
        thr = np.asarray(thresholds[k], dtype=np.float32)
        thr = thr[idx[1]] if thr.ndim == 2 else thr
        T = s.rowsums[k].shape[-4]
        thr = np.concatenate([thr, np.full(T - len(thr), np.nan, dtype=np.float32)])
        want, valid = yardstick_rowsums(x, tp[(k, idx)], thr, s.scales, below)
        assert np.array_equal(s.rowsums[k][idx].numpy(), want), (k, idx)
        assert np.array_equal(s.valid[k][idx].numpy(), valid), (k, idx)
        n += 1
    assert n == s.rowsums_table.shape[0]


@pytest.mark.parametrize("n_lat,n_lon,scales", [(17, 32, (1, 3, 5)), (9, 45, (45, 3)), (3, 64, (9, 63, 1))])
@pytest.mark.parametrize("below", (False, True))
def test_cpu_event_scores_equal_the_yardstick(n_lat, n_lon, scales, below):
    pred, truth = red_noise_batch(n_lat, n_lon, seed=1), red_noise_batch(n_lat, n_lon, seed=2)
    pred.surf_vars["2t"][0, -1, 1, 0] = float("nan")
    truth.atmos_vars["z"][1, -1, 2, n_lat - 1, n_lon - 1] = float("inf")
    thr = thresholds_for(pred, truth)
    s = event_scores(pred, truth, thr, scales=scales, below=below)
    S = len(set(scales) | {1})
    assert isinstance(s, EventScores) and s.scales == tuple(sorted(set(scales) | {1})) and set(s.fss) == {"2t", "z"}
    assert s.fss["2t"].shape == (2, 3, S) and s.fss["z"].shape == (2, 3, 3, S) and s.fss["z"].dtype == torch.float64
    for prop in ("hits", "misses", "false_alarms", "correct_negatives"):
        assert getattr(s, prop)["z"].shape == (2, 3, 3) and getattr(s, prop)["2t"].dtype == torch.int64
    for prop in ("csi", "pod", "far", "frequency_bias", "ets", "base_rate", "forecast_rate", "fss_uniform"):
        assert getattr(s, prop)["2t"].shape == (2, 3) and getattr(s, prop)["z"].dtype == torch.float64
    assert s.count["z"].shape == (2, 3) and s.rowsums["z"].shape == (2, 3, 3, S, n_lat, 3) and s.valid["2t"].shape == (2, n_lat)
    assert s.count["2t"].tolist() == [n_lat * n_lon - 1, n_lat * n_lon]
    assert torch.isnan(s.fss["z"][..., 2, :]).all() and torch.isnan(s.csi["z"][..., 2]).all()    # the NaN-padded slot
    assert_equals_yardstick(s, pred, truth, thr, below)
    # the scores from the yardstick's integers, in numpy
    w = latitude_weights(pred.metadata.lat.numpy())
    r = s.rowsums["2t"].numpy().astype(np.float64)
    ws = (r * w[:, None]).sum(axis=-2)
    # (absolute: 1 - q with q <= 1 a ratio of two sums of <= n_lat terms, each within n_lat u relative whatever the order of
    #  additions, so q is within (2 n_lat + 2) u <= 8e-15 on either side for n_lat <= 17)
    np.testing.assert_allclose(s.fss["2t"].numpy(), 1 - ws[..., 0] / (ws[..., 1] + ws[..., 2]), rtol=0, atol=2e-14)
    hits = (r[:, :, 0, :, 1] + r[:, :, 0, :, 2] - r[:, :, 0, :, 0]) / 2
    H, F, M = (hits * w).sum(-1), ((r[:, :, 0, :, 1] - hits) * w).sum(-1), ((r[:, :, 0, :, 2] - hits) * w).sum(-1)
    N = (s.valid["2t"].numpy() * w).sum(-1)[:, None]
    R = (H + M) * (H + F) / N
    div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1.0), np.nan)   # noqa: E731  (a zero denominator gives NaN)
    for prop, want in (("csi", div(H, H + M + F)), ("pod", div(H, H + M)), ("far", div(F, H + F)),
                       ("frequency_bias", div(H + F, H + M)), ("ets", div(H - R, H + M + F - R)), ("base_rate", div(H + M, N)),
                       ("forecast_rate", div(H + F, N)), ("fss_uniform", 0.5 + div(H + M, N) / 2)):
        got = getattr(s, prop)["2t"].numpy()
        if prop == "ets":          # H + M + F - R cancels to rounding noise when every point is an event: ill-conditioned there
            fair = np.abs(H + M + F - R) > 1e-9 * N
            got, want = np.where(fair, got, 0.0), np.where(fair, want, 0.0)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14, err_msg=prop)


def test_identities():
    n_lat, n_lon = 17, 32
    pred, truth = red_noise_batch(n_lat, n_lon, seed=3), red_noise_batch(n_lat, n_lon, seed=4)
    x = truth.surf_vars["2t"][:, -1].numpy()
    hi, lo = np.float32(x.max() + 1000), np.float32(min(x.min(), pred.surf_vars["2t"].min().item()) - 1000)
    thr = {"2t": [*quantile_thresholds(x)[:2], hi, lo]}
    scales = (1, 3, 9)
    # pred == truth: FSS 1 wherever there is an event, no miss, no false alarm
    same = event_scores(truth, truth, thr, scales=scales)
    assert (same.fss["2t"][:, [0, 1, 3]] == 1).all() and (same.misses["2t"] == 0).all() and (same.false_alarms["2t"] == 0).all()
    s = event_scores(pred, truth, thr, scales=scales)
    h, m, fa, cn = s.hits["2t"], s.misses["2t"], s.false_alarms["2t"], s.correct_negatives["2t"]
    assert torch.equal(h + m + fa + cn, s.count["2t"][:, None].expand(2, 4)) and (s.count["2t"] == n_lat * n_lon).all()
    # a threshold above every value: no event; below every value: everything is one
    assert torch.isnan(s.fss["2t"][:, 2]).all() and (s.base_rate["2t"][:, 2] == 0).all() and (h[:, 2] == 0).all()
    assert (s.fss["2t"][:, 3] == 1).all() and (s.base_rate["2t"][:, 3] == 1).all() and (cn[:, 3] == 0).all()
    # n = 1 from the unweighted rows: fss = 1 - (FA + miss) / (2 hits + FA + miss), exactly
    r = s.rowsums["2t"][:, :, 0].sum(dim=-2)
    assert torch.equal(r[..., 0], fa + m) and torch.equal(r[..., 1] + r[..., 2], 2 * h + fa + m)
    one = Batch(pred.surf_vars, {}, {}, Metadata(lat=torch.zeros(1, dtype=torch.float64), lon=pred.metadata.lon,
                                                 time=pred.metadata.time, atmos_levels=()))
    crop = lambda b: Batch({"2t": b.surf_vars["2t"][..., 5:6, :]}, {}, {}, one.metadata)  # noqa: E731
    s1 = event_scores(crop(pred), crop(truth), {"2t": thr["2t"][:2]})
    f1, m1, h1 = (x["2t"].double() for x in (s1.false_alarms, s1.misses, s1.hits))
    assert torch.equal(s1.fss["2t"][..., 0], 1 - (f1 + m1) / (2 * h1 + f1 + m1))
    # below = True is the negated problem
    neg = lambda b: Batch({k: -v for k, v in b.surf_vars.items()}, {}, {}, b.metadata)  # noqa: E731
    b = event_scores(pred, truth, thr, scales=scales, below=True)
    n = event_scores(neg(pred), neg(truth), {"2t": [-v for v in thr["2t"]]}, scales=scales)
    assert b.below and not n.below and torch.equal(b.rowsums_table, n.rowsums_table)
    assert torch.equal(b.fss_table.nan_to_num(-1), n.fss_table.nan_to_num(-1))
    # 1 is inserted; a shorter list is padded with NaN and scores NaN
    assert event_scores(pred, truth, thr, scales=(5, 3)).scales == (1, 3, 5) and event_scores(pred, truth, thr).scales == (1,)
    two = event_scores(pred, truth, {"2t": thr["2t"][:1], "msl": thr["2t"][:2]}, scales=(3,))
    assert torch.isnan(two.fss["2t"][:, 1]).all() and torch.isnan(two.pod["2t"][:, 1]).all() and not torch.isnan(two.fss["2t"][:, 0]).any()
    assert (two.hits["2t"][:, 1] == 0).all() and list(two.fss) == ["2t", "msl"]


def test_argument_errors():
    truth, pred = red_noise_batch(17, 32, seed=10), red_noise_batch(17, 32, seed=11)
    md = truth.metadata
    thr = {"2t": [5e4]}
    for bad, word in (((1, 4), "odd"), ((65,), "63"), ((33,), "32 longitudes"), ((3, 3), "distinct"), ((2.5,), "whole"),
                      ((1, 3, 5, 7, 9, 11, 13, 15, 17), "at most 8")):
        with pytest.raises(ValueError, match=f"(?=.*scales).*{word}"):
            event_scores(pred, truth, thr, scales=bad)
    with pytest.raises(ValueError, match="thresholds.*'2t' has 9"):
        event_scores(pred, truth, {"2t": np.arange(9.0)})
    with pytest.raises(ValueError, match="'10u'"):
        event_scores(pred, truth, {"2t": [1.0], "10u": [1.0]})
    del truth.surf_vars["msl"]
    with pytest.raises(ValueError, match="'msl'"):
        event_scores(pred, truth, {"msl": [1.0]})
    with pytest.raises(ValueError, match=r"'z'.*\(2, 2\).*C = 3"):
        event_scores(pred, truth, {"z": np.zeros((2, 2))})
    with pytest.raises(ValueError, match="'2t'.*shape"):
        event_scores(pred, truth, {"2t": np.zeros((2, 2))})
    with pytest.raises(ValueError, match="mapping"):
        event_scores(pred, truth, {})
    band = BandBatch(truth.surf_vars, {}, truth.atmos_vars, md, full_patch_rows=4, band=(0, 4))
    with pytest.raises(ValueError, match="BandBatch"):
        event_scores(pred, band, thr)
    with pytest.raises(ValueError, match=r"lat.*truth\.crop\(model\.patch_size\)"):
        event_scores(pred.crop(4), truth, thr)
    with pytest.raises(ValueError, match="lon"):
        event_scores(pred, red_noise_batch(17, 16, seed=10), thr)
    lat2, lon2 = md.lat[:, None].expand(17, 32), md.lon[None, :].expand(17, 32)
    with pytest.raises(ValueError, match="matrices"):
        event_scores(Batch(pred.surf_vars, {}, pred.atmos_vars, Metadata(lat=lat2, lon=lon2, time=md.time, atmos_levels=md.atmos_levels)),
                     truth, thr)


def test_library_exports_and_argument_errors_surface_without_a_gpu():
    from aurora_amd.build import PKG, build_library
    from aurora_amd.engine import lib

    header = (PKG.parent / "include" / "aurora_hip.h").read_text()
    raw = ctypes.CDLL(str(build_library(force=False, verbose=False)))
    for name in ("aurora_hip_event_scores", "aurora_hip_event_scores_workspace_bytes"):
        assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    for args in ((69, 721, 1440, 3, 5), (1, 1, 1, 1, 1), (2, 70, 4096, 8, 8), (0, 0, 0, 0, 0)):
        assert lib.event_scores_workspace_bytes(*args) == 0               # the call needs no workspace, whatever its sizes
    L = lib.load()
    sc = lambda *n: (ctypes.c_int32 * len(n))(*n)  # noqa: E731
    call = lambda planes, n_lat, n_lon, T, scales, ptr=8: L.aurora_hip_event_scores(  # noqa: E731
        ptr, ptr, planes, n_lat, n_lon, ptr, T, scales, len(scales) if scales is not None else 1, 0, ptr, ptr, None, 0, None)
    err = L.aurora_hip_last_error
    assert call(0, 17, 32, 1, None, None) == 0                            # an empty call is a no-op
    assert call(4, 17, 32, 1, sc(1), None) == -1 and b"null" in err()
    assert call(4, 17, 32, 1, None) == -1 and b"null" in err()
    assert call(4, 17, 32, 1, sc(3, 5)) == -1 and b"scales[0]" in err()
    assert call(4, 17, 32, 1, sc(1, 5, 3)) == -1 and b"ascending" in err()
    assert call(4, 17, 32, 1, sc(1, 3, 3)) == -1 and b"ascending" in err()
    assert call(4, 17, 32, 1, sc(1, 4)) == -1 and b"odd" in err()
    assert call(4, 17, 32, 1, sc(1, 65)) == -1 and b"63" in err()
    assert call(4, 17, 32, 1, sc(1, 33)) == -1 and b"longitudes" in err()
    assert call(4, 17, 32, 9, sc(1)) == -1 and b"n_thresholds" in err()
    assert call(4, 17, 32, 0, sc(1)) == -1 and b"n_thresholds" in err()
    assert call(4, 17, 32, 1, sc(1, 3, 5, 7, 9, 11, 13, 15, 17)) == -1 and b"n_scales" in err()
    assert call(4, 17, 4097, 1, sc(1)) == -1 and b"n_lon" in err()
    assert call(4, 0, 32, 1, sc(1)) == -1 and b"sizes" in err()
    assert call(4, 17, 32, 1, sc(1), 12) == -1 and b"aligned" in err()
