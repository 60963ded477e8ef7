"""`aurora_amd.probability_scores` on the host: the definitions, the identities of the Brier decomposition and of the ROC curve,
the ties to `event_scores` and `ensemble_scores`, argument errors and the C ABI of the device path (no GPU needed).

The yardstick `yardstick_rows` is the module text of aurora_amd/probability.py written out in plain numpy here (one boolean
mask per (o, k) bin, summed along the row), independently of `aurora_amd.probability._rows_host` (code under test, which uses
one bincount per plane and threshold).  It is checked below against a brute-force loop over every point.  Everything is an
integer, so every comparison with it is exact; tests/test_gpu_probability_scores.py compares the kernel with the same function.

Inputs: truth y = `red_noise`, members x_m = fp32(y + red_noise(seed 1000 + m, mean 0, amp 250)); thresholds are the 0.5 / 0.9 /
0.99 quantiles of y, one value above the maximum and (by padding) NaN.  `assert_not_trivial` asserts on each input that, at
the median threshold, both corner bins (o = 0, k = 0) and (o = 1, k = M) and at least half of the interior bins 0 < k < M hold
points, so that no table test passes on a table that exercises one bin."""
import ctypes

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, ensemble_scores, event_scores, probability_scores
from aurora_amd.batch import BandBatch
from aurora_amd.probability import ProbabilityScores
from aurora_amd.scores import latitude_weights
from tests.verification_inputs import planes_of, quantile_thresholds, red_noise, red_noise_batch


def yardstick_rows(x, y, thr, below):
    """ONE plane: members x (M, n_lat, n_lon), truth y (n_lat, n_lon), T thresholds -> (n_lat, T, 2, M + 1) int64."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    M, n_lat = x.shape[0], y.shape[0]
    ok = np.isfinite(y) & np.isfinite(x).all(axis=0)
    out = np.zeros((n_lat, len(thr), 2, M + 1), dtype=np.int64)
    for t, th in enumerate(np.asarray(thr, dtype=np.float32)):
        with np.errstate(invalid="ignore"):
            k = ((x <= th) if below else (x >= th)).sum(axis=0)
            o = (y <= th) if below else (y >= th)
        for oo in (0, 1):
            for kk in range(M + 1):
                out[:, t, oo, kk] = (ok & (o == bool(oo)) & (k == kk)).sum(axis=1)
    return out


def brute_rows(x, y, th, below):
    M, n_lat, n_lon = x.shape
    out = np.zeros((n_lat, 2, M + 1), dtype=np.int64)
    for i in range(n_lat):
        for j in range(n_lon):
            if not (np.isfinite(y[i, j]) and all(np.isfinite(x[m, i, j]) for m in range(M))):
                continue
            ev = lambda v: bool(v <= th if below else v >= th)  # noqa: E731
            out[i, int(ev(y[i, j])), sum(ev(x[m, i, j]) for m in range(M))] += 1
    return out


def perturbed(y: np.ndarray, m: int, salt: int = 0) -> np.ndarray:
    """Member m of truth y: fp32(y + red noise of mean 0 and amplitude 250)."""
    if y.shape[-1] == 1:                                                # (red noise needs a wavenumber: a column of its own)
        return (y + 250 * np.random.default_rng(1000 + m + salt).standard_normal(y.shape)).astype(np.float32)
    return (y + red_noise(y.shape, 1000 + m + salt, mean=0, amp=250)).astype(np.float32)


def make_ensemble(n_lat, n_lon, M, seed=0, B=2):
    """(M member batches, truth) in the form of `make_batch`."""
    truth = red_noise_batch(n_lat, n_lon, seed=seed, B=B)
    members = []
    for m in range(M):
        f = lambda d, s: {k: torch.from_numpy(perturbed(v.numpy(), m, 100 * (s + i))) for i, (k, v) in enumerate(d.items())}  # noqa: E731
        members.append(Batch(f(truth.surf_vars, 0), truth.static_vars, f(truth.atmos_vars, 5), truth.metadata))
    return members, truth


def assert_not_trivial(table, M):
    """table (..., n_lat, T, 2, M + 1) with the median threshold at t = 0: see the module's text."""
    c = np.asarray(table).reshape(-1, *np.shape(table)[-3:])[:, 0].sum(axis=0)      # (2, M + 1)
    assert c[0, 0] > 0 and c[1, M] > 0, c
    assert 2 * int(((c[0, 1:M] + c[1, 1:M]) > 0).sum()) >= M - 1, c


def thresholds_for(truth):
    z = truth.atmos_vars["z"][:, -1].numpy()
    x = truth.surf_vars["2t"][:, -1].numpy()
    return {"2t": quantile_thresholds(x, extra=(x.max() + 1000,)),
            "z": np.stack([quantile_thresholds(z[:, c])[:2] for c in range(z.shape[1])])}


def assert_equals_yardstick(s: ProbabilityScores, members, truth, thresholds, below=False):
    s = s.cpu()
    mp = [{(k, idx): x for k, idx, x in planes_of(b)} for b in members]
    n = 0
    for k, idx, y in planes_of(truth):
        if k not in thresholds:
            continue
        thr = np.asarray(thresholds[k], dtype=np.float32)
        thr = thr[idx[1]] if thr.ndim == 2 else thr
        T = s.rows[k].shape[-3]
        thr = np.concatenate([thr, np.full(T - len(thr), np.nan, dtype=np.float32)])
        want = yardstick_rows(np.stack([p[(k, idx)] for p in mp]), y, thr, below)
        assert s.rows[k].dtype == torch.int32 and np.array_equal(s.rows[k][idx].numpy(), want), (k, idx)
        n += 1
    assert n == s.rows_table.shape[0]


FLOAT_PROPS = ("brier", "fair_brier", "brier_skill", "reliability", "resolution", "uncertainty", "base_rate", "roc_area")


def test_public_names():
    assert aurora_amd.probability_scores is probability_scores and aurora_amd.ProbabilityScores is ProbabilityScores
    assert "probability_scores" in aurora_amd.__all__ and "ProbabilityScores" in aurora_amd.__all__


@pytest.mark.parametrize("n_lat,n_lon", [(5, 7), (4, 9)])
@pytest.mark.parametrize("below", (False, True))
def test_the_yardstick_against_a_brute_force_loop(n_lat, n_lon, below):
    M = 3
    y = red_noise((n_lat, n_lon), 1)
    x = np.stack([perturbed(y, m) for m in range(M)])
    x[0, 1, 0], y[2, n_lon - 1], x[2, 3, 3] = np.nan, np.inf, -np.inf
    thr = quantile_thresholds(y, extra=(np.nan,))[[0, 1, 3]]
    got = yardstick_rows(x, y, thr, below)
    assert got.sum(axis=(2, 3)).tolist() == [[n_lon - (i in (1, 2, 3))] * 3 for i in range(n_lat)]
    for t, th in enumerate(thr):
        assert np.array_equal(got[:, t], brute_rows(x, y, th, below)), t
    assert got[:, 2, 0, 0].sum() == n_lat * n_lon - 3 and got[:, 2].sum() == n_lat * n_lon - 3     # the NaN threshold: k = 0, o = 0
    assert (got[:, 0, :, 1:M].sum() > 0) and got[:, 0, 0, 0].sum() > 0 and got[:, 0, 1, M].sum() > 0


@pytest.mark.parametrize("n_lat,n_lon,M", [(17, 32, 5), (9, 45, 2), (33, 90, 16)])
@pytest.mark.parametrize("below", (False, True))
def test_cpu_probability_scores_equal_the_yardstick_and_keep_the_identities(n_lat, n_lon, M, below):
    members, truth = make_ensemble(n_lat, n_lon, M, seed=1)
    members[0].surf_vars["2t"][0, -1, 1, 0] = float("nan")
    truth.atmos_vars["z"][1, -1, 2, n_lat - 1, n_lon - 1] = float("inf")
    thr = thresholds_for(truth)
    s = probability_scores(members, truth, thr, below=below)
    assert isinstance(s, ProbabilityScores) and s.members == M and s.below is below and set(s.brier) == {"2t", "z"}
    T = 4
    for prop in FLOAT_PROPS:
        v = getattr(s, prop)
        assert v["2t"].shape == (2, T) and v["z"].shape == (2, 3, T) and v["z"].dtype == torch.float64, prop
    for prop, last in (("observed_frequency", M + 1), ("forecast_weight", M + 1), ("hit_rate", M + 2), ("false_alarm_rate", M + 2)):
        v = getattr(s, prop)
        assert v["2t"].shape == (2, T, last) and v["z"].shape == (2, 3, T, last) and v["2t"].dtype == torch.float64, prop
    assert s.counts["z"].shape == (2, 3, T, 2, M + 1) and s.counts["2t"].dtype == torch.int64
    assert s.rows["z"].shape == (2, 3, n_lat, T, 2, M + 1) and s.rows["2t"].shape == (2, n_lat, T, 2, M + 1)
    assert s.count["z"].shape == (2, 3) and s.count["2t"].dtype == torch.int64
    assert s.count["2t"].tolist() == [n_lat * n_lon - 1, n_lat * n_lon] and s.count["z"][1, 2] == n_lat * n_lon - 1
    assert torch.equal(s.forecast_probability, torch.arange(M + 1, dtype=torch.float64) / M)
    assert_equals_yardstick(s, members, truth, thr, below)
    assert_not_trivial(s.rows["2t"].numpy(), M)
    assert_not_trivial(s.rows["z"].numpy(), M)
    # z has two thresholds: slots 2 and 3 are padded, every score of them is NaN and their points sit in bin (0, 0)
    for prop in FLOAT_PROPS + ("observed_frequency", "forecast_weight", "hit_rate", "false_alarm_rate"):
        v = getattr(s, prop)["z"]
        assert torch.isnan(v[:, :, 2:]).all() and not torch.isnan(v[:, :, :2]).all(), prop
    assert torch.equal(s.counts["z"][:, :, 2:, 0, 0], s.count["z"][..., None].expand(2, 3, 2))
    # the threshold above every value (below: every value is an event): no skill can be defined, the rest is finite
    top = 3
    assert torch.isnan(s.brier_skill["2t"][:, top]).all() and torch.isnan(s.roc_area["2t"][:, top]).all()
    assert (s.base_rate["2t"][:, top] == (1.0 if below else 0.0)).all() and (s.uncertainty["2t"][:, top] == 0).all()
    for k in ("2t", "z"):
        rows, counts = s.rows[k].to(torch.int64), s.counts[k]
        live = slice(0, 3) if k == "2t" else slice(0, 2)
        # bins of a row sum to its valid count; counts are the rows summed
        per_row = rows.sum(dim=(-1, -2))
        assert torch.equal(per_row, per_row[..., :1].expand_as(per_row)) and torch.equal(per_row[..., 0].sum(-1), s.count[k])
        assert torch.equal(counts, rows.sum(dim=-4))
        # brier = reliability - resolution + uncertainty: each side a sum of at most 2 (M + 1) non-negative terms totalling
        # <= 1, each formed with a handful of roundings
        b = s.brier[k][..., live]
        parts = s.reliability[k][..., live] - s.resolution[k][..., live] + s.uncertainty[k][..., live]
        assert (b - parts).abs().max().item() <= 32 * (M + 1) * 2.0 ** -52
        assert (s.fair_brier[k][..., live] <= b).all() and (b >= 0).all() and (b <= 1).all()
        assert (s.reliability[k][..., live] >= 0).all() and (s.resolution[k][..., live] >= 0).all()
        # ROC: monotone from (0, 0) to (1, 1)
        for rate in (s.hit_rate[k][..., :3 if k == "2t" else 2, :], s.false_alarm_rate[k][..., :3 if k == "2t" else 2, :]):
            assert (rate[..., 0] == 0).all() and (rate[..., -1] == 1).all() and (rate.diff(dim=-1) >= 0).all()
        area = s.roc_area[k][..., live]
        assert (area > 0.5).all() and (area <= 1).all()                  # members = truth + noise: better than chance
        # forecast_weight sums to 1; observed frequency is a frequency
        fw = s.forecast_weight[k][..., live, :]
        assert (fw.sum(-1) - 1).abs().max().item() <= 4 * (M + 1) * 2.0 ** -52
        of = s.observed_frequency[k][..., live, :]
        assert ((of >= 0) & (of <= 1) | torch.isnan(of)).all() and torch.equal(torch.isnan(of), fw == 0)
    # the scores from the yardstick's integers, in numpy fp64 (any order of addition: relative 1e-12 is generous)
    w = latitude_weights(truth.metadata.lat.numpy())
    W = (s.rows["2t"].numpy().astype(np.float64) * w[:, None, None, None]).sum(axis=1)[:, :3]      # (B, 3, 2, M + 1)
    n_k, N, p = W.sum(axis=2), W.sum(axis=(2, 3)), np.arange(M + 1) / M
    obar = W[:, :, 1].sum(-1) / N
    brier = (W[:, :, 1] * (1 - p) ** 2 + W[:, :, 0] * p ** 2).sum(-1) / N
    np.testing.assert_allclose(s.brier["2t"][:, :3].numpy(), brier, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(s.base_rate["2t"][:, :3].numpy(), obar, rtol=1e-12)
    np.testing.assert_allclose(s.brier_skill["2t"][:, :3].numpy(), 1 - brier / (obar * (1 - obar)), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(s.fair_brier["2t"][:, :3].numpy(),
                               brier - (n_k * (np.arange(M + 1) * (M - np.arange(M + 1)))).sum(-1) / (M * M * (M - 1)) / N,
                               rtol=1e-12, atol=1e-15)
    H = np.concatenate([np.zeros((2, 3, 1)), np.cumsum(W[:, :, 1, ::-1], axis=-1)], axis=-1) / W[:, :, 1].sum(-1)[..., None]
    F = np.concatenate([np.zeros((2, 3, 1)), np.cumsum(W[:, :, 0, ::-1], axis=-1)], axis=-1) / W[:, :, 0].sum(-1)[..., None]
    np.testing.assert_allclose(s.hit_rate["2t"][:, :3].numpy(), H, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(s.false_alarm_rate["2t"][:, :3].numpy(), F, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(s.roc_area["2t"][:, :3].numpy(), ((F[..., 1:] - F[..., :-1]) * (H[..., 1:] + H[..., :-1]) / 2).sum(-1),
                               rtol=1e-12)


def test_a_perfect_ensemble():
    _, truth = make_ensemble(17, 32, 2, seed=2)
    thr = {"2t": thresholds_for(truth)["2t"][:3]}
    s = probability_scores([truth] * 4, truth, thr)
    assert (s.brier["2t"] == 0).all() and (s.roc_area["2t"] == 1).all() and (s.reliability["2t"] == 0).all()
    assert (s.brier_skill["2t"] == 1).all() and (s.uncertainty["2t"] > 0).all()
    assert (s.counts["2t"][..., 0, 1:] == 0).all() and (s.counts["2t"][..., 1, :4] == 0).all()


def test_identical_members_give_the_contingency_table_of_event_scores():
    members, truth = make_ensemble(17, 32, 2, seed=3)
    pred = members[0]
    pred.surf_vars["2t"][1, -1, 5, 5] = float("nan")
    thr = {"2t": thresholds_for(truth)["2t"], "z": [5e4, 5e4 + 100]}
    for M, below in ((3, False), (6, True)):
        s, e = probability_scores([pred] * M, truth, thr, below=below), event_scores(pred, truth, thr, below=below)
        for k in ("2t", "z"):
            c = s.counts[k]
            assert torch.equal(c[..., 1, M], e.hits[k]) and torch.equal(c[..., 0, M], e.false_alarms[k])
            assert torch.equal(c[..., 1, 0], e.misses[k]) and torch.equal(c[..., 0, 0], e.correct_negatives[k])
            assert (c[..., 1:M] == 0).all() and e.hits[k].sum() > 0 and e.misses[k].sum() > 0 and e.false_alarms[k].sum() > 0
            assert np.array_equal(s.base_rate[k].numpy(), e.base_rate[k].numpy(), equal_nan=True)       # bit for bit
            assert torch.equal(s.count[k], e.count[k])


def test_count_is_the_count_of_ensemble_scores():
    members, truth = make_ensemble(9, 45, 5, seed=4)
    members[4].atmos_vars["z"][0, -1, 1, 3, 3] = float("inf")
    truth.surf_vars["msl"][1, -1, 0, :] = float("nan")
    s, e = probability_scores(members, truth, {"2t": [5e4], "msl": [5e4], "z": [5e4]}), ensemble_scores(members, truth)
    for k in ("2t", "msl", "z"):
        assert torch.equal(s.count[k], e.count[k])
    assert s.count["msl"].tolist() == [9 * 45, 8 * 45] and s.count["z"][0, 1] == 9 * 45 - 1


def assert_same_scores(a: ProbabilityScores, b: ProbabilityScores):
    assert a.members == b.members and a.below == b.below and a.layout == b.layout
    for f in ("rows_table", "counts_table", "forecast_probability"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    for f in ("scores_table", "bins_table", "roc_table"):                # float64, NaN matching NaN: equal, not close
        assert np.array_equal(getattr(a, f).numpy(), getattr(b, f).numpy(), equal_nan=True), f


def test_member_order_does_not_matter():
    members, truth = make_ensemble(17, 32, 5, seed=5)
    members[1].surf_vars["2t"][0, -1, 2, 2] = float("nan")
    thr = thresholds_for(truth)
    assert_same_scores(probability_scores(members, truth, thr), probability_scores(members[::-1], truth, thr))
    assert_same_scores(probability_scores(members, truth, thr), probability_scores([members[i] for i in (3, 0, 4, 2, 1)], truth, thr))


def test_invalid_points_and_a_plane_without_a_valid_point():
    n_lat, n_lon, M = 9, 45, 3
    members, truth = make_ensemble(n_lat, n_lon, M, seed=6)
    thr = {"2t": thresholds_for(truth)["2t"][:2]}
    base = probability_scores(members, truth, thr)
    members[0].surf_vars["2t"][0, -1, 0, 0] = float("nan")
    members[M - 1].surf_vars["2t"][0, -1, 0, n_lon - 1] = float("inf")
    truth.surf_vars["2t"][0, -1, 4, 7] = float("-inf")
    truth.surf_vars["2t"][0, -1, 6, :] = float("nan")
    s = probability_scores(members, truth, thr)
    assert s.count["2t"].tolist() == [n_lat * n_lon - 3 - n_lon, n_lat * n_lon]
    assert s.rows["2t"][0].sum(dim=(-1, -2))[:, 0].tolist() == [n_lon - 2, n_lon, n_lon, n_lon, n_lon - 1, n_lon, 0, n_lon, n_lon]
    assert torch.equal(s.rows["2t"][1], base.rows["2t"][1]) and not torch.equal(s.rows["2t"][0], base.rows["2t"][0])
    assert np.array_equal(s.scores_table[1].numpy(), base.scores_table[1].numpy())
    assert_equals_yardstick(s, members, truth, thr)
    members[1].surf_vars["2t"][1, -1] = float("nan")                    # a whole plane: NaN scores, zero counts
    s = probability_scores(members, truth, thr)
    assert (s.count["2t"] == torch.tensor([n_lat * n_lon - 3 - n_lon, 0])).all() and (s.counts["2t"][1] == 0).all()
    for prop in FLOAT_PROPS + ("observed_frequency", "forecast_weight", "hit_rate", "false_alarm_rate"):
        assert torch.isnan(getattr(s, prop)["2t"][1]).all() and not torch.isnan(getattr(s, prop)["2t"][0]).all(), prop


def test_one_batch_of_members_equals_the_sequence_form():
    members, truth = make_ensemble(17, 32, 4, seed=7, B=1)
    cat = lambda grp: {k: torch.cat([getattr(b, grp)[k] for b in members]) for k in getattr(truth, grp)}  # noqa: E731
    md = truth.metadata
    one = Batch(cat("surf_vars"), truth.static_vars, cat("atmos_vars"),
                Metadata(lat=md.lat, lon=md.lon, time=md.time * 4, atmos_levels=md.atmos_levels))
    thr = thresholds_for(truth)
    a, b = probability_scores(one, truth, thr), probability_scores(members, truth, thr)
    assert a.brier["z"].shape == (1, 3, 4) and a.members == 4
    assert_same_scores(a, b)
    with pytest.raises(ValueError, match="probability_scores: members is ONE Batch.*batch size 1"):
        probability_scores(one, red_noise_batch(17, 32, seed=7, B=2), thr)
    with pytest.raises(ValueError, match="probability_scores: members is ONE Batch.*2 to 64"):
        probability_scores(truth, truth, thr)


def test_argument_errors():
    members, truth = make_ensemble(17, 32, 3, seed=8)
    md = truth.metadata
    thr = {"2t": [5e4]}
    with pytest.raises(ValueError, match="probability_scores: members must hold 2 to 64"):
        probability_scores(members[:1], truth, thr)
    with pytest.raises(ValueError, match="probability_scores: members must hold 2 to 64"):
        probability_scores(members * 22, truth, thr)
    with pytest.raises(TypeError, match=r"probability_scores: members\[1\] must be a Batch"):
        probability_scores([members[0], 3], truth, thr)
    with pytest.raises(TypeError, match="probability_scores: truth must be a Batch"):
        probability_scores(members, None, thr)
    with pytest.raises(ValueError, match="probability_scores: 1 to 8 thresholds.*'2t' has 9"):
        probability_scores(members, truth, {"2t": np.arange(9.0)})
    with pytest.raises(ValueError, match="probability_scores: thresholds name the variable '10u'"):
        probability_scores(members, truth, {"2t": [1.0], "10u": [1.0]})
    with pytest.raises(ValueError, match=r"probability_scores: .*'z'.*\(2, 2\).*C = 3"):
        probability_scores(members, truth, {"z": np.zeros((2, 2))})
    with pytest.raises(ValueError, match="probability_scores: .*'2t'.*shape"):
        probability_scores(members, truth, {"2t": np.zeros((2, 2))})
    with pytest.raises(ValueError, match="probability_scores: thresholds must be a non-empty mapping"):
        probability_scores(members, truth, {})
    short = Batch({k: v for k, v in members[2].surf_vars.items() if k != "msl"}, {}, members[2].atmos_vars, md)
    with pytest.raises(ValueError, match="probability_scores: thresholds name the variable 'msl'"):
        probability_scores([members[0], members[1], short], truth, {"msl": [1.0]})
    band = BandBatch(truth.surf_vars, {}, truth.atmos_vars, md, full_patch_rows=4, band=(0, 4))
    with pytest.raises(ValueError, match="probability_scores: truth is a latitude band"):
        probability_scores(members, band, thr)
    with pytest.raises(ValueError, match=r"probability_scores: members\[1\] is a latitude band"):
        probability_scores([members[0], band], truth, thr)
    with pytest.raises(ValueError, match=r"probability_scores: members\[0\] and truth differ in lat"):
        probability_scores([b.crop(4) for b in members], truth, thr)
    with pytest.raises(ValueError, match=r"probability_scores: members\[0\] and truth differ in lon"):
        probability_scores(members, red_noise_batch(17, 16, seed=8), thr)
    with pytest.raises(ValueError, match=r"probability_scores: members\[0\] and truth differ in batch size"):
        probability_scores(members, red_noise_batch(17, 32, seed=8, B=3), thr)
    lat2, lon2 = md.lat[:, None].expand(17, 32), md.lon[None, :].expand(17, 32)
    matrices = Batch(truth.surf_vars, {}, truth.atmos_vars, Metadata(lat=lat2, lon=lon2, time=md.time, atmos_levels=md.atmos_levels))
    with pytest.raises(ValueError, match="probability_scores: .*matrices"):
        probability_scores(members, matrices, thr)


def test_library_exports_and_argument_errors_surface_without_a_gpu():
    from aurora_amd.build import PKG, build_library
    from aurora_amd.engine import lib

    header = (PKG.parent / "include" / "aurora_hip.h").read_text()
    raw = ctypes.CDLL(str(build_library(force=False, verbose=False)))
    name = "aurora_hip_probability_scores"
    assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    assert not hasattr(raw, name + "_workspace_bytes")                   # the call has no workspace
    L = lib.load()
    call = lambda M, planes, n_lat, n_lon, T, members=8, truth=8, thr=8, rows=8: L.aurora_hip_probability_scores(  # noqa: E731
        members, truth, M, planes, n_lat, n_lon, thr, T, 0, rows, None)
    err = L.aurora_hip_last_error
    assert call(8, 0, 17, 32, 3, None, None, None, None) == 0            # an empty call is a no-op
    for M in (1, 65, 0, -3):
        assert call(M, 4, 17, 32, 3) == -1 and b"n_members" in err()
    for T in (0, 9):
        assert call(8, 4, 17, 32, T) == -1 and b"n_thresholds" in err()
    assert call(8, 4, 0, 32, 3) == -1 and b"sizes" in err()
    assert call(8, 4, 17, 0, 3) == -1 and b"sizes" in err()
    assert call(8, -1, 17, 32, 3) == -1 and b"sizes" in err()
    for null in ("members", "truth", "thr", "rows"):
        assert call(8, 4, 17, 32, 3, **{null: None}) == -1 and b"null" in err()
    assert call(8, 4, 17, 32, 3, rows=10) == -1 and b"aligned" in err() and b"rows" in err()
    assert call(8, 4, 17, 32, 3, thr=9) == -1 and b"aligned" in err()
    assert call(8, 2 ** 31 - 1, 17, 32, 3) == -1 and b"too many planes" in err()
