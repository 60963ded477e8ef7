"""`aurora_amd.ensemble_scores` on the host: closed forms, member order, NaN masks, both call forms, argument errors and the
C ABI of the device path (no GPU needed).

The yardstick `yardstick_ensemble` is the table of include/aurora_hip.h written out in numpy fp64 here, with the PAIRWISE
form of g and `np.sum`, independently of `aurora_amd.ensemble._ensemble_sums_host` (code under test, which takes the sorted
form); tests/test_gpu_ensemble_scores.py compares the kernel with the same function.

Bound (derived in tests/test_gpu_ensemble_scores.py, the figure of tests/test_gpu_scores.py): REL = 1e-9; S1, S5 to REL
relative; S2, S4 to REL S5; S6 to REL 2 S5; S3 to REL Q; S7 to REL 2 Q with Q = sum w q, q = (sum_m d_m^2) / M; the counts
exactly."""
import ctypes

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, ensemble_scores
from aurora_amd.batch import BandBatch
from aurora_amd.ensemble import EnsembleScores, _ensemble_sums_host
from tests.verification_inputs import cos_weights, every, randn_batch, shifted

REL = 1e-9


def yardstick_ensemble(members, truth, w):
    """ONE plane: members (M, n_lat, n_lon), truth (n_lat, n_lon), w (n_lat,) -> (the eight sums, the M + 1 bins, the ties,
    Q), straight from the table: fp64 differences to truth over the points where truth and all members are finite, g as
    the double sum over pairs."""
    x, y = np.asarray(members), np.asarray(truth)
    M = x.shape[0]
    valid = np.isfinite(y) & np.isfinite(x).all(axis=0)
    W = np.repeat(np.asarray(w, dtype=np.float64)[:, None], y.shape[1], axis=1)[valid]
    xv, yv = x[:, valid], y[valid]
    d = xv.astype(np.float64) - yv.astype(np.float64)
    e = np.sum(d, axis=0) / M
    a = np.sum(np.abs(d), axis=0) / M
    g = np.zeros_like(e)
    for i in range(M):
        g += np.sum(np.abs(d[i] - d), axis=0)
    g /= M * M
    v = np.sum((d - e) ** 2, axis=0) / (M - 1)
    q = np.sum(d * d, axis=0) / M
    sums = np.array([float(valid.sum()), np.sum(W), np.sum(W * e), np.sum(W * e * e), np.sum(W * np.abs(e)), np.sum(W * a),
                     np.sum(W * g), np.sum(W * v)])
    below = np.sum(xv < yv, axis=0)
    bins = np.array([int(np.sum(below == b)) for b in range(M + 1)], dtype=np.int64)
    ties = int(np.sum(np.any(xv == yv, axis=0)))
    return sums, bins, ties, float(np.sum(W * q))


def assert_ensemble_sums_match(got, got_hist, want, what):
    """got (8,), got_hist (M + 2,) of one plane against the yardstick's tuple: the bound of the module's text."""
    sums, bins, ties, Q = want
    print(f"{what}: got {np.asarray(got).tolist()} {np.asarray(got_hist).tolist()} want {sums.tolist()} {bins.tolist()} "
          f"{ties} Q {Q}")
    assert got[0] == sums[0], (what, "count", got[0], sums[0])
    assert np.array_equal(np.asarray(got_hist)[:-1], bins), (what, "bins", got_hist, bins)
    assert int(got_hist[-1]) == ties, (what, "ties", got_hist[-1], ties)
    assert int(np.sum(np.asarray(got_hist)[:-1])) == int(sums[0]), (what, "the bins add up to the count")
    for s, scale in ((1, sums[1]), (5, sums[5]), (2, sums[5]), (4, sums[5]), (6, 2 * sums[5]), (3, Q), (7, 2 * Q)):
        assert abs(got[s] - sums[s]) <= REL * scale, (what, s, got[s], sums[s], scale)


def pressure_ensemble(M, n_planes, n_lat, n_lon, seed):
    """truth = 101325 + 300 randn, members = truth + 0.5 + 2 randn, float32: (M, n_planes, n_lat, n_lon), (n_planes, ...)."""
    g = torch.Generator().manual_seed(seed)
    t = 101325 + 300 * torch.randn(n_planes, n_lat, n_lon, generator=g, dtype=torch.float64)
    x = t + 0.5 + 2 * torch.randn(M, n_planes, n_lat, n_lon, generator=g, dtype=torch.float64)
    return x.float(), t.float()


def lagged(M, n_lat=17, n_lon=32, seed=0, B=2, dtype=torch.float32):
    truth = randn_batch(n_lat, n_lon, seed=seed, B=B, offset=280.0, scale=15.0, dtype=dtype)
    members = []
    for m in range(M):
        err = randn_batch(n_lat, n_lon, seed=seed + 1 + m, B=B, offset=0.3, scale=1.5, dtype=dtype)
        members.append(Batch({k: v + err.surf_vars[k] for k, v in truth.surf_vars.items()}, truth.static_vars,
                             {k: v + err.atmos_vars[k] for k, v in truth.atmos_vars.items()}, truth.metadata))
    return members, truth


def assert_finalised_match(s, k, idx, y, M, what):
    """The finalised columns of one plane against the yardstick's sums (the inheritance of the bound is written out in
    tests/test_gpu_ensemble_scores.py)."""
    S, _, _, Q = y
    a_bar, q_bar = S[5] / S[1], Q / S[1]
    rmse, spread = np.sqrt(S[3] / S[1]), np.sqrt(S[7] / S[1])
    assert int(s.count[k][idx]) == S[0]
    assert abs(float(s.bias[k][idx]) - S[2] / S[1]) <= 2 * REL * a_bar, (what, k, idx, "bias")
    assert abs(float(s.mae[k][idx]) - S[4] / S[1]) <= 2 * REL * a_bar, (what, k, idx, "mae")
    assert abs(float(s.crps[k][idx]) - (S[5] - S[6] / 2) / S[1]) <= 4 * REL * a_bar, (what, k, idx, "crps")
    fair = (S[5] - S[6] / 2 * M / (M - 1)) / S[1]
    assert abs(float(s.fair_crps[k][idx]) - fair) <= 6 * REL * a_bar, (what, k, idx, "fair_crps")
    for name, got, want, du in (("rmse", float(s.rmse[k][idx]), rmse, 2 * REL * q_bar),
                                ("spread", float(s.spread[k][idx]), spread, 4 * REL * q_bar)):
        bound = min(np.sqrt(du), du / want if want > 0 else np.inf)
        assert abs(got - want) <= bound, (what, k, idx, name, got, want, bound)


def assert_batch_matches_yardstick(s, members, truth, what):
    """Raw sums, counts and finalised columns of every plane of an `EnsembleScores` against the yardstick."""
    s = s.cpu()
    M = len(members)
    w = cos_weights(truth.metadata.lat.double().cpu().numpy())
    n = 0
    for grp in ("surf_vars", "atmos_vars"):
        for k, t in getattr(truth, grp).items():
            tk = t[:, -1].cpu().numpy()
            xk = np.stack([getattr(b, grp)[k][:, -1].cpu().numpy() for b in members])
            lead = tk.shape[:-2]
            assert tuple(s.crps[k].shape) == lead and tuple(s.rank_hist[k].shape) == lead + (M + 1,)
            for idx in np.ndindex(*lead):
                y = yardstick_ensemble(xk[(slice(None),) + idx], tk[idx], w)
                hist = np.concatenate([s.rank_hist[k][idx].numpy(), [int(s.ties[k][idx])]])
                assert_ensemble_sums_match(s.sums[k][idx].numpy(), hist, y, f"{what} {k}{idx}")
                if y[0][0] > 0:
                    assert_finalised_match(s, k, idx, y, M, what)
                n += 1
    assert n == s.table.shape[0] == s.hist.shape[0]


# ---- names, closed forms ---------------------------------------------------------------------------------------------
def test_public_names():
    assert aurora_amd.ensemble_scores is ensemble_scores and aurora_amd.EnsembleScores is EnsembleScores
    assert "ensemble_scores" in aurora_amd.__all__ and "EnsembleScores" in aurora_amd.__all__


@pytest.mark.parametrize("d1,d2", [(1.5, -0.5), (2.0, 3.0), (-1.25, -1.25)])
def test_two_members_on_constant_differences(d1, d2):
    """M = 2: a = (|d1| + |d2|) / 2, g = |d1 - d2| / 2, crps = a - g / 2, fair CRPS = a - |d1 - d2| / 2,
    e = (d1 + d2) / 2, v = (d1 - d2)^2 / 2."""
    truth = randn_batch(17, 32, seed=1, offset=280.0, scale=10.0, dtype=torch.float64)
    s = ensemble_scores([shifted(truth, lambda v: v + d1), shifted(truth, lambda v: v + d2)], truth)
    assert isinstance(s, EnsembleScores) and s.members == 2
    assert s.crps["2t"].shape == (2,) and s.crps["z"].shape == (2, 3) and s.crps["z"].dtype == torch.float64
    assert set(s.crps) == {"2t", "msl", "z"}                      # static variables are not scored
    a, gap, e = (abs(d1) + abs(d2)) / 2, abs(d1 - d2), (d1 + d2) / 2
    tol = dict(rtol=1e-11, atol=1e-11)                            # ((280 + d) - 280 in fp64 carries 280 x 2^-53)
    np.testing.assert_allclose(every(s.crps), a - gap / 4, **tol)
    np.testing.assert_allclose(every(s.fair_crps), a - gap / 2, **tol)
    np.testing.assert_allclose(every(s.bias), e, **tol)
    np.testing.assert_allclose(every(s.rmse), abs(e), **tol)
    np.testing.assert_allclose(every(s.mae), abs(e), **tol)
    if gap:
        np.testing.assert_allclose(every(s.spread), gap / np.sqrt(2), **tol)
        np.testing.assert_allclose(every(s.spread_skill), np.sqrt(1.5) * gap / np.sqrt(2) / abs(e), rtol=1e-10)
    sums = every(s.sums).reshape(-1, 8)
    np.testing.assert_allclose(sums[:, 5] / sums[:, 1], a, **tol)
    np.testing.assert_allclose(sums[:, 6] / sums[:, 1], gap / 2, **tol)
    assert s.count["z"].dtype == torch.int64 and (every(s.count) == 17 * 32).all()
    bin_ = int(d1 < 0) + int(d2 < 0)
    hist = every(s.rank_hist).reshape(-1, 3)
    assert s.rank_hist["z"].dtype == torch.int64 and s.rank_hist["z"].shape == (2, 3, 3)
    assert (hist[:, bin_] == 17 * 32).all() and hist.sum() == hist[:, bin_].sum() and (every(s.ties) == 0).all()


@pytest.mark.parametrize("M", (2, 5))
def test_equal_members_give_the_deterministic_scores(M):
    truth = randn_batch(17, 32, seed=2, offset=280.0, scale=10.0)
    member = randn_batch(17, 32, seed=3, offset=280.5, scale=10.0)
    s = ensemble_scores([member] * M, truth)
    d = aurora_amd.scores(member, truth)
    np.testing.assert_allclose(every(s.crps), every(s.mae), rtol=1e-14)
    np.testing.assert_allclose(every(s.fair_crps), every(s.mae), rtol=1e-14)
    np.testing.assert_allclose(every(s.mae), every(d.mae), rtol=1e-12)
    np.testing.assert_allclose(every(s.rmse), every(d.rmse), rtol=1e-12)
    np.testing.assert_allclose(every(s.bias), every(d.bias), rtol=1e-12, atol=1e-12)
    assert (every(s.sums).reshape(-1, 8)[:, 6] == 0).all()
    assert (every(s.spread) == 0).all() and (every(s.spread_skill) == 0).all()
    # a perfect ensemble of equal members: rmse = 0, so the ratio is NaN (and only there)
    p = ensemble_scores([truth] * M, truth)
    assert (every(p.rmse) == 0).all() and (every(p.crps) == 0).all() and np.isnan(every(p.spread_skill)).all()
    assert (every(p.ties) == 17 * 32).all() and (every(p.rank_hist).reshape(-1, M + 1)[:, 0] == 17 * 32).all()


@pytest.mark.parametrize("M", (2, 3, 9))
def test_truth_outside_the_ensemble_and_ties(M):
    members, truth = lagged(M, seed=4)
    n = 17 * 32
    low = ensemble_scores(members, shifted(truth, lambda v: v - 1e3))      # truth below every member: bin 0
    high = ensemble_scores(members, shifted(truth, lambda v: v + 1e3))     # above every member: bin M
    for s, b in ((low, 0), (high, M)):
        hist = every(s.rank_hist).reshape(-1, M + 1)
        assert (hist[:, b] == n).all() and hist.sum() == hist[:, b].sum() and (every(s.ties) == 0).all()
    # truth equal to member 1 at 11 points of one plane: counted in ties, and ranked by the members strictly below
    t = shifted(truth, lambda v: v)
    t.surf_vars["2t"][1, -1].view(-1)[5:16] = members[1].surf_vars["2t"][1, -1].view(-1)[5:16]
    s = ensemble_scores(members, t)
    assert s.ties["2t"].tolist() == [0, 11] and every(s.ties).sum() == 11
    assert_batch_matches_yardstick(s, members, t, "ties")


# ---- the yardstick, member order ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (2, 3, 8, 17, 51))
def test_host_sums_equal_the_yardstick(M):
    x, t = pressure_ensemble(M, 3, 33, 61, seed=10 + M)
    w = cos_weights(np.linspace(90, -90, 33))
    sums, hist = _ensemble_sums_host(x.numpy(), t.numpy(), w)
    assert sums.shape == (3, 8) and hist.shape == (3, M + 2) and hist.dtype == np.int64
    for k in range(3):
        assert_ensemble_sums_match(sums[k], hist[k], yardstick_ensemble(x[:, k].numpy(), t[k].numpy(), w), f"M={M} plane {k}")


def test_batches_equal_the_yardstick_and_the_order_of_the_members_does_not_matter():
    members, truth = lagged(7, n_lat=33, n_lon=64, seed=20)
    s = ensemble_scores(members, truth)
    assert_batch_matches_yardstick(s, members, truth, "lagged")
    perm = [3, 0, 6, 5, 1, 2, 4]
    p = ensemble_scores([members[i] for i in perm], truth)
    assert torch.equal(p.hist, s.hist)
    assert torch.equal(p.table[:, 0], s.table[:, 0])
    assert torch.equal(p.table[:, 6], s.table[:, 6])              # the sorted form: bit for bit
    for col, scale in ((1, s.table[:, 1]), (5, s.table[:, 5]), (2, s.table[:, 5]), (4, s.table[:, 5])):
        assert ((p.table[:, col] - s.table[:, col]).abs() <= 2 * REL * scale).all(), col
    assert_batch_matches_yardstick(p, [members[i] for i in perm], truth, "permuted")


# ---- NaN masks -----------------------------------------------------------------------------------------------------------
def test_nan_masks():
    members, truth = lagged(4, seed=30)
    n = 17 * 32
    members = [shifted(b, lambda v: v) for b in members]
    truth = shifted(truth, lambda v: v)
    members[2].surf_vars["2t"][0, -1, 3, 4:9] = float("nan")      # 5 points in one member
    members[0].surf_vars["2t"][0, -1, 3, 7:11] = float("inf")     # 4 points in another, 2 of them the same
    truth.surf_vars["msl"][1, -1, 0, :] = float("-inf")           # a row of truth
    members[1].atmos_vars["z"][0, -1, 1] = float("nan")           # a whole plane of one member
    members[3].surf_vars["2t"][0, 0] = float("nan")               # history: not scored
    s = ensemble_scores(members, truth)
    assert s.count["2t"].tolist() == [n - 7, n] and s.count["msl"].tolist() == [n, n - 32]
    assert s.count["z"].tolist() == [[n, 0, n], [n, n, n]]
    assert every(s.rank_hist).reshape(-1, 5).sum(axis=1).tolist() == every(s.count).tolist()
    for name in ("crps", "fair_crps", "rmse", "bias", "mae", "spread", "spread_skill"):
        v = getattr(s, name)["z"]
        assert torch.isnan(v[0, 1]) and torch.isfinite(v).sum() == 5, name
    assert (s.rank_hist["z"][0, 1] == 0).all() and s.ties["z"][0, 1] == 0 and (s.sums["z"][0, 1] == 0).all()
    assert_batch_matches_yardstick(s, members, truth, "nan masks")


# ---- both call forms -------------------------------------------------------------------------------------------------------
def test_one_batch_of_members_equals_a_sequence_of_batches():
    members, truth = lagged(5, seed=40, B=1)
    cat = lambda d: {k: torch.cat([getattr(b, d)[k] for b in members]) for k in getattr(truth, d)}  # noqa: E731
    md = truth.metadata
    one = Batch(cat("surf_vars"), truth.static_vars, cat("atmos_vars"),
                Metadata(md.lat, md.lon, tuple(md.time[0] for _ in range(5)), md.atmos_levels))
    a, b = ensemble_scores(one, truth), ensemble_scores(members, truth)
    assert a.members == b.members == 5 and a.layout == b.layout
    assert torch.equal(a.table, b.table) and torch.equal(a.hist, b.hist)
    assert a.crps["2t"].shape == (1,) and a.rank_hist["z"].shape == (1, 3, 6)
    c = a.cpu()
    assert torch.equal(c.table, a.table) and c.members == 5


def test_only_common_variables_and_the_last_history_entry_are_scored():
    members, truth = lagged(3, seed=50)
    less = Batch({"2t": members[1].surf_vars["2t"]}, {}, members[1].atmos_vars, truth.metadata)
    s = ensemble_scores([members[0], less, members[2]], truth)
    assert list(s.crps) == ["2t", "z"]
    full = ensemble_scores(members, truth)
    assert torch.equal(s.crps["z"], full.crps["z"]) and torch.equal(s.rank_hist["2t"], full.rank_hist["2t"])
    moved = [shifted(b, lambda v: torch.cat([v[:, :1] + 7.0, v[:, 1:]], dim=1)) for b in members]
    assert torch.equal(ensemble_scores(moved, truth).table, full.table)


def test_float64_fields_are_scored_on_the_host():
    truth = randn_batch(17, 32, seed=60, dtype=torch.float64, offset=1e5)
    s = ensemble_scores([shifted(truth, lambda v: v + 1e-3), shifted(truth, lambda v: v + 3e-3)], truth)
    np.testing.assert_allclose(every(s.bias), 2e-3, rtol=1e-6)    # offsets an fp32 field could not hold at 1e5
    np.testing.assert_allclose(every(s.crps), 2e-3 - 0.5e-3, rtol=1e-6)


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors():
    members, truth = lagged(3, seed=70)
    md = truth.metadata

    def with_md(b, **kw):
        return Batch(b.surf_vars, b.static_vars, b.atmos_vars, Metadata(**{**dict(lat=md.lat, lon=md.lon, time=md.time,
                     atmos_levels=md.atmos_levels), **kw}))

    with pytest.raises(ValueError, match=r"members must hold 2 to 64 batches, got 1"):
        ensemble_scores(members[:1], truth)
    with pytest.raises(ValueError, match=r"members must hold 2 to 64 batches, got 65"):
        ensemble_scores([members[0]] * 65, truth)
    assert ensemble_scores([members[0]] * 64, truth).members == 64
    # ONE batch: its batch size is M, truth must have batch size 1
    with pytest.raises(ValueError, match=r"members is ONE Batch.*truth must have batch size 1"):
        ensemble_scores(members[0], truth)
    one, single = lagged(2, seed=71, B=1)
    with pytest.raises(ValueError, match=r"members is ONE Batch.*2 to 64, got \[1\]"):
        ensemble_scores(one[0], single)
    with pytest.raises(ValueError, match=r"members\[2\] and truth differ in batch size for '2t'"):
        ensemble_scores(members[:2] + [lagged(1, seed=72, B=3)[0][0]], truth)
    # grids
    cropped = [b.crop(4) for b in members]
    with pytest.raises(ValueError, match=r"members\[0\] and truth differ in lat.*truth\.crop\(model\.patch_size\)"):
        ensemble_scores(cropped, truth)
    assert ensemble_scores(cropped, truth.crop(4)).count["2t"].tolist() == [16 * 32] * 2
    with pytest.raises(ValueError, match=r"members\[1\] and truth differ in lon"):
        ensemble_scores([members[0], with_md(members[1], lon=md.lon + 0.5)], truth)
    with pytest.raises(ValueError, match=r"members\[2\] and truth differ in atmos_levels"):
        ensemble_scores(members[:2] + [with_md(members[2], atmos_levels=(100, 500, 900))], truth)
    lat2, lon2 = md.lat[:, None].expand(17, 32), md.lon[None, :].expand(17, 32)
    with pytest.raises(ValueError, match=r"members\[0\] has matrices"):
        ensemble_scores([with_md(b, lat=lat2, lon=lon2) for b in members], with_md(truth, lat=lat2, lon=lon2))
    with pytest.raises(ValueError, match=r"truth has matrices"):
        ensemble_scores(members, with_md(truth, lat=lat2, lon=lon2))
    band = BandBatch(truth.surf_vars, {}, truth.atmos_vars, md, full_patch_rows=4, band=(0, 4))
    with pytest.raises(ValueError, match=r"truth is a latitude band \(BandBatch\)"):
        ensemble_scores(members, band)
    with pytest.raises(ValueError, match=r"members\[1\] is a latitude band \(BandBatch\)"):
        ensemble_scores([members[0], band], truth)
    with pytest.raises(ValueError, match=r"members is a latitude band \(BandBatch\)"):
        ensemble_scores(band, truth)
    with pytest.raises(TypeError, match=r"members\[1\] must be a Batch"):
        ensemble_scores([members[0], None], truth)
    with pytest.raises(ValueError, match="no surface or atmospheric variable in common"):
        ensemble_scores([Batch({}, {}, {}, md)] * 2, truth)


def test_device_path_argument_checks_need_no_kernel():
    """What `lib.ensemble_scores_sums` refuses is refused before any launch."""
    from aurora_amd.engine import lib

    z = torch.zeros(1, 17, 32)
    with pytest.raises(AssertionError, match="row_w"):
        lib.ensemble_scores_sums([[z], [z]], [z], torch.ones(17, dtype=torch.float64))


def test_library_exports_workspace_size_and_argument_errors():
    from aurora_amd.build import build_library
    from aurora_amd.engine import lib

    raw = ctypes.CDLL(str(build_library(force=False, verbose=False)))
    names = {"aurora_hip_ensemble_scores", "aurora_hip_ensemble_scores_workspace_bytes"}
    assert all(hasattr(raw, n) for n in names) and names <= set(lib.EXPORTED_SYMBOLS)
    ws = lib.ensemble_scores_workspace_bytes
    for M in (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 51, 64):
        for args in ((1, 1, 1), (4, 17, 32), (69, 721, 1440), (141, 1801, 3600)):
            assert ws(M, *args) > 0 and ws(M, *args) % 8 == 0, (M, args)
        assert ws(M, 69, 721, 1440) == 69 * ws(M, 1, 721, 1440)     # the row chunks do not depend on the number of planes
        assert ws(M, 69, 721, 1440) < 721 * 1440 * 4                # far below one plane
    assert ws(3, 4, 17, 32) == ws(4, 4, 17, 32) and ws(33, 4, 17, 32) == ws(64, 4, 17, 32)   # a function of the bucket
    for bad in ((1, 4, 17, 32), (65, 4, 17, 32), (0, 4, 17, 32), (8, 0, 17, 32), (8, 4, 0, 32), (8, 4, 17, -1)):
        assert ws(*bad) == 0, bad
    # argument errors surface without a GPU; an empty call is a no-op
    L = lib.load()
    err = L.aurora_hip_last_error
    f = L.aurora_hip_ensemble_scores
    assert f(None, None, 8, 0, 17, 32, None, None, None, None, None) == 0
    assert f(None, None, 8, 4, 17, 32, None, None, None, None, None) == -1 and b"null" in err()
    for M in (1, 0, -3, 65):
        assert f(None, None, M, 4, 17, 32, None, None, None, None, None) == -1 and b"n_members" in err(), M
    assert f(None, None, 8, 4, 0, 32, None, None, None, None, None) == -1 and b"sizes" in err()
    assert f(None, None, 8, -1, 17, 32, None, None, None, None, None) == -1 and b"sizes" in err()
    # host addresses will do: alignment is checked before anything is launched or read
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert f(p, p, 8, 4, 17, 32, p, p + 4, p, p, None) == -1 and b"aligned" in err()
    assert f(p, p, 8, 4, 17, 32, p, p, p, p + 2, None) == -1 and b"aligned" in err()
