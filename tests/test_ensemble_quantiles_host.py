"""`aurora_amd.ensemble_quantiles` on the host: the rule against a yardstick written here and against numpy, ordering
properties, signed zeros, NaN / Inf, the rank map, member order, both call forms, `as_batch` and argument errors (no GPU
needed).

Yardstick: `yardstick_quantiles` is the rule of aurora_amd/quantiles.py for ONE plane, written independently of
`aurora_amd.quantiles._quantiles_host` (code under test): the order through `np.lexsort` on (value, sign) -- not through the
integer key --, then the three fp64 operations a + g (b - a), each a numpy operation of its own (numpy has no fused
multiply-add), then one cast.  The code under test and the kernel (tests/test_gpu_ensemble_quantiles.py) must equal it in
every bit; NaN positions must be the same, NaN payloads are not compared.

Bound against `np.quantile(x.astype(np.float64), q, axis=0, method="linear")` (derived, not tuned): numpy takes
a + g (b - a) for g < 0.5 and b - (b - a)(1 - g) otherwise; both forms are within a few fp64 units in the last place of the
exact value, so after the one rounding to fp32 they are at most one fp32 unit in the last place (of the numpy value)
apart; where g = 0 (q = 0, q = 1, q = 0.5 with an odd M) both are x_(j) exactly."""
import ctypes

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, FieldStats, Metadata, ensemble_quantiles, ensemble_scores, scores
from aurora_amd.batch import BandBatch
from aurora_amd.quantiles import EnsembleQuantiles, _quantiles_host
from tests.test_ensemble_scores_host import lagged, pressure_ensemble
from tests.verification_inputs import shifted

Q1, Q8 = (0.5,), (0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1)


def yardstick_quantiles(x, q, y=None):
    """ONE plane: x (M, n_lat, n_lon) float32, q a sequence, y (n_lat, n_lon) float32 or None -> (Q, n_lat, n_lon) float32
    and the int8 rank map (None without y)."""
    x = np.asarray(x, dtype=np.float32)
    M = x.shape[0]
    order = np.lexsort((~np.signbit(x), x), axis=0)               # by value; of equal values (+-0) the negative one first
    s = np.take_along_axis(x, order, axis=0).astype(np.float64)
    valid = np.isfinite(x).all(axis=0)
    out = np.full((len(q), *x.shape[1:]), np.nan, dtype=np.float32)
    for i, qi in enumerate(q):
        h = (M - 1) * np.float64(qi)
        j = min(int(np.floor(h)), M - 1)
        g = h - j
        a, b = s[j][valid], s[min(j + 1, M - 1)][valid]
        d = b - a
        t = g * d
        out[i][valid] = (a + t).astype(np.float32)
    rank = None
    if y is not None:
        y = np.asarray(y, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            rank = np.where(valid & np.isfinite(y), (x < y).sum(axis=0), -1).astype(np.int8)
    return out, rank


def assert_same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions differ")
    same = got.view(np.int32) == want.view(np.int32)
    assert (same | nan).all(), (what, int((~(same | nan)).sum()), "values differ in their bits")


def numpy_quantiles(x, q):
    return np.quantile(np.asarray(x).astype(np.float64), q, axis=0, method="linear")


def assert_within_one_ulp_of_numpy(got, x, q, what=""):
    """got (Q, ...) float32 of finite members x (M, ...): the bound of the module's text."""
    M = x.shape[0]
    ref = numpy_quantiles(x, q).astype(np.float32)
    for i, qi in enumerate(q):
        h = (M - 1) * np.float64(qi)
        err = np.abs(got[i].astype(np.float64) - ref[i].astype(np.float64))
        worst = float((err / np.spacing(np.abs(ref[i])).astype(np.float64)).max())
        print(f"{what} q={qi}: worst distance to numpy {worst:.3f} fp32 ulp")
        assert worst <= (0.0 if h == np.floor(h) else 1.0), (what, qi, worst)


def host_maps(x, q, t=None):
    """(M, n_planes, ...) -> the code under test."""
    return _quantiles_host(np.asarray(x), None if t is None else np.asarray(t), q)


# ---- names ---------------------------------------------------------------------------------------------------------------
def test_public_names():
    assert aurora_amd.ensemble_quantiles is ensemble_quantiles and aurora_amd.EnsembleQuantiles is EnsembleQuantiles
    assert "ensemble_quantiles" in aurora_amd.__all__ and "EnsembleQuantiles" in aurora_amd.__all__


# ---- the yardstick, numpy, ordering ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", (Q1, Q8), ids=("median", "eight"))
@pytest.mark.parametrize("M", (2, 3, 8, 17, 64))
def test_host_path_equals_the_yardstick_and_numpy(M, q):
    x, t = pressure_ensemble(M, 2, 33, 61, seed=300 + M)
    x, t = x.numpy(), t.numpy()
    maps, rank = host_maps(x, q, t)
    assert maps.shape == (2, len(q), 33, 61) and maps.dtype == np.float32 and rank.shape == (2, 33, 61) and rank.dtype == np.int8
    for k in range(2):
        want, want_rank = yardstick_quantiles(x[:, k], q, t[k])
        assert_same_bits(maps[k], want, f"M={M} plane {k}")
        assert np.array_equal(rank[k], want_rank)
        assert_within_one_ulp_of_numpy(maps[k], x[:, k], q, f"M={M} plane {k}")


@pytest.mark.parametrize("M", (2, 3, 8, 17, 64))
def test_maps_ascend_in_q_and_end_at_minimum_and_maximum(M):
    x, _ = pressure_ensemble(M, 2, 33, 61, seed=320 + M)
    x = x.numpy()
    maps, rank = host_maps(x, Q8)
    assert rank is None
    assert (np.diff(maps.astype(np.float64), axis=1) >= 0).all()
    assert np.array_equal(maps[:, 0], x.min(axis=0)) and np.array_equal(maps[:, -1], x.max(axis=0))


def test_signed_zeros():
    """A variable clamped at zero with +0 and -0 mixed among the members: the key order puts -0 below +0 whatever the input
    order, so the bits are the yardstick's; numerically it is numpy's value."""
    M = 9
    x, _ = pressure_ensemble(M, 2, 33, 61, seed=77)
    x = ((x - 101325.0).clamp(min=0.0) / 100).numpy()
    g = np.random.default_rng(5)
    x[(x == 0) & (g.random(x.shape) < 0.5)] = -0.0
    assert (np.signbit(x) & (x == 0)).sum() > 100 and ((x == 0).sum(axis=0) >= 2).sum() > 100
    maps, _ = host_maps(x, Q8)
    for k in range(2):
        assert_same_bits(maps[k], yardstick_quantiles(x[:, k], Q8)[0], f"zeros plane {k}")
        assert_within_one_ulp_of_numpy(maps[k], x[:, k], Q8, f"zeros plane {k}")
        assert np.array_equal(maps[k, 0], x[:, k].min(axis=0)) and np.array_equal(maps[k, -1], x[:, k].max(axis=0))   # (-0 == +0)
    # the order of the members does not reach the sign of a zero
    again, _ = host_maps(x[::-1], Q8)
    assert np.array_equal(again.view(np.int32), maps.view(np.int32))


def special_values(M, n_planes=2, n_lat=33, n_lon=61, seed=0):
    """A land mask that is NaN in every member and stray NaN, +Inf, -Inf in single members: (clean members, members, truth,
    the mask of the points that are not valid)."""
    x, t = pressure_ensemble(M, n_planes, n_lat, n_lon, seed=340 + M + seed)
    clean = x.clone()
    g = torch.Generator().manual_seed(22)
    land = torch.rand(n_lat, n_lon, generator=g) < 0.3
    x[:, :, land] = float("nan")
    sea = (~land).nonzero().tolist()
    bad = land[None].repeat(n_planes, 1, 1)
    for (m, k, value), points in zip(((0, 0, "nan"), (M - 1, 1, "inf"), (1, 1, "-inf"), (M // 2, 0, "inf")),
                                     (sea[:5], sea[10:17], sea[14:20], sea[40:41])):
        for i, j in points:
            x[m, k, i, j] = float(value)
            bad[k, i, j] = True
    t[0, sea[30][0], sea[30][1]] = float("nan")                   # truth: the rank, not the quantiles
    t[1, sea[31][0], sea[31][1]] = float("inf")
    return clean.numpy(), x.numpy(), t.numpy(), bad.numpy()


def test_nan_and_inf_make_exactly_their_points_nan():
    M = 11
    clean, x, t, bad = special_values(M)
    want, _ = host_maps(clean, Q8)
    maps, rank = host_maps(x, Q8, t)
    assert np.array_equal(np.isnan(maps), np.broadcast_to(bad[:, None], maps.shape))
    keep = np.broadcast_to(~bad[:, None], maps.shape)
    assert np.array_equal(maps[keep].view(np.int32), want[keep].view(np.int32))
    for k in range(2):
        got, got_rank = yardstick_quantiles(x[:, k], Q8, t[k])
        assert_same_bits(maps[k], got, f"special plane {k}")
        assert np.array_equal(rank[k], got_rank)
    assert np.array_equal(rank == -1, bad | ~np.isfinite(t))


@pytest.mark.parametrize("M", (3, 11))
def test_rank_map_counts_to_the_rank_histogram(M):
    members, truth = lagged(M, n_lat=17, n_lon=32, seed=360 + M)
    members = [shifted(b, lambda v: v) for b in members]
    members[1].surf_vars["2t"][0, -1, 3, 4:9] = float("nan")
    truth = shifted(truth, lambda v: v)
    truth.surf_vars["msl"][1, -1, 0, :] = float("-inf")
    truth.atmos_vars["z"][0, -1, 1, 2, :7] = members[0].atmos_vars["z"][0, -1, 1, 2, :7]      # ties are not below
    eq = ensemble_quantiles(members, truth=truth)
    hist = ensemble_scores(members, truth).rank_hist
    for name, rank in eq.rank.items():
        assert rank.dtype == torch.int8 and rank.shape == truth.surf_vars.get(name, truth.atmos_vars.get(name))[:, -1].shape
        x = np.stack([(b.surf_vars.get(name, b.atmos_vars.get(name)))[:, -1].numpy() for b in members])
        y = truth.surf_vars.get(name, truth.atmos_vars.get(name))[:, -1].numpy()
        ok = np.isfinite(y) & np.isfinite(x).all(axis=0)
        assert np.array_equal(rank.numpy(), np.where(ok, (x < y).sum(0), -1).astype(np.int8))
        assert np.array_equal(rank.numpy() == -1, ~ok)
        flat, h = rank.numpy().reshape(-1, 17 * 32), hist[name].numpy().reshape(-1, M + 1)
        for k in range(flat.shape[0]):
            assert np.array_equal(np.bincount(flat[k][flat[k] >= 0], minlength=M + 1), h[k]), (name, k)


# ---- member order, call forms, as_batch ---------------------------------------------------------------------------------
def test_member_order_and_the_one_batch_form_change_no_bit():
    members, truth = lagged(5, seed=40, B=1)
    a = ensemble_quantiles(members, Q8, truth)
    b = ensemble_quantiles([members[i] for i in (3, 0, 4, 1, 2)], Q8, truth)
    assert torch.equal(a.maps.view(torch.int32), b.maps.view(torch.int32)) and torch.equal(a.ranks, b.ranks)
    cat = lambda d: {k: torch.cat([getattr(m, d)[k] for m in members]) for k in getattr(truth, d)}  # noqa: E731
    md = truth.metadata
    one = Batch(cat("surf_vars"), truth.static_vars, cat("atmos_vars"),
                Metadata(md.lat, md.lon, tuple(md.time[0] for _ in range(5)), md.atmos_levels))
    c = ensemble_quantiles(one, Q8, truth)
    assert c.members == a.members == 5 and c.layout == a.layout and c.q == a.q == tuple(float(v) for v in Q8)
    assert torch.equal(a.maps.view(torch.int32), c.maps.view(torch.int32)) and torch.equal(a.ranks, c.ranks)
    assert c.quantile["2t"].shape == (1, 8, 17, 32) and c.quantile["z"].shape == (1, 3, 8, 17, 32)
    assert c.rank["z"].shape == (1, 3, 17, 32) and set(c.quantile) == {"2t", "msl", "z"}
    assert len(c.as_batch(0.5).metadata.time) == 1
    without = ensemble_quantiles(one, Q8)                           # the quantiles do not depend on the truth
    assert torch.equal(without.maps.view(torch.int32), a.maps.view(torch.int32)) and without.ranks is None
    assert without.cpu().q == a.q


def test_batches_equal_the_yardstick_and_only_the_last_history_entry_counts():
    members, truth = lagged(7, n_lat=33, n_lon=61, seed=20)
    eq = ensemble_quantiles(members, truth=truth)
    assert eq.q == (0.1, 0.5, 0.9) and eq.members == 7 and eq.quantile["z"].shape == (2, 3, 3, 33, 61)
    for name in ("2t", "msl", "z"):
        x = np.stack([b.surf_vars.get(name, b.atmos_vars.get(name))[:, -1].numpy() for b in members])
        got = eq.quantile[name].numpy()
        for idx in np.ndindex(*x.shape[1:-2]):
            assert_same_bits(got[idx], yardstick_quantiles(x[(slice(None),) + idx], eq.q)[0], f"{name}{idx}")
    moved = [shifted(b, lambda v: torch.cat([v[:, :1] + 7.0, v[:, 1:]], dim=1)) for b in members]
    assert torch.equal(ensemble_quantiles(moved, truth=truth).maps, eq.maps)
    less = Batch({"2t": members[1].surf_vars["2t"]}, {}, members[1].atmos_vars, truth.metadata)
    assert list(ensemble_quantiles([members[0], less, members[2]]).quantile) == ["2t", "z"]


def test_as_batch_feeds_the_other_front_ends():
    members, truth = lagged(5, seed=50)
    eq = ensemble_quantiles(members, (0.9, 0.5), truth)
    med = eq.as_batch(0.5)
    assert med.metadata is not None and med.metadata.time == members[0].metadata.time
    assert torch.equal(med.metadata.lat, members[0].metadata.lat) and set(med.static_vars) == set(members[0].static_vars)
    assert med.surf_vars["2t"].shape == (2, 1, 17, 32) and med.atmos_vars["z"].shape == (2, 1, 3, 17, 32)
    assert med.surf_vars["2t"].dtype == torch.float32
    assert torch.equal(med.surf_vars["2t"][:, 0], eq.quantile["2t"][:, 1])
    assert torch.equal(eq.as_batch(0.9).atmos_vars["z"][:, 0], eq.quantile["z"][:, :, 0])
    s = scores(med, truth)
    assert set(s.rmse) == {"2t", "msl", "z"} and torch.isfinite(s.rmse["z"]).all()
    acc = FieldStats()
    acc.update(med)
    acc.update(eq.as_batch(0.9))
    assert torch.isfinite(acc.mean["2t"]).all() and int(acc.count["2t"].max()) == 2
    with pytest.raises(ValueError, match=r"as_batch offers the requested q \(0\.9, 0\.5\), got 0\.1"):
        eq.as_batch(0.1)
    with pytest.raises(ValueError, match="no truth was given"):
        ensemble_quantiles(members).rank


def test_float64_fields_are_taken_as_float32_on_the_host():
    members, truth = lagged(4, seed=60, dtype=torch.float64)
    a = ensemble_quantiles(members, truth=truth)
    b = ensemble_quantiles([m.type(torch.float32) for m in members], truth=truth.type(torch.float32))
    assert a.maps.dtype == torch.float32 and torch.equal(a.maps, b.maps) and torch.equal(a.ranks, b.ranks)


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors():
    members, truth = lagged(3, seed=70)
    md = truth.metadata

    def with_md(b, **kw):
        return Batch(b.surf_vars, b.static_vars, b.atmos_vars, Metadata(**{**dict(lat=md.lat, lon=md.lon, time=md.time,
                     atmos_levels=md.atmos_levels), **kw}))

    with pytest.raises(ValueError, match=r"1 to 8 values of q, got 0"):
        ensemble_quantiles(members, ())
    with pytest.raises(ValueError, match=r"1 to 8 values of q, got 9"):
        ensemble_quantiles(members, [0.1] * 9)
    assert ensemble_quantiles(members, [0.1] * 8).maps.shape[1] == 8 and ensemble_quantiles(members, 0.5).q == (0.5,)
    for bad in ((0.5, 1.5), (-0.1,), (float("nan"),), (float("inf"),)):
        with pytest.raises(ValueError, match=r"q must be finite values in \[0, 1\]"):
            ensemble_quantiles(members, bad)
    with pytest.raises(ValueError, match="q must be numbers"):
        ensemble_quantiles(members, ("median",))
    with pytest.raises(ValueError, match=r"members must hold 2 to 64 batches, got 1"):
        ensemble_quantiles(members[:1])
    with pytest.raises(ValueError, match=r"members must hold 2 to 64 batches, got 65"):
        ensemble_quantiles([members[0]] * 65)
    assert ensemble_quantiles([members[0]] * 64, (1.0,)).members == 64
    one, single = lagged(2, seed=71, B=1)
    with pytest.raises(ValueError, match=r"members is ONE Batch.*2 to 64, got \[1\]"):
        ensemble_quantiles(one[0])
    with pytest.raises(ValueError, match=r"members is ONE Batch.*truth must have batch size 1"):
        ensemble_quantiles(members[0], truth=truth)
    with pytest.raises(ValueError, match=r"members\[2\] and members\[0\] differ in batch size for '2t'"):
        ensemble_quantiles(members[:2] + [lagged(1, seed=72, B=3)[0][0]])
    with pytest.raises(ValueError, match=r"truth and members\[0\] differ in batch size for '2t'"):
        ensemble_quantiles(members, truth=single)
    # grids and levels
    with pytest.raises(ValueError, match=r"members\[1\] and members\[0\] differ in lat"):
        ensemble_quantiles([members[0], members[1].crop(4), members[2]])
    with pytest.raises(ValueError, match=r"truth and members\[0\] differ in lat"):
        ensemble_quantiles(members, truth=truth.crop(4))
    with pytest.raises(ValueError, match=r"members\[1\] and members\[0\] differ in lon"):
        ensemble_quantiles([members[0], with_md(members[1], lon=md.lon + 0.5)])
    with pytest.raises(ValueError, match=r"members\[2\] and members\[0\] differ in atmos_levels"):
        ensemble_quantiles(members[:2] + [with_md(members[2], atmos_levels=(100, 500, 900))])
    lat2, lon2 = md.lat[:, None].expand(17, 32), md.lon[None, :].expand(17, 32)
    with pytest.raises(ValueError, match=r"members\[0\] has matrices"):
        ensemble_quantiles([with_md(b, lat=lat2, lon=lon2) for b in members])
    band = BandBatch(truth.surf_vars, {}, truth.atmos_vars, md, full_patch_rows=4, band=(0, 4))
    with pytest.raises(ValueError, match=r"members\[1\] is a latitude band \(BandBatch\)"):
        ensemble_quantiles([members[0], band])
    with pytest.raises(ValueError, match=r"members is a latitude band \(BandBatch\)"):
        ensemble_quantiles(band)
    with pytest.raises(ValueError, match=r"truth is a latitude band \(BandBatch\)"):
        ensemble_quantiles(members, truth=band)
    with pytest.raises(TypeError, match=r"members\[1\] must be a Batch"):
        ensemble_quantiles([members[0], None])
    with pytest.raises(TypeError, match=r"truth must be a Batch or None"):
        ensemble_quantiles(members, truth=3)
    with pytest.raises(ValueError, match="no surface or atmospheric variable in common"):
        ensemble_quantiles([Batch({}, {}, {}, md)] * 2)
    with pytest.raises(ValueError, match="members and truth have no surface or atmospheric variable in common"):
        ensemble_quantiles(members, truth=Batch({}, {}, {}, md))


def test_library_exports_the_entry_point_and_its_argument_errors():
    """Argument errors surface before any launch, so without a GPU; an empty call is a no-op."""
    from aurora_amd.build import build_library
    from aurora_amd.engine import lib

    raw = ctypes.CDLL(str(build_library(force=False, verbose=False)))
    assert hasattr(raw, "aurora_hip_ensemble_quantiles") and "aurora_hip_ensemble_quantiles" in lib.EXPORTED_SYMBOLS
    L = lib.load()
    err, f = L.aurora_hip_last_error, L.aurora_hip_ensemble_quantiles
    q = (ctypes.c_double * 9)(0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0, 0.5)
    buf = (ctypes.c_double * 8)()
    p, qp = ctypes.addressof(buf), ctypes.addressof(q)
    assert f(None, None, 8, 0, 17, 32, qp, 8, None, None, None) == 0
    for M in (1, 0, 65):
        assert f(p, None, M, 4, 17, 32, qp, 3, p, None, None) == -1 and b"n_members" in err(), M
    for n_q in (0, 9, -1):
        assert f(p, None, 8, 4, 17, 32, qp, n_q, p, None, None) == -1 and b"n_q" in err(), n_q
    assert f(p, p, 8, 4, 17, 32, qp, 3, p, None, None) == -1 and b"rank" in err()          # a truth without a rank map
    assert f(p, None, 8, 4, 17, 32, qp, 3, p, p, None) == -1 and b"rank" in err()          # a rank map without a truth
    assert f(p, None, 8, 4, 0, 32, qp, 3, p, None, None) == -1 and b"sizes" in err()
    assert f(p, None, 8, 4, 17, 32, None, 3, p, None, None) == -1 and b"null q" in err()
    assert f(None, None, 8, 4, 17, 32, qp, 3, p, None, None) == -1 and b"null" in err()
    assert f(p, None, 8, 4, 17, 32, qp, 3, p + 2, None, None) == -1 and b"aligned" in err()
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        one = (ctypes.c_double * 1)(bad)
        assert f(p, None, 8, 4, 17, 32, ctypes.addressof(one), 1, p, None, None) == -1 and b"[0, 1]" in err(), bad
    # what the binding refuses is refused before any launch
    z = torch.zeros(1, 17, 32)
    with pytest.raises(AssertionError, match="members must hold 2..64"):
        lib.ensemble_quantiles([[z]], None, (0.5,))
    with pytest.raises(AssertionError, match="1..8 values of q"):
        lib.ensemble_quantiles([[z], [z]], None, ())
