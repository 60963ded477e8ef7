"""`aurora_amd.conditional_scores` on the CPU against a numpy fp64 yardstick written here.

Yardstick: `yardstick_sums` follows the module's text literally -- one boolean mask per bin from a >= e * sigma, np.sum over
the mask -- and is itself checked against a Python loop over the points of a tiny grid.  `aurora_amd.conditional._sums_host`
is code under test and is not used as a yardstick.

Bound (derived as in tests/test_gpu_scores.py): a sum of N fp64 terms in any order is within N 2^-53 sum|term| of the exact
sum, and both sides carry that, so with N <= 721 x 1440 (2 N 2^-53 = 2.3e-10) the count is exact, S1, S3 and S4 agree to 1e-9
relative and S2 to 1e-9 x S4; finalised: rmse to 1e-9 relative, mae to 2e-9 relative, bias to 2e-9 x mae.  The bin of a point
comes from single correctly rounded fp64 operations on both sides, so the integers must be equal."""
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, FieldStats, Metadata, conditional_scores, scores
from aurora_amd.conditional import ConditionalScores
from tests.verification_inputs import cos_weights, red_noise, weights

REL = 1e-9
UNIT_EDGES = (-1.5, -0.5, 0.5, 1.5)                    # in units of the scale
LEVELS = (100, 500, 850)


# ---- the yardstick -----------------------------------------------------------------------------------------------------
def yardstick_sums(pred, truth, centre, scale, edges, by, w) -> np.ndarray:
    """(E + 1, 5) sums of ONE plane (n_lat, n_lon): count, w, w d, w d^2, w |d| per bin; fp64 throughout."""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float32).astype(np.float64)
    valid = np.isfinite(p) & np.isfinite(t)
    v = p if by == "pred" else t
    with np.errstate(invalid="ignore"):
        if centre is not None:
            c = np.asarray(centre, dtype=np.float64)
            valid &= np.isfinite(c)
            a = v - c
        else:
            a = v
        if scale is not None:
            s = np.asarray(scale, dtype=np.float64)
            valid &= np.isfinite(s) & (s >= 0)
            passed = [a >= ej * s for ej in e]
        else:
            passed = [a >= ej for ej in e]
    bins = np.sum(passed, axis=0)
    W = np.broadcast_to(np.asarray(w, dtype=np.float64)[:, None], p.shape)
    out = np.zeros((len(e) + 1, 5))
    for b in range(len(e) + 1):
        m = valid & (bins == b)
        d, wm = p[m] - t[m], W[m]
        out[b] = m.sum(), np.sum(wm), np.sum(wm * d), np.sum(wm * d * d), np.sum(wm * np.abs(d))
    return out


def brute_force_sums(pred, truth, centre, scale, edges, by, w) -> np.ndarray:
    out = np.zeros((len(edges) + 1, 5))
    for i in range(pred.shape[0]):
        for j in range(pred.shape[1]):
            p, t = float(pred[i, j]), float(truth[i, j])
            c = 0.0 if centre is None else float(centre[i, j])
            s = 1.0 if scale is None else float(scale[i, j])
            if not (np.isfinite(p) and np.isfinite(t) and np.isfinite(c) and np.isfinite(s) and s >= 0):
                continue
            a = (p if by == "pred" else t) - c
            b = sum(1 for e in edges if a >= float(np.float32(e)) * s)
            d = p - t
            out[b] += (1, w[i], w[i] * d, w[i] * d * d, w[i] * abs(d))
    return out


def assert_sums_match(got: np.ndarray, want: np.ndarray, what: str):
    """got / want: (bins, 5) sums of one plane, the bound of the module's text."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:, 0], want[:, 0]), (what, "count", got[:, 0], want[:, 0])
    for s in (1, 3, 4):
        assert (np.abs(got[:, s] - want[:, s]) <= REL * want[:, s]).all(), (what, s, got[:, s], want[:, s])
    assert (np.abs(got[:, 2] - want[:, 2]) <= REL * want[:, 4]).all(), (what, 2, got[:, 2], want[:, 2])


def finalised(y: np.ndarray):
    """bias, rmse, mae of (..., 5) sums by direct numpy evaluation; NaN without weight."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return y[..., 2] / y[..., 1], np.sqrt(y[..., 3] / y[..., 1]), y[..., 4] / y[..., 1]


def assert_rates_match(got_bias, got_rmse, got_mae, y: np.ndarray, what: str):
    bias, rmse, mae = finalised(y)
    empty = y[..., 1] == 0
    for g in (got_bias, got_rmse, got_mae):
        assert np.array_equal(np.isnan(g), empty), (what, g, y[..., 1])
    k = ~empty
    assert (np.abs(got_rmse[k] - rmse[k]) <= REL * rmse[k]).all(), (what, "rmse")
    assert (np.abs(got_mae[k] - mae[k]) <= 2 * REL * mae[k]).all(), (what, "mae")
    assert (np.abs(got_bias[k] - bias[k]) <= 2 * REL * mae[k]).all(), (what, "bias")


# ---- inputs ------------------------------------------------------------------------------------------------------------
def planes(n_planes, n_lat, n_lon, seed):
    """(pred, truth, centre, scale), each (n_planes, n_lat, n_lon) float32.  Truth: red noise about 0 (amplitude 500);
    centre: a smooth map of amplitude 350; scale: a positive map about 200 that holds a few exact zeros; pred: truth + noise
    - 0.3 (truth - centre), so that the highs are under-forecast and the lows over-forecast."""
    g = np.random.default_rng(seed)
    truth = red_noise((n_planes, n_lat, n_lon), seed, mean=0.0, amp=500.0)
    i = np.arange(n_lat, dtype=np.float64)[:, None] / max(n_lat, 2)
    j = np.arange(n_lon, dtype=np.float64)[None, :] / max(n_lon, 2)
    k = np.arange(n_planes, dtype=np.float64)[:, None, None]
    centre = (350.0 * np.sin(2 * np.pi * (2.3 * i + 1.7 * j) + 0.9 * k)).astype(np.float32)
    scale = (200.0 * (1.0 + 0.3 * np.cos(2 * np.pi * (1.1 * i - 0.6 * j) + k))).astype(np.float32)
    flat = scale.reshape(n_planes, -1)
    flat[:, :: max(flat.shape[1] // 5, 7)] = 0.0
    pred = (truth + 40.0 * g.standard_normal(truth.shape) - 0.3 * (truth.astype(np.float64) - centre)).astype(np.float32)
    return pred, truth, centre, scale


def assert_not_trivial(pred, truth, centre, scale, w):
    """A condition on the INPUT, from the yardstick alone: with the edges (-1.5, -0.5, 0.5, 1.5) in units of the scale every
    one of the five bins of every plane holds at least 1 % of the valid points, and the conditional bias shows."""
    for k in range(pred.shape[0]):
        y = yardstick_sums(pred[k], truth[k], centre[k], scale[k], UNIT_EDGES, "truth", w)
        assert (y[:, 0] >= 0.01 * y[:, 0].sum()).all() and (y[:, 0] >= 1).all(), (k, y[:, 0])
        bias = y[:, 2] / y[:, 1]
        assert bias[0] > 0 > bias[-1], (k, bias)


GRIDS = [(3, 17, 32), (2, 9, 45), (2, 1, 90), (1, 40, 1), (2, 6, 7), (2, 33, 90), (1, 17, 3600), (2, 721, 1440)]


def make_batches(n_lat, n_lon, seed, B=2, T=2, levels=LEVELS):
    """pred, truth, centre, scale batches: 2 surface variables and a three-level one, two history entries."""
    n = B * T * (2 + len(levels))
    arrays = planes(n, n_lat, n_lon, seed)
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1)[:-1],
                  time=tuple(datetime(2023, 1, 1, 6) for _ in range(B)), atmos_levels=tuple(levels))
    out = []
    for a in arrays:
        x = torch.from_numpy(a)
        surf, atmos = x[: 2 * B * T].view(2, B, T, n_lat, n_lon), x[2 * B * T:].view(B, T, len(levels), n_lat, n_lon)
        out.append(Batch({"2t": surf[0].clone(), "msl": surf[1].clone()}, {}, {"z": atmos.clone()}, md))
    return out


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_public_names():
    assert aurora_amd.conditional_scores is conditional_scores and aurora_amd.ConditionalScores is ConditionalScores
    assert "conditional_scores" in aurora_amd.__all__ and "ConditionalScores" in aurora_amd.__all__


@pytest.mark.parametrize("by", ["truth", "pred"])
def test_yardstick_equals_a_loop_over_the_points(by):
    p, t, c, s = planes(1, 5, 7, seed=3)
    p[0, 0, 0] = np.nan
    t[0, 4, 6] = np.inf
    c[0, 2, 3] = np.nan
    s[0, 1, 1] = -1.0
    w = weights(5)
    for cc, ss in ((None, None), (c[0], None), (None, s[0]), (c[0], s[0])):
        edges = UNIT_EDGES if ss is not None else (-300.0, -100.0, 100.0, 300.0)
        y, b = yardstick_sums(p[0], t[0], cc, ss, edges, by, w), brute_force_sums(p[0], t[0], cc, ss, edges, by, w)
        assert np.array_equal(y[:, 0], b[:, 0]) and y[:, 0].sum() == 35 - 2 - (cc is not None) - (ss is not None)
        np.testing.assert_allclose(y, b, rtol=1e-13, atol=1e-9)


@pytest.mark.parametrize("n_planes,n_lat,n_lon", GRIDS)
def test_the_inputs_of_the_table_tests_fill_every_bin(n_planes, n_lat, n_lon):
    """The condition the device tests assert on their inputs holds for every grid they use (checked without a device)."""
    assert_not_trivial(*planes(n_planes, n_lat, n_lon, seed=n_lat + n_lon), weights(n_lat))


def per_plane(batch, name):
    group = batch.surf_vars if name in batch.surf_vars else batch.atmos_vars
    return group[name][:, -1].numpy()


def check_against_yardstick(s, pred, truth, centre, scale, edges, by, what):
    """Every plane and bin of a result against the yardstick: raw sums, bin scores, tails, counts."""
    w = cos_weights(pred.metadata.lat.double().numpy())
    E = max(np.asarray(v).shape[-1] for v in edges.values())
    n = 0
    for name in edges:
        pk, tk = per_plane(pred, name), per_plane(truth, name)
        ck = None if centre is None else np.broadcast_to(per_plane(centre, name), pk.shape)
        sk = None if scale is None else np.broadcast_to(per_plane(scale, name), pk.shape)
        lead = pk.shape[:-2]
        assert tuple(s.sums[name].shape) == (*lead, E + 1, 5) and s.count[name].dtype == torch.int64
        for idx in np.ndindex(*lead):
            e = np.asarray(edges[name], dtype=np.float64)
            e = e[idx[1]] if e.ndim == 2 else e
            y = yardstick_sums(pk[idx], tk[idx], None if ck is None else ck[idx], None if sk is None else sk[idx], e, by, w)
            Ev = len(e)
            got = s.sums[name][idx].numpy()
            assert_sums_match(got[: Ev + 1], y, f"{what} {name}{idx}")
            assert (got[Ev + 1:] == 0).all()
            assert np.array_equal(s.count[name][idx].numpy(), got[:, 0].astype(np.int64))
            assert_rates_match(s.bias[name][idx].numpy()[: Ev + 1], s.rmse[name][idx].numpy()[: Ev + 1],
                               s.mae[name][idx].numpy()[: Ev + 1], y, f"{what} {name}{idx} bins")
            for prop in ("bias", "rmse", "mae"):                                 # padded bins and padded edges: NaN
                assert torch.isnan(getattr(s, prop)[name][idx][Ev + 1:]).all()
            for prop in ("bias_above", "rmse_above", "mae_above", "bias_below", "rmse_below", "mae_below"):
                assert torch.isnan(getattr(s, prop)[name][idx][Ev:]).all()
            if y[:, 1].sum() > 0:                                                # (an empty bin holds none of the weight)
                assert (s.fraction[name][idx][Ev + 1:] == 0).all()
                np.testing.assert_allclose(s.fraction[name][idx].numpy()[: Ev + 1], y[:, 1] / y[:, 1].sum(), rtol=2 * REL)
            else:
                assert torch.isnan(s.fraction[name][idx]).all()
            above = np.stack([y[j + 1:].sum(axis=0) for j in range(Ev)])
            below = np.stack([y[: j + 1].sum(axis=0) for j in range(Ev)])
            assert np.array_equal(s.count_above[name][idx].numpy()[:Ev], above[:, 0])
            assert np.array_equal(s.count_below[name][idx].numpy()[:Ev], below[:, 0])
            total = int(y[:, 0].sum())
            assert ((s.count_above[name][idx] + s.count_below[name][idx]) == total).all()
            assert_rates_match(s.bias_above[name][idx].numpy()[:Ev], s.rmse_above[name][idx].numpy()[:Ev],
                               s.mae_above[name][idx].numpy()[:Ev], above, f"{what} {name}{idx} above")
            assert_rates_match(s.bias_below[name][idx].numpy()[:Ev], s.rmse_below[name][idx].numpy()[:Ev],
                               s.mae_below[name][idx].numpy()[:Ev], below, f"{what} {name}{idx} below")
            n += 1
    assert n == s.sums_table.shape[0]


Z_EDGES = np.array([[-1.0, 0.0, 1.0], [-2.0, 0.5, 2.5], [-0.25, 0.25, 3.0]])
EDGE_SETS = {
    "one": {"2t": (0.25,)},
    "padded": {"2t": UNIT_EDGES, "msl": (-0.5, 1.0), "z": Z_EDGES},
    "eight": {"z": (-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0), "msl": (-np.inf, 0.0, np.inf)},
}


@pytest.mark.parametrize("by", ["truth", "pred"])
@pytest.mark.parametrize("maps", ["none", "centre", "scale", "both"])
@pytest.mark.parametrize("which", list(EDGE_SETS))
def test_cpu_path_equals_the_yardstick(which, maps, by):
    pred, truth, centre, scale = make_batches(9, 21, seed=11)
    centre = centre if maps in ("centre", "both") else None
    scale = scale if maps in ("scale", "both") else None
    unit = 1.0 if scale is not None else 200.0
    edges = {k: np.asarray(v) * unit for k, v in EDGE_SETS[which].items()}
    s = conditional_scores(pred, truth, edges, centre=centre, scale=scale, by=by)
    assert s.by == by and s.rmse[next(iter(edges))].dtype == torch.float64 and list(s.rmse) == [k for k in ("2t", "msl", "z") if k in edges]
    for k, v in edges.items():
        got = s.edges[k].numpy()
        assert got.dtype == np.float32 and np.array_equal(got[0, ..., : v.shape[-1]], np.broadcast_to(v.astype(np.float32), got[0, ..., : v.shape[-1]].shape))
    check_against_yardstick(s, pred, truth, centre, scale, edges, by, f"{which} {maps} {by}")


def test_invalid_points_and_counts_against_scores():
    pred, truth, centre, scale = make_batches(9, 21, seed=12)
    pred.surf_vars["2t"][0, -1, 0, 0] = float("nan")
    truth.surf_vars["2t"][1, -1, 8, 20] = float("inf")
    truth.atmos_vars["z"][0, -1, 1] = float("nan")                                # a whole plane
    edges = {"2t": UNIT_EDGES, "z": (-1.0, 1.0)}
    raw = {k: np.asarray(v) * 200.0 for k, v in edges.items()}
    plain = conditional_scores(pred, truth, raw)
    ref = scores(pred, truth)
    for k in edges:                                                               # no map adds invalid points
        assert torch.equal(plain.count[k].sum(dim=-1), ref.count[k])
    assert plain.count["z"][0, 1].sum() == 0 and torch.isnan(plain.rmse["z"][0, 1]).all() and (plain.sums["z"][0, 1] == 0).all()
    centre.surf_vars["2t"][0, -1, 3, 3] = float("nan")
    scale.surf_vars["2t"][0, -1, 4, 4] = -1.0
    scale.surf_vars["2t"][1, -1, 5, 5] = float("inf")
    s = conditional_scores(pred, truth, edges, centre=centre, scale=scale)
    assert s.count["2t"].sum(dim=-1).tolist() == [9 * 21 - 3, 9 * 21 - 2]
    check_against_yardstick(s, pred, truth, centre, scale, {k: np.asarray(v) for k, v in edges.items()}, "truth", "invalid")


def test_maps_with_batch_size_one_are_repeated():
    pred, truth, centre, scale = make_batches(9, 21, seed=13)
    one = lambda b: Batch({k: v[:1] for k, v in b.surf_vars.items()}, {}, {k: v[:1] for k, v in b.atmos_vars.items()},  # noqa: E731
                          Metadata(b.metadata.lat, b.metadata.lon, b.metadata.time[:1], b.metadata.atmos_levels))
    twice = lambda b: Batch({k: v[:1].repeat(2, 1, 1, 1) for k, v in b.surf_vars.items()}, {},  # noqa: E731
                            {k: v[:1].repeat(2, 1, 1, 1, 1) for k, v in b.atmos_vars.items()}, b.metadata)
    edges = {"2t": UNIT_EDGES, "z": (-1.0, 1.0)}
    a = conditional_scores(pred, truth, edges, centre=one(centre), scale=one(scale))
    b = conditional_scores(pred, truth, edges, centre=twice(centre), scale=twice(scale))
    assert torch.equal(a.sums_table, b.sums_table) and a.sums_table[:, :, 0].sum() == 2 * 4 * 9 * 21
    check_against_yardstick(a, pred, truth, twice(centre), twice(scale), {k: np.asarray(v) for k, v in edges.items()}, "truth", "B=1")


def test_centre_and_scale_from_field_stats():
    """The chain of the module's text: climatology maps from a FieldStats accumulator, then the thresholded RMSE."""
    pred, truth, _, _ = make_batches(9, 21, seed=14, B=1)
    stats = FieldStats()
    for k in range(6):
        stats.update(make_batches(9, 21, seed=20 + k, B=1)[1])
    centre, scale = stats.as_batch("mean"), stats.as_batch("std", ddof=1)
    edges = {"2t": (-1.0, 0.0, 1.0), "z": (1.0,)}
    s = conditional_scores(pred, truth, edges, centre=centre, scale=scale)
    check_against_yardstick(s, pred, truth, centre, scale, {k: np.asarray(v) for k, v in edges.items()}, "truth", "FieldStats")
    assert (s.count["2t"] > 0).all() and (s.count_above["z"][..., 0] > 0).all()


def test_argument_errors():
    pred, truth, centre, scale = make_batches(9, 21, seed=15)
    with pytest.raises(ValueError, match="ascending.*'2t'|'2t'.*ascending"):
        conditional_scores(pred, truth, {"2t": (0.5, -0.5)})
    with pytest.raises(ValueError, match="ascending"):
        conditional_scores(pred, truth, {"z": np.array([[0.0, 1.0], [1.0, 1.0], [0.0, 1.0]])})
    with pytest.raises(ValueError, match="'10u'"):
        conditional_scores(pred, truth, {"10u": (0.0,)})
    with pytest.raises(ValueError, match="1 to 8 edges per variable, '2t' has 9"):
        conditional_scores(pred, truth, {"2t": tuple(range(9))})
    with pytest.raises(ValueError, match="the edges of '2t' must be numbers"):
        conditional_scores(pred, truth, {"2t": ("warm",)})
    with pytest.raises(ValueError, match="the edges of 'z' have shape"):
        conditional_scores(pred, truth, {"z": np.zeros((2, 3))})
    with pytest.raises(ValueError, match="the edges of '2t' have shape"):
        conditional_scores(pred, truth, {"2t": np.zeros((2, 3))})
    with pytest.raises(ValueError, match="non-empty mapping"):
        conditional_scores(pred, truth, {})
    lacking = Batch({"msl": centre.surf_vars["msl"]}, {}, centre.atmos_vars, centre.metadata)
    with pytest.raises(ValueError, match="centre has no surf variable '2t'"):
        conditional_scores(pred, truth, {"2t": (0.0,)}, centre=lacking)
    with pytest.raises(ValueError, match="scale has no surf variable '2t'"):
        conditional_scores(pred, truth, {"2t": (0.0,)}, centre=centre, scale=lacking)
    with pytest.raises(ValueError, match="by must be"):
        conditional_scores(pred, truth, {"2t": (0.0,)}, by="error")
    p3, t3, c3, _ = make_batches(9, 21, seed=16, B=3)
    two = Batch({k: v[:2] for k, v in c3.surf_vars.items()}, {}, {k: v[:2] for k, v in c3.atmos_vars.items()},
                Metadata(c3.metadata.lat, c3.metadata.lon, c3.metadata.time[:2], c3.metadata.atmos_levels))
    with pytest.raises(ValueError, match="batch size"):
        conditional_scores(p3, t3, {"2t": (0.0,)}, centre=two)
    with pytest.raises(TypeError, match="Batch"):
        conditional_scores(pred, truth, {"2t": (0.0,)}, scale=1.0)
