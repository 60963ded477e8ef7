"""`aurora_amd.FieldStats` on the host against a yardstick written HERE: a two-pass numpy fp64 evaluation of every quantity
from the stacked samples (not `aurora_amd.fieldstats._update_host`, which is code under test).

Bounds (derived, not tuned; u = 2^-53).  With a point's valid samples v_1 .. v_n, origin o = fp32(v_1) and d_i = v_i - o, both
sides form the SAME d_i bit for bit (v is one correctly rounded fp64 difference of fp32 values, o is exact in fp64, d is one
rounding of v - o).  A sum of n fp64 terms in any order is within n u sum|term| of the exact sum, and both sides carry that:
    |s1 - s1'| <= 2 n u sum|d|
    |s2 - s2'| <= 2 (n + 1) u sum d^2      (one more u for the rounding of each d^2, which a fused multiply-add skips)
n, argmin, argmax, exceed, run, longest are integers and origin, vmin, vmax single roundings of v: all exact.
Finalised maps against the two-pass values (mean m = sum v / n, var = sum (v - m)^2 / (n - ddof), mean square = sum v^2 / n):
    mean        (n + 4) u mean|v| (the yardstick's own sum of raw values) + 2 n u mean|d|
    var         3 (n + 3) u sum d^2 / (n - ddof)     (s2 - s1^2 / n cancels at the size of sum d^2 >= sum (v - m)^2)
    mean square (n + 6) u (sum d^2 + 2 |o| sum|d| + n o^2 + sum v^2) / n      (the magnitudes of the three terms it adds)
"""
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, FieldStats, Metadata, scores
from aurora_amd.batch import BandBatch

U = 2.0 ** -53
LEVELS = (500, 850)


# ---- the yardstick --------------------------------------------------------------------------------------------------
def yardstick(x, b=None, r=None, thr=None, below=False, index0=0):
    """x: (S, ...) float32 samples; b: the second operand (same shape) or None; r: (...) reference or None; thr: a list of T
    arrays that broadcast against x[0].  Every quantity per point as a dict of arrays of x[0]'s shape (per threshold: (T, ...)),
    from the stacked samples in two passes."""
    x = np.asarray(x, dtype=np.float32)
    S = x.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ok = np.isfinite(x)
        if b is not None:
            b = np.asarray(b, dtype=np.float32)
            ok &= np.isfinite(b)
            x = np.sqrt(x.astype(np.float64) ** 2 + b.astype(np.float64) ** 2).astype(np.float32)
            ok &= np.isfinite(x)
        v = x.astype(np.float64)
        if r is not None:
            r = np.asarray(r, dtype=np.float32)
            ok &= np.isfinite(r)[None]
            v = v - r.astype(np.float64)[None]
        w = v.astype(np.float32)
        n = ok.sum(axis=0)
        some = n > 0
        first = np.argmax(ok, axis=0)
        origin = np.where(some, np.take_along_axis(w, first[None], axis=0)[0], 0).astype(np.float32)
        vz = np.where(ok, v, 0.0)
        d = np.where(ok, v - origin.astype(np.float64), 0.0)
        out = {"n": n, "origin": origin, "s1": d.sum(axis=0), "s2": (d * d).sum(axis=0), "sum_abs_d": np.abs(d).sum(axis=0),
               "sum_abs_v": np.abs(vz).sum(axis=0), "sum_v2": (vz * vz).sum(axis=0), "w": w, "ok": ok}
        nn = np.where(some, n, 1)
        mean = vz.sum(axis=0) / nn
        dev2 = (np.where(ok, v - mean, 0.0) ** 2).sum(axis=0)
        out["mean"] = np.where(some, mean, np.nan)
        out["dev2"] = dev2
        out["ms"] = np.where(some, out["sum_v2"] / nn, np.nan)
        lo, hi = np.where(ok, w, np.inf).min(axis=0), np.where(ok, w, -np.inf).max(axis=0)
        out["vmin"], out["vmax"] = np.where(some, lo, np.nan), np.where(some, hi, np.nan)
        out["argmin"] = np.where(some, np.argmax(ok & (w == lo), axis=0) + index0, -1)
        out["argmax"] = np.where(some, np.argmax(ok & (w == hi), axis=0) + index0, -1)
        if thr is not None:
            ex, lg, rn = [], [], []
            for t in thr:
                t = np.broadcast_to(np.asarray(t, dtype=np.float32), x.shape[1:])
                ev = ((w <= t) if below else (w >= t)) & ok
                run, longest = np.zeros(x.shape[1:], dtype=np.int64), np.zeros(x.shape[1:], dtype=np.int64)
                for s in range(S):                                   # a skipped sample neither extends nor breaks a run
                    run = np.where(ok[s], np.where(ev[s], run + 1, 0), run)
                    longest = np.maximum(longest, run)
                ex.append(ev.sum(axis=0)), lg.append(longest), rn.append(run)
            out["exceed"], out["longest"], out["run"] = np.stack(ex), np.stack(lg), np.stack(rn)
    return out


def assert_state_matches(state, y, what, per_thr_index=None):
    """state: dict of numpy arrays of one variable shaped like the yardstick's (per threshold: (T, ...)); every point."""
    n = y["n"]
    for k in ("n", "argmin", "argmax"):
        got = state[k] if k == "n" else np.where(n > 0, state[k], -1)
        assert np.array_equal(got, y[k]), (what, k)
    some = n > 0
    for k in ("origin", "vmin", "vmax"):
        want = np.where(some, y[k], 0).astype(np.float32)
        assert np.array_equal(np.where(some, state[k], 0).astype(np.float32).view(np.int32), want.view(np.int32)), (what, k)
    e1, e2 = np.abs(state["s1"] - y["s1"]), np.abs(state["s2"] - y["s2"])
    print(f"{what}: max |s1 error| / bound {np.max(e1 / np.maximum(2 * n * U * y['sum_abs_d'], 1e-300)):.3g}, "
          f"max |s2 error| / bound {np.max(e2 / np.maximum(2 * (n + 1) * U * y['s2'], 1e-300)):.3g}")
    assert (e1 <= 2 * n * U * y["sum_abs_d"]).all(), (what, "s1")
    assert (e2 <= 2 * (n + 1) * U * y["s2"]).all(), (what, "s2")
    if "exceed" in y:
        for k in ("exceed", "run", "longest"):
            assert np.array_equal(state[k], y[k]), (what, k)


def assert_maps_match(acc, name, y, what, ddof=1):
    n = y["n"].astype(np.float64)
    some = n > 0
    nn = np.where(some, n, 1)
    mean, var, rms = (t[name].numpy() for t in (acc.mean, acc.var(ddof), acc.rms))
    assert mean.dtype == var.dtype == rms.dtype == np.float64
    assert np.array_equal(np.isnan(mean), ~some) and np.array_equal(np.isnan(rms), ~some) and np.array_equal(np.isnan(var), n <= ddof)
    tol = U * ((n + 4) * y["sum_abs_v"] / nn + 2 * n * y["sum_abs_d"] / nn)
    assert (np.abs(mean - y["mean"])[some] <= tol[some]).all(), (what, "mean")
    ok = n > ddof
    dn = np.where(ok, n - ddof, 1)
    assert (np.abs(var - y["dev2"] / dn)[ok] <= (3 * (n + 3) * U * y["s2"] / dn)[ok]).all(), (what, "var")
    o = np.abs(y["origin"].astype(np.float64))
    tol = (n + 6) * U * (y["s2"] + 2 * o * y["sum_abs_d"] + n * o * o + y["sum_v2"]) / nn
    assert (np.abs(rms ** 2 - y["ms"])[some] <= tol[some]).all(), (what, "rms")
    for k, prop in (("vmin", acc.min), ("vmax", acc.max)):
        got = prop[name].numpy()
        assert got.dtype == np.float64 and np.array_equal(got[some], y[k][some]) and np.isnan(got[~some]).all(), (what, k)
    for k, prop in (("argmin", acc.argmin), ("argmax", acc.argmax), ("n", acc.count)):
        assert prop[name].dtype == torch.int32 and np.array_equal(prop[name].numpy(), y[k]), (what, k)


def variable_state(acc, name):
    """The raw state of one variable of a (host) accumulator, shaped (B, [C,] H, W); per threshold (T, B, [C,] H, W)."""
    first, shape = next((f, s) for k, _, f, s in acc.layout if k == name)
    n = int(np.prod(shape))
    H, W = acc.mean[name].shape[-2:]
    out = {}
    for k, v in acc.state.items():
        v = v[first:first + n].numpy()
        out[k] = np.moveaxis(v.reshape(*shape, -1, H, W), len(shape), 0) if v.ndim == 3 else v.reshape(*shape, H, W)
    return out


# ---- data --------------------------------------------------------------------------------------------------------------
def make_batch(n_lat, n_lon, seed, B=2, T=2, wind=True, device="cpu"):
    """Pressure-like msl (1e5 +- 300: a raw-value formulation of the variance would lose five digits), 2t, wind components
    at the surface and on two levels, z; two history entries (only the last one is a sample)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda off, sc, *s: (off + sc * torch.randn(*s, n_lat, n_lon, generator=g, dtype=torch.float64)).float()  # noqa: E731
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1)[:-1],
                  time=tuple(datetime(2023, 1, 1, 6) for _ in range(B)), atmos_levels=LEVELS)
    surf = {"2t": r(300, 8, B, T), "msl": r(101325, 300, B, T)}
    atmos = {"z": r(5e4, 500, B, T, len(LEVELS))}
    if wind:
        surf.update({"10u": r(3, 12, B, T), "10v": r(-2, 12, B, T)})
        atmos.update({"u": r(10, 20, B, T, len(LEVELS)), "v": r(0, 20, B, T, len(LEVELS))})
    return Batch(surf, {"lsm": r(0, 1)}, atmos, md).to(device)


THRESHOLDS = {"2t": [303.15, 308.15], "10ws": [17.2], "z": [[5e4, 5.05e4], [4.95e4, float("nan")]]}


def sample_batches(n_lat=9, n_lon=14, S=7, B=2):
    batches = [make_batch(n_lat, n_lon, seed=100 + s, B=B) for s in range(S)]
    batches[2].surf_vars["2t"][:, -1, 1, 2] = float("nan")              # a stray NaN, an infinity, a NaN in a wind component
    batches[4].surf_vars["msl"][0, -1, 3, 3] = float("inf")
    batches[3].surf_vars["10v"][1, -1, 0, 0] = float("nan")
    for b in batches:                                                    # a land mask: never valid
        b.atmos_vars["z"][:, -1, 0, 5:, :3] = float("nan")
    batches[0].surf_vars["2t"][:, -1, 4, 4] = float("nan")              # the first sample is missing: origin from the second
    return batches


def stacked(batches, name, group="surf_vars"):
    return np.stack([getattr(b, group)[name][:, -1].numpy() for b in batches])


def thr_arrays(name, shape):
    """The thresholds of THRESHOLDS[name] as a list of arrays that broadcast against (B, [C,] H, W)."""
    a = np.asarray(THRESHOLDS[name], dtype=np.float32)
    if a.ndim == 1:
        return [np.float32(t) for t in a]
    return [a[:, t].reshape(1, -1, 1, 1) for t in range(a.shape[1])]


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_public_names():
    assert aurora_amd.FieldStats is FieldStats and "FieldStats" in aurora_amd.__all__


@pytest.mark.parametrize("below", [False, True])
def test_the_host_path_equals_the_yardstick(below):
    batches = sample_batches()
    acc = FieldStats(thresholds=THRESHOLDS, below=below, derived=("10ws", "ws"))
    for b in batches:
        assert acc.update(b) is acc
    assert [k for k, *_ in acc.layout] == ["2t", "msl", "10u", "10v", "10ws", "z", "u", "v", "ws"]
    checked = 0
    for name, group, _, shape in acc.layout:
        if name in ("10ws", "ws"):
            a, b = ("10u", "10v") if name == "10ws" else ("u", "v")
            x, second = stacked(batches, a, group), stacked(batches, b, group)
        else:
            x, second = stacked(batches, name, group), None
        thr = thr_arrays(name, shape) if name in THRESHOLDS else None
        y = yardstick(x, second, None, thr, below)
        state = variable_state(acc, name)
        if thr is None:
            state = {k: v for k, v in state.items() if k not in ("exceed", "run", "longest")}
        else:
            state = {k: (v[:len(thr)] if k in ("exceed", "run", "longest") else v) for k, v in state.items()}
        assert_state_matches(state, y, f"{name} below={below}")
        assert_maps_match(acc, name, y, name)
        assert acc.mean[name].shape == (2, 9, 14) if group == "surf_vars" else (2, 2, 9, 14)
        checked += int(np.prod(shape))
        if thr is not None:
            T = 2                                                        # the longest list; shorter ones are padded with NaN
            want = (2, T, 9, 14) if group == "surf_vars" else (2, T, 2, 9, 14)
            ex, lg, fr = acc.exceed_count[name], acc.longest_run[name], acc.exceed_fraction[name]
            assert tuple(ex.shape) == tuple(lg.shape) == tuple(fr.shape) == want and ex.dtype == lg.dtype == torch.int32
            assert np.array_equal(np.moveaxis(ex.numpy(), 1, 0)[:len(thr)], y["exceed"])
            assert np.array_equal(np.moveaxis(lg.numpy(), 1, 0)[:len(thr)], y["longest"])
            frac = np.moveaxis(fr.numpy(), 1, 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                want_frac = y["exceed"] / y["n"]
            keep = ~np.isnan(np.broadcast_to(np.stack([np.broadcast_to(t, y["n"].shape) for t in thr]), want_frac.shape))
            assert np.array_equal(np.isnan(frac[:len(thr)]), ~keep | (y["n"] == 0))
            assert np.array_equal(np.nan_to_num(frac[:len(thr)][keep]), np.nan_to_num(want_frac[keep]))
            if len(thr) < T:
                assert (np.moveaxis(ex.numpy(), 1, 0)[len(thr):] == 0).all() and np.isnan(frac[len(thr):]).all()
    assert checked == acc.state["n"].shape[0] == 2 * (5 + 4 * 2)
    assert set(acc.exceed_count) == set(THRESHOLDS)
    # the planted cases are in: the land mask gives n = 0, NaN and -1; the stray values are skipped, exactly
    assert (acc.count["z"][:, 0, 5:, :3] == 0).all() and torch.isnan(acc.mean["z"][:, 0, 5:, :3]).all()
    assert (acc.argmax["z"][:, 0, 5:, :3] == -1).all() and (acc.count["z"][:, 1] == 7).all()
    assert acc.count["2t"][0, 1, 2] == 6 and acc.count["msl"][0, 3, 3] == 6 and acc.count["msl"][1, 3, 3] == 7
    assert acc.count["10ws"][1, 0, 0] == 6 and acc.count["10v"][1, 0, 0] == 6 and acc.count["10u"][1, 0, 0] == 7
    assert acc.count["2t"][0, 4, 4] == 6 and acc.state["origin"][0].reshape(9, 14)[4, 4] == batches[1].surf_vars["2t"][0, -1, 4, 4]


def test_shifted_sums_keep_the_digits_of_a_pressure():
    """std of msl (1e5 +- 300) to ~1e-13 relative; the raw-value formula in fp64 would be good to ~1e-9 only."""
    batches = sample_batches(S=9)
    acc = FieldStats()
    for b in batches:
        acc.update(b)
    x = stacked(batches, "msl").astype(np.float64)
    x[4, 0, 3, 3] = np.nan
    np.testing.assert_allclose(acc.std(ddof=1)["msl"].numpy(), np.nanstd(x, axis=0, ddof=1), rtol=1e-12)
    np.testing.assert_allclose(acc.mean["msl"].numpy(), np.nanmean(x, axis=0), rtol=1e-14)


@pytest.mark.parametrize("below", [False, True])
def test_planted_runs(below):
    """12 samples at one point with known runs, one of them at the end, a threshold equal to a value, and a skipped sample
    inside a run (it neither extends nor breaks it)."""
    seq = [1, 5, 5, 0, 5, float("nan"), 5, 5, 2, 3, 5, 5]             # thr 5: events at 1,2 | 4,(skip),6,7 | 10,11
    md = Metadata(lat=torch.tensor([10.0, 0.0]), lon=torch.tensor([0.0, 90.0, 180.0]), time=(datetime(2023, 1, 1),), atmos_levels=())
    acc = FieldStats(thresholds={"x": [5.0, 3.0, 6.0]}, below=below)
    for s in seq:
        f = torch.full((1, 1, 2, 3), float(s))
        f[0, 0, 1, 2] = 9.0 if not below else -9.0                      # another point: always an event
        acc.update(Batch({"x": f}, {}, {}, md))
    ex, lg, run = acc.exceed_count["x"][0, :, 0, 0].tolist(), acc.longest_run["x"][0, :, 0, 0].tolist(), \
        acc.state["run"][0, :, 0].tolist()
    if not below:
        assert ex == [7, 8, 0] and lg == [3, 3, 0] and run == [2, 3, 0]
    else:                                                              # <=: thr 5 and 6 always, thr 3: 1 | 0 | 2, 3
        assert ex == [11, 4, 11] and lg == [11, 2, 11] and run == [11, 0, 11]
    assert acc.count["x"][0, 0, 0] == 11 and acc.longest_run["x"][0, 0, 1, 2] == 12
    y = yardstick(np.asarray(seq, dtype=np.float32)[:, None], thr=[5.0, 3.0, 6.0], below=below)
    assert y["exceed"][:, 0].tolist() == ex and y["longest"][:, 0].tolist() == lg and y["run"][:, 0].tolist() == run


def test_over_batch_takes_the_batch_elements_as_samples():
    members = make_batch(5, 8, seed=7, B=6)
    one_by_one, at_once = FieldStats(thresholds={"2t": [300.0]}, derived=("10ws",)), FieldStats(thresholds={"2t": [300.0]}, derived=("10ws",))
    at_once.update(members, over="batch")
    for m in range(6):
        sl = lambda d: {k: v[m:m + 1] for k, v in d.items()}  # noqa: E731
        md = Metadata(members.metadata.lat, members.metadata.lon, members.metadata.time[:1], LEVELS)
        one_by_one.update(Batch(sl(members.surf_vars), members.static_vars, sl(members.atmos_vars), md))
    assert at_once.mean["2t"].shape == (1, 5, 8) and at_once.mean["z"].shape == (1, 2, 5, 8) and (at_once.count["z"] == 6).all()
    for k, v in at_once.state.items():
        assert torch.equal(v, one_by_one.state[k]), k
    y = yardstick(members.surf_vars["2t"][:, -1].numpy()[:, None])
    assert_maps_match(at_once, "2t", y, "over=batch")
    assert len(at_once.as_batch("mean").metadata.time) == 1
    at_once.update(members, over="batch")                               # the sample index runs on over the updates
    assert (at_once.count["2t"] == 12).all() and int(at_once.argmax["2t"].max()) < 6
    with pytest.raises(ValueError, match="2 to 64"):
        FieldStats().update(make_batch(5, 8, seed=1, B=1), over="batch")
    with pytest.raises(ValueError, match="over must be"):
        FieldStats().update(members, over="time")
    with pytest.raises(ValueError, match="batch size"):
        at_once.update(members)


def test_minus_accumulates_the_difference():
    preds = [make_batch(5, 8, seed=20 + s, wind=False) for s in range(5)]
    truths = [make_batch(5, 8, seed=40 + s, wind=False) for s in range(5)]
    truths[1].surf_vars["msl"][0, -1, 2, 2] = float("nan")
    acc = FieldStats(thresholds={"msl": [0.0]})
    for p, t in zip(preds, truths):
        acc.update(p, minus=t)
    for name, group, _, _ in acc.layout:
        x = np.stack([getattr(p, group)[name][:, -1].numpy().astype(np.float64) - getattr(t, group)[name][:, -1].numpy().astype(np.float64)
                      for p, t in zip(preds, truths)])
        w = x.astype(np.float32)
        y = yardstick(w)                                                # w = fp32(x - r), rounded once ...
        for k in ("vmin", "vmax", "argmin", "argmax", "n"):
            got = variable_state(acc, name)[k]
            assert np.array_equal(got, y[k].astype(got.dtype)), (name, k)
        np.testing.assert_allclose(acc.mean[name].numpy(), np.nanmean(x, axis=0), rtol=0, atol=1e-11)   # ... but v is not rounded to fp32
        np.testing.assert_allclose(acc.rms[name].numpy(), np.sqrt(np.nanmean(x * x, axis=0)), rtol=1e-13)
    assert acc.count["msl"][0, 2, 2] == 4
    with pytest.raises(ValueError, match="minus has no variable"):
        FieldStats().update(make_batch(5, 8, seed=1), minus=preds[0])
    with pytest.raises(ValueError, match="differ in lat"):
        FieldStats().update(preds[0], minus=make_batch(6, 8, seed=1, wind=False))
    with pytest.raises(ValueError, match="derived variable '10ws'"):
        FieldStats(derived=("10ws",)).update(make_batch(5, 8, seed=1), minus=make_batch(5, 8, seed=2))


def test_argument_errors():
    b = make_batch(5, 8, seed=3)
    with pytest.raises(ValueError, match="derived offers"):
        FieldStats(derived=("speed",))
    with pytest.raises(ValueError, match="mapping"):
        FieldStats(thresholds=[1.0])
    with pytest.raises(ValueError, match="thresholds name the variable 'tp'"):
        FieldStats(thresholds={"tp": [1.0]}).update(b)
    with pytest.raises(ValueError, match="1 to 8 thresholds"):
        FieldStats(thresholds={"2t": list(range(9))}).update(b)
    with pytest.raises(ValueError, match=r"\(C, T\) array needs C = 2"):
        FieldStats(thresholds={"z": np.zeros((3, 2))}).update(b)
    with pytest.raises(ValueError, match="needs '10u' and '10v'"):
        FieldStats(derived=("10ws",)).update(make_batch(5, 8, seed=3, wind=False))
    with pytest.raises(TypeError, match="must be a Batch"):
        FieldStats().update({"2t": 1})
    with pytest.raises(ValueError, match="BandBatch"):
        FieldStats().update(BandBatch(b.surf_vars, b.static_vars, b.atmos_vars, b.metadata))
    with pytest.raises(ValueError, match="no update yet"):
        FieldStats().mean
    acc = FieldStats().update(b)
    with pytest.raises(ValueError, match="no thresholds"):
        acc.exceed_count
    with pytest.raises(ValueError, match="as_batch offers"):
        acc.as_batch("count")
    with pytest.raises(ValueError, match="differ in lat: 6 against 5"):
        acc.update(make_batch(6, 8, seed=3))
    other = make_batch(5, 8, seed=3)
    other.metadata.lon = other.metadata.lon + 1.0
    with pytest.raises(ValueError, match="differ in lon .same length"):
        acc.update(other)
    other = make_batch(5, 8, seed=3)
    other.metadata.atmos_levels = (1, 2)
    with pytest.raises(ValueError, match="atmos_levels"):
        acc.update(other)
    with pytest.raises(ValueError, match="batch size"):
        acc.update(make_batch(5, 8, seed=3, B=3))
    with pytest.raises(ValueError, match="holds the variables"):
        acc.update(make_batch(5, 8, seed=3, wind=False))
    bad = make_batch(5, 8, seed=3)
    bad.surf_vars["2t"] = bad.surf_vars["2t"][..., :4]
    with pytest.raises(ValueError, match="does not fit a 5 x 8 grid"):
        FieldStats().update(bad)


def test_reset_and_cpu():
    b = make_batch(5, 8, seed=5)
    acc = FieldStats(thresholds={"2t": [300.0]}).update(b).update(make_batch(5, 8, seed=6))
    first = FieldStats(thresholds={"2t": [300.0]}).update(b)
    copy = acc.cpu()
    assert acc.reset() is acc and (acc.count["2t"] == 0).all() and torch.isnan(acc.mean["2t"]).all() and (acc.argmin["z"] == -1).all()
    assert (copy.count["2t"] == 2).all()                                # the copy kept its own state
    acc.update(b)
    for k, v in acc.state.items():
        assert torch.equal(v, first.state[k]), k                        # (argmax 0 again: the sample index was reset too)


def test_as_batch_feeds_scores_and_netcdf(tmp_path):
    batches = [make_batch(9, 16, seed=60 + s) for s in range(4)]
    acc = FieldStats(derived=("10ws", "ws"))
    for b in batches:
        acc.update(b)
    mean = acc.as_batch("mean")
    assert isinstance(mean, Batch) and mean.metadata is batches[-1].metadata and set(mean.static_vars) == {"lsm"}
    assert mean.surf_vars["10ws"].shape == (2, 1, 9, 16) and mean.atmos_vars["ws"].shape == (2, 1, 2, 9, 16)
    assert all(v.dtype == torch.float32 for v in (*mean.surf_vars.values(), *mean.atmos_vars.values()))
    assert torch.equal(mean.surf_vars["2t"][:, 0], acc.mean["2t"].float())
    s = scores(mean, batches[0])                                        # the mean of four against one of them
    assert set(s.rmse) == {"2t", "msl", "10u", "10v", "z", "u", "v"} and bool((s.rmse["2t"] > 0).all())
    spread = acc.as_batch("std", ddof=1)
    assert torch.equal(spread.atmos_vars["z"][:, 0], acc.std(ddof=1)["z"].float())
    path = tmp_path / "mean.nc"
    mean.to_netcdf(path)
    back = Batch.from_netcdf(path)
    assert torch.equal(back.surf_vars["10ws"], mean.surf_vars["10ws"]) and torch.equal(back.atmos_vars["ws"], mean.atmos_vars["ws"])
    assert mean.regrid(45.0).surf_vars["2t"].shape[0] == 2


def test_other_precisions_are_converted_on_the_host():
    b = make_batch(5, 8, seed=8, wind=False)
    acc64 = FieldStats().update(b.type(torch.float64))
    acc32 = FieldStats().update(b)
    assert torch.equal(acc64.mean["z"], acc32.mean["z"])
