"""`aurora_amd.diagnostics` on the host against a yardstick written HERE, in plain numpy fp64, straight from the formulas of
include/aurora_hip.h (its own row table, its own level weights; nothing of `aurora_amd.diagnostics` but the public function
is called).

Bounds (derived, not tuned; u = 2^-53, gamma_k = k u / (1 - k u)).
Stencils.  y = A ((f_e - f_w) L' + s (m0 a + m1 b + m2 c)), s = -1 (vorticity) or +1 (divergence), with fp32 inputs that are
exact in fp64.  Whatever the order of the additions, and with or without fused multiply-adds, an input reaches the result
through at most 5 roundings (its product, two additions of the three-term sum, the addition of the two parts, the product with
A; the longitude part: difference, product, addition, product) and the tables the two sides build from the same latitudes may
differ by an ulp or two of their own: 8 roundings cover both, so an evaluation is within gamma_8 S of the exact value with
    S = |A| ((|f_e| + |f_w|) |L'| + |m0 a| + |m1 b| + |m2 c|),
and two evaluations differ by at most 2 gamma_8 S.  The fp32 result is a correct rounding of the fp64 one:
    |got - y64| <= 2 gamma_8 S + 1/2 spacing32(max(|got|, |fp32(y64)|)).
The winds carry a large mean (40 + 5 randn), so the differences cancel for real and S is far above |y|.
Columns.  A sum of C terms, each a product of up to three factors: |delta| <= 2 gamma_{C+2} sum |w q u| before the fp32
rounding (tcwv: sum |w q|); ivt = sqrt(ivtu^2 + ivtv^2) is 1-Lipschitz in each sum and its own evaluation (two squares, a sum,
a correctly rounded root) costs 2 u ivt on each side: |delta| <= |delta ivtu| + |delta ivtv| + 4 u ivt.
Wind speed.  Both squares are exact in fp64, their sum is rounded once, the root is correctly rounded and the fp32 rounding is
one more correct rounding on both sides: bit-equal.
Analytic cases.  On an equally spaced grid the latitude stencil is the centred difference of f(phi) = u cos phi, with the
truncation error h^2 / 6 |f'''| + O(h^4); for f = U cos^2 phi, |f'''| = 4 U |sin 2 phi| <= 4 U.  The bound the case states,
(h^2 / 6) 4 U / (a cos phi), is REACHED at 45 degrees up to the h^4 term (6e-5 of it), so what the fp32 grid adds is stated
beside it, not hidden in it: the field handed over is fp32(U cos phi), off by at most 1/2 spacing32 per value, which the
stencil carries to |A| (|m0| e_{i-1} + |m1| e_i + |m2| e_{i+1}); and the evaluation and the fp32 result cost the rounding bound
above.  A case passes within truncation bound + those two rounding terms (together 1.4 % of the truncation bound where they
are largest; the largest error found is 1.0006 of the truncation bound alone, at 45 degrees).
"""
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, FieldStats, Metadata, diagnostics, event_scores, scores
from aurora_amd.batch import BandBatch, derive_metadata

U = 2.0 ** -53
A_EARTH, G = 6371229.0, 9.80665
ALL = ("ws", "vo", "d", "10ws", "10vo", "10d", "tcwv", "ivtu", "ivtv", "ivt")


def gamma(k):
    return k * U / (1 - k * U)


# ---- the yardstick --------------------------------------------------------------------------------------------------
def yardstick_rows(lat):
    """(n_lat, 4) fp64: A, m0, m1, m2 per row, row by row."""
    lat = np.asarray(lat, dtype=np.float64)
    phi = lat * (np.pi / 180.0)
    n = len(lat)
    t = np.zeros((n, 4))
    for i in range(n):
        t[i, 0] = np.nan if abs(lat[i]) >= 90.0 - 1e-9 else 1.0 / (A_EARTH * np.cos(phi[i]))
        if i == 0:
            h2 = phi[1] - phi[0]
            c, rows = (0.0, -1.0 / h2, 1.0 / h2), (0, 0, 1)
        elif i == n - 1:
            h1 = phi[i] - phi[i - 1]
            c, rows = (-1.0 / h1, 1.0 / h1, 0.0), (i - 1, i, i)
        else:
            h1, h2 = phi[i] - phi[i - 1], phi[i + 1] - phi[i]
            c, rows = (-h2 / (h1 * (h1 + h2)), (h2 - h1) / (h1 * h2), h1 / (h2 * (h1 + h2))), (i - 1, i, i + 1)
        for k in range(3):
            t[i, 1 + k] = c[k] * np.cos(phi[rows[k]])
    return t


def longitude_factor(lon, wrap):
    n = len(lon)
    step = 360.0 / n if wrap else (float(lon[-1]) - float(lon[0])) / (n - 1)
    return 1.0 / (2.0 * (step * (np.pi / 180.0)))


def yardstick_wind(u, v, lat, lon, wrap):
    """u, v: (..., n_lat, n_lon) float32.  {"vo": (y64, S), "d": (y64, S), "ws": float32}."""
    u, v = np.asarray(u, dtype=np.float32).astype(np.float64), np.asarray(v, dtype=np.float32).astype(np.float64)
    H, W = u.shape[-2:]
    t = yardstick_rows(lat)
    L = longitude_factor(np.asarray(lon, dtype=np.float64), wrap)
    j = np.arange(W)
    if wrap:
        east, west, Lp = (j + 1) % W, (j - 1) % W, np.full(W, L)
    else:
        east, west = np.minimum(j + 1, W - 1), np.maximum(j - 1, 0)
        Lp = np.where((j == 0) | (j == W - 1), 2.0 * L, L)
    out = {k: (np.empty_like(u), np.empty_like(u)) for k in ("vo", "d")}
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(H):
            A, m0, m1, m2 = t[i]
            north, south = max(i - 1, 0), min(i + 1, H - 1)
            for key, f, g, sign in (("vo", v, u, -1.0), ("d", u, v, 1.0)):
                fe, fw = f[..., i, east], f[..., i, west]
                a, b, c = g[..., north, :], g[..., i, :], g[..., south, :]
                out[key][0][..., i, :] = A * ((fe - fw) * Lp + sign * (m0 * a + m1 * b + m2 * c))
                out[key][1][..., i, :] = abs(A) * ((abs(fe) + abs(fw)) * abs(Lp) + abs(m0 * a) + abs(m1 * b) + abs(m2 * c))
        ws = np.sqrt(u * u + v * v).astype(np.float32)
        ws[~np.isfinite(ws)] = np.nan
    out["ws"] = ws
    return out


def yardstick_weights(levels):
    p = [float(x) for x in levels]
    s = sorted(p)
    w = []
    for x in p:
        k = s.index(x)
        lo, hi = s[max(k - 1, 0)], s[min(k + 1, len(s) - 1)]
        w.append(100.0 * (hi - lo) / (2.0 * G))
    return np.array(w)


def yardstick_columns(q, u, v, levels):
    """q, u, v: (B, C, n_lat, n_lon) float32.  name -> (y64, bound before the fp32 rounding)."""
    q, u, v = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (q, u, v))
    w = yardstick_weights(levels)[None, :, None, None]
    g = 2 * gamma(q.shape[1] + 2)
    with np.errstate(invalid="ignore", over="ignore"):
        t, iu, iv = (w * q).sum(axis=1), (w * q * u).sum(axis=1), (w * q * v).sum(axis=1)
        bt, bu, bv = g * np.abs(w * q).sum(axis=1), g * np.abs(w * q * u).sum(axis=1), g * np.abs(w * q * v).sum(axis=1)
        ivt = np.sqrt(iu * iu + iv * iv)
    return {"tcwv": (t, bt), "ivtu": (iu, bu), "ivtv": (iv, bv), "ivt": (ivt, bu + bv + 4 * U * ivt)}


def assert_within(got, y64, bound, what):
    """|got - y64| <= bound + 1/2 spacing32(max(|got|, |fp32(y64)|)) at every point; NaN exactly where fp32(y64) is not
    finite."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == y64.shape, (what, got.dtype, got.shape, y64.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        y32 = y64.astype(np.float32)
        bad = ~np.isfinite(y32)
        assert np.array_equal(np.isnan(got), bad) and np.isfinite(got[~bad]).all(), (what, "NaN pattern")
        tol = bound + 0.5 * np.spacing(np.maximum(np.abs(got), np.abs(y32))).astype(np.float64)
        err = np.abs(got.astype(np.float64) - y64)
    ok = ~bad
    if ok.any():
        print(f"{what}: max |error| / bound {np.max(err[ok] / np.maximum(tol[ok], 1e-300)):.3g}, "
              f"max |y| / S-bound {np.max(np.abs(y64[ok]) / np.maximum(bound[ok], 1e-300)):.3g}")
    assert (err[ok] <= tol[ok]).all(), what


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN pattern")
    both = ~np.isnan(got)
    assert np.array_equal(got[both].view(np.int32), want[both].view(np.int32)), what


def check_batch(d, batch, wrap, names=ALL, what=""):
    """Every requested field of d = diagnostics(batch, ...) (host tensors) against the yardstick, every point."""
    md = batch.metadata
    lat, lon = md.lat.double().cpu().numpy(), md.lon.double().cpu().numpy()
    last = lambda f: f[:, -1].float().cpu().numpy()  # noqa: E731
    B = next(iter(batch.surf_vars.values())).shape[0]
    for prefix, group, (a, b) in (("", "atmos_vars", ("u", "v")), ("10", "surf_vars", ("10u", "10v"))):
        if not any(prefix + k in names for k in ("ws", "vo", "d")):
            continue
        y = yardstick_wind(last(getattr(batch, group)[a]), last(getattr(batch, group)[b]), lat, lon, wrap)
        for k in ("vo", "d"):
            if prefix + k in names:
                got = getattr(d, group)[prefix + k]
                assert got.shape == (B, 1, *y[k][0].shape[1:]) and got.dtype == torch.float32
                assert_within(got[:, 0].cpu().numpy(), y[k][0], 2 * gamma(8) * y[k][1], f"{what} {prefix + k}")
        if prefix + "ws" in names:
            assert_bit_equal(getattr(d, group)[prefix + "ws"][:, 0].cpu().numpy(), y["ws"], f"{what} {prefix}ws")
    if any(k in names for k in ("tcwv", "ivtu", "ivtv", "ivt")):
        zero = np.zeros_like(last(batch.atmos_vars["q"]))
        y = yardstick_columns(last(batch.atmos_vars["q"]), last(batch.atmos_vars["u"]) if "u" in batch.atmos_vars else zero,
                              last(batch.atmos_vars["v"]) if "v" in batch.atmos_vars else zero, md.atmos_levels)
        for k in ("tcwv", "ivtu", "ivtv", "ivt"):
            if k in names:
                got = d.surf_vars[k]
                assert got.shape == (B, 1, len(lat), len(lon)) and got.dtype == torch.float32
                assert_within(got[:, 0].cpu().numpy(), y[k][0], y[k][1], f"{what} {k}")


# ---- data --------------------------------------------------------------------------------------------------------------
def make_batch(lat, lon, levels=(850, 1000, 500, 700), B=2, T=2, seed=0, device="cpu"):
    """Winds with a large mean (the stencil's differences cancel for real), a specific humidity around 5 g / kg, a
    temperature that the diagnostics do not touch; two history entries (only the last one is used)."""
    lat, lon = torch.as_tensor(lat, dtype=torch.float64), torch.as_tensor(lon, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed)
    H, W, C = len(lat), len(lon), len(levels)
    r = lambda off, sc, *s: (off + sc * torch.randn(*s, H, W, generator=g, dtype=torch.float64)).float()  # noqa: E731
    md = Metadata(lat=torch.linspace(1, -1, H, dtype=torch.float64), lon=torch.linspace(0, 1, W, dtype=torch.float64),
                  time=tuple(datetime(2023, 1, 1, 6) for _ in range(B)), atmos_levels=tuple(levels))
    md = derive_metadata(md, lat=lat, lon=lon)                   # (the constructor takes descending latitudes only)
    surf = {"2t": r(285, 8, B, T), "10u": r(40, 5, B, T), "10v": r(-35, 5, B, T)}
    atmos = {"u": r(40, 5, B, T, C), "v": r(-30, 5, B, T, C), "q": (0.005 * (1 + 0.3 * r(0, 1, B, T, C))).abs(), "t": r(270, 10, B, T, C)}
    return Batch(surf, {"lsm": r(0, 1)}, atmos, md).to(device)


def global_grid(n_lat, n_lon, ascending=False, poles=True):
    lat = np.linspace(90, -90, n_lat) if poles else np.linspace(90, -90, n_lat + 2)[1:-1]
    return (lat[::-1].copy() if ascending else lat), np.arange(n_lon) * (360.0 / n_lon)


GRIDS = {
    "global descending with poles": (*global_grid(19, 36), True),
    "global ascending without poles": (*global_grid(12, 20, ascending=True, poles=False), True),
    "regional unequal latitudes": (np.array([61.0, 58.5, 57.0, 52.0, 51.5, 47.0, 44.0]), 10.0 + 2.5 * np.arange(9), False),
}


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_public_names():
    assert aurora_amd.diagnostics is diagnostics and "diagnostics" in aurora_amd.__all__


@pytest.mark.parametrize("levels,B", [((850, 1000, 500, 700), 2), ((500, 850), 1)])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_the_host_path_equals_the_yardstick(grid, levels, B):
    lat, lon, wrap = GRIDS[grid]
    batch = make_batch(lat, lon, levels, B=B, seed=len(grid) + B)
    d = diagnostics(batch, ALL)
    assert list(d.surf_vars) == [k for k in ALL if k in d.surf_vars] and list(d.atmos_vars) == ["ws", "vo", "d"]
    assert d.metadata.time == batch.metadata.time and d.metadata.atmos_levels == tuple(levels)
    assert d.metadata.lat is batch.metadata.lat and set(d.static_vars) == {"lsm"}
    check_batch(d, batch, wrap, what=grid)
    one = diagnostics(batch, "ivt")                                # a string, and an output on its own
    assert list(one.surf_vars) == ["ivt"] and not one.atmos_vars
    assert torch.equal(one.surf_vars["ivt"], d.surf_vars["ivt"])


def analytic_cases(ascending):
    """1-degree global grid, interior rows: u = U cos(phi), v = 0 has vo = 2 U sin(phi) / a and d = 0; u = 0, v = V cos(phi)
    has d = -2 V sin(phi) / a.  Signs and units.  Returns the fields, checked."""
    lat, lon = global_grid(181, 360, ascending=ascending)
    phi = np.deg2rad(lat)
    speed, h = 40.0, np.deg2rad(1.0)
    profile = torch.from_numpy(speed * np.cos(phi))[None, None, :, None].expand(1, 1, 181, 360).float().contiguous()
    zero = torch.zeros_like(profile)
    md = derive_metadata(make_batch(*global_grid(3, 4), B=1).metadata, lat=torch.from_numpy(lat), lon=torch.from_numpy(lon))
    rows = yardstick_rows(lat)
    A, m = np.abs(rows[:, 0]), np.abs(rows[:, 1:])
    p32 = profile[0, 0, :, 0].numpy()
    e = 0.5 * np.spacing(p32).astype(np.float64)                 # what fp32(U cos phi) is off by, at most
    north, south = np.maximum(np.arange(181) - 1, 0), np.minimum(np.arange(181) + 1, 180)
    quantisation = A * (m[:, 0] * e[north] + m[:, 1] * e + m[:, 2] * e[south])
    S = A * (m[:, 0] * p32[north] + m[:, 1] * p32 + m[:, 2] * p32[south])
    truncation = (h * h / 6) * 4 * speed / (A_EARTH * np.cos(phi))
    interior = slice(1, -1)
    results = {}
    for name, surf, want in (("10vo", {"10u": profile, "10v": zero}, 2 * speed * np.sin(phi) / A_EARTH),
                             ("10d", {"10u": zero, "10v": profile}, -2 * speed * np.sin(phi) / A_EARTH)):
        d = diagnostics(Batch(surf, {}, {}, md), ("10vo", "10d"))
        got = d.surf_vars[name][0, 0].numpy().astype(np.float64)
        other = d.surf_vars["10d" if name == "10vo" else "10vo"][0, 0].numpy()
        rounding = quantisation + 2 * gamma(8) * S + 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        err = np.abs(got - want[:, None]).max(axis=1)
        print(f"{name}: max error / truncation bound {np.max(err[interior] / truncation[interior]):.4f}, rounding terms / "
              f"truncation bound {np.max(rounding[interior] / truncation[interior]):.2e}")
        assert (err[interior] <= (truncation + rounding)[interior]).all(), name
        assert (err[interior] >= 0.5 * truncation[interior] * np.abs(np.sin(2 * phi[interior]))).all()   # (second order, not better)
        # the other field is 0 within the rounding bound: its terms are differences of equal values and products with 0
        assert (np.abs(other[interior]) <= 2 * gamma(8) * S[interior, None]).all(), name
        assert np.isnan(got[[0, -1]]).all()                          # pole rows
        results[name] = got
    return results


def test_solid_body_rotation_and_its_divergent_twin_in_both_latitude_orders():
    a, b = (analytic_cases(asc) for asc in (False, True))                # each checked against the analytic fields ...
    lat, _ = global_grid(181, 360)
    rows = yardstick_rows(lat)
    S = np.abs(rows[:, 0]) * 40.0 * np.abs(rows[:, 1:]).sum(axis=1)
    for name in a:
        x, y = a[name][1:-1], b[name][::-1][1:-1]
        tol = 4 * gamma(8) * S[1:-1, None] + np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
        assert (np.abs(x - y) <= tol).all(), name                        # ... and against each other


def test_poles_infinities_and_nans_stay_where_the_formulas_read_them():
    lat, lon, wrap = GRIDS["global descending with poles"]
    batch = make_batch(lat, lon, B=1, seed=5)
    clean = diagnostics(batch, ALL)
    for k in ("vo", "d"):
        f = clean.atmos_vars[k]
        assert torch.isnan(f[..., [0, -1], :]).all() and torch.isfinite(f[..., 1:-1, :]).all()
    assert torch.isfinite(clean.atmos_vars["ws"]).all() and all(torch.isfinite(clean.surf_vars[k]).all() for k in ("tcwv", "ivt"))

    i, j, W = 7, 0, len(lon)                                       # an infinity in 10u at the wrap column
    batch.surf_vars["10u"][0, -1, i, j] = float("inf")
    batch.atmos_vars["q"][0, -1, 2, 4, 9] = float("nan")           # a NaN in one level of one column
    batch.atmos_vars["v"][0, -1, 1, 11, 3] = float("nan")          # v: ivtv and ivt, and the stencils of level 1
    d = diagnostics(batch, ALL)
    changed = lambda name, group="surf_vars": set(map(tuple, (torch.isnan(getattr(d, group)[name]) &  # noqa: E731
                                                             ~torch.isnan(getattr(clean, group)[name])).nonzero()[:, -2:].tolist()))
    assert changed("10ws") == {(i, j)}
    assert changed("10vo") == {(i - 1, j), (i, j), (i + 1, j)}       # u enters vorticity through the latitude stencil
    assert changed("10d") == {(i, 1), (i, W - 1)}                  # and divergence through the longitude difference (wrapped)
    assert changed("tcwv") == {(4, 9)} and changed("ivtu") == {(4, 9)}
    assert changed("ivtv") == {(4, 9), (11, 3)} and changed("ivt") == {(4, 9), (11, 3)}
    at_level = lambda name: set(map(tuple, (torch.isnan(d.atmos_vars[name]) & ~torch.isnan(clean.atmos_vars[name]))  # noqa: E731
                                    .nonzero()[:, -3:].tolist()))
    assert at_level("ws") == {(1, 11, 3)}
    assert at_level("vo") == {(1, 11, 2), (1, 11, 4)} and at_level("d") == {(1, 10, 3), (1, 11, 3), (1, 12, 3)}
    check_batch(d, batch, wrap, what="with an infinity and NaNs")


def test_trapezoid_weights():
    from aurora_amd.diagnostics import level_weights

    for levels in ((850, 1000, 500, 700), (500, 850), (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)):
        w = level_weights(levels)
        assert np.allclose(w, yardstick_weights(levels), rtol=4 * U, atol=0)
        total = 100.0 * (max(levels) - min(levels)) / G
        assert abs(w.sum() - total) <= gamma(len(levels) + 2) * total
        lat, lon, _ = GRIDS["regional unequal latitudes"]
        batch = make_batch(lat, lon, levels, B=1)
        batch.atmos_vars["q"].fill_(1.0)
        got = diagnostics(batch, "tcwv").surf_vars["tcwv"].numpy().astype(np.float64)
        assert (np.abs(got - total) <= 2 * gamma(len(levels) + 2) * total + 0.5 * np.spacing(np.float32(total))).all()


def test_errors():
    lat, lon, _ = GRIDS["global descending with poles"]
    batch = make_batch(lat, lon)
    with pytest.raises(ValueError, match="which offers .*'10d'.*'ws'.* got 'vort'"):
        diagnostics(batch, ("vo", "vort"))
    with pytest.raises(ValueError, match="names no field"):
        diagnostics(batch, ())
    with pytest.raises(TypeError, match="must be a Batch"):
        diagnostics({"u": 1}, "vo")
    band = BandBatch(batch.surf_vars, batch.static_vars, batch.atmos_vars, batch.metadata)
    with pytest.raises(ValueError, match=r"latitude band \(BandBatch\); gather the forecast first"):
        diagnostics(band, "vo")
    lat2, lon2 = torch.meshgrid(batch.metadata.lat, batch.metadata.lon, indexing="ij")
    matrices = Batch(batch.surf_vars, batch.static_vars, batch.atmos_vars, derive_metadata(batch.metadata, lat=lat2, lon=lon2))
    with pytest.raises(ValueError, match="matrices for latitudes / longitudes; vector coordinates are needed"):
        diagnostics(matrices, "vo")

    def with_md(**changes):
        return Batch(batch.surf_vars, batch.static_vars, batch.atmos_vars, derive_metadata(batch.metadata, **changes))

    bad_lat = torch.from_numpy(lat.copy())
    bad_lat[3] = bad_lat[2]
    with pytest.raises(ValueError, match="strictly monotonic"):
        diagnostics(with_md(lat=bad_lat), "vo")
    bad_lon = torch.from_numpy(lon.copy())
    bad_lon[5] += 1e-4
    with pytest.raises(ValueError, match="equally spaced"):
        diagnostics(with_md(lon=bad_lon), "vo")
    one_row = Batch({k: v[..., :1, :] for k, v in batch.surf_vars.items()}, {}, {}, derive_metadata(batch.metadata, lat=batch.metadata.lat[:1]))
    with pytest.raises(ValueError, match="at least 2 of each"):
        diagnostics(one_row, "10vo")
    one_col = Batch({k: v[..., :1] for k, v in batch.surf_vars.items()}, {}, {}, derive_metadata(batch.metadata, lon=batch.metadata.lon[:1]))
    with pytest.raises(ValueError, match="at least 2 of each"):
        diagnostics(one_col, "10ws")

    no_v = Batch(batch.surf_vars, batch.static_vars, {k: v for k, v in batch.atmos_vars.items() if k != "v"}, batch.metadata)
    with pytest.raises(ValueError, match="'ivt' needs 'v' in batch.atmos_vars"):
        diagnostics(no_v, ("tcwv", "ivtu", "ivt"))
    assert list(diagnostics(no_v, ("tcwv", "ivtu")).surf_vars) == ["tcwv", "ivtu"]
    with pytest.raises(ValueError, match="'10d' needs '10u' in batch.surf_vars"):
        diagnostics(Batch({"10v": batch.surf_vars["10v"]}, {}, batch.atmos_vars, batch.metadata), "10d")
    holds = Batch({**batch.surf_vars, "ivt": batch.surf_vars["2t"]}, {}, batch.atmos_vars, batch.metadata)
    with pytest.raises(ValueError, match="already holds 'ivt'"):
        diagnostics(holds, "ivt")
    wrong = Batch(batch.surf_vars, {}, {**batch.atmos_vars, "u": batch.atmos_vars["u"][..., :-1]}, batch.metadata)
    with pytest.raises(ValueError, match="does not fit a 19 x 36 grid"):
        diagnostics(wrong, "ws")

    one_level = Batch(batch.surf_vars, {}, {k: v[:, :, :1] for k, v in batch.atmos_vars.items()}, derive_metadata(batch.metadata, atmos_levels=(850,)))
    with pytest.raises(ValueError, match="2 to 64 pressure levels, the batch has 1"):
        diagnostics(one_level, "tcwv")
    assert diagnostics(one_level, "vo").atmos_vars["vo"].shape == (2, 1, 1, 19, 36)      # (the stencils take any level count)
    many = Batch({}, {}, {"q": batch.atmos_vars["q"][:, :, :1].expand(2, 2, 65, 19, 36)}, derive_metadata(batch.metadata, atmos_levels=tuple(range(65))))
    with pytest.raises(ValueError, match="2 to 64 pressure levels, the batch has 65"):
        diagnostics(many, "tcwv")
    with pytest.raises(ValueError, match="distinct pressure levels"):
        diagnostics(with_md(atmos_levels=(850, 500, 850, 700)), "tcwv")


def test_keep_holds_the_last_history_entry_of_the_inputs():
    lat, lon, _ = GRIDS["regional unequal latitudes"]
    batch = make_batch(lat, lon)
    d = diagnostics(batch, ("vo", "ivt"), keep=True)
    assert list(d.surf_vars) == ["2t", "10u", "10v", "ivt"] and list(d.atmos_vars) == ["u", "v", "q", "t", "vo"]
    for group in ("surf_vars", "atmos_vars"):
        for k, v in getattr(batch, group).items():
            assert torch.equal(getattr(d, group)[k], v[:, -1:])
    assert torch.equal(d.atmos_vars["vo"], diagnostics(batch, "vo").atmos_vars["vo"])
    assert not diagnostics(batch, "vo").surf_vars


def test_the_result_feeds_the_scorers_field_stats_and_regrid():
    lat, lon, _ = GRIDS["global descending with poles"]
    names = ("vo", "ivt", "10ws")
    pred, truth = (diagnostics(make_batch(lat, lon, seed=s), names) for s in (1, 2))
    s = scores(pred, truth)
    assert set(s.rmse) == set(names) and s.rmse["vo"].shape == (2, 4) and torch.isfinite(s.rmse["vo"]).all()
    assert (s.count["vo"] == 17 * 36).all() and (s.count["ivt"] == 19 * 36).all()          # the pole rows are skipped
    ev = event_scores(pred, truth, {"ivt": [250.0, 500.0]})
    assert ev.hits["ivt"].shape[0] == 2
    acc = FieldStats().update(pred).update(truth)
    assert acc.mean["10ws"].shape == (2, 19, 36) and (acc.count["vo"][:, :, 1:-1] == 2).all() and (acc.count["vo"][:, :, 0] == 0).all()
    coarse = pred.regrid(20.0)
    assert coarse.surf_vars["ivt"].shape[:2] == (2, 1) and coarse.atmos_vars["vo"].shape[:3] == (2, 1, 4)
