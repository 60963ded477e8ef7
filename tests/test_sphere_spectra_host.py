"""`aurora_amd.sphere_spectra` on the host: the weights, the table, orthonormality, single harmonics and a band-limited
synthesis, validity, the kinetic-energy spectrum, refusals, and the yardstick and the bound that tests/test_gpu_sphere_spectra.py
holds the device to (no GPU needed).

Yardstick.  `yardstick_sphere_spectra` is THE RULE of aurora_amd/sphere_spectra.py for one plane in np.longdouble (u = 2^-64):
direct cosine and sine sums (no FFT), the Legendre sum over the fp64 table of the rule converted exactly, the squares and the m
sum.  Its own error is checked below against a 50-digit evaluation.

Bound (derived, not tuned; `sphere_spectra_bound` evaluates it), of |device - rule| for one plane, with u = 2^-53:
  * Zonal stage.  The DFT term is `spectra_bound`'s (tests/test_spectra_host.py): |X^ - X| <= E_i = (N + 8) u sum_n |x_i[n]|
    for row i, so |dF_m(i)| <= E_i / N for every m.
  * Legendre sum.  a_lm = sum_i A[m][l][i] F_m(i) is accumulated recursively over at most H products (steps that lie beyond
    the rows multiply zeros); with the product's rounding and the two of the scaling by 1 / N that is (H + 2) u sum |A| |F|,
    and the error of F is carried through by the same weights (a complex modulus throughout: Minkowski's inequality takes the
    bounds of the real and the imaginary sums to the modulus):
        D_lm = sum_i |A[m][l][i]| (E_i / N + (H + 2) u |F_m(i)|).
  * The square.  | |a^|^2 - |a|^2 | <= 2 |a| D + D^2.  The error coefficient is a^pred - a^truth of the two accumulators, so
    its D is D(pred) + D(truth).
  * The m sum.  S_l adds at most lmax + 1 nonnegative terms in segments and the segments after them, fewer than 2 (lmax + 1)
    additions; the three roundings of c_m (re^2 + im^2) and the two of the error's differences make six more:
        bound_l = sum_m c_m (2 |a_lm| D_lm + D_lm^2) + (2 (lmax + 1) + 6) u S_l.
A row that enters as zeros (a dropped pole row) has E_i = 0 and F = 0."""
import ctypes
import importlib
import math
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, sphere_spectra
from aurora_amd._sphere import EARTH_RADIUS
from aurora_amd.batch import BandBatch
from tests.verification_inputs import red_noise

ss = importlib.import_module("aurora_amd.sphere_spectra")   # (the package's attribute of that name is the function)

U = 2.0 ** -53
GRIDS = {
    "721": np.linspace(90, -90, 721), "720": np.linspace(90, -89.75, 720), "9": np.linspace(90, -90, 9),
    "17": np.linspace(90, -90, 17), "8 without the south pole": np.linspace(90, -67.5, 8),
    "12 ascending without poles": np.linspace(-82.5, 82.5, 12),
}
SMALL = ("9", "17", "8 without the south pole", "12 ascending without poles")


def metadata(lat, n_lon, B=1, levels=()):
    return Metadata(lat=torch.as_tensor(np.asarray(lat), dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1, dtype=torch.float64)[:-1],
                    time=tuple(datetime(2023, 1, 1, 6) for _ in range(B)), atmos_levels=tuple(levels))


def surface_batch(lat, fields: dict) -> Batch:
    """name -> (B, H, N) array: a batch of surface variables with one history entry."""
    first = next(iter(fields.values()))
    return Batch({k: torch.as_tensor(np.asarray(v))[:, None] for k, v in fields.items()}, {}, {}, metadata(lat, first.shape[-1], first.shape[0]))


# ---- the yardstick and the bound ---------------------------------------------------------------------------------------------
def entering_rows(p, t, lat):
    """(valid, zeroed rows) of one plane by VALIDITY of the rule."""
    bad = ~np.isfinite(p).all(axis=-1)
    if t is not None:
        bad |= ~np.isfinite(t).all(axis=-1)
    pole = np.abs(np.asarray(lat)) == 90.0
    return not (bad & ~pole).any(), bad & pole


def yardstick_sphere_spectra(p, t, lat, lmax, dtype=np.longdouble):
    """ONE plane (H, N): power (1 or 3, lmax + 1), valid, pole rows dropped, straight from the rule in `dtype`."""
    H, N = p.shape
    valid, zeroed = entering_rows(p, t, lat)
    n_fields = 1 if t is None else 3
    if not valid:
        return np.full((n_fields, lmax + 1), np.nan), False, int(zeroed.sum())
    A = ss.analysis_table(lat, lmax).astype(dtype)
    pi = dtype("3.14159265358979323846264338327950288") if dtype is np.longdouble else np.pi
    n, m = np.arange(N, dtype=dtype), np.arange(lmax + 1, dtype=dtype)
    ang = (np.outer(m, n) % N) * (2 * pi / N)                            # (the product is exact; reduced before the scaling)
    C, S = np.cos(ang), np.sin(ang)
    coeff = []
    for x in (p,) if t is None else (p, t):
        x = np.where(zeroed[:, None], 0.0, x).astype(dtype)
        Fre, Fim = (x @ C.T) / dtype(N), -(x @ S.T) / dtype(N)          # (H, lmax + 1)
        a = np.zeros((2, lmax + 1, lmax + 1), dtype=dtype)             # [re / im][m][l]
        for mm in range(lmax + 1):
            r = ss.row_of(lmax, mm, mm)
            Am = A[r:r + lmax + 1 - mm]
            a[0, mm, mm:], a[1, mm, mm:] = Am @ Fre[:, mm], Am @ Fim[:, mm]
        coeff.append(a)
    if t is not None:
        coeff.append(coeff[0] - coeff[1])
    cm = np.full(lmax + 1, 2.0, dtype=dtype)
    cm[0] = 1.0
    power = np.stack([(cm[:, None] * (a[0] ** 2 + a[1] ** 2)).sum(axis=0) for a in coeff])
    return power, True, int(zeroed.sum())


def sphere_spectra_bound(p, t, lat, lmax):
    """The bound of this module's text on |device - rule| for one valid plane: (1 or 3, lmax + 1)."""
    H, N = p.shape
    _, zeroed = entering_rows(p, t, lat)
    A = np.abs(ss.analysis_table(lat, lmax))
    per_field = []
    for x in (p,) if t is None else (p, t):
        x = np.where(zeroed[:, None], 0.0, x).astype(np.float64)
        E = (N + 8) * U * np.abs(x).sum(axis=-1) / N                    # (H,)
        F = np.abs(np.fft.rfft(x, axis=-1)[:, :lmax + 1]) / N           # (H, lmax + 1)
        a = np.zeros((lmax + 1, lmax + 1), dtype=np.complex128)
        D = np.zeros((lmax + 1, lmax + 1))
        Fc = np.fft.rfft(x, axis=-1)[:, :lmax + 1] / N
        for m in range(lmax + 1):
            r = ss.row_of(lmax, m, m)
            Am = A[r:r + lmax + 1 - m]
            D[m, m:] = Am @ (E + (H + 2) * U * F[:, m])
            a[m, m:] = ss.coefficients(ss.analysis_table(lat, lmax), lmax, m, Fc[None, :, m])[0]
        per_field.append((a, D))
    if t is not None:
        per_field.append((per_field[0][0] - per_field[1][0], per_field[0][1] + per_field[1][1]))
    cm = np.full(lmax + 1, 2.0)
    cm[0] = 1.0
    out = []
    for a, D in per_field:
        S = (cm[:, None] * np.abs(a) ** 2).sum(axis=0)
        out.append((cm[:, None] * (2 * np.abs(a) * D + D * D)).sum(axis=0) + (2 * (lmax + 1) + 6) * U * S)
    return np.stack(out)


def test_public_names():
    assert aurora_amd.sphere_spectra is ss.sphere_spectra and aurora_amd.SphereSpectra is ss.SphereSpectra
    assert {"sphere_spectra", "SphereSpectra"} <= set(aurora_amd.__all__)
    assert "sphere_spectra.hip" in __import__("aurora_amd.build", fromlist=["SOURCES"]).SOURCES
    for word in ("least-squares", "synthesis", "coefficients as an output", "vector harmonics", "BandBatch", "16 (lmax + 1) H"):
        assert word in ss.__doc__, word


# ---- weights -------------------------------------------------------------------------------------------------------------------
def clenshaw_curtis(H: int) -> np.ndarray:
    """The closed form on n = H - 1 intervals: w_k = c_k / n (1 - sum_j b_j cos(2 j k pi / n) / (4 j^2 - 1))."""
    n = H - 1
    k = np.arange(H)
    w = np.ones(H)
    for j in range(1, n // 2 + 1):
        w -= (1.0 if 2 * j == n else 2.0) * np.cos(2.0 * j * k * np.pi / n) / (4.0 * j * j - 1.0)
    return w * np.where((k == 0) | (k == n), 1.0, 2.0) / n


@pytest.mark.parametrize("name", ("9", "17", "721"))
def test_weights_of_a_symmetric_grid_with_poles_are_clenshaw_curtis(name):
    w = ss.quadrature_weights(GRIDS[name])
    assert np.abs(w - clenshaw_curtis(len(w))).max() <= 1e-13
    assert abs(w.sum() - 2.0) <= 1e-13


@pytest.mark.parametrize("name", GRIDS)
def test_weights_integrate_every_monomial_below_H(name):
    """A monomial is a combination of Legendre polynomials with nonnegative coefficients that add up to 1, so its quadrature
    error is at most the largest residual of the solved system: H u |V| |w| <= 2 H^2 u for a backward-stable solve (|P_n| <= 1,
    sum |w| about 2), plus 2 H u for the sum taken here."""
    lat = GRIDS[name]
    w = ss.quadrature_weights(lat)
    x, _ = ss.nodes(lat)
    H = len(lat)
    tol = (2 * H * H + 2 * H) * U
    worst = 0.0
    for k in range(H):
        exact = 2.0 / (k + 1) if k % 2 == 0 else 0.0
        worst = max(worst, abs(float((w * x ** k).sum()) - exact))
    print(f"{name}: worst monomial error {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol
    assert abs(w.sum() - 2.0) <= tol and w.min() >= ss.WEIGHT_FLOOR


def test_poles_are_exact_and_a_bad_grid_is_refused():
    x, c = ss.nodes(np.array([90.0, 0.0, -90.0]))
    assert x.tolist() == [1.0, 0.0, -1.0] and c.tolist() == [0.0, 1.0, 0.0]
    lat = np.array([80.0, 79.9999, 79.9998, 10.0, 9.9999, -50.0, -50.0001, -89.0])           # clustered: ill-conditioned
    with pytest.raises(ValueError, match="smallest weight"):
        ss.quadrature_weights(lat)


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_the_table_against_scipy():
    from scipy.special import lpmv

    for lat, lmax in ((GRIDS["17"], 8), (np.linspace(-87, 87, 30), 12)):
        x, _ = ss.nodes(lat)
        P = ss.basis(lat, lmax)
        assert P.shape == (ss.table_rows(lmax), len(lat))
        for m in range(lmax + 1):
            for l in range(m, lmax + 1):
                norm = math.sqrt((2 * l + 1) * math.factorial(l - m) / math.factorial(l + m))
                want = (-1) ** m * norm * lpmv(m, l, x)                 # (scipy carries the Condon-Shortley phase)
                assert np.abs(P[ss.row_of(lmax, m, l)] - want).max() <= 1e-13, (m, l)
        A = ss.analysis_table(lat, lmax)
        assert np.array_equal(A, P * (0.5 * ss.quadrature_weights(lat))[None, :]) and not A.flags.writeable


@pytest.mark.parametrize("name", GRIDS)
def test_orthonormality_at_the_default_lmax(name):
    lat = GRIDS[name]
    H = len(lat)
    lmax = ss.largest_lmax(H, 4096)
    assert lmax == (H - 1) // 2 and {"721": 360, "720": 359}.get(name, lmax) == lmax
    w, P = ss.quadrature_weights(lat), ss.basis(lat, lmax)
    worst, at = 0.0, 0
    for m in range(lmax + 1):
        r = ss.row_of(lmax, m, m)
        Pm = P[r:r + lmax + 1 - m]
        e = float(np.abs(0.5 * (Pm * w) @ Pm.T - np.eye(len(Pm))).max())
        if e > worst:
            worst, at = e, m
    print(f"{name}: max |0.5 sum w Pbar_l^m Pbar_k^m - [l = k]| = {worst:.3e} at m = {at}")
    assert worst <= (1e-12 if name in SMALL else 1e-11)


# ---- harmonics ---------------------------------------------------------------------------------------------------------------
def synthesis(lat, N, lmax, a):
    """sum_l a_l0 Pbar_l^0 + sum_{m > 0} 2 Re(a_lm e^{i m phi}) Pbar_l^m on the grid: a[m][l] complex, (H, N) fp64."""
    P = ss.basis(lat, lmax)
    phi = 2.0 * np.pi * np.arange(N) / N
    f = np.zeros((len(lat), N))
    for m in range(lmax + 1):
        for l in range(m, lmax + 1):
            wave = a[m, l].real * np.cos(m * phi) - a[m, l].imag * np.sin(m * phi)
            f += (1.0 if m == 0 else 2.0) * P[ss.row_of(lmax, m, l)][:, None] * wave[None, :]
    return f


@pytest.mark.parametrize("l,m", [(0, 0), (5, 0), (5, 3), (8, 8), (1, 1)])
def test_a_single_harmonic_has_one_degree(l, m):
    lat, N, lmax = GRIDS["17"], 32, 8
    a = np.zeros((lmax + 1, lmax + 1), dtype=np.complex128)
    a[m, l] = 0.6 - 0.8j if m else 1.0
    s = sphere_spectra(surface_batch(lat, {"x": synthesis(lat, N, lmax, a)[None]}))
    p = s.power["x"][0].numpy()
    assert s.degree.tolist() == list(range(lmax + 1)) and p.shape == (lmax + 1,)
    np.testing.assert_allclose(p[l], 2.0 if m else 1.0, rtol=1e-13)     # c_m |a_lm|^2
    assert (np.delete(p, l) < 1e-27).all()


def test_a_band_limited_synthesis_returns_its_coefficients_and_its_parseval_sum():
    lat, N, lmax = GRIDS["17"], 32, 8
    g = np.random.default_rng(3)
    a = np.zeros((lmax + 1, lmax + 1), dtype=np.complex128)
    for m in range(lmax + 1):
        a[m, m:] = g.standard_normal(lmax + 1 - m) + (1j * g.standard_normal(lmax + 1 - m) if m else 0.0)
    f = synthesis(lat, N, lmax, a)
    A = ss.analysis_table(lat, lmax)
    F = np.fft.rfft(f, axis=-1)[:, :lmax + 1] / N
    worst = max(float(np.abs(ss.coefficients(A, lmax, m, F[None, :, m])[0] - a[m, m:]).max()) for m in range(lmax + 1))
    print(f"max |a_lm returned - a_lm| = {worst:.3e}")
    assert worst <= 1e-13
    s = sphere_spectra(surface_batch(lat, {"x": f[None]}))
    cm = np.where(np.arange(lmax + 1) == 0, 1.0, 2.0)[:, None]
    np.testing.assert_allclose(s.power["x"][0].numpy(), (cm * np.abs(a) ** 2).sum(axis=0), rtol=1e-12)
    area_mean = (0.5 * ss.quadrature_weights(lat) * (f * f).mean(axis=-1)).sum()
    np.testing.assert_allclose(s.power["x"][0].sum().item(), area_mean, rtol=1e-13)


def test_the_numpy_path_equals_a_plain_python_triple_loop():
    lat, N = GRIDS["9"], 16
    lmax = 4
    p = red_noise((1, 9, N), seed=5)
    s = sphere_spectra(surface_batch(lat, {"x": p}))
    A = ss.analysis_table(lat, lmax)
    want = [0.0] * (lmax + 1)
    for m in range(lmax + 1):
        for l in range(m, lmax + 1):
            re = im = 0.0
            for i in range(9):
                fre = sum(float(p[0, i, n]) * math.cos(2 * math.pi * m * n / N) for n in range(N)) / N
                fim = -sum(float(p[0, i, n]) * math.sin(2 * math.pi * m * n / N) for n in range(N)) / N
                re += A[ss.row_of(lmax, m, l), i] * fre
                im += A[ss.row_of(lmax, m, l), i] * fim
            want[l] += (1.0 if m == 0 else 2.0) * (re * re + im * im)
    got = s.power["x"][0].numpy()
    assert np.abs(got - np.asarray(want)).max() <= 1e-12 * max(want)
    assert np.abs(got - np.asarray(want)).max() <= sphere_spectra_bound(p[0], None, lat, lmax).max()


# ---- the yardstick and the bound -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", [("9", 16), ("8 without the south pole", 37), ("12 ascending without poles", 24)])
def test_the_yardstick_against_fifty_digits(name, N):
    """The long-double yardstick's own error is under a tenth of the bound (it is near 2^-11 of it: u of the format)."""
    import mpmath

    lat = GRIDS[name]
    H = len(lat)
    lmax = ss.largest_lmax(H, N)
    p, t = red_noise((H, N), seed=1), red_noise((H, N), seed=2)
    got, valid, dropped = yardstick_sphere_spectra(p, t, lat, lmax)
    assert valid and dropped == 0
    A = ss.analysis_table(lat, lmax)
    with mpmath.workdps(50):
        tw = [(mpmath.cos(2 * mpmath.pi * k / N), mpmath.sin(2 * mpmath.pi * k / N)) for k in range(N)]
        exact = [[mpmath.mpf(0)] * (lmax + 1) for _ in range(3)]
        for m in range(lmax + 1):
            F = []
            for x in (p, t):
                F.append([(sum(mpmath.mpf(float(x[i, n])) * tw[(m * n) % N][0] for n in range(N)) / N,
                           -sum(mpmath.mpf(float(x[i, n])) * tw[(m * n) % N][1] for n in range(N)) / N) for i in range(H)])
            for l in range(m, lmax + 1):
                row = A[ss.row_of(lmax, m, l)]
                a = [[sum(mpmath.mpf(float(row[i])) * F[f][i][c] for i in range(H)) for c in (0, 1)] for f in (0, 1)]
                a.append([a[0][0] - a[1][0], a[0][1] - a[1][1]])
                for f in range(3):
                    exact[f][l] += (1 if m == 0 else 2) * (a[f][0] ** 2 + a[f][1] ** 2)
        def mp(v):                                                       # a long double, exactly: its fp64 head and the rest
            head = float(v)
            return mpmath.mpf(head) + mpmath.mpf(float(v - np.longdouble(head)))

        err = np.array([[float(abs(mp(got[f, l]) - exact[f][l])) for l in range(lmax + 1)] for f in range(3)])
    bound = sphere_spectra_bound(p, t, lat, lmax)
    print(f"{name} x {N}: max yardstick error / bound = {(err / bound).max():.3e}")
    assert (err <= 0.1 * bound).all()
    # ... and the numpy path is inside the bound of the device (it follows the same rule in fp64)
    # (through the rule's own function: a `Metadata` takes descending latitudes only, the rule either direction)
    have, valid, dropped = ss._power_host(p[None], t[None], lat, lmax)
    assert valid.tolist() == [True] and dropped.tolist() == [0]
    assert (np.abs(have[0] - got.astype(np.float64)) <= bound).all()


def test_error_power_is_the_power_of_the_difference():
    lat, N = GRIDS["17"], 32
    p, t = red_noise((2, 17, N), seed=7).astype(np.float64), red_noise((2, 17, N), seed=8).astype(np.float64)
    s = sphere_spectra(surface_batch(lat, {"x": p}), surface_batch(lat, {"x": t}))
    d = sphere_spectra(surface_batch(lat, {"x": p - t}))
    assert s.error_power["x"].shape == (2, 9) and s.ratio is not None and d.ratio is None and d.error_power is None
    for b in range(2):
        bound = sphere_spectra_bound(p[b], t[b], lat, 8)[2] + sphere_spectra_bound(p[b] - t[b], None, lat, 8)[0]
        assert (np.abs(s.error_power["x"][b].numpy() - d.power["x"][b].numpy()) <= bound).all()
    assert torch.equal(s.ratio["x"], s.power["x"] / s.truth_power["x"])


# ---- validity ----------------------------------------------------------------------------------------------------------------------
def test_validity_and_dropped_pole_rows():
    lat, N = GRIDS["17"], 32
    p, t = red_noise((3, 17, N), seed=9), red_noise((3, 17, N), seed=10)
    base = sphere_spectra(surface_batch(lat, {"x": p}), surface_batch(lat, {"x": t}))
    assert base.valid["x"].tolist() == [True] * 3 and base.pole_rows_dropped["x"].tolist() == [0] * 3
    assert base.valid["x"].dtype == torch.bool and base.pole_rows_dropped["x"].dtype == torch.int32
    # a NaN inside a plane invalidates that plane alone
    q = p.copy()
    q[1, 5, 7] = np.nan
    s = sphere_spectra(surface_batch(lat, {"x": q}), surface_batch(lat, {"x": t}))
    assert s.valid["x"].tolist() == [True, False, True] and torch.isnan(s.table[1]).all()
    assert torch.equal(s.table[0], base.table[0]) and torch.equal(s.table[2], base.table[2])
    # NaN pole rows are dropped and counted: the same as zeros in their place
    q, z = p.copy(), p.copy()
    q[0, 0], q[0, -1], q[2, 0, 3] = np.nan, np.inf, -np.inf
    z[0, 0], z[0, -1], z[2, 0] = 0.0, 0.0, 0.0
    s = sphere_spectra(surface_batch(lat, {"x": q}))
    assert s.valid["x"].tolist() == [True] * 3 and s.pole_rows_dropped["x"].tolist() == [2, 0, 1]
    assert torch.equal(s.table, sphere_spectra(surface_batch(lat, {"x": z})).table)
    # a NaN pole row in the truth alone zeroes that row in pred too
    tq, tz = t.copy(), t.copy()
    tq[1, -1, 4] = np.nan
    tz[1, -1] = 0.0
    z = p.copy()
    z[1, -1] = 0.0
    s = sphere_spectra(surface_batch(lat, {"x": p}), surface_batch(lat, {"x": tq}))
    want = sphere_spectra(surface_batch(lat, {"x": z}), surface_batch(lat, {"x": tz}))
    assert s.pole_rows_dropped["x"].tolist() == [0, 1, 0] and torch.equal(s.table, want.table)
    assert not torch.equal(s.table[1, 0], base.table[1, 0])
    # a grid without poles has no row to drop
    lat12 = GRIDS["12 ascending without poles"]
    q = red_noise((1, 12, 24), seed=11)
    q[0, 0, 0] = np.nan
    power, valid, dropped = ss._power_host(q, None, lat12, 5)
    assert valid.tolist() == [False] and dropped.tolist() == [0] and np.isnan(power).all()


# ---- kinetic energy --------------------------------------------------------------------------------------------------------------
def test_kinetic_energy_of_solid_body_rotation():
    lat, N, Uwind = GRIDS["17"], 32, 40.0
    vo = np.broadcast_to((2.0 * Uwind * np.sin(np.deg2rad(lat)) / EARTH_RADIUS)[None, :, None], (2, 17, N)).copy()
    b = surface_batch(lat, {"vo": vo, "d": np.zeros_like(vo), "other": vo})
    s = sphere_spectra(b, b)
    e = s.kinetic_energy()
    assert e.shape == (2, 9) and e.dtype == torch.float64
    np.testing.assert_allclose(e[:, 1].numpy(), Uwind ** 2 / 3.0, rtol=1e-12)
    assert (np.delete(e.numpy(), 1, axis=1) < 1e-24).all() and (e[:, 0] == 0).all()
    assert torch.equal(s.kinetic_energy(vo="vo", d="d", which="truth"), e) and (s.kinetic_energy(which="error") == 0).all()
    with pytest.raises(ValueError, match="'div'"):
        s.kinetic_energy(d="div")
    with pytest.raises(ValueError, match="which"):
        s.kinetic_energy(which="both")
    with pytest.raises(ValueError, match="truth"):
        sphere_spectra(b).kinetic_energy(which="error")


# ---- selection, layout, refusals --------------------------------------------------------------------------------------------------
def test_layout_selection_and_only():
    from tests.verification_inputs import red_noise_batch

    pred, truth = red_noise_batch(17, 32, seed=1), red_noise_batch(17, 32, seed=2)
    s = sphere_spectra(pred, truth)
    assert s.lmax == 8 and s.power["2t"].shape == (2, 9) and s.power["z"].shape == (2, 3, 9) and set(s.power) == {"2t", "msl", "z"}
    assert s.valid["z"].shape == (2, 3) and s.pole_rows_dropped["2t"].shape == (2,) and s.cpu().table.device.type == "cpu"
    one = sphere_spectra(pred, truth, lmax=5, only=["z"])
    assert list(one.power) == ["z"] and one.power["z"].shape == (2, 3, 6)
    assert sphere_spectra(pred, only="msl").power["msl"].shape == (2, 9)
    # the spectrum up to a smaller lmax is the head of the full one (the same table rows, the same products)
    np.testing.assert_allclose(one.power["z"].numpy(), s.power["z"][..., :6].numpy(), rtol=1e-13)
    # the last history entry is the one taken
    pred.surf_vars["2t"][:, 0] = float("nan")
    assert sphere_spectra(pred).valid["2t"].all()


def test_refusals():
    from tests.verification_inputs import red_noise_batch

    pred, truth = red_noise_batch(17, 32, seed=1), red_noise_batch(17, 32, seed=2)
    md = pred.metadata

    def with_md(b, **kw):
        return Batch(b.surf_vars, b.static_vars, b.atmos_vars, Metadata(**{**dict(lat=md.lat, lon=md.lon, time=md.time,
                     atmos_levels=md.atmos_levels), **kw}))

    with pytest.raises(ValueError, match="full circle"):
        sphere_spectra(with_md(pred, lon=md.lon * 0.5))                  # a regional grid
    with pytest.raises(ValueError, match=r"lmax = 9 is above .* = 8 .*exact"):
        sphere_spectra(pred, lmax=9)
    with pytest.raises(ValueError, match="at least 1"):
        sphere_spectra(pred, lmax=0)
    with pytest.raises(ValueError, match="whole number"):
        sphere_spectra(pred, lmax=2.5)
    with pytest.raises(ValueError, match="only names the variable 'vo'"):
        sphere_spectra(pred, only=["2t", "vo"])
    lat, lon = md.lat.numpy(), md.lon.numpy()
    with pytest.raises(ValueError, match="strictly monotonic"):          # (a `Metadata` refuses such latitudes before the rule does)
        ss.check_grid(np.concatenate([lat[:8], lat[7:8], lat[9:]]), lon, None)
    assert ss.check_grid(lat[::-1], lon, None) == 8 and ss.check_grid(lat[1:-1], lon, 3) == 3   # ascending; without poles
    with pytest.raises(ValueError, match="BandBatch"):
        sphere_spectra(BandBatch(truth.surf_vars, {}, truth.atmos_vars, md, full_patch_rows=4, band=(0, 4)))
    with pytest.raises(ValueError, match="matrices"):
        sphere_spectra(with_md(pred, lat=md.lat[:, None].expand(17, 32), lon=md.lon[None, :].expand(17, 32)))
    with pytest.raises(ValueError, match="atmos_levels"):
        sphere_spectra(pred, with_md(truth, atmos_levels=(100, 500, 900)))
    # the 1 GiB cap, before any table is built: 1441 rows at lmax 720 would take 3 GB
    H, N = 1441, 1442
    big = Batch({"x": torch.zeros(1, 1, H, N)}, {}, {}, metadata(np.linspace(90, -90, H), N))
    with pytest.raises(ValueError, match=r"above the cap of 1 GiB; the largest lmax that fits is 430"):
        sphere_spectra(big)
    assert ss.table_rows(430) * H * 8 <= ss.TABLE_CAP < ss.table_rows(431) * H * 8
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):     # mixed devices
            sphere_spectra(pred.to("cuda:0"), truth)


def test_mixed_devices_are_refused_by_the_placement_helper():
    """(The refusal `sphere_spectra` relies on, where no GPU is present: fields on two devices.)"""
    from aurora_amd import _fields

    fields = [torch.zeros(1, 3, 4), torch.zeros(1, 3, 4, device="meta")]
    with pytest.raises(ValueError, match="move the batches to the CPU or to one GPU first"):
        _fields.device_of("sphere_spectra", fields)


def test_tiny_grids_take_their_largest_lmax():
    for H, N, want in ((2, 4, 0), (3, 8, 1), (9, 37, 4)):
        lat = np.linspace(90, -90, H)
        p = red_noise((1, H, N), seed=H)
        s = sphere_spectra(surface_batch(lat, {"x": p}))
        assert s.lmax == want and s.power["x"].shape == (1, want + 1)
        got, _, _ = yardstick_sphere_spectra(p[0], None, lat, want)
        assert (np.abs(s.power["x"][0].numpy() - got.astype(np.float64)) <= sphere_spectra_bound(p[0], None, lat, want)[0]).all()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_library_exports_workspace_size_and_refusals():
    from aurora_amd.build import build_library
    from aurora_amd.engine import lib

    header = (build_library.__globals__["PKG"].parent / "include" / "aurora_hip.h").read_text()
    raw = ctypes.CDLL(str(build_library(force=False, verbose=False)))
    for name in ("aurora_hip_sphere_spectra", "aurora_hip_sphere_spectra_workspace_bytes"):
        assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    ws = lib.sphere_spectra_workspace_bytes
    for n, H, N, lmax, tr in ((1, 2, 4, 0, False), (3, 17, 32, 8, True), (69, 721, 1440, 360, True), (69, 721, 1440, 360, False),
                              (2, 720, 1440, 359, True), (5, 65, 130, 17, False)):
        n_in, n_out, L = (2 if tr else 1), (3 if tr else 1), lmax + 1
        want = n * n_in * 16 * L * H + n * n_out * -(-L // 16) * L * 8 + n * -(-H // 32) * 8
        assert ws(n, H, N, lmax, tr) == -(-want // 16) * 16, (n, H, N, lmax, tr)
    assert ws(69, 721, 1440, 360, False) >= 69 * 16 * 361 * 721            # the figure of the module's text: 287 MB
    for args in ((0, 17, 32, 8, 0), (1, 1, 32, 0, 0), (1, 17, 1, 0, 0), (1, 17, 4097, 8, 0), (1, 17, 32, 9, 0), (1, 17, 32, -1, 0)):
        assert ws(*args) == 0, args
    L = lib.load()
    err = lambda: L.aurora_hip_last_error()  # noqa: E731
    call = L.aurora_hip_sphere_spectra
    assert call(None, None, 0, 17, 32, 8, 3, None, None, None, None, None, None, 0, None) == 0       # an empty call is a no-op
    assert call(None, None, 4, 17, 32, 8, 3, None, None, None, None, None, None, 0, None) == -1 and b"null" in err()
    assert call(16, None, 4, 17, 32, 8, 3, 16, 16, 16, 16, 16, 24, 1 << 30, None) == -1 and b"misaligned" in err()
    assert call(16, None, 4, 17, 32, 8, 3, 16, 16, 16, 16, 16, 32, 64, None) == -1 and b"workspace holds 64 bytes" in err()
    assert call(16, None, 4, 17, 32, 9, 3, 16, 16, 16, 16, 16, 32, 1 << 30, None) == -1 and b"lmax must be in 0..8" in err()
    assert call(16, None, 4, 17, 32, -1, 3, 16, 16, 16, 16, 16, 32, 1 << 30, None) == -1 and b"lmax" in err()
    assert call(16, None, 4, 1441, 1442, 720, 3, 16, 16, 16, 16, 16, 32, 1 << 40, None) == -1
    assert b"cap of 1 GiB" in err() and b"largest lmax that fits is 430" in err()
    assert call(16, None, 4, 17, 1, 0, 0, 16, 16, 16, 16, 16, 32, 1 << 30, None) == -1 and b"n_lon" in err()
    with pytest.raises(AssertionError, match="table"):
        lib.sphere_spectra_power([torch.zeros(1, 17, 32)], None, torch.ones(45, 17, dtype=torch.float64), 8, 3)
