"""`aurora_amd.sphere_transform` on the host: coefficients, synthesis and filters on small grids, validity, refusals, and the
yardstick and the bounds that tests/test_gpu_sphere_transform.py holds the device to (no GPU needed).

Yardstick.  `yardstick_analysis` and `yardstick_synthesis` are THE RULE of aurora_amd/sphere_transform.py for one plane in
np.longdouble (u = 2^-64): direct cosine and sine sums (no FFT) over the fp64 tables of the rule converted exactly.  Their own
error is checked below against a 50-digit evaluation.

Bounds (derived, not tuned), of |path - rule| for one plane, u = 2^-53; the text of tests/test_sphere_spectra_host.py has the
first two steps.
  * Coefficients (`coefficient_bound`): that module's D_lm = sum_i |A[m][l][i]| (E_i / N + (H + 2) u |F_m(i)|), E_i = (N + 8) u
    sum_n |x_i[n]|, a bound of the complex modulus |a^_lm - a_lm|.
  * Field (`field_bound`), for coefficients b with an error of at most D (0 where the exact fp64 coefficients are given):
      - inverse Legendre: G_m(i) = sum_l b_lm P[m][l][i] is accumulated over at most lmax + 1 products (steps beyond lmax multiply
        zeros): with the products' rounding (lmax + 2) u sum_l |b_lm| |P|, and D is carried through by the same weights:
            dG_m(i) = sum_l |P[m][l][i]| (D_lm + (lmax + 2) u |b_lm|),      a bound of the modulus |G^_m(i) - G_m(i)|;
      - inverse zonal: the m sum is the DFT sum of `spectra_bound` with lmax + 1 terms in the place of N -- at most lmax + 1
        accumulations, and 8 u for the table entry, the product, the scaling by c_m (exact) and E -+ O -- over the terms' sizes,
        and dG is carried through (|Re(dG e^{i m lambda})| <= |dG|):
            dy_i = sum_m c_m dG_m(i) + (lmax + 1 + 8) u sum_m c_m (|Re G_m(i)| + |Im G_m(i)|);
      - the one rounding to fp32: half an fp32 ulp of the yardstick's value.
    bound_i[n] = dy_i + ulp32(y_i[n]) / 2.
  * Through a second analysis (`carried`): a perturbation d of a field, |d_i[n]| <= d_i, moves F_m(i) by at most d_i (a mean of N
    values times a unit factor) and so a_lm by at most R_lm = sum_i |A[m][l][i]| d_i; a perturbation R of coefficients moves
    the field by at most sum_m c_m sum_l |P[m][l][i]| R_lm."""
import ctypes
import dataclasses
import importlib

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, sphere_analysis, sphere_filter, sphere_spectra, sphere_synthesis
from aurora_amd.batch import BandBatch
from tests.test_sphere_spectra_host import (GRIDS, SMALL, U, entering_rows, metadata, sphere_spectra_bound, surface_batch, synthesis,
                                            yardstick_sphere_spectra)
from tests.verification_inputs import red_noise, red_noise_batch

ss = importlib.import_module("aurora_amd.sphere_spectra")
st = importlib.import_module("aurora_amd.sphere_transform")
LD = np.longdouble


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def _waves(N, lmax, dtype):
    pi = dtype("3.14159265358979323846264338327950288") if dtype is LD else np.pi
    n, m = np.arange(N, dtype=dtype), np.arange(lmax + 1, dtype=dtype)
    ang = (np.outer(m, n) % N) * (2 * pi / N)                            # (the product is exact; reduced before the scaling)
    return np.cos(ang), np.sin(ang)                                      # (lmax + 1, N)


def yardstick_analysis(p, lat, lmax, dtype=LD):
    """ONE plane (H, N): a[re / im][m][l] (2, lmax + 1, lmax + 1), valid, pole rows dropped, straight from the rule in `dtype`."""
    H, N = p.shape
    valid, zeroed = entering_rows(p, None, lat)
    if not valid:
        return np.full((2, lmax + 1, lmax + 1), np.nan), False, int(zeroed.sum())
    A = ss.analysis_table(lat, lmax).astype(dtype)
    C, S = _waves(N, lmax, dtype)
    x = np.where(zeroed[:, None], 0.0, p).astype(dtype)
    Fre, Fim = (x @ C.T) / dtype(N), -(x @ S.T) / dtype(N)              # (H, lmax + 1)
    a = np.zeros((2, lmax + 1, lmax + 1), dtype=dtype)
    for m in range(lmax + 1):
        r = ss.row_of(lmax, m, m)
        Am = A[r:r + lmax + 1 - m]
        a[0, m, m:], a[1, m, m:] = Am @ Fre[:, m], Am @ Fim[:, m]
    return a, True, int(zeroed.sum())


def zonal_coefficients(b, lat, lmax, dtype=LD):
    """G[re / im] (2, H, lmax + 1) of b[re / im][m][l]: INVERSE LEGENDRE of the rule in `dtype`."""
    P = st.synthesis_table(lat, lmax).astype(dtype)
    G = np.zeros((2, len(lat), lmax + 1), dtype=dtype)
    for m in range(lmax + 1):
        r = ss.row_of(lmax, m, m)
        Pm = P[r:r + lmax + 1 - m]
        G[0, :, m], G[1, :, m] = b[0, m, m:].astype(dtype) @ Pm, b[1, m, m:].astype(dtype) @ Pm
    return G


def yardstick_synthesis(b, lat, N, lmax, dtype=LD):
    """ONE plane: y (H, N) in `dtype`, before the rounding to fp32, of b[re / im][m][l] (2, lmax + 1, lmax + 1)."""
    G = zonal_coefficients(b, lat, lmax, dtype)
    C, S = _waves(N, lmax, dtype)
    cm = np.full(lmax + 1, 2.0, dtype=dtype)
    cm[0] = 1.0
    return (G[0] * cm) @ C - (G[1] * cm) @ S


def parts(c):
    """complex (..., L, L) -> [re / im] (2, ..., L, L) fp64"""
    c = np.asarray(c)
    return np.stack([c.real, c.imag])


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def coefficient_bound(p, lat, lmax):
    """D[m][l] of this module's text for one valid plane."""
    H, N = p.shape
    _, zeroed = entering_rows(p, None, lat)
    A = np.abs(ss.analysis_table(lat, lmax))
    x = np.where(zeroed[:, None], 0.0, p).astype(np.float64)
    E = (N + 8) * U * np.abs(x).sum(axis=-1) / N
    F = np.abs(np.fft.rfft(x, axis=-1)[:, :lmax + 1]) / N
    D = np.zeros((lmax + 1, lmax + 1))
    for m in range(lmax + 1):
        r = ss.row_of(lmax, m, m)
        D[m, m:] = A[r:r + lmax + 1 - m] @ (E + (H + 2) * U * F[:, m])
    return D


def carried(R, lat, lmax):
    """sum_m c_m sum_l |P[m][l][i]| R[m][l]: (H,)."""
    P = np.abs(st.synthesis_table(lat, lmax))
    out = np.zeros(len(lat))
    for m in range(lmax + 1):
        r = ss.row_of(lmax, m, m)
        out += (1.0 if m == 0 else 2.0) * (R[m, m:] @ P[r:r + lmax + 1 - m])
    return out


def through_analysis(d, lat, lmax):
    """R[m][l] = sum_i |A[m][l][i]| d_i for a field perturbation of at most d_i in row i."""
    A = np.abs(ss.analysis_table(lat, lmax))
    R = np.zeros((lmax + 1, lmax + 1))
    for m in range(lmax + 1):
        r = ss.row_of(lmax, m, m)
        R[m, m:] = A[r:r + lmax + 1 - m] @ d
    return R


def field_bound(b, D, lat, N, lmax, y):
    """bound[i][n] of this module's text: b[re / im][m][l] fp64, D[m][l] or None, y the yardstick's field."""
    mod = np.hypot(b[0], b[1])
    dG = carried((0.0 if D is None else D) + (lmax + 2) * U * mod, lat, lmax)
    G = np.abs(zonal_coefficients(b, lat, lmax, np.float64))
    cm = np.where(np.arange(lmax + 1) == 0, 1.0, 2.0)
    dy = dG + (lmax + 1 + 8) * U * ((G[0] + G[1]) * cm).sum(axis=-1)
    return dy[:, None] + 0.5 * np.spacing(np.abs(np.asarray(y, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def random_coefficients(lmax, seed, scale=1.0):
    g = np.random.default_rng(seed)
    a = np.zeros((lmax + 1, lmax + 1), dtype=np.complex128)
    for m in range(lmax + 1):
        a[m, m:] = g.standard_normal(lmax + 1 - m) + (1j * g.standard_normal(lmax + 1 - m) if m else 0.0)
    return scale * a


def band_limited(lat, N, lmax, seed, offset=0.0):
    """(b, x): random coefficients and the fp32 rounding of the yardstick's field of them."""
    b = random_coefficients(lmax, seed)
    b[0, 0] += offset
    return b, yardstick_synthesis(parts(b), lat, N, lmax).astype(np.float64).astype(np.float32)


def half_ulp32(x):
    return 0.5 * np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ---- names -------------------------------------------------------------------------------------------------------------------------
def test_public_names():
    for name in ("sphere_analysis", "sphere_synthesis", "sphere_filter", "SphereCoefficients"):
        assert getattr(aurora_amd, name) is getattr(st, name) and name in aurora_amd.__all__
    assert "sphere_transform.hip" in __import__("aurora_amd.build", fromlist=["SOURCES"]).SOURCES
    for word in ("ANALYSIS", "SYNTHESIS TABLE", "INVERSE LEGENDRE", "INVERSE ZONAL", "ALIASING", "FOLDED", "377 MB", "16 (lmax + 1)^2"):
        assert word in st.__doc__, word
    assert "sphere_transform" in ss.__doc__


def test_the_synthesis_table_is_the_basis_without_the_weights():
    lat = GRIDS["17"]
    P, A = st.synthesis_table(lat, 8), ss.analysis_table(lat, 8)
    assert P.shape == A.shape and not P.flags.writeable and np.array_equal(P, ss.basis(lat, 8))
    assert np.array_equal(A, P * (0.5 * ss.quadrature_weights(lat))[None, :])


# ---- the yardstick and the numpy path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", [("9", 16), ("8 without the south pole", 37)])
def test_the_yardstick_against_fifty_digits(name, N):
    """The long-double yardstick's own error is under a tenth of the bounds (it is near 2^-11 of them: u of the format)."""
    import mpmath

    lat = GRIDS[name]
    H = len(lat)
    lmax = ss.largest_lmax(H, N)
    p = red_noise((H, N), seed=1)
    a, valid, dropped = yardstick_analysis(p, lat, lmax)
    assert valid and dropped == 0
    b = parts(random_coefficients(lmax, 2, scale=100.0))
    y = yardstick_synthesis(b, lat, N, lmax)
    A, P = ss.analysis_table(lat, lmax), st.synthesis_table(lat, lmax)

    def mp(v):                                                           # a long double, exactly: its fp64 head and the rest
        head = float(v)
        return mpmath.mpf(head) + mpmath.mpf(float(v - LD(head)))

    with mpmath.workdps(50):
        tw = [(mpmath.cos(2 * mpmath.pi * k / N), mpmath.sin(2 * mpmath.pi * k / N)) for k in range(N)]
        err_a = np.zeros((lmax + 1, lmax + 1))
        err_y = np.zeros((H, N))
        G = [[None] * (lmax + 1) for _ in range(H)]
        for m in range(lmax + 1):
            F = [(sum(mpmath.mpf(float(p[i, n])) * tw[(m * n) % N][0] for n in range(N)) / N,
                  -sum(mpmath.mpf(float(p[i, n])) * tw[(m * n) % N][1] for n in range(N)) / N) for i in range(H)]
            for l in range(m, lmax + 1):
                row = A[ss.row_of(lmax, m, l)]
                exact = [sum(mpmath.mpf(float(row[i])) * F[i][c] for i in range(H)) for c in (0, 1)]
                err_a[m, l] = float(mpmath.sqrt((mp(a[0, m, l]) - exact[0]) ** 2 + (mp(a[1, m, l]) - exact[1]) ** 2))
            for i in range(H):
                G[i][m] = [sum(mpmath.mpf(float(b[c, m, l])) * mpmath.mpf(float(P[ss.row_of(lmax, m, l), i])) for l in range(m, lmax + 1))
                           for c in (0, 1)]
        for i in range(H):
            for n in range(N):
                exact = sum((1 if m == 0 else 2) * (G[i][m][0] * tw[(m * n) % N][0] - G[i][m][1] * tw[(m * n) % N][1])
                            for m in range(lmax + 1))
                err_y[i, n] = float(abs(mp(y[i, n]) - exact))
    D = coefficient_bound(p, lat, lmax)
    live = np.triu(np.ones_like(D, dtype=bool))
    bound = field_bound(b, None, lat, N, lmax, y)
    print(f"{name} x {N}: yardstick error / bound: coefficients {(err_a[live] / D[live]).max():.3e}, field {(err_y / bound).max():.3e}")
    assert (err_a[live] <= 0.1 * D[live]).all() and (err_a[~live] == 0).all() and (err_y <= 0.1 * bound).all()


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("N", (16, 37))
def test_the_numpy_path_is_inside_the_bounds(name, N):
    lat = GRIDS[name]
    H = len(lat)
    lmax = ss.largest_lmax(H, N)
    p = red_noise((2, H, N), seed=H + N)
    a, valid, dropped = st._analysis_host(p, lat, lmax)
    assert a.shape == (2, lmax + 1, lmax + 1) and a.dtype == np.complex128 and valid.all() and not dropped.any()
    for k in range(2):
        want, _, _ = yardstick_analysis(p[k], lat, lmax)
        err = np.hypot(a[k].real - want[0].astype(np.float64), a[k].imag - want[1].astype(np.float64))
        assert (err <= coefficient_bound(p[k], lat, lmax)).all() and (np.tril(a[k], -1) == 0).all()
        b = parts(a[k])                                                  # the yardstick's field of the numpy coefficients
        y = yardstick_synthesis(b, lat, N, lmax)
        got = st._synthesis_host(a[k:k + 1], np.array([True]), lat, N, lmax)[0]
        assert got.dtype == np.float32
        ratio = np.abs(got.astype(np.float64) - y.astype(np.float64)) / field_bound(b, None, lat, N, lmax, y)
        print(f"{name} x {N} plane {k}: max |numpy - yardstick| / bound = {ratio.max():.3e}")
        assert (ratio <= 1).all()


# ---- physics -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", [("9", 16), ("17", 32)])
def test_a_single_harmonic_analyses_to_one_coefficient(name, N):
    lat = GRIDS[name]
    lmax = ss.largest_lmax(len(lat), N)
    a = np.zeros((lmax + 1, lmax + 1), dtype=np.complex128)
    a[1, 2] = 0.5                                                        # Pbar_2^1 cos(lambda) = 2 Re(0.5 e^{i lambda}) Pbar_2^1
    x = synthesis(lat, N, lmax, a)
    P21 = ss.basis(lat, lmax)[ss.row_of(lmax, 1, 2)]
    assert np.abs(x - P21[:, None] * np.cos(2 * np.pi * np.arange(N) / N)[None, :]).max() <= 1e-14
    c = sphere_analysis(surface_batch(lat, {"x": x[None]}))
    got = c.coeff["x"][0].numpy()
    assert got.shape == (lmax + 1, lmax + 1) and c.lmax == lmax and c.degree.tolist() == list(range(lmax + 1))
    assert abs(got[1, 2] - 0.5) <= 1e-13 and np.abs(np.where(a != 0, 0, got)).max() <= 1e-13


@pytest.mark.parametrize("name", ("9", "17"))
def test_a00_is_the_area_mean_of_the_quadrature(name):
    lat = GRIDS[name]
    H, N = len(lat), 20
    p = red_noise((1, H, N), seed=3)
    a00 = sphere_analysis(surface_batch(lat, {"x": p})).coeff["x"][0, 0, 0]
    mean = float((0.5 * ss.quadrature_weights(lat) * p[0].astype(np.float64).mean(axis=-1)).sum())
    # (the bound of the coefficient, and the roundings of the mean formed here: N + H additions of values of at most max |p|)
    assert a00.imag == 0 and abs(a00.real.item() - mean) <= coefficient_bound(p[0], lat, 1)[0, 0] + (H + N + 4) * U * np.abs(p).max()


@pytest.mark.parametrize("name,N", [("9", 16), ("17", 37), ("8 without the south pole", 16), ("12 ascending without poles", 24)])
def test_a_band_limited_field_survives_analysis_then_synthesis(name, N):
    """x = fl32(S b) differs from the band-limited S b by at most half an fp32 ulp, d; analysis then synthesis of the rule returns
    S b + S A (x - S b), so |path - x| <= field bound of the path + carried(through_analysis(d)) + d."""
    lat = GRIDS[name]
    lmax = ss.largest_lmax(len(lat), N)
    _, x = band_limited(lat, N, lmax, seed=len(lat), offset=300.0)
    a, _, _ = st._analysis_host(x[None], lat, lmax)
    got = st._synthesis_host(a, np.array([True]), lat, N, lmax)[0].astype(np.float64)
    d = half_ulp32(x).max(axis=-1)
    bound = field_bound(parts(a[0]), coefficient_bound(x, lat, lmax), lat, N, lmax, x) + (carried(through_analysis(d, lat, lmax), lat, lmax) + d)[:, None]
    ratio = np.abs(got - x) / bound
    print(f"{name} x {N}: max |synthesis(analysis(x)) - x| / bound = {ratio.max():.3e}; in fp32 ulps {np.abs(got - x).max() / np.spacing(np.float32(300)):.2f}")
    assert (ratio <= 1).all()


def test_a_zero_one_response_is_idempotent_and_the_bands_add_up():
    lat, N = GRIDS["17"], 32
    Lmax, L = 8, 3
    x = red_noise_batch(17, N, seed=5)
    low, high, full = sphere_filter(x, lmax=L), sphere_filter(x, lmin=L + 1, lmax=Lmax), sphere_filter(x, lmax=Lmax)
    assert set(low.surf_vars) == {"2t", "msl"} and low.surf_vars["2t"].shape == (2, 1, 17, N) and low.atmos_vars["z"].shape == (2, 1, 3, 17, N)
    assert low.surf_vars["2t"].dtype == torch.float32 and low.static_vars.keys() == x.static_vars.keys() and low.metadata is x.metadata
    twice = sphere_filter(low, lmax=L)
    c = sphere_analysis(x, lmax=Lmax)
    for k, idx, plane in _planes(x):
        lo, hi, fu, tw = (_plane(b, k, idx) for b in (low, high, full, twice))
        # the rule's three fields are exactly additive; each path value is within its field bound of the rule's
        a = c.coeff[k][idx].numpy()
        D = coefficient_bound(plane, lat, Lmax)
        h = (np.arange(Lmax + 1) <= L).astype(np.float64)
        bl, bh, bf = parts(a * h), parts(a * (1 - h)), parts(a)
        fb = lambda b, y: field_bound(b, D, lat, N, Lmax, y)  # noqa: E731
        assert (np.abs((lo + hi) - fu) <= fb(bl, lo) + fb(bh, hi) + fb(bf, fu)).all(), (k, idx)
        # (those bounds are the roundings to fp32 of the two parts and of the whole, half an ulp each, and the fp64 terms)
        # idempotent: the second pass analyses low = S h a + d, |d| within the first bound, and returns S h (a + A d)
        d = fb(bl, lo).max(axis=-1)
        again = field_bound(bl[:, :L + 1, :L + 1], coefficient_bound(lo.astype(np.float32), lat, L) + through_analysis(d, lat, L), lat, N, L, lo)
        assert (np.abs(tw - lo) <= again + d[:, None]).all(), (k, idx)


def _planes(b):
    for grp in ("surf_vars", "atmos_vars"):
        for k, v in getattr(b, grp).items():
            last = v[:, -1].numpy()
            for idx in np.ndindex(*last.shape[:-2]):
                yield k, idx, last[idx]


def _plane(b, k, idx):
    return (b.surf_vars[k] if k in b.surf_vars else b.atmos_vars[k])[:, -1][idx].numpy().astype(np.float64)


def test_the_power_of_a_truncated_field_and_of_the_coefficients():
    """y = fl32-path(S h A x) is the band-limited S h a plus d, |d_i[n]| <= d_i = max_n field bound: analysed again it returns
    h a + A d with |A d|_lm <= R_lm = through_analysis(d).  So the power of y is that of x up to L within
    sum_m c_m (2 |a| R + R^2) plus the bounds of the two spectra, and beyond L at most sum_m c_m R^2 plus the bound of the
    spectrum of y: the level of the fp32 rounding, squared."""
    lat, N, Lmax, L = GRIDS["17"], 32, 8, 4
    p = red_noise((2, 17, N), seed=9)
    x = surface_batch(lat, {"x": p})
    y = sphere_filter(x, lmax=L)
    sx, sy, c = sphere_spectra(x), sphere_spectra(y), sphere_analysis(x)
    cm = np.where(np.arange(Lmax + 1) == 0, 1.0, 2.0)[:, None]
    for k in range(2):
        yk = y.surf_vars["x"][k, 0].numpy()
        a = c.coeff["x"][k].numpy()
        h = (np.arange(Lmax + 1) <= L).astype(np.float64)
        d = field_bound(parts(a[:L + 1, :L + 1]), coefficient_bound(p[k], lat, L), lat, N, L, yk).max(axis=-1)
        R = through_analysis(d, lat, Lmax)
        level = (cm * (2 * np.abs(a * h) * R + R * R)).sum(axis=0) + sphere_spectra_bound(yk, None, lat, Lmax)[0]
        px, py = sx.power["x"][k].numpy(), sy.power["x"][k].numpy()
        kept = level[:L + 1] + sphere_spectra_bound(p[k], None, lat, Lmax)[0][:L + 1]
        print(f"plane {k}: kept degrees |dS| / level {(np.abs(py - px)[:L + 1] / kept).max():.3e}; beyond L: S / level "
              f"{(py[L + 1:] / level[L + 1:]).max():.3e}, S / S_0 {py[L + 1:].max() / py[0]:.3e}")
        assert (np.abs(py - px)[:L + 1] <= kept).all() and (py[L + 1:] <= level[L + 1:]).all()
        # c.power() is the same sum of the same coefficients in another order: inside the bound of the spectrum
        assert (np.abs(c.power()["x"][k].numpy() - px) <= sphere_spectra_bound(p[k], None, lat, Lmax)[0]).all()


def test_a_gaussian_response_leaves_a_constant_field_unchanged():
    lat, N = GRIDS["17"], 32
    l = np.arange(9)
    x = surface_batch(lat, {"x": np.full((1, 17, N), 287.5, dtype=np.float32)})
    y = sphere_filter(x, response=np.exp(-l * (l + 1) * 0.2 ** 2))
    assert y.surf_vars["x"].shape == (1, 1, 17, N) and (y.surf_vars["x"] == 287.5).all()
    z = sphere_filter(x, response=torch.as_tensor(np.exp(-l[:5] * (l[:5] + 1) * 0.2 ** 2)))    # a tensor; the cutoff is its length - 1
    assert (z.surf_vars["x"] == 287.5).all()


def test_scaled_and_coefficients_made_in_torch():
    x = red_noise_batch(17, 32, seed=6)
    c = sphere_analysis(x, lmax=6, only=["z", "2t"])
    assert list(c.coeff) == ["2t", "z"] and c.coeff["z"].shape == (2, 3, 7, 7) and c.coeff["z"].dtype == torch.complex128
    assert c.valid["z"].shape == (2, 3) and c.pole_rows_dropped["2t"].dtype == torch.int32 and c.cpu().table.device.type == "cpu"
    h = np.linspace(1.0, 0.25, 7)
    s = c.scaled(h)
    assert torch.equal(torch.view_as_real(s.table), torch.view_as_real(c.table) * torch.from_numpy(h)[None, None, :, None])
    y = sphere_synthesis(s)
    assert set(y.atmos_vars) == {"z"} and set(y.surf_vars) == {"2t"} and y.atmos_vars["z"].shape == (2, 1, 3, 17, 32)
    # coefficients changed in torch: the difference of two analyses is synthesised on the grid the first was analysed on
    other = sphere_analysis(red_noise_batch(17, 32, seed=7), lmax=6, only=["z", "2t"])
    diff = sphere_synthesis(dataclasses.replace(c, table=c.table - other.table))
    want = sphere_synthesis(c).atmos_vars["z"].double() - sphere_synthesis(other).atmos_vars["z"].double()
    # (three roundings to fp32 of values below 65536, half an ulp each; the fp64 terms of the bounds are below 1e-8 here)
    assert (diff.atmos_vars["z"].double() - want).abs().max() <= 1.5 * np.spacing(np.float32(5e4)) + 1e-8
    with pytest.raises(ValueError, match="7 values"):
        c.scaled(np.ones(6))
    with pytest.raises(ValueError, match="complex128 tensor of shape"):
        sphere_synthesis(dataclasses.replace(c, table=c.table[:, :5, :5]))
    with pytest.raises(TypeError, match="SphereCoefficients"):
        sphere_synthesis(x)


# ---- validity ----------------------------------------------------------------------------------------------------------------------
def test_validity_and_dropped_pole_rows():
    lat, N = GRIDS["17"], 32
    p = red_noise((4, 17, N), seed=9)
    base = sphere_filter(surface_batch(lat, {"x": p}), lmax=5).surf_vars["x"]
    q, z = p.copy(), p.copy()
    q[1, 5, 7] = np.nan                                                  # a NaN plane
    q[2, 0], q[2, -1] = np.nan, np.nan                                   # NaN pole rows, as diagnostics("vo") leaves them
    q[3, -1, 3] = -np.inf                                                # -Inf at a pole
    z[2, 0], z[2, -1], z[3, -1] = 0.0, 0.0, 0.0
    c = sphere_analysis(surface_batch(lat, {"x": q}), lmax=5)
    assert c.valid["x"].tolist() == [True, False, True, True] and c.pole_rows_dropped["x"].tolist() == [0, 0, 2, 1]
    assert torch.isnan(torch.view_as_real(c.table[1])).all() and torch.isnan(c.power()["x"][1]).all()
    assert torch.equal(c.table[[0, 2, 3]], sphere_analysis(surface_batch(lat, {"x": z}), lmax=5).table[[0, 2, 3]])
    y = sphere_synthesis(c).surf_vars["x"]
    assert torch.equal(y[0], base[0]) and torch.isnan(y[1]).all() and torch.isfinite(y[[0, 2, 3]]).all()   # finite poles
    assert torch.equal(y[2:], sphere_filter(surface_batch(lat, {"x": z}), lmax=5).surf_vars["x"][2:])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    x = red_noise_batch(17, 32, seed=1)
    md = x.metadata

    def with_md(b, **kw):
        return Batch(b.surf_vars, b.static_vars, b.atmos_vars, Metadata(**{**dict(lat=md.lat, lon=md.lon, time=md.time,
                     atmos_levels=md.atmos_levels), **kw}))

    for fn in (sphere_analysis, sphere_filter):
        with pytest.raises(ValueError, match="full circle"):
            fn(with_md(x, lon=md.lon * 0.5))                             # a regional grid
        with pytest.raises(ValueError, match=r"lmax = 9 is above .* = 8 .*exact"):
            fn(x, lmax=9)
        with pytest.raises(ValueError, match="BandBatch"):
            fn(BandBatch(x.surf_vars, {}, x.atmos_vars, md, full_patch_rows=4, band=(0, 4)))
        with pytest.raises(ValueError, match="only names the variable 'vo'"):
            fn(x, only=["2t", "vo"])
        with pytest.raises(TypeError, match="must be a Batch"):
            fn(x.surf_vars["2t"])
    with pytest.raises(ValueError, match=r"lmax = 9 is above"):
        sphere_filter(x, response=np.ones(10))                           # a response longer than the limit + 1
    with pytest.raises(ValueError, match="cannot be given with it"):
        sphere_filter(x, lmax=4, response=np.ones(5))
    with pytest.raises(ValueError, match="cannot be given with it"):
        sphere_filter(x, lmin=1, response=np.ones(5))
    with pytest.raises(ValueError, match="must be finite"):
        sphere_filter(x, response=[1.0, np.nan, 1.0])
    with pytest.raises(ValueError, match="sequence of"):
        sphere_filter(x, response=np.ones((3, 3)))
    with pytest.raises(ValueError, match="lmin = 5 is above lmax = 4"):
        sphere_filter(x, lmax=4, lmin=5)
    with pytest.raises(ValueError, match="lmin = 9 is above lmax = 8"):
        sphere_filter(x, lmin=9)
    with pytest.raises(ValueError, match="lmin must be a whole number"):
        sphere_filter(x, lmin=-1)
    # the 1 GiB cap, before any table is built
    H, N = 1441, 1442
    big = Batch({"x": torch.zeros(1, 1, H, N)}, {}, {}, metadata(np.linspace(90, -90, H), N))
    for fn in (sphere_analysis, sphere_filter):
        with pytest.raises(ValueError, match=r"above the cap of 1 GiB; the largest lmax that fits is 430"):
            fn(big)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):     # mixed devices
            sphere_analysis(Batch({"a": x.surf_vars["2t"].cuda(), "b": x.surf_vars["msl"]}, {}, {}, md))


def test_mixed_devices_are_refused():
    """(Where no GPU is present: coefficients on one device and their validity on another.)"""
    c = sphere_analysis(red_noise_batch(9, 16, seed=1), only="2t")
    with pytest.raises(ValueError, match="move the coefficients to the CPU or to one GPU first"):
        sphere_synthesis(dataclasses.replace(c, valid_table=torch.ones(2, dtype=torch.bool, device="meta")))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_workspace_sizes_and_refusals():
    from aurora_amd.build import build_library
    from aurora_amd.engine import lib

    header = (build_library.__globals__["PKG"].parent / "include" / "aurora_hip.h").read_text()
    raw = ctypes.CDLL(str(build_library(force=False, verbose=False)))
    for name in ("aurora_hip_sphere_analysis", "aurora_hip_sphere_analysis_workspace_bytes", "aurora_hip_sphere_synthesis",
                 "aurora_hip_sphere_synthesis_workspace_bytes"):
        assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    for n, H, N, lmax in ((1, 2, 4, 0), (3, 17, 32, 8), (69, 721, 1440, 360), (2, 720, 1440, 359), (5, 65, 130, 17)):
        F = n * 16 * (lmax + 1) * H
        assert lib.sphere_synthesis_workspace_bytes(n, H, N, lmax) == F
        assert lib.sphere_analysis_workspace_bytes(n, H, N, lmax) == -(-(F + n * -(-H // 32) * 8) // 16) * 16
    for args in ((0, 17, 32, 8), (1, 1, 32, 0), (1, 17, 1, 0), (1, 17, 4097, 8), (1, 17, 32, 9), (1, 17, 32, -1)):
        assert lib.sphere_analysis_workspace_bytes(*args) == 0 and lib.sphere_synthesis_workspace_bytes(*args) == 0, args
    L = lib.load()
    err = lambda: L.aurora_hip_last_error()  # noqa: E731
    ana, syn = L.aurora_hip_sphere_analysis, L.aurora_hip_sphere_synthesis
    assert ana(None, 0, 17, 32, 8, 3, None, None, None, None, None, None, 0, None) == 0            # an empty call is a no-op
    assert syn(None, None, 0, 17, 32, 8, None, None, None, None, 0, None) == 0
    assert ana(None, 4, 17, 32, 8, 3, None, None, None, None, None, None, 0, None) == -1 and b"null" in err()
    assert syn(None, None, 4, 17, 32, 8, None, None, None, None, 0, None) == -1 and b"null" in err()
    assert ana(16, 4, 17, 32, 8, 3, 16, 16, 24, 16, 16, 32, 1 << 30, None) == -1 and b"misaligned" in err()
    assert syn(24, None, 4, 17, 32, 8, 16, 16, 16, 32, 1 << 30, None) == -1 and b"misaligned" in err()
    assert ana(16, 4, 17, 32, 8, 3, 16, 16, 16, 16, 16, 32, 64, None) == -1 and b"workspace holds 64 bytes" in err()
    assert syn(16, None, 4, 17, 32, 8, 16, 16, 16, 32, 64, None) == -1 and b"workspace holds 64 bytes" in err()
    assert ana(16, 4, 17, 32, 9, 3, 16, 16, 16, 16, 16, 32, 1 << 30, None) == -1 and b"sphere_analysis: lmax must be in 0..8" in err()
    assert syn(16, None, 4, 17, 32, 9, 16, 16, 16, 32, 1 << 30, None) == -1 and b"sphere_synthesis: lmax must be in 0..8" in err()
    assert ana(16, 4, 1441, 1442, 720, 3, 16, 16, 16, 16, 16, 32, 1 << 40, None) == -1 and b"largest lmax that fits is 430" in err()
    assert syn(16, None, 4, 17, 1, 0, 16, 16, 16, 32, 1 << 30, None) == -1 and b"n_lon" in err()
    assert ana(16, 4, 17, 32, 8, 4, 16, 16, 16, 16, 16, 32, 1 << 30, None) == -1 and b"pole_rows" in err()
    with pytest.raises(AssertionError, match="table"):
        lib.sphere_analysis([torch.zeros(1, 17, 32)], torch.ones(45, 17, dtype=torch.float64), 8, 3)
