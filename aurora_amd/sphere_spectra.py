"""Whether a forecast has blurred, in the units every paper uses: the power spectrum by TOTAL wavenumber l -- the degree of the
spherical harmonics -- per variable and level, of the prediction, of the truth and of the error, and the kinetic-energy
spectrum from vorticity and divergence (not in the reference, which has no spectrum code).  `spectra` gives the zonal spectrum
per latitude band, whose wavenumber is a different length at every latitude; this one can be compared between grids.

    s = aurora_amd.sphere_spectra(pred, truth=None, lmax=None, only=None)
    s.power["2t"]          # (B, lmax + 1) float64 on pred's device; s.power["z"]: (B, C, lmax + 1)
    s.truth_power, s.error_power, s.ratio     # as in `spectra`; None without a truth
    s.valid                # bool per plane; s.pole_rows_dropped int32 per plane
    s.degree               # (lmax + 1,) int64
    s.kinetic_energy(vo="vo", d="d")          # (B[, C], lmax + 1): from the power of two variables of the result
    s.cpu()                # the one call that waits for the device

THE RULE (stated here; include/aurora_hip.h repeats it for the device; both paths follow it).

GRID.  THE GRID RULE of aurora_amd/_sphere.py: a full circle of N equally spaced longitudes, 2 <= N <= 4096 (a regional grid is
    refused); H >= 2 latitudes, strictly monotonic in either direction, with or without pole rows.  x_i = sin(lat_i), exactly
    +-1 where |lat_i| = 90.
WEIGHTS.  The interpolatory quadrature of the latitude nodes: the fp64 solution of sum_i w_i P_n(x_i) = 2 [n = 0], n = 0 .. H-1,
    P_n the Legendre polynomials, solved once per grid on the host (`numpy.polynomial.legendre.legvander`,
    `numpy.linalg.solve`).  On a symmetric grid with poles these are the Clenshaw-Curtis weights.  A grid with a weight below
    -1e-9 or a condition number above 1e6 is refused; the message names the smallest weight.
BASIS.  The 4 pi-normalised associated Legendre functions, (1/2) int Pbar_l^m Pbar_k^m dx = [l = k], by the standard
    recurrences in fp64, every operation rounded on its own, with c_i = cos(lat_i) set to exactly 0 at a pole:
        Pbar_0^0 = 1,   Pbar_m^m = sqrt((2m+1)/(2m)) c Pbar_{m-1}^{m-1},   Pbar_{m+1}^m = sqrt(2m+3) x Pbar_m^m,
        Pbar_l^m = a (x Pbar_{l-1}^m - b Pbar_{l-2}^m),  a = sqrt((4l^2-1)/(l^2-m^2)),  b = sqrt(((l-1)^2-m^2)/(4(l-1)^2-1)).
    Underflow to 0 near the poles is part of the rule.  The analysis table is A[m][l][i] = 0.5 w_i Pbar_l^m(x_i), m <= l <= lmax,
    built in numpy only and packed triangularly (m outermost, then l from m upwards, then the latitude).
LMAX.  The default and the largest accepted value is min((H - 1) // 2, (N - 1) // 2): the quadrature is exact for every
    product of two basis functions up to that degree and no further (360 on the 721-row grid, 359 on the 720-row one).  Any
    lmax from 1 up to it is accepted (and 0 where that is the largest: a grid of two rows has its mean and nothing else).
TRANSFORM.  F_m(i) = (1/N) sum_n x_i[n] exp(-2 pi i m n / N), m = 0 .. lmax, the fp32 inputs converted to fp64 exactly;
    a_lm = sum_i A[m][l][i] F_m(i), rows ascending;  S_l = sum_{m=0..l} c_m |a_lm|^2, c_0 = 1 and c_m = 2 otherwise, m ascending.
    For a field band-limited at lmax, sum_l S_l is the area mean of the squared field.
TRUTH.  With a truth the same S is formed from a^truth and from a^pred - a^truth; ratio = power / truth_power.
VALIDITY.  A plane is valid where every value of every input given is finite; an invalid plane gives NaN in every spectrum
    and valid = False.  One exception serves `diagnostics`, whose pole rows are NaN: a pole row (|lat| = 90) that holds a
    non-finite value in any input enters as zeros in every input; its weight is not redistributed, and it is counted in
    `pole_rows_dropped`.  (Pole rows reach m = 0 only, with a weight of about 2e-6 at 0.25 degrees.)
KINETIC ENERGY.  kinetic_energy(vo, d) is E_l = R^2 (S_l(vo) + S_l(d)) / (2 l (l + 1)) for l >= 1 and E_0 = 0, R the Earth
    radius of aurora_amd/_sphere.py, formed in torch from the power tables with the same bits on either device; of `power` by
    default, of the truth's or the error's with which="truth" | "error".

Sizes.  The table holds (lmax + 1)(lmax + 2) / 2 x H doubles: 377 MB at 721 rows and lmax 360.  It is kept on the device per
(latitudes, lmax), so a second call uploads nothing; a table above 1 GiB is refused on either path (the message names the
largest lmax that fits).  The device path's workspace takes 16 (lmax + 1) H bytes per plane and field -- 287 MB for 69 planes at
0.25 degrees, twice that with a truth -- plus the partial sums (8 (lmax + 1) ceil((lmax + 1) / 16) bytes per plane and
spectrum) and two flag words per plane and 32 rows; `lib.sphere_spectra_workspace_bytes` returns the figure.  On the host the
table of the last grid and lmax stays in memory (one table: 377 MB at production size), and its first upload to a device
makes one more copy for as long as the upload takes.

Fields on one GPU (fp32 planes) are transformed by ONE aurora_hip_sphere_spectra call of three launches: the folded DFT of
`spectra` for m <= lmax, the Legendre stage as a triangular batch of fp64 GEMMs on the matrix pipe, and a finish that adds the
partial sums in a fixed order.  No floating-point atomics: the result is repeatable bit for bit, a plane's spectrum does not
depend on what else is transformed with it, nothing is read back, and after one eager call on the grid the call can be
captured in a graph.  Fields on the CPU take THE RULE in numpy: `np.fft.rfft`, then one matrix product per m with the same
table.

Not offered: degrees above (H - 1) // 2 (a least-squares analysis), synthesis, the coefficients as an output, vector harmonics
from u and v directly, latitude bands and `BandBatch`.  (The coefficients, the synthesis and filters by total wavenumber built
from them are aurora_amd/sphere_transform.py's: `sphere_analysis`, `sphere_synthesis`, `sphere_filter`.)
"""

from __future__ import annotations

import dataclasses
import functools
from typing import Optional, Sequence

import numpy as np
import torch

from aurora_amd import _fields, _sphere
from aurora_amd._sphere import EARTH_RADIUS
from aurora_amd.batch import Batch

__all__ = ["sphere_spectra", "SphereSpectra"]

TABLE_CAP = 1 << 30           # bytes
WEIGHT_FLOOR, CONDITION_CAP = -1e-9, 1e6

_ON_CAPTURE = ("sphere_spectra: call once on this grid and lmax before capturing a graph (the analysis table is uploaded on "
               "the first call, which a captured graph cannot replay)")


# ---- the grid, the weights, the table --------------------------------------------------------------------------------------
def nodes(lat: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(x, c) = (sin lat, cos lat) in fp64, exactly (+-1, 0) at a pole."""
    lat = np.asarray(lat, dtype=np.float64)
    pole = np.abs(lat) == 90.0
    x = np.where(pole, np.sign(lat), np.sin(np.deg2rad(lat)))
    c = np.where(pole, 0.0, np.cos(np.deg2rad(lat)))
    return x, c


def quadrature_weights(lat: np.ndarray) -> np.ndarray:
    """WEIGHTS of the rule for checked latitudes; raises where the grid is refused."""
    x, _ = nodes(lat)
    H = x.shape[0]
    V = np.polynomial.legendre.legvander(x, H - 1)          # V[i][n] = P_n(x_i)
    cond = float(np.linalg.cond(V))
    rhs = np.zeros(H)
    rhs[0] = 2.0
    w = np.linalg.solve(V.T, rhs) if np.isfinite(cond) else np.full(H, np.nan)
    least = float(np.min(w)) if np.all(np.isfinite(w)) else float("nan")
    if not cond <= CONDITION_CAP or not least >= WEIGHT_FLOOR:
        raise ValueError(f"sphere_spectra: the latitudes give no usable quadrature: the smallest weight is {least:.3g} (at "
                         f"least {WEIGHT_FLOOR:g} is needed) and the condition number {cond:.3g} (at most {CONDITION_CAP:g})")
    return w


def largest_lmax(H: int, N: int) -> int:
    return min((H - 1) // 2, (N - 1) // 2)


def table_rows(lmax: int) -> int:
    return (lmax + 1) * (lmax + 2) // 2


def row_of(lmax: int, m: int, l: int) -> int:
    """The row (of H doubles) of (m, l) in the packed table."""
    return m * (lmax + 1) - m * (m - 1) // 2 + (l - m)


def largest_lmax_that_fits(H: int) -> int:
    lmax = -1
    while table_rows(lmax + 1) * H * 8 <= TABLE_CAP:
        lmax += 1
    return lmax


def basis(lat: np.ndarray, lmax: int) -> np.ndarray:
    """BASIS of the rule: Pbar_l^m(x_i) as a (table_rows(lmax), H) fp64 array in the packed order."""
    x, c = nodes(lat)
    P = np.empty((table_rows(lmax), x.shape[0]))
    pmm = np.ones_like(x)
    for m in range(lmax + 1):
        if m > 0:
            pmm = np.sqrt((2.0 * m + 1.0) / (2.0 * m)) * c * pmm
        r = row_of(lmax, m, m)
        P[r] = pmm
        if m < lmax:
            P[r + 1] = np.sqrt(2.0 * m + 3.0) * x * pmm
        for l in range(m + 2, lmax + 1):
            a = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
            k = r + l - m
            P[k] = a * (x * P[k - 1] - b * P[k - 2])
    return P


@functools.lru_cache(maxsize=1)
def _table(lat_bytes: bytes, lmax: int) -> np.ndarray:
    lat = np.frombuffer(lat_bytes, dtype=np.float64)
    with np.errstate(under="ignore"):
        A = basis(lat, lmax) * (0.5 * quadrature_weights(lat))[None, :]
    A.setflags(write=False)
    return A


def analysis_table(lat: np.ndarray, lmax: int) -> np.ndarray:
    """A[m][l][i] = 0.5 w_i Pbar_l^m(x_i), packed: (table_rows(lmax), H) fp64 (kept for the last grid and lmax)."""
    return _table(np.ascontiguousarray(lat, dtype=np.float64).tobytes(), int(lmax))


def check_grid(lat: np.ndarray, lon: np.ndarray, lmax) -> int:
    """GRID and LMAX of the rule: the checked lmax (the default where None)."""
    H, N = lat.shape[0], lon.shape[0]
    if not 2 <= N <= _sphere.MAX_LON:
        raise ValueError(f"sphere_spectra: the grid has {N} longitudes; 2 to {_sphere.MAX_LON} are supported")
    if not _sphere.full_circle(lon):
        raise ValueError("sphere_spectra: the longitudes must be equally spaced and cover the full circle (a spherical-harmonic "
                         "spectrum of a regional or irregular grid is not defined)")
    if H < 2:
        raise ValueError(f"sphere_spectra: the grid has {H} latitude; at least 2 are needed")
    _sphere.check_latitudes("sphere_spectra", lat)
    most = largest_lmax(H, N)
    if lmax is None:
        lmax = most
    if isinstance(lmax, bool) or not isinstance(lmax, (int, np.integer)):
        raise ValueError(f"sphere_spectra: lmax must be a whole number, got {lmax!r}")
    lmax = int(lmax)
    if lmax > most:
        raise ValueError(f"sphere_spectra: lmax = {lmax} is above min((H - 1) // 2, (N - 1) // 2) = {most} on this {H} x {N} "
                         "grid: the quadrature is exact for every product of two basis functions up to that degree and no "
                         "further")
    if lmax < min(1, most):
        raise ValueError(f"sphere_spectra: lmax must be at least {min(1, most)}, got {lmax}")
    if table_rows(lmax) * H * 8 > TABLE_CAP:
        raise ValueError(f"sphere_spectra: the table of lmax = {lmax} on {H} rows takes {table_rows(lmax) * H * 8} bytes, above "
                         f"the cap of 1 GiB; the largest lmax that fits is {largest_lmax_that_fits(H)}")
    return lmax


def pole_rows(lat: np.ndarray) -> int:
    """Bit 0: row 0 is a pole; bit 1: the last row is one (strictly monotonic latitudes have no other)."""
    return int(abs(lat[0]) == 90.0) | (int(abs(lat[-1]) == 90.0) << 1)


# ---- the rule on the host ----------------------------------------------------------------------------------------------------
def _power_host(pred: np.ndarray, truth: Optional[np.ndarray], lat: np.ndarray, lmax: int):
    """THE RULE for (n_planes, H, N) arrays in numpy fp64: power (n_planes, 1 or 3, lmax + 1), valid, pole_rows_dropped."""
    n_planes, H, N = pred.shape
    A = analysis_table(lat, lmax)
    fields = [pred.astype(np.float64)] + ([truth.astype(np.float64)] if truth is not None else [])
    bad_row = np.any([~np.isfinite(f).all(axis=-1) for f in fields], axis=0)            # (n_planes, H)
    pole = np.abs(lat) == 90.0
    dropped = (bad_row & pole[None, :]).sum(axis=1).astype(np.int32)
    valid = ~(bad_row & ~pole[None, :]).any(axis=1)
    zero = (bad_row & pole[None, :]) | ~valid[:, None]                                  # (an invalid plane is NaN below)
    F = [np.fft.rfft(np.where(zero[..., None], 0.0, f), axis=-1)[..., :lmax + 1] / float(N) for f in fields]
    power = np.zeros((n_planes, 3 if truth is not None else 1, lmax + 1))
    for m in range(lmax + 1):
        a = [coefficients(A, lmax, m, f[:, :, m]) for f in F]
        if truth is not None:
            a.append(a[0] - a[1])
        cm = 1.0 if m == 0 else 2.0
        for f, alm in enumerate(a):
            power[:, f, m:] += cm * (alm.real ** 2 + alm.imag ** 2)
    power[~valid] = np.nan
    return power, valid, dropped


def coefficients(A: np.ndarray, lmax: int, m: int, Fm: np.ndarray) -> np.ndarray:
    """a_lm, l = m .. lmax, of the (n_planes, H) complex zonal coefficients F_m: one matrix product with the table's rows of m."""
    r = row_of(lmax, m, m)
    Am = A[r:r + lmax + 1 - m]                                                          # (lmax + 1 - m, H)
    return Fm.real @ Am.T + 1j * (Fm.imag @ Am.T)


# ---- the result ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class SphereSpectra(_fields.PowerViews):
    """Result of `sphere_spectra`: every property but `degree` is a dict name -> tensor with the leading shape (B,) for a
    surface variable and (B, C) for an atmospheric one, on the device of the prediction."""

    table: torch.Tensor                                    # (n_planes, 1 or 3, lmax + 1) float64: pred, truth, error
    valid_table: torch.Tensor                              # (n_planes,) bool
    dropped_table: torch.Tensor                            # (n_planes,) int32
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    lmax: int

    @property
    def valid(self) -> dict[str, torch.Tensor]:
        return self._field(self.valid_table)

    @property
    def pole_rows_dropped(self) -> dict[str, torch.Tensor]:
        return self._field(self.dropped_table)

    @property
    def degree(self) -> torch.Tensor:
        return torch.arange(self.lmax + 1, dtype=torch.int64, device=self.table.device)

    def kinetic_energy(self, vo: str = "vo", d: str = "d", which: str = "pred") -> torch.Tensor:
        """E_l = R^2 (S_l(vo) + S_l(d)) / (2 l (l + 1)) for l >= 1, E_0 = 0, in m^2 s^-2: (B[, C], lmax + 1), from the power of
        the two variables `vo` (relative vorticity) and `d` (divergence) of this result -- of the prediction, or with
        which="truth" | "error" of the truth or the error."""
        tables = {"pred": self.power, "truth": self.truth_power, "error": self.error_power}
        if which not in tables:
            raise ValueError(f"sphere_spectra: which must be 'pred', 'truth' or 'error', got {which!r}")
        by_name = tables[which]
        if by_name is None:
            raise ValueError(f"sphere_spectra: kinetic_energy(which={which!r}) needs a result that was formed with a truth")
        for k in (vo, d):
            if k not in by_name:
                raise ValueError(f"sphere_spectra: kinetic_energy needs the variable {k!r}, which the result does not hold "
                                 f"(it holds {sorted(by_name)})")
        if by_name[vo].shape != by_name[d].shape:
            raise ValueError(f"sphere_spectra: {vo!r} and {d!r} differ in shape: {tuple(by_name[vo].shape)} against "
                             f"{tuple(by_name[d].shape)}")
        l = self.degree.to(torch.float64)
        den = 2.0 * l * (l + 1.0)
        total = (by_name[vo] + by_name[d]) * (EARTH_RADIUS * EARTH_RADIUS)
        e = total / torch.where(den > 0, den, torch.ones_like(den))      # (a quotient of two tensors: the same bits on either device)
        return torch.where(den > 0, e, torch.zeros_like(e))

    def cpu(self) -> "SphereSpectra":
        """The same spectra with host tensors (one wait for the device)."""
        return dataclasses.replace(self, table=self.table.cpu(), valid_table=self.valid_table.cpu(),
                                   dropped_table=self.dropped_table.cpu())


# ---- public function -----------------------------------------------------------------------------------------------------------
def sphere_spectra(pred: Batch, truth: Optional[Batch] = None, lmax: Optional[int] = None,
                   only: Optional[Sequence[str]] = None) -> SphereSpectra:
    """Power spectra by total wavenumber of the last history entry of every surface and atmospheric variable of `pred` (of
    those named in `only`; with a `truth`: of every variable both hold, for pred, truth and pred - truth); see the module's
    text."""
    if not isinstance(pred, Batch):
        raise TypeError(f"sphere_spectra: pred must be a Batch, got {type(pred).__name__}")
    if truth is not None and not isinstance(truth, Batch):
        raise TypeError(f"sphere_spectra: truth must be a Batch or None, got {type(truth).__name__}")
    _fields.check_same_grid("sphere_spectra", pred, truth if truth is not None else pred, "pred", "truth", "the prediction")
    lat, lon = _fields._host(pred.metadata.lat), _fields._host(pred.metadata.lon)
    n_lat, n_lon = lat.shape[0], lon.shape[0]
    lmax = check_grid(lat, lon, lmax)
    if isinstance(only, str):
        only = (only,)
    others = [("truth", truth)] if truth is not None else []
    names, fields, layout = _fields.select_pair("sphere_spectra", pred, others, only)
    for k in (only if only is not None else ()):
        if k not in names:
            raise ValueError(f"sphere_spectra: only names the variable {k!r}, which pred" + (" and truth do" if others else " does")
                             + " not hold as a surface or atmospheric variable")
    if not names:
        raise ValueError("sphere_spectra: pred and truth have no surface or atmospheric variable in common" if others
                         else "sphere_spectra: pred has no surface or atmospheric variable")
    device = _fields.place("sphere_spectra", [(what, names, fs) for what, fs in zip(("pred", "truth"), fields)], n_lat, n_lon,
                           task="transforms float32 fields (move the batches to the CPU for other precisions)")
    if device == "cpu":
        power, valid, dropped = _power_host(_fields.stack(fields[0], n_lat, n_lon),
                                            _fields.stack(fields[1], n_lat, n_lon) if others else None, lat, lmax)
        power, valid, dropped = torch.from_numpy(power), torch.from_numpy(valid), torch.from_numpy(dropped)
    else:
        from aurora_amd.engine import lib

        table = _fields.tables.get(("sphere analysis", lat.tobytes(), lmax), device,
                                   lambda: np.array(analysis_table(lat, lmax)), _ON_CAPTURE)   # (a writable copy for the upload)
        power, valid, dropped = lib.sphere_spectra_power(fields[0], fields[1] if others else None, table, lmax, pole_rows(lat))
    return SphereSpectra(power, valid, dropped, layout, lmax)
