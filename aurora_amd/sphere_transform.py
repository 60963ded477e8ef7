"""A field truncated or weighted by TOTAL wavenumber, on its own grid: the step every scorecard that separates scales needs --
RMSE / ACC of the T42-truncated field, the synoptic band alone, the error of the planetary waves, a blur check a map can show
(not in the reference, which has no spectral code).  `sphere_spectra` analyses a field and keeps only the power; this module
gives the coefficients themselves, the synthesis back to the grid, and the two chained with a response in between.  The result
of `sphere_filter` is a `Batch`, so `scores`, `event_scores`, `objects`, `smooth`, `extrema` and `FieldStats` take it unchanged:

    c = aurora_amd.sphere_analysis(batch, lmax=None, only=None)      # -> SphereCoefficients
    c.coeff["2t"]        # (B, lmax + 1 [m], lmax + 1 [l]) complex128 on batch's device, exactly 0 where l < m; c.coeff["z"]: (B, C, ...)
    c.valid, c.pole_rows_dropped, c.degree, c.lmax, c.cpu()          # as in `sphere_spectra`
    c.scaled(response)   # h_l a_lm for a (lmax + 1,) fp64 response: one fp64 multiply in torch, the same bits on either device
    c.power()            # S_l = sum_m c_m |a_lm|^2 in torch (a convenience: `sphere_spectra` stays the fast path for spectra)

    y = aurora_amd.sphere_synthesis(c)                               # -> float32 Batch on the analysed grid
    y = aurora_amd.sphere_filter(batch, lmax=None, *, lmin=0, response=None, only=None)   # analysis -> scale -> synthesis

`sphere_filter(x, lmax=L)` is the triangular truncation, h_l = 1 for lmin <= l <= L and 0 elsewhere; `lmin` makes a high-pass or
a band-pass.  `response` is a sequence of finite numbers indexed by l -- an isotropic Gaussian is
`response=np.exp(-l * (l + 1) * s ** 2)` -- whose length sets the cutoff, len(response) - 1; `lmax` or `lmin` beside it is an
error.  The last history entry of the inputs is used; the outputs are float32, (B, 1, H, W) for a surface variable and (B, 1, C,
H, W) for an atmospheric one, and the returned batch carries the metadata and the static variables of the input, like `smooth`.
`SphereCoefficients` carries the metadata -- the latitudes and longitudes -- it was analysed on: coefficients that were made or
changed in torch (`dataclasses.replace(c, table=...)`, cross-spectra and coherence of forecast and truth are sums over `c.table`)
are synthesised on that grid, and on no other.

THE RULE (stated here; include/aurora_hip.h repeats it for the device; both paths follow it).

ANALYSIS.  GRID, WEIGHTS, BASIS, LMAX, TRANSFORM and VALIDITY of aurora_amd/sphere_spectra.py, without a truth:
    a_lm = sum_i A[m][l][i] F_m(i), rows ascending, with the same table `sphere_spectra.analysis_table`; a dropped pole row
    enters as zeros and is counted; an invalid plane has every coefficient NaN and valid = False; a_lm is exactly 0 where l < m.
SYNTHESIS TABLE.  P[m][l][i] = Pbar_l^m(x_i): `sphere_spectra.basis`, the analysis table without the weights, built in numpy
    only, packed like it (m outermost, then l from m upwards, then the latitude), under the same cap of 1 GiB, and kept per
    (latitudes, lmax) like it.  (It is not A divided by the weights: a quadrature weight may be 0.)
INVERSE LEGENDRE.  G_m(i) = sum_{l = m .. lmax} b_lm P[m][l][i], l ascending, in fp64.
INVERSE ZONAL.  y_i[n] = sum_{m = 0 .. lmax} c_m (Re G_m(i) cos(2 pi m n / N) - Im G_m(i) sin(2 pi m n / N)), c_0 = 1 and
    c_m = 2 otherwise, m ascending (lmax < N / 2: m has no Nyquist column); rounded to fp32 once.  The device forms it FOLDED:
    for 0 <= n <= N/2, E = sum c_m Re G cos and O = sum c_m Im G sin, y[n] = E - O and, for 0 < n < N/2, y[N - n] = E + O.
INVALID PLANES AND DROPPED POLE ROWS.  A plane with valid = False is NaN at every point.  A dropped pole row is synthesised
    like any other row: the output has finite poles.
RESPONSE.  b_lm = h_l a_lm: one fp64 multiplication of the real and of the imaginary part, in torch.
ALIASING.  A field that is not band-limited at lmax aliases under the quadrature: degrees above lmax leak into the a_lm, and
    analysis followed by synthesis is the exact projection onto the degrees up to lmax only for band-limited input (for which
    the quadrature of every product of two basis functions is exact).  On 0.25-degree fields at lmax 360 the leak is what the
    tail of the spectrum holds above 360.

Sizes.  The synthesis table is a second table of (lmax + 1)(lmax + 2) / 2 x H doubles: another 377 MB at 721 rows and lmax 360,
on the device per (latitudes, lmax) and on the host for the last grid and lmax.  Coefficients take 16 (lmax + 1)^2 bytes per plane
(2.1 MB at lmax 360, 144 MB for 69 planes); each of the two device calls has a workspace of 16 (lmax + 1) H bytes per plane (287
MB for 69 planes at 0.25 degrees; `lib.sphere_analysis_workspace_bytes`, `lib.sphere_synthesis_workspace_bytes`), freed to
torch's allocator between them.

Fields on one GPU (fp32 planes) take ONE aurora_hip_sphere_analysis call (the zonal stage of `sphere_spectra`, then its Legendre
stage storing the coefficients where that squares them) and ONE aurora_hip_sphere_synthesis call (the inverse Legendre stage as a
triangular batch of fp64 GEMMs on the matrix pipe, then the folded inverse DFT tile): two launches each.  No floating-point
atomics: the result is repeatable bit for bit, a plane's result does not depend on what else is transformed with it or on
pointer alignment, nothing is read back, and after one eager call on the grid (with the response) the calls can be captured in
a graph.  Fields on the CPU take THE RULE in numpy: `np.fft.rfft` / `np.fft.irfft` and one matrix product per m each way.  The
two paths are not bit-equal; both are held to the same long-double yardstick under a derived bound
(tests/test_sphere_transform_host.py).

Not offered: synthesis onto another grid (spectral regridding), vector harmonics from u and v, degrees above (H - 1) // 2,
latitude bands and `BandBatch`, a truth operand (analyse both fields and subtract the coefficients in torch).
"""

from __future__ import annotations

import dataclasses
import functools
import importlib
from typing import Optional, Sequence

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd.batch import Batch, Metadata

ss = importlib.import_module("aurora_amd.sphere_spectra")   # (the package's attribute of that name is the function)

__all__ = ["sphere_analysis", "sphere_synthesis", "sphere_filter", "SphereCoefficients", "synthesis_table"]

_ON_CAPTURE = ("sphere_transform: call once on this grid, lmax and response before capturing a graph (the tables are uploaded on "
               "the first call, which a captured graph cannot replay)")
_TASK = "transforms float32 fields (move the batch to the CPU for other precisions)"


# ---- the synthesis table -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _table(lat_bytes: bytes, lmax: int) -> np.ndarray:
    with np.errstate(under="ignore"):
        P = ss.basis(np.frombuffer(lat_bytes, dtype=np.float64), lmax)
    P.setflags(write=False)
    return P


def synthesis_table(lat: np.ndarray, lmax: int) -> np.ndarray:
    """P[m][l][i] = Pbar_l^m(x_i), packed like the analysis table: (table_rows(lmax), H) fp64 (kept for the last grid and lmax)."""
    return _table(np.ascontiguousarray(lat, dtype=np.float64).tobytes(), int(lmax))


# ---- the rule on the host ----------------------------------------------------------------------------------------------------
def _analysis_host(x: np.ndarray, lat: np.ndarray, lmax: int):
    """ANALYSIS for an (n_planes, H, N) array in numpy fp64: a (n_planes, lmax + 1 [m], lmax + 1 [l]) complex128, valid,
    pole_rows_dropped."""
    n_planes, H, N = x.shape
    A = ss.analysis_table(lat, lmax)
    f = x.astype(np.float64)
    bad_row = ~np.isfinite(f).all(axis=-1)                                               # (n_planes, H)
    pole = np.abs(lat) == 90.0
    dropped = (bad_row & pole[None, :]).sum(axis=1).astype(np.int32)
    valid = ~(bad_row & ~pole[None, :]).any(axis=1)
    zero = (bad_row & pole[None, :]) | ~valid[:, None]                                  # (an invalid plane is NaN below)
    F = np.fft.rfft(np.where(zero[..., None], 0.0, f), axis=-1)[..., :lmax + 1] / float(N)
    a = np.zeros((n_planes, lmax + 1, lmax + 1), dtype=np.complex128)
    for m in range(lmax + 1):
        a[:, m, m:] = ss.coefficients(A, lmax, m, F[:, :, m])
    a[~valid] = complex(np.nan, np.nan)
    return a, valid, dropped


def _field_host(b: np.ndarray, lat: np.ndarray, N: int, lmax: int) -> np.ndarray:
    """INVERSE LEGENDRE and INVERSE ZONAL for (n_planes, lmax + 1, lmax + 1) complex128 coefficients, before the rounding to
    fp32: (n_planes, H, N) float64."""
    P = synthesis_table(lat, lmax)
    G = np.zeros((b.shape[0], lat.shape[0], N // 2 + 1), dtype=np.complex128)
    for m in range(lmax + 1):
        r = ss.row_of(lmax, m, m)
        Pm, bm = P[r:r + lmax + 1 - m], b[:, m, m:]
        G[:, :, m] = bm.real @ Pm + 1j * (bm.imag @ Pm)
    with np.errstate(invalid="ignore"):
        return np.fft.irfft(G * float(N), n=N, axis=-1)                                 # (irfft divides by N and doubles m > 0)


def _synthesis_host(b: np.ndarray, valid: np.ndarray, lat: np.ndarray, N: int, lmax: int) -> np.ndarray:
    """The synthesis of the rule: `_field_host` rounded to fp32 once, NaN for an invalid plane: (n_planes, H, N) float32."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = _field_host(b, lat, N, lmax).astype(np.float32)
    y[~valid] = np.float32("nan")
    return y


# ---- the result ----------------------------------------------------------------------------------------------------------------
def _response(fn: str, response, length: Optional[int] = None) -> np.ndarray:
    try:
        h = np.array(response, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: response must be a sequence of finite numbers indexed by l") from None
    if h.ndim != 1 or h.size == 0 or (length is not None and h.size != length):
        want = "at least one value" if length is None else f"{length} values (lmax + 1)"
        raise ValueError(f"{fn}: response must be a sequence of {want} indexed by l, got shape {h.shape}")
    if not np.isfinite(h).all():
        raise ValueError(f"{fn}: response must be finite, got {h[~np.isfinite(h)][0]} at l = {int(np.argmin(np.isfinite(h)))}")
    return h


@dataclasses.dataclass(frozen=True)
class SphereCoefficients:
    """Result of `sphere_analysis` and operand of `sphere_synthesis`: every property but `degree` is a dict name -> tensor with
    the leading shape (B,) for a surface variable and (B, C) for an atmospheric one, on the device of the analysed batch."""

    table: torch.Tensor                                    # (n_planes, lmax + 1 [m], lmax + 1 [l]) complex128
    valid_table: torch.Tensor                              # (n_planes,) bool
    dropped_table: torch.Tensor                            # (n_planes,) int32
    layout: _fields.Layout                                 # (name, first plane, shape) per variable
    lmax: int
    metadata: Metadata                                     # of the analysed batch: the grid the coefficients belong to
    static_vars: dict                                      # of the analysed batch, passed through to the synthesis
    surface: tuple[str, ...]                               # the names of `layout` that are surface variables

    @property
    def coeff(self) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, self.table)

    @property
    def valid(self) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, self.valid_table)

    @property
    def pole_rows_dropped(self) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, self.dropped_table)

    @property
    def degree(self) -> torch.Tensor:
        return torch.arange(self.lmax + 1, dtype=torch.int64, device=self.table.device)

    def scaled(self, response) -> "SphereCoefficients":
        """h_l a_lm for a response of lmax + 1 finite numbers indexed by l."""
        h = _response("sphere_transform", response.detach().cpu().numpy() if isinstance(response, torch.Tensor) else response,
                      self.lmax + 1)
        dev = self.table.device
        ht = torch.from_numpy(h) if dev.type == "cpu" else _fields.tables.get(("sphere response", h.tobytes()), dev, lambda: h,
                                                                               _ON_CAPTURE)
        table = torch.view_as_complex(torch.view_as_real(self.table) * ht[None, None, :, None])
        return dataclasses.replace(self, table=table)

    def power(self) -> dict[str, torch.Tensor]:
        """S_l = sum_{m = 0 .. l} c_m |a_lm|^2, (B[, C], lmax + 1) float64, formed in torch."""
        ri = torch.view_as_real(self.table)
        cm = torch.full((self.lmax + 1,), 2.0, dtype=torch.float64)
        cm[0] = 1.0
        cm = cm.to(self.table.device)
        return _fields.by_variable(self.layout, ((ri[..., 0] ** 2 + ri[..., 1] ** 2) * cm[None, :, None]).sum(dim=1))

    def cpu(self) -> "SphereCoefficients":
        """The same coefficients with host tensors (one wait for the device)."""
        return dataclasses.replace(self, table=self.table.cpu(), valid_table=self.valid_table.cpu(),
                                   dropped_table=self.dropped_table.cpu())


# ---- public functions ----------------------------------------------------------------------------------------------------------
def _grid(md: Metadata):
    lat, lon = _fields._host(md.lat), _fields._host(md.lon)
    return lat, lon, lat.shape[0], lon.shape[0]


def _analysis(fn: str, batch: Batch, lmax, only, check=None) -> SphereCoefficients:
    if not isinstance(batch, Batch):
        raise TypeError(f"{fn}: batch must be a Batch, got {type(batch).__name__}")
    _fields.check_vector_grid(fn, batch, "batch", band="fields")
    lat, lon, n_lat, n_lon = _grid(batch.metadata)
    lmax = ss.check_grid(lat, lon, lmax)
    if check is not None:
        check(lmax)
    if isinstance(only, str):
        only = (only,)
    names, fields, layout = _fields.select_one(fn, batch, "batch", only)
    if not names:
        raise ValueError(f"{fn}: batch holds no surface or atmospheric variable")
    device = _fields.place(fn, [("batch", names, fields)], n_lat, n_lon, task=_TASK)
    if device == "cpu":
        a, valid, dropped = (torch.from_numpy(v) for v in _analysis_host(_fields.stack(fields, n_lat, n_lon), lat, lmax))
    else:
        from aurora_amd.engine import lib

        table = _fields.tables.get(("sphere analysis", lat.tobytes(), lmax), device,
                                   lambda: np.array(ss.analysis_table(lat, lmax)), _ON_CAPTURE)   # (shared with `sphere_spectra`)
        a, valid, dropped = lib.sphere_analysis(fields, table, lmax, ss.pole_rows(lat))
    return SphereCoefficients(a, valid, dropped, layout, lmax, batch.metadata, dict(batch.static_vars),
                              tuple(k for k in names if k in batch.surf_vars))


def sphere_analysis(batch: Batch, lmax: Optional[int] = None, only: Optional[Sequence[str]] = None) -> SphereCoefficients:
    """The spherical-harmonic coefficients up to `lmax` of the last history entry of every surface and atmospheric variable of
    `batch` (of those named in `only`); see the module's text."""
    return _analysis("sphere_analysis", batch, lmax, only)


def sphere_synthesis(c: SphereCoefficients) -> Batch:
    """The fields of the coefficients on the grid they were analysed on, as a float32 `Batch` on their device; see the module's
    text."""
    fn = "sphere_synthesis"
    if not isinstance(c, SphereCoefficients):
        raise TypeError(f"{fn}: c must be SphereCoefficients, got {type(c).__name__}")
    lat, lon, n_lat, n_lon = _grid(c.metadata)
    lmax = ss.check_grid(lat, lon, int(c.lmax))
    n_planes = sum(int(np.prod(shape)) for _, _, shape in c.layout)
    if c.table.dtype != torch.complex128 or tuple(c.table.shape) != (n_planes, lmax + 1, lmax + 1):
        raise ValueError(f"{fn}: the coefficients must be a complex128 tensor of shape {(n_planes, lmax + 1, lmax + 1)}, got "
                         f"{c.table.dtype} of shape {tuple(c.table.shape)}")
    if c.valid_table.dtype != torch.bool or tuple(c.valid_table.shape) != (n_planes,):
        raise ValueError(f"{fn}: valid must be a bool tensor of shape {(n_planes,)}, got {c.valid_table.dtype} of shape "
                         f"{tuple(c.valid_table.shape)}")
    device = _fields.device_of(fn, [c.table, c.valid_table], fields="the coefficients and their validity", batches="coefficients")
    if device == "cpu":
        y = torch.from_numpy(_synthesis_host(c.table.detach().numpy(), c.valid_table.numpy(), lat, n_lon, lmax))
    else:
        from aurora_amd.engine import lib

        table = _fields.tables.get(("sphere synthesis", lat.tobytes(), lmax), device,
                                   lambda: np.array(synthesis_table(lat, lmax)), _ON_CAPTURE)    # (a writable copy for the upload)
        y = lib.sphere_synthesis(c.table.contiguous(), table, n_lon, c.valid_table.contiguous())
    by_name = _fields.by_variable(c.layout, y)
    surf = {k: v[:, None] for k, v in by_name.items() if k in c.surface}
    atmos = {k: v[:, None] for k, v in by_name.items() if k not in c.surface}
    return Batch(surf, dict(c.static_vars), atmos, c.metadata)


def sphere_filter(batch: Batch, lmax: Optional[int] = None, *, lmin: int = 0, response=None,
                  only: Optional[Sequence[str]] = None) -> Batch:
    """`batch` with every field weighted by total wavenumber: the triangular truncation at `lmax` (from `lmin` upwards), or h_l
    of `response`; analysis, one multiplication, synthesis; see the module's text."""
    fn = "sphere_filter"
    if response is not None:
        if lmax is not None or lmin != 0:
            raise ValueError(f"{fn}: response sets the cutoff (its length - 1); lmax and lmin cannot be given with it")
        h = _response(fn, response.detach().cpu().numpy() if isinstance(response, torch.Tensor) else response)
        return sphere_synthesis(_analysis(fn, batch, h.size - 1, only).scaled(h))
    if isinstance(lmin, bool) or not isinstance(lmin, (int, np.integer)) or lmin < 0:
        raise ValueError(f"{fn}: lmin must be a whole number of at least 0, got {lmin!r}")

    def check(cutoff: int) -> None:
        if lmin > cutoff:
            raise ValueError(f"{fn}: lmin = {lmin} is above lmax = {cutoff}: the band holds no degree")

    c = _analysis(fn, batch, lmax, only, check)
    h = np.zeros(c.lmax + 1)
    h[int(lmin):] = 1.0
    return sphere_synthesis(c.scaled(h))
