"""Whether a forecast keeps its small scales: latitude-weighted zonal power spectra per variable and level, of the
prediction, of the truth and of the error (not in the reference, which has no spectrum code).

    s = aurora_amd.spectra(pred, truth=None, bands=None)    # bands: sequence of (south, north) in degrees; default ((-90, 90),)
    s.power["2t"]       # (B, n_bands, K)    float64, on pred's device
    s.power["z"]        # (B, C, n_bands, K) one spectrum per pressure level
    s.truth_power, s.error_power     # the same for truth and for pred - truth; None without a truth
    s.ratio             # power / truth_power: below 1 at high wavenumbers where the forecast has blurred
    s.rows              # int64 (B, [C,] n_bands): the valid rows behind each spectrum
    s.wavenumber        # (K,) int64: 0 .. K-1
    s.cpu()             # the same object with host tensors: the one call that waits for the device

For one plane (n_lat x n_lon, N = n_lon) and its row i, with K = N // 2 + 1:

    X_i[k] = sum_n x_i[n] exp(-2 pi i k n / N),  k = 0 .. K-1          P_i[k] = c_k |X_i[k]|^2 / N^2

with c_0 = 1, c_{N/2} = 1 for an even N and c_k = 2 otherwise, so that sum_k P_i[k] = mean_n x_i[n]^2 (Parseval).  A row is
VALID when all N values of every input present (pred and, if given, truth) are finite; an invalid row contributes nothing.
Row i belongs to the band (south, north) when south <= lat_i <= north, and with w_i = `latitude_weights(lat)[i]`

    S_b[k] = sum_{i valid, i in b} w_i P_i[k] / sum_{i valid, i in b} w_i        rows_b = the number of valid rows in b;

a band without a valid row gives NaN and rows 0.  With a truth the same S is formed for pred, for truth and for the error
d = pred - truth (in fp64; the transform is linear, so the device takes X_pred - X_truth); over the full band
sum_k S_err[k] = sum w d^2 / sum w, which is `scores(pred, truth).rmse ** 2` when every point is finite.

Fields on one GPU are transformed by ONE aurora_hip_spectra call: the fp32 rows are converted to fp64 exactly and multiplied
on the fp64 matrix pipe against a cosine / sine table computed on the host in fp64 (an fp32 transform of a 500 hPa
geopotential row would carry an error above the tail it is meant to measure).  The result is repeatable bit for bit, a
plane's spectrum does not depend on what else is transformed with it, and nothing is read back, so a roll-out can be
tracked step by step and read once at the end.  Fields on the CPU take the same quantities in numpy fp64 (`np.fft.rfft` of the
fp64 cast).
"""

from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._fields import MAX_LON, latitude_weights  # noqa: F401  (MAX_LON: the limit lives with the longitude check)
from aurora_amd.batch import Batch

__all__ = ["spectra", "Spectra"]

MAX_BANDS = 8


@dataclasses.dataclass(frozen=True)
class Spectra(_fields.PowerViews):
    """Result of `spectra`: every property but `wavenumber` is a dict name -> tensor with the leading shape (B,) for a surface
    variable and (B, C) for an atmospheric one, on the device of the prediction."""

    table: torch.Tensor                                  # (n_planes, 1 or 3, n_bands, K) float64: pred, truth, error
    rows_table: torch.Tensor                             # (n_planes, n_bands) int64
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    bands: tuple[tuple[float, float], ...]

    @property
    def rows(self) -> dict[str, torch.Tensor]:
        return self._field(self.rows_table)

    @property
    def wavenumber(self) -> torch.Tensor:
        return torch.arange(self.table.shape[-1], dtype=torch.int64, device=self.table.device)

    def cpu(self) -> "Spectra":
        """The same spectra with host tensors (one wait for the device)."""
        return dataclasses.replace(self, table=self.table.cpu(), rows_table=self.rows_table.cpu())


# ---- bands -------------------------------------------------------------------------------------------------------
def _check_bands(bands) -> tuple[tuple[float, float], ...]:
    if bands is None:
        return ((-90.0, 90.0),)
    try:
        out = tuple((float(s), float(n)) for s, n in bands)
    except (TypeError, ValueError):
        raise ValueError("spectra: bands must be a sequence of (south, north) pairs in degrees") from None
    if not 1 <= len(out) <= MAX_BANDS:
        raise ValueError(f"spectra: 1 to {MAX_BANDS} bands can be taken at a time, got {len(out)}")
    for s, n in out:
        if not (-90.0 <= s <= n <= 90.0):
            raise ValueError(f"spectra: a band needs -90 <= south <= north <= 90, got ({s}, {n})")
    return out


def band_weights(lat: np.ndarray, bands: Sequence[tuple[float, float]]) -> np.ndarray:
    """(n_bands, n_lat) fp64: `latitude_weights(lat)[i]` where south <= lat[i] <= north, 0 elsewhere.  Membership is
    carried by the sign (include/aurora_hip.h: a row belongs to a band where its weight is > 0), so a member whose cosine
    weight came out as exactly 0 is given the smallest positive double: it still counts in `rows`."""
    w = np.maximum(latitude_weights(lat), np.finfo(np.float64).tiny)
    lat = np.asarray(lat, dtype=np.float64)
    return np.stack([np.where((lat >= s) & (lat <= n), w, 0.0) for s, n in bands])


# ---- the spectra on the host ---------------------------------------------------------------------------------------
def _power_host(pred: np.ndarray, truth: Optional[np.ndarray], bw: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The definitions of the module's text for (n_planes, n_lat, n_lon) arrays, in numpy fp64:
    power (n_planes, 1 or 3, n_bands, K) and rows (n_planes, n_bands)."""
    n_planes, _, N = pred.shape
    K = N // 2 + 1
    c = np.full(K, 2.0)
    c[0] = 1.0
    if N % 2 == 0:
        c[-1] = 1.0
    fields = [pred.astype(np.float64)] + ([truth.astype(np.float64)] if truth is not None else [])
    valid = np.all([np.isfinite(f).all(axis=-1) for f in fields], axis=0)              # (n_planes, n_lat)
    X = [np.fft.rfft(np.where(valid[..., None], f, 0.0), axis=-1) for f in fields]
    if truth is not None:
        X.append(X[0] - X[1])
    P = np.stack([(x.real ** 2 + x.imag ** 2) * c / (float(N) * float(N)) for x in X], axis=1)   # (n_planes, F, n_lat, K)
    w = bw[None] * valid[:, None, :]                                                   # (n_planes, n_bands, n_lat)
    rows = ((bw[None] > 0) & valid[:, None, :]).sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        power = np.einsum("pbi,pfik->pfbk", w, P) / w.sum(axis=-1)[:, None, :, None]
    power[np.broadcast_to((rows == 0)[:, None, :, None], power.shape)] = np.nan
    return power, rows.astype(np.int64)


# ---- public function -------------------------------------------------------------------------------------------------
def spectra(pred: Batch, truth: Optional[Batch] = None, bands=None) -> Spectra:
    """Zonal power spectra, per latitude band, of the last history entry of every surface and atmospheric variable of `pred`
    (with a `truth`: of every variable both hold, for pred, truth and pred - truth); see the module's text."""
    bands = _check_bands(bands)
    _fields.check_same_grid("scores", pred, truth if truth is not None else pred, "pred", "truth", "the prediction")
    n_lat, n_lon = pred.metadata.lat.shape[0], pred.metadata.lon.shape[0]
    _fields.check_longitudes(_fields._host(pred.metadata.lon))
    others = [("truth", truth)] if truth is not None else []
    names, fields, layout = _fields.select_pair("spectra", pred, others)
    if not names:
        raise ValueError("spectra: pred and truth have no surface or atmospheric variable in common" if truth is not None
                         else "spectra: pred has no surface or atmospheric variable")

    device = _fields.place("spectra", [(what, names, fs) for what, fs in zip(("pred", "truth"), fields)], n_lat, n_lon,
                           task="transforms float32 fields (move the batches to the CPU for other precisions)")
    lat = _fields._host(pred.metadata.lat)
    if device == "cpu":
        power, rows = _power_host(_fields.stack(fields[0], n_lat, n_lon),
                                  _fields.stack(fields[1], n_lat, n_lon) if truth is not None else None, band_weights(lat, bands))
        power, rows = torch.from_numpy(power), torch.from_numpy(rows)
    else:
        from aurora_amd.engine import lib

        band_w = _fields.tables.get(("band weights", lat.tobytes(), bands), device, lambda: band_weights(lat, bands),
                                    "spectra: call once with these bands before capturing a graph (the band weights are "
                                    "uploaded on the first call, which a captured graph cannot replay)")
        power, rows = lib.spectra_power(fields[0], fields[1] if truth is not None else None, band_w)
    return Spectra(power, rows, layout, bands)
