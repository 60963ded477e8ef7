"""Did the forecast put the extremes where they were: contingency tables and the Fractions Skill Score (FSS, Roberts & Lean
2008) of threshold exceedances, per variable and level (not in the reference, which has no scoring function).

    s = aurora_amd.event_scores(pred, truth, {"10u": (10.8, 17.2), "t": (273.15,)}, scales=(1, 5, 9, 17, 33), below=False)
    s.fss["10u"]        # (B, T, S)    float64, on pred's device: one value per threshold and window size
    s.fss["t"]          # (B, C, T, S) one table per pressure level
    s.hits, s.misses, s.false_alarms, s.correct_negatives      # (B[, C], T) int64: the unweighted contingency table
    s.csi, s.pod, s.far, s.frequency_bias, s.ets, s.base_rate, s.forecast_rate      # (B[, C], T) float64, latitude-weighted
    s.fss_uniform       # 0.5 + base_rate / 2: the FSS above which a scale is usually called useful
    s.count             # (B[, C]) int64: the valid points
    s.rowsums, s.valid  # the raw integer tables (B[, C], T, S, n_lat, 3) and (B[, C], n_lat): FSS of any latitude band
    s.scales            # the window sizes that were used: sorted, with 1 in front
    s.cpu()             # the same object with host tensors: the one call that waits for the device

`thresholds` maps a variable name to its T_v values: a sequence for a surface variable; for an atmospheric variable a
sequence (used at every level) or a (C, T_v) array.  Only the variables named there are scored.  T = max T_v <= 8; a shorter
list is padded with NaN, and every score of a padded slot is NaN.  The values are ROUNDED TO FLOAT32 ONCE, here, and compared
with the fields in float32 on either device.

A point (i, j) of a plane is VALID where pred and truth are both finite.  For a threshold thr

    f(i,j) = valid && pred >= thr        o(i,j) = valid && truth >= thr            (`below=True`: both <=)

and for an odd window size n = 2 h + 1 (in GRID POINTS; 1 <= n <= 63, n <= n_lon, at most 8 of them)

    cf(i,j) = sum_{|di| <= h, |dj| <= h} f(i + di, (j + dj) mod n_lon),   co likewise:

periodic in longitude; rows outside the grid and invalid points count zero (the zero padding of the usual uniform_filter).
Per row i, over its valid centre columns j:  A_i = sum_j (cf - co)^2,  Bf_i = sum_j cf^2,  Bo_i = sum_j co^2 -- integers, exact
on either device.  With w = `latitude_weights(lat)`

    FSS = 1 - sum_i w_i A_i / (sum_i w_i Bf_i + sum_i w_i Bo_i)       (the n^4 of the fractions cancels; NaN without an event)

and at n = 1, where cf^2 = f, co^2 = o, (cf - co)^2 = f + o - 2 f o:  hits_i = (Bf_i + Bo_i - A_i) / 2,  false alarms_i =
Bf_i - hits_i,  misses_i = Bo_i - hits_i,  correct negatives_i = valid_i - the other three -- which is why window size 1 is
always part of a call (it is inserted when the caller leaves it out).  From the latitude-weighted H, F, M, C and N = H + F +
M + C:  csi = H / (H + M + F),  pod = H / (H + M),  far = F / (H + F),  frequency_bias = (H + F) / (H + M),  base_rate =
(H + M) / N,  forecast_rate = (H + F) / N,  ets = (H - R) / (H + M + F - R) with R = (H + M)(H + F) / N.  A zero
denominator gives NaN.

Limitation: the window is n grid points, so on a latitude-longitude grid it narrows in kilometres towards the poles; the
cos(lat) weight of the centre point is the only area correction.

Fields on one GPU are reduced by ONE aurora_hip_event_scores call (every value read once per tile, no plane-sized temporary,
nothing read back), fields on the CPU by the same integer arithmetic in numpy; the finalisation is the same torch code on
either device, with the row reduction written as a fixed pairwise tree of elementwise operations, so that the float64 scores
agree bit for bit between the devices as well.
"""

from __future__ import annotations

import dataclasses
from typing import Mapping, Sequence

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._fields import latitude_weights, ratio as _ratio, tree_sum as _tree_sum
from aurora_amd.batch import Batch

__all__ = ["event_scores", "EventScores"]

MAX_THRESHOLDS, MAX_LON = _fields.MAX_THRESHOLDS, _fields.MAX_LON
MAX_SCALES, MAX_SCALE = 8, 63
_CSI, _POD, _FAR, _FBIAS, _ETS, _BASE, _FRATE = range(7)


@dataclasses.dataclass(frozen=True)
class EventScores:
    """Result of `event_scores`: every property but `scales` is a dict name -> tensor with the leading shape (B,) for a
    surface variable and (B, C) for an atmospheric one, on the device of the prediction."""

    rowsums_table: torch.Tensor                          # (n_planes, T, S, n_lat, 3) int64: A, Bf, Bo per row
    valid_table: torch.Tensor                            # (n_planes, n_lat) int64
    fss_table: torch.Tensor                              # (n_planes, T, S) float64
    counts_table: torch.Tensor                           # (n_planes, T, 4) int64: hits, misses, false alarms, correct negatives
    rates_table: torch.Tensor                            # (n_planes, T, 7) float64: csi, pod, far, bias, ets, base, forecast
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    scales: tuple[int, ...]
    below: bool

    def _field(self, t: torch.Tensor) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, t)

    @property
    def fss(self) -> dict[str, torch.Tensor]:
        return self._field(self.fss_table)

    @property
    def hits(self) -> dict[str, torch.Tensor]:
        return self._field(self.counts_table[..., 0])

    @property
    def misses(self) -> dict[str, torch.Tensor]:
        return self._field(self.counts_table[..., 1])

    @property
    def false_alarms(self) -> dict[str, torch.Tensor]:
        return self._field(self.counts_table[..., 2])

    @property
    def correct_negatives(self) -> dict[str, torch.Tensor]:
        return self._field(self.counts_table[..., 3])

    @property
    def csi(self) -> dict[str, torch.Tensor]:
        return self._field(self.rates_table[..., _CSI])

    @property
    def pod(self) -> dict[str, torch.Tensor]:
        return self._field(self.rates_table[..., _POD])

    @property
    def far(self) -> dict[str, torch.Tensor]:
        return self._field(self.rates_table[..., _FAR])

    @property
    def frequency_bias(self) -> dict[str, torch.Tensor]:
        return self._field(self.rates_table[..., _FBIAS])

    @property
    def ets(self) -> dict[str, torch.Tensor]:
        return self._field(self.rates_table[..., _ETS])

    @property
    def base_rate(self) -> dict[str, torch.Tensor]:
        return self._field(self.rates_table[..., _BASE])

    @property
    def forecast_rate(self) -> dict[str, torch.Tensor]:
        return self._field(self.rates_table[..., _FRATE])

    @property
    def fss_uniform(self) -> dict[str, torch.Tensor]:
        return self._field(0.5 + self.rates_table[..., _BASE] / 2)

    @property
    def count(self) -> dict[str, torch.Tensor]:
        return self._field(self.valid_table.sum(dim=-1))

    @property
    def rowsums(self) -> dict[str, torch.Tensor]:
        return self._field(self.rowsums_table)

    @property
    def valid(self) -> dict[str, torch.Tensor]:
        return self._field(self.valid_table)

    def cpu(self) -> "EventScores":
        """The same scores with host tensors (waits for the device)."""
        moved = {f: getattr(self, f).cpu() for f in ("rowsums_table", "valid_table", "fss_table", "counts_table", "rates_table")}
        return dataclasses.replace(self, **moved)


# ---- arguments -------------------------------------------------------------------------------------------------------
def _check_scales(scales, n_lon: int) -> tuple[int, ...]:
    try:
        raw = [s for s in scales]
    except TypeError:
        raise ValueError("event_scores: scales must be a sequence of odd window sizes") from None
    out = set()
    for s in raw:
        if isinstance(s, bool) or int(s) != s:
            raise ValueError(f"event_scores: scales must be whole numbers, got {s!r}")
        s = int(s)
        if s % 2 == 0:
            raise ValueError(f"event_scores: scales must be odd (a window has a centre point), got {s}")
        if not 1 <= s <= MAX_SCALE:
            raise ValueError(f"event_scores: scales must be within 1..{MAX_SCALE}, got {s}")
        if s > n_lon:
            raise ValueError(f"event_scores: scales must not be wider than the grid's {n_lon} longitudes, got {s}")
        if s in out:
            raise ValueError(f"event_scores: scales must be distinct, {s} is given twice")
        out.add(s)
    out.add(1)
    if len(out) > MAX_SCALES:
        raise ValueError(f"event_scores: at most {MAX_SCALES} scales can be taken at a time (1 included), got {len(out)}")
    return tuple(sorted(out))


# ---- the integers on the host ------------------------------------------------------------------------------------------
def _rowsums_host(pred: np.ndarray, truth: np.ndarray, thr: np.ndarray, scales: Sequence[int],
                  below: bool) -> tuple[np.ndarray, np.ndarray]:
    """The tables of include/aurora_hip.h for (n_planes, n_lat, n_lon) arrays and (n_planes, T) float32 thresholds, in numpy
    integers (window sums from a two-dimensional running sum): rowsums (n_planes, T, S, n_lat, 3) and valid (n_planes, n_lat)."""
    n_planes, n_lat, n_lon = pred.shape
    T, S = thr.shape[1], len(scales)
    rowsums = np.zeros((n_planes, T, S, n_lat, 3), dtype=np.int64)
    valid = np.zeros((n_planes, n_lat), dtype=np.int64)
    cmp = np.less_equal if below else np.greater_equal
    for k in range(n_planes):
        p, t = pred[k], truth[k]
        ok = np.isfinite(p) & np.isfinite(t)
        valid[k] = ok.sum(axis=1)
        with np.errstate(invalid="ignore"):
            fields = [np.stack([ok & cmp(x, th) for th in thr[k]]).astype(np.int64) for x in (p, t)]   # (T, n_lat, n_lon) each
        for s, n in enumerate(scales):
            h = n // 2
            counts = []
            for f in fields:
                ext = np.concatenate([f[..., n_lon - h:], f, f[..., :h]], axis=-1) if h else f      # periodic in longitude
                ext = np.pad(ext, ((0, 0), (h + 1, h), (1, 0)))                                       # zero rows; a leading 0
                c = ext.cumsum(axis=1).cumsum(axis=2)
                counts.append(c[:, n:, n:] - c[:, :-n, n:] - c[:, n:, :-n] + c[:, :-n, :-n])
            cf, co = counts
            rowsums[k, :, s, :, 0] = ((cf - co) ** 2 * ok).sum(axis=-1)
            rowsums[k, :, s, :, 1] = (cf ** 2 * ok).sum(axis=-1)
            rowsums[k, :, s, :, 2] = (co ** 2 * ok).sum(axis=-1)
    return rowsums, valid


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
def _finalise(rowsums: torch.Tensor, valid: torch.Tensor, w: torch.Tensor,
              thr: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(fss (P, T, S) fp64, counts (P, T, 4) int64, rates (P, T, 7) fp64) from the integer tables; no read-back."""
    r = rowsums.to(torch.float64)                                        # exact: every entry is below 2^36
    ws = _tree_sum((r * w[:, None]).transpose(-1, -2))                   # (P, T, S, 3)
    padded = torch.isnan(thr)                                            # (P, T)
    nan = float("nan")
    fss = 1.0 - _ratio(ws[..., 0], ws[..., 1] + ws[..., 2])
    fss = torch.where(padded[..., None], torch.full_like(fss, nan), fss)
    a, bf, bo = rowsums[:, :, 0, :, 0], rowsums[:, :, 0, :, 1], rowsums[:, :, 0, :, 2]   # window size 1: (P, T, n_lat)
    hits = (bf + bo - a) // 2
    fa, miss = bf - hits, bo - hits
    cn = valid[:, None, :] - hits - fa - miss
    counts = torch.stack([hits.sum(-1), miss.sum(-1), fa.sum(-1), cn.sum(-1)], dim=-1)
    H, F, M = (_tree_sum(x.to(torch.float64) * w) for x in (hits, fa, miss))
    N = _tree_sum(valid.to(torch.float64) * w)[:, None].expand_as(H)
    R = _ratio((H + M) * (H + F), N)
    rates = torch.stack([_ratio(H, H + M + F), _ratio(H, H + M), _ratio(F, H + F), _ratio(H + F, H + M),
                         _ratio(H - R, H + M + F - R), _ratio(H + M, N), _ratio(H + F, N)], dim=-1)
    rates = torch.where(padded[..., None], torch.full_like(rates, nan), rates)
    return fss, counts, rates


# ---- public function -----------------------------------------------------------------------------------------------------
def event_scores(pred: Batch, truth: Batch, thresholds: Mapping[str, object], scales: Sequence[int] = (1,),
                 below: bool = False) -> EventScores:
    """Contingency tables and fractions skill scores of the last history entry of the variables named in `thresholds`; see the
    module's text.  The thresholds are rounded to float32 once and compared in float32."""
    _fields.check_same_grid("scores", pred, truth, "pred", "truth", "the prediction")
    n_lat, n_lon = pred.metadata.lat.shape[0], pred.metadata.lon.shape[0]
    if not 1 <= n_lon <= MAX_LON:
        raise ValueError(f"event_scores: the grid has {n_lon} longitudes; 1 to {MAX_LON} are supported")
    scales = _check_scales(scales, n_lon)
    if not isinstance(thresholds, Mapping) or not thresholds:
        raise ValueError("event_scores: thresholds must be a non-empty mapping from variable name to values")
    names, fields, layout = _fields.select_pair("event_scores", pred, [("truth", truth)], only=thresholds)
    thr = _fields.threshold_table("event_scores", thresholds, layout) if names else None
    for k in thresholds:
        if k not in names:
            raise ValueError(f"event_scores: thresholds name the variable {k!r}, which pred and truth do not both hold as a "
                             "surface or atmospheric variable")

    device = _fields.place("event_scores", [("pred", names, fields[0]), ("truth", names, fields[1])], n_lat, n_lon)
    lat = _fields._host(pred.metadata.lat)
    if device == "cpu":
        rowsums, valid = _rowsums_host(_fields.stack(fields[0], n_lat, n_lon), _fields.stack(fields[1], n_lat, n_lon), thr,
                                       scales, bool(below))
        rowsums, valid, thr_t = torch.from_numpy(rowsums), torch.from_numpy(valid), torch.from_numpy(thr)
        w = torch.from_numpy(latitude_weights(lat))
    else:
        from aurora_amd.engine import lib

        thr_t = _fields.device_thresholds("event_scores", thr, device)
        rowsums, valid = lib.event_rowsums(fields[0], fields[1], thr_t, scales, bool(below))
        w = _fields.device_weights("event_scores", lat, device)
    fss, counts, rates = _finalise(rowsums, valid, w, thr_t)
    return EventScores(rowsums, valid, fss, counts, rates, layout, scales, bool(below))
