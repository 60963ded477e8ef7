"""What is this field's 99th percentile: the SPATIAL quantiles of every plane, by area or by count, where the plane lives (not
in the reference).  The event modules take absolute thresholds -- `event_scores`, `probability_scores`, `objects`, and
`conditional_scores` as edges -- and in practice those are percentiles of the field: Roberts & Lean's FSS thresholds at a
percentile to take the bias out, object catalogues threshold IVT or vorticity at the plane's 0.9 / 0.99 quantile.

    fq = aurora_amd.field_quantiles(batch, q=(0.5, 0.9, 0.99), kind="area", only=None)
    fq.value["2t"]        # (B, Q) float32 on the batch's device; (B, C, Q) for an atmospheric variable
    fq.valid["2t"]        # (B[, C]) int64: the number n of finite points
    fq.total["2t"]        # (B[, C]) int64: W, the sum of the row units over them (kind="count": n)
    fq.q, fq.kind         # the q values as given (fp64 tuple), "area" or "count"
    fq.cpu()              # the same object with host tensors
    fq.thresholds(b=0)    # name -> (T,) / (C, T) float32 numpy arrays of batch element b: what the event modules take, so
    event_scores(pred, truth, field_quantiles(truth, (0.9, 0.99)).thresholds())        # is one line

`only` names the variables to take (None: every surface and atmospheric variable); the last history entry is used, as in
`scores`.  `q` is 1 to 8 finite values in [0, 1], in any order, repeats allowed.  Fields of another precision (CPU batches
only) are rounded to float32 first.

THE RULE (both paths and the tests refer to this text), per plane -- one batch element, one level:

    validity   a point is valid where its value is finite: NaN and +-Inf drop out (NaN masks).  `valid` is their number n.
    order      by the 32-bit key K(v) of `objects` (`objects.value_keys`): ascending with the value, -0 below +0.
    count      numpy's method="linear" over the valid points, by the expression of `ensemble_quantiles` with n in place of M:
               h = (double)(n - 1) q, j = min(floor(h), n - 1), g = h - j, hi = min(j + 1, n - 1),
               value = (float32)(a + g (b - a)) with a = x_(j), b = x_(hi) in fp64, the three operations rounded one by one
               (no fused multiply-add).  n = 0 gives NaN.  (j, g) are formed on the device, where n is known, by the same fp64
               operations as here, so they have the same bits.  `total` = n.
    area       (the default: on a latitude-longitude grid "the 99th percentile by area") row i carries the integer weight
               unit[i] = llrint(w_i 2^32) of `objects.area_units`.  W = sum of unit over the valid points = `total`;
               target = min(max((int64)ceil(q (double)W), 1), W); value = the smallest valid x with
               U(x) = sum{unit : K <= K(x)} >= target: the inverted CDF, no interpolation.  W = 0 gives NaN: no valid point,
               or all valid points on pole rows, whose unit is 0.  (The weights are normalised by their mean, so a pole row has
               unit 0 only beside rows that are no poles.)

A plane's result depends on its own values, the grid's latitudes and q alone.  Everything accumulated is an integer, so the two
paths agree bit for bit.

Fields on one GPU take ONE aurora_hip_field_quantiles call (`aurora_amd/csrc/field_quantiles.hip`): an exact radix select over
K, four passes over the planes with 256-bin integer histograms, no sort, no plane-sized temporary, nothing read back.  Fields
on the CPU take the rule in numpy (a stable sort by K and a cumulative sum).  `thresholds()` is the one call that waits for the
device.

Not offered: thresholds as device tensors to the other modules, regions or masks (NaN masks), quantiles over time or members
(`FieldStats`, `ensemble_quantiles`), the histograms themselves, latitude bands (`BandBatch`).
"""

from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd.batch import Batch
from aurora_amd.objects import area_units, value_keys

__all__ = ["field_quantiles", "FieldQuantiles", "MAX_QUANTILES", "KINDS"]

MAX_QUANTILES = 8
KINDS = ("area", "count")
_ON_CAPTURE = ("field_quantiles: call once on this grid before capturing a graph (the area units are uploaded on the first "
               "call, which a captured graph cannot replay)")


# ---- the rule on the host ---------------------------------------------------------------------------------------------
def plane_quantiles(plane: np.ndarray, q: Sequence[float], unit: Optional[np.ndarray]) -> tuple[np.ndarray, int, int]:
    """THE RULE for one (n_lat, n_lon) float32 plane: (Q float32 values, valid, total); unit: (n_lat,) int64 or None (count)."""
    v = np.ascontiguousarray(plane, dtype=np.float32)
    finite = np.isfinite(v)
    x = v[finite]
    order = np.argsort(value_keys(x, False), kind="stable")
    x = x[order]
    n = int(x.shape[0])
    out = np.full(len(q), np.nan, dtype=np.float32)
    if unit is None:
        if n:
            for i, qi in enumerate(q):
                h = np.float64(n - 1) * np.float64(qi)
                j = min(int(np.floor(h)), n - 1)
                g = h - np.float64(j)
                a, b = np.float64(x[j]), np.float64(x[min(j + 1, n - 1)])
                d = b - a
                t = g * d
                out[i] = np.float32(a + t)
        return out, n, n
    cum = np.cumsum(np.broadcast_to(np.asarray(unit, dtype=np.int64)[:, None], v.shape)[finite][order], dtype=np.int64)
    W = int(cum[-1]) if n else 0
    if W:
        for i, qi in enumerate(q):
            target = min(max(int(np.ceil(np.float64(qi) * np.float64(W))), 1), W)
            out[i] = x[np.searchsorted(cum, target, side="left")]
    return out, n, W


def _quantiles_host(planes: np.ndarray, q: Sequence[float], unit: Optional[np.ndarray]):
    """THE RULE for (n_planes, n_lat, n_lon) planes: (n_planes, Q) float32, (n_planes,) int64, (n_planes,) int64."""
    n_planes = planes.shape[0]
    values = np.empty((n_planes, len(q)), dtype=np.float32)
    valid, total = np.empty(n_planes, dtype=np.int64), np.empty(n_planes, dtype=np.int64)
    for p in range(n_planes):
        with np.errstate(over="ignore", invalid="ignore"):
            plane = planes[p].astype(np.float32)
        values[p], valid[p], total[p] = plane_quantiles(plane, q, unit)
    return values, valid, total


@dataclasses.dataclass(frozen=True)
class FieldQuantiles:
    """Result of `field_quantiles`: every property is a dict name -> tensor with the leading shape (B,) for a surface variable
    and (B, C) for an atmospheric one, on the device of the batch; see the module's text."""

    value_table: torch.Tensor                            # (n_planes, Q) float32
    valid_table: torch.Tensor                            # (n_planes,) int64
    total_table: torch.Tensor                            # (n_planes,) int64
    layout: _fields.Layout                               # (name, first plane, shape) per variable
    q: tuple[float, ...]
    kind: str

    @property
    def value(self) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, self.value_table)

    @property
    def valid(self) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, self.valid_table)

    @property
    def total(self) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, self.total_table)

    def cpu(self) -> "FieldQuantiles":
        """The same quantiles with host tensors (waits for the device)."""
        return dataclasses.replace(self, value_table=self.value_table.cpu(), valid_table=self.valid_table.cpu(),
                                   total_table=self.total_table.cpu())

    def thresholds(self, b: int = 0) -> dict[str, np.ndarray]:
        """The quantiles of batch element `b` as the thresholds the event modules take (waits for the device): name -> (T,)
        float32 for a surface variable and (C, T) for an atmospheric one, each row's values without duplicates and NaN, in
        ascending order (so they also serve as `conditional_scores` edges); a shorter row of a (C, T) array, and a row without
        any value, is padded with NaN, which the event modules read as "no event"."""
        out = {}
        for name, v in self.value.items():
            if not -v.shape[0] <= b < v.shape[0]:
                raise IndexError(f"field_quantiles: thresholds of batch element {b}, but {name!r} has batch size {v.shape[0]}")
            a = v[b].cpu().numpy()
            rows = [np.unique(r[~np.isnan(r)]) for r in a.reshape(-1, a.shape[-1])]
            T = max(1, max(r.shape[0] for r in rows))
            t = np.stack([np.pad(r, (0, T - r.shape[0]), constant_values=np.nan) for r in rows]).astype(np.float32)
            out[name] = t if a.ndim == 2 else t[0]
        return out


# ---- public function -------------------------------------------------------------------------------------------------
def field_quantiles(batch: Batch, q: Sequence[float] = (0.5, 0.9, 0.99), kind: str = "area",
                    only: Optional[Sequence[str]] = None) -> FieldQuantiles:
    """The spatial quantiles of the last history entry of every variable (of `only`, if given); see the module's text."""
    if not isinstance(batch, Batch):
        raise TypeError(f"field_quantiles: batch must be a Batch, got {type(batch).__name__}")
    _fields.check_vector_grid("field_quantiles", batch, "batch", band="quantiles")
    try:
        qs = tuple(float(v) for v in (q if np.ndim(q) else (q,)))
    except (TypeError, ValueError):
        raise ValueError("field_quantiles: q must be numbers") from None
    if not 1 <= len(qs) <= MAX_QUANTILES:
        raise ValueError(f"field_quantiles: 1 to {MAX_QUANTILES} values of q, got {len(qs)}")
    if not all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in qs):
        raise ValueError(f"field_quantiles: q must be finite values in [0, 1], got {qs}")
    if kind not in KINDS:
        raise ValueError(f"field_quantiles: kind must be one of {KINDS}, got {kind!r}")
    if isinstance(only, str):
        only = (only,)
    names, fields, layout = _fields.select_one("field_quantiles", batch, "batch", only)
    if not names:
        raise ValueError("field_quantiles: batch has no surface or atmospheric variable")
    n_lat, n_lon = batch.metadata.lat.shape[0], batch.metadata.lon.shape[0]
    device = _fields.place("field_quantiles", [("batch", names, fields)], n_lat, n_lon, _fields.TAKES_TASK)
    lat = _fields._host(batch.metadata.lat)
    if device == "cpu":
        values, valid, total = (torch.from_numpy(x) for x in _quantiles_host(
            _fields.stack([f.to(torch.float32) for f in fields], n_lat, n_lon), qs, area_units(lat) if kind == "area" else None))
    else:
        from aurora_amd.engine import lib

        unit = None
        if kind == "area":
            unit = _fields.tables.get(("object units", lat.tobytes()), device, lambda: area_units(lat), _ON_CAPTURE)
        values, valid, total = lib.field_quantile_values(fields, qs, unit)
    return FieldQuantiles(values, valid, total, layout, qs, kind)
