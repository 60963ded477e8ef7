"""How large is the error where the truth was extreme: bias, RMSE and MAE per bin of the truth, and over its tails, per
variable and level (not in the reference, which has no scoring function).

    s = aurora_amd.conditional_scores(pred, truth, {"2t": (-1.5, -0.5, 0.5, 1.5)}, centre=None, scale=None, by="truth")
    s.count["2t"]       # (B, E + 1) int64, on pred's device; atmospheric: (B, C, E + 1).  The valid points of every bin
    s.weight            # (B[, C], E + 1) float64: the sum of latitude weights of every bin;  s.fraction = weight / total
    s.bias, s.rmse, s.mae                 # (B[, C], E + 1) float64 per bin; NaN for an empty bin
    s.rmse_above, s.bias_above, s.mae_above, s.count_above    # (B[, C], E): over the points AT OR BEYOND edge j (upper tail)
    s.rmse_below, s.bias_below, s.mae_below, s.count_below    # (B[, C], E): over the points SHORT OF edge j (lower tail)
    s.sums              # (B[, C], E + 1, 5) float64: the raw table
    s.edges             # the float32 table that was used, (B[, C], E);  s.by
    s.cpu()             # the same object with host tensors: the one call that waits for the device

`edges` maps a variable name to its E_v values, 1 to 8 of them: a sequence for a surface variable; for an atmospheric variable
a sequence (used at every level) or a (C, E_v) array.  Only the variables named there are scored.  E = max E_v; a shorter
list is padded with NaN.  The values are ROUNDED TO FLOAT32 ONCE, here; the values of a row that are not NaN must ascend
strictly (-inf and inf are allowed).  `centre` and `scale` are optional batches on the grid and levels of `pred` that hold
every variable named in `edges` -- for example `FieldStats.as_batch("mean")` and `as_batch("std")`, which makes an edge k
the threshold mean + k std of the thresholded RMSE -- with the batch size of `pred` or with batch size 1 (the one plane is
then used for every batch element; nothing is copied).  `by` says which field is binned: "truth" (the error given what
happened) or "pred" (the error given what was forecast).

THE RULE, the same on both devices.  With v the binned field, c the centre (0 without one), sigma the scale (1 without
one) and e_j the edges of the plane, all float32:

    a = (double)v - (double)c                              one float64 subtraction
    bin = #{ j : a >= (double)e_j * (double)sigma }        one float64 product per edge, alone on its side of the comparison

so bin b lies between edge b - 1 and edge b.  A NaN edge is never passed: the bins beyond a variable's own E_v stay empty,
and their scores, like the tails of a padded edge, are NaN.  A point is VALID where pred and truth are finite, every given one
of centre and scale is finite, and sigma >= 0; sigma = 0 is legal (the products are +-0 and the point falls by the sign of a).

Per plane and bin, over its valid points, with w = `latitude_weights(lat)` of the row and d = (double)pred - (double)truth:
count, S1 = sum w, S2 = sum w d, S3 = sum w d^2, S4 = sum w |d| -- the first five sums of `scores`, so that

    bias = S2 / S1      rmse = sqrt(S3 / S1)      mae = S4 / S1      fraction = S1 / (S1 summed over the bins)

The tail beyond edge j takes the five sums of the bins j + 1 .. E, added in DESCENDING bin order (the top bin first), and the
tail short of it those of the bins 0 .. j in ASCENDING order, and forms the same ratios; the counts are integer sums.

Fields on one GPU are reduced by ONE aurora_hip_conditional_scores call (every input read once, fp64 throughout, the fixed
reduction tree of `scores`: repeatable bit for bit, and the sums of a bin depend on the points of that bin alone -- not on the
other planes and not on how many other edges the call has), fields on the CPU by the same rule in numpy fp64; the
finalisation is the same torch code on either device, so a roll-out can be scored step by step and read once at the end.
"""

from __future__ import annotations

import dataclasses
from typing import Mapping, Optional

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._fields import latitude_weights, ratio as _ratio, tree_sum as _tree_sum
from aurora_amd.batch import Batch

__all__ = ["conditional_scores", "ConditionalScores"]

MAX_EDGES = _fields.MAX_THRESHOLDS
_FRACTION, _BIAS, _RMSE, _MAE = range(4)


@dataclasses.dataclass(frozen=True)
class ConditionalScores:
    """Result of `conditional_scores`: every property but `by` is a dict name -> tensor with the leading shape (B,) for a
    surface variable and (B, C) for an atmospheric one, on the device of the prediction."""

    sums_table: torch.Tensor                             # (n_planes, E + 1, 5) float64: count, S1 .. S4 per bin
    bins_table: torch.Tensor                             # (n_planes, E + 1, 4) float64: fraction, bias, rmse, mae
    above_sums: torch.Tensor                             # (n_planes, E, 5): the bins j + 1 .. E
    above_table: torch.Tensor                            # (n_planes, E, 4)
    below_sums: torch.Tensor                             # (n_planes, E, 5): the bins 0 .. j
    below_table: torch.Tensor                            # (n_planes, E, 4)
    edges_table: torch.Tensor                            # (n_planes, E) float32
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    by: str

    def _field(self, t: torch.Tensor) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, t)

    @property
    def sums(self) -> dict[str, torch.Tensor]:
        return self._field(self.sums_table)

    @property
    def count(self) -> dict[str, torch.Tensor]:
        return self._field(self.sums_table[..., 0].to(torch.int64))

    @property
    def weight(self) -> dict[str, torch.Tensor]:
        return self._field(self.sums_table[..., 1])

    @property
    def fraction(self) -> dict[str, torch.Tensor]:
        return self._field(self.bins_table[..., _FRACTION])

    @property
    def bias(self) -> dict[str, torch.Tensor]:
        return self._field(self.bins_table[..., _BIAS])

    @property
    def rmse(self) -> dict[str, torch.Tensor]:
        return self._field(self.bins_table[..., _RMSE])

    @property
    def mae(self) -> dict[str, torch.Tensor]:
        return self._field(self.bins_table[..., _MAE])

    @property
    def count_above(self) -> dict[str, torch.Tensor]:
        return self._field(self.above_sums[..., 0].to(torch.int64))

    @property
    def bias_above(self) -> dict[str, torch.Tensor]:
        return self._field(self.above_table[..., _BIAS])

    @property
    def rmse_above(self) -> dict[str, torch.Tensor]:
        return self._field(self.above_table[..., _RMSE])

    @property
    def mae_above(self) -> dict[str, torch.Tensor]:
        return self._field(self.above_table[..., _MAE])

    @property
    def count_below(self) -> dict[str, torch.Tensor]:
        return self._field(self.below_sums[..., 0].to(torch.int64))

    @property
    def bias_below(self) -> dict[str, torch.Tensor]:
        return self._field(self.below_table[..., _BIAS])

    @property
    def rmse_below(self) -> dict[str, torch.Tensor]:
        return self._field(self.below_table[..., _RMSE])

    @property
    def mae_below(self) -> dict[str, torch.Tensor]:
        return self._field(self.below_table[..., _MAE])

    @property
    def edges(self) -> dict[str, torch.Tensor]:
        return self._field(self.edges_table)

    def cpu(self) -> "ConditionalScores":
        """The same scores with host tensors (waits for the device)."""
        tables = ("sums_table", "bins_table", "above_sums", "above_table", "below_sums", "below_table", "edges_table")
        return dataclasses.replace(self, **{f: getattr(self, f).cpu() for f in tables})


# ---- the sums on the host ------------------------------------------------------------------------------------------------
def _sums_host(pred: np.ndarray, truth: np.ndarray, centre: Optional[np.ndarray], scale: Optional[np.ndarray],
               edges: np.ndarray, by_pred: bool, w: np.ndarray) -> np.ndarray:
    """The table of include/aurora_hip.h for (n_planes, n_lat, n_lon) arrays and (n_planes, E) float32 edges, in numpy fp64:
    (n_planes, E + 1, 5).  The bin of every point is counted once, then the sums are taken bin by bin."""
    n_planes, E = edges.shape
    out = np.zeros((n_planes, E + 1, 5))
    w = np.asarray(w, dtype=np.float64)[:, None]
    for k in range(n_planes):
        p, t = pred[k].astype(np.float64), truth[k].astype(np.float64)
        ok = np.isfinite(p) & np.isfinite(t)
        a = p if by_pred else t
        if centre is not None:
            c = centre[k].astype(np.float64)
            ok &= np.isfinite(c)
            with np.errstate(invalid="ignore"):
                a = a - c
        sigma = None
        if scale is not None:
            sigma = scale[k].astype(np.float64)
            ok &= np.isfinite(sigma) & (sigma >= 0)
        bins = np.zeros(p.shape, dtype=np.int64)
        with np.errstate(invalid="ignore"):
            for e in edges[k].astype(np.float64):
                bins += a >= (e * sigma if sigma is not None else e)
        d = np.where(ok, p, 0.0) - np.where(ok, t, 0.0)
        wk = np.broadcast_to(w, p.shape)
        for b in range(E + 1):
            m = ok & (bins == b)
            wb, db = wk[m], d[m]
            out[k, b] = m.sum(), wb.sum(), (wb * db).sum(), (wb * db * db).sum(), (wb * np.abs(db)).sum()
    return out


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
def _rates(sums: torch.Tensor, total: torch.Tensor) -> torch.Tensor:
    """(..., 5) sums -> (..., 4): fraction of `total`, bias, rmse, mae; NaN without weight."""
    s1 = sums[..., 1]
    return torch.stack([_ratio(s1, total.expand_as(s1)), _ratio(sums[..., 2], s1), torch.sqrt(_ratio(sums[..., 3], s1)),
                        _ratio(sums[..., 4], s1)], dim=-1)


def _finalise(sums: torch.Tensor, edges: torch.Tensor):
    """(n_planes, E + 1, 5) sums and the (n_planes, E) edges -> (bins, above sums, above, below sums, below); elementwise
    torch operations on the device of `sums`, no read-back."""
    E = edges.shape[1]
    total = _tree_sum(sums[..., 1])[:, None]                             # (n_planes, 1)
    bins = _rates(sums, total)
    above, below = [None] * E, [None] * E
    acc = sums[:, E]
    for j in range(E - 1, -1, -1):                                       # the top bin first, then E - 1, E - 2, ...
        above[j] = acc
        acc = acc + sums[:, j]
    acc = sums[:, 0]
    for j in range(E):                                                   # bin 0 first, then 1, 2, ...
        below[j] = acc
        if j + 1 < E:
            acc = acc + sums[:, j + 1]
    above_sums, below_sums = torch.stack(above, dim=1), torch.stack(below, dim=1)
    padded = torch.isnan(edges)[..., None]
    nan = float("nan")
    tails = []
    for t in (above_sums, below_sums):
        r = _rates(t, total)
        tails.append(torch.where(padded, torch.full_like(r, nan), r))
    return bins, above_sums, tails[0], below_sums, tails[1]


# ---- public function -----------------------------------------------------------------------------------------------------
def conditional_scores(pred: Batch, truth: Batch, edges: Mapping[str, object], centre: Optional[Batch] = None,
                       scale: Optional[Batch] = None, by: str = "truth") -> ConditionalScores:
    """Bias, RMSE and MAE of the last history entry of the variables named in `edges`, per bin of the truth (or of the
    prediction) and over its tails; see the module's text.  The edges are rounded to float32 once."""
    if by not in ("truth", "pred"):
        raise ValueError(f"conditional_scores: by must be 'truth' or 'pred', got {by!r}")
    others = [("truth", truth)] + [(what, b) for what, b in (("centre", centre), ("scale", scale)) if b is not None]
    for what, b in others:
        if not isinstance(b, Batch):
            raise TypeError(f"conditional_scores: {what} must be a Batch, got {type(b).__name__}")
        _fields.check_same_grid("conditional_scores", pred, b, "pred", what, "the prediction")
    n_lat, n_lon = pred.metadata.lat.shape[0], pred.metadata.lon.shape[0]
    if not isinstance(edges, Mapping) or not edges:
        raise ValueError("conditional_scores: edges must be a non-empty mapping from variable name to values")
    names, fields, layout = _fields.select_pair("conditional_scores", pred, others, only=edges, repeated=("centre", "scale"))
    for k in edges:
        if k not in names:
            raise ValueError(f"conditional_scores: edges name the variable {k!r}, which pred and truth do not both hold as a "
                             "surface or atmospheric variable")
    table = _fields.threshold_table("conditional_scores", edges, layout, noun="edges")
    _fields.check_ascending("conditional_scores", table, layout)

    whats = ["pred"] + [what for what, _ in others]
    device = _fields.place("conditional_scores", [(what, names, fs) for what, fs in zip(whats, fields)], n_lat, n_lon)
    operands = dict(zip(whats, fields))
    lat = _fields._host(pred.metadata.lat)
    if device == "cpu":
        host = {what: _fields.stack(fs, n_lat, n_lon) for what, fs in operands.items()}
        sums = torch.from_numpy(_sums_host(host["pred"], host["truth"], host.get("centre"), host.get("scale"), table,
                                           by == "pred", latitude_weights(lat)))
        edges_t = torch.from_numpy(table)
    else:
        from aurora_amd.engine import lib

        edges_t = _fields.device_thresholds("conditional_scores", table, device)
        sums = lib.conditional_sums(operands["pred"], operands["truth"], operands.get("centre"), operands.get("scale"), edges_t,
                                    by == "pred", _fields.device_weights("conditional_scores", lat, device))
    return ConditionalScores(sums, *_finalise(sums, edges_t), edges_t, layout, by)
