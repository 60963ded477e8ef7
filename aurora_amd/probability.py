"""How good is the ensemble's "30 % chance of a gale": the Brier score and its skill score, the reliability / resolution /
uncertainty decomposition, the reliability diagram and the ROC curve of the fraction of members over a threshold, per variable
and level against truth (not in the reference, which has no scoring function).

    s = aurora_amd.probability_scores(members, truth, {"10u": (10.8, 17.2), "t": (273.15,)}, below=False)
    s.brier["10u"]              # (B, T) float64 on the members' device; atmospheric: (B, C, T)
    s.fair_brier, s.brier_skill, s.reliability, s.resolution, s.uncertainty, s.base_rate, s.roc_area     # same shape
    s.observed_frequency["10u"] # (B[, C], T, M + 1): observed relative frequency where k of M members forecast the event
    s.forecast_weight           # (B[, C], T, M + 1) float64: latitude-weighted share of the valid points in each bin (sharpness)
    s.forecast_probability      # (M + 1,) float64: k / M
    s.hit_rate, s.false_alarm_rate   # (B[, C], T, M + 2): the ROC points for "warn when k >= c", c = M + 1, M, ..., 0
    s.counts                    # (B[, C], T, 2, M + 1) int64: unweighted points by (event observed, k)
    s.count                     # (B[, C]) int64: valid points
    s.rows                      # (B[, C], n_lat, T, 2, M + 1) int32: the raw per-row table; any latitude band afterwards
    s.members                   # M
    s.cpu()                     # the same object with host tensors: the one call that waits for the device

`members` and `truth` are those of `ensemble_scores`: a sequence of 2..64 `Batch`es with the batch size of `truth`, or ONE
`Batch` whose M batch elements are the members against a `truth` of batch size 1; the last history entry is scored.
`thresholds` and `below` are those of `event_scores`: a variable name maps to its T_v values, a sequence (an atmospheric
variable: used at every level) or a (C, T_v) array; only the variables named there are scored.  T = max T_v <= 8; a shorter
list is padded with NaN, and every score of a padded slot is NaN.  The values are ROUNDED TO FLOAT32 ONCE, here, and compared
with the fields in float32 on either device.

A point (i, j) of a plane is VALID where truth and all M members are finite.  For a threshold thr, over the valid points,

    k(i,j) = #{m : x_m >= thr}  in 0..M          o(i,j) = [y >= thr]          (`below=True`: both <=; NaN thr: k = 0, o = 0)
    n_i[o][k] = number of valid points of row i with that (o, k)               -- exact integers, `rows`

With w = `latitude_weights(lat)`, W[o][k] = sum_i w_i n_i[o][k], n_k = W[0][k] + W[1][k], N = sum_k n_k (formed as
sum_i w_i valid_i, the number `event_scores` divides by) and p_k = k / M, the forecast probability:

    brier        = sum_k (W[1][k] (1 - p_k)^2 + W[0][k] p_k^2) / N
    base_rate    = obar = sum_k W[1][k] / N            uncertainty = obar (1 - obar)
    obar_k       = W[1][k] / n_k   (observed_frequency; NaN where n_k = 0, such bins add 0 to the sums below)
    reliability  = sum_k n_k (p_k - obar_k)^2 / N       resolution = sum_k n_k (obar_k - obar)^2 / N
    brier_skill  = 1 - brier / uncertainty              (NaN where uncertainty = 0)
    fair_brier   = brier - sum_k n_k k (M - k) / (M^2 (M - 1)) / N           (Ferro 2014: unbiased in M)
    hit_rate[c]  = sum_{k >= c} W[1][k] / sum_k W[1][k],  false_alarm_rate[c] likewise with W[0];  c = M + 1 gives (0, 0), c = 0 gives (1, 1)
    roc_area     = sum_{c=0}^{M} (F_c - F_{c+1}) (H_c + H_{c+1}) / 2          (NaN without an event or without a non-event)
    forecast_weight = n_k / N

A plane without a valid point gives NaN scores and zero counts.  brier = reliability - resolution + uncertainty holds
algebraically: the forecast takes only M + 1 values, so the decomposition is exact rather than binned.  The sums over k >= c of
the ROC are taken per row in integers and weighted afterwards (sum_i w_i sum_{k >= c} n_i[o][k]), so the curve is monotone and
ends at exactly (0, 0) and (1, 1) whatever the rounding.

Fields on one GPU are counted by ONE aurora_hip_probability_scores call (every plane read once, one launch, nothing read
back), fields on the CPU by the same integer arithmetic in numpy; the finalisation is the same torch code on either device,
with every floating-point sum written as a fixed pairwise tree of elementwise operations, so that the float64 scores agree bit
for bit between the devices as well.
"""

from __future__ import annotations

import dataclasses
from typing import Mapping, Sequence, Union

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._fields import latitude_weights, ratio as _ratio, tree_sum as _tree_sum, tree_sum_rows as _tree_sum_rows
from aurora_amd.batch import Batch

__all__ = ["probability_scores", "ProbabilityScores"]

_BRIER, _FAIR, _SKILL, _REL, _RES, _UNC, _BASE, _AREA = range(8)


@dataclasses.dataclass(frozen=True)
class ProbabilityScores:
    """Result of `probability_scores`: every property but `forecast_probability` and `members` is a dict name -> tensor with
    the leading shape (B,) for a surface variable and (B, C) for an atmospheric one, on the device of the members."""

    rows_table: torch.Tensor                             # (n_planes, n_lat, T, 2, M + 1) int32
    counts_table: torch.Tensor                           # (n_planes, T, 2, M + 1) int64
    scores_table: torch.Tensor                           # (n_planes, T, 8) float64: brier, fair, skill, rel, res, unc, base, area
    bins_table: torch.Tensor                             # (n_planes, T, 2, M + 1) float64: observed frequency, forecast weight
    roc_table: torch.Tensor                              # (n_planes, T, 2, M + 2) float64: hit rate, false alarm rate
    forecast_probability: torch.Tensor                   # (M + 1,) float64
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    members: int
    below: bool

    def _field(self, t: torch.Tensor) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, t)

    brier = property(lambda self: self._field(self.scores_table[..., _BRIER]))
    fair_brier = property(lambda self: self._field(self.scores_table[..., _FAIR]))
    brier_skill = property(lambda self: self._field(self.scores_table[..., _SKILL]))
    reliability = property(lambda self: self._field(self.scores_table[..., _REL]))
    resolution = property(lambda self: self._field(self.scores_table[..., _RES]))
    uncertainty = property(lambda self: self._field(self.scores_table[..., _UNC]))
    base_rate = property(lambda self: self._field(self.scores_table[..., _BASE]))
    roc_area = property(lambda self: self._field(self.scores_table[..., _AREA]))
    observed_frequency = property(lambda self: self._field(self.bins_table[:, :, 0]))
    forecast_weight = property(lambda self: self._field(self.bins_table[:, :, 1]))
    hit_rate = property(lambda self: self._field(self.roc_table[:, :, 0]))
    false_alarm_rate = property(lambda self: self._field(self.roc_table[:, :, 1]))
    counts = property(lambda self: self._field(self.counts_table))
    rows = property(lambda self: self._field(self.rows_table))

    @property
    def count(self) -> dict[str, torch.Tensor]:
        return self._field(self.counts_table[:, 0].sum(dim=(-1, -2)))

    def cpu(self) -> "ProbabilityScores":
        """The same scores with host tensors (waits for the device)."""
        moved = {f: getattr(self, f).cpu() for f in ("rows_table", "counts_table", "scores_table", "bins_table", "roc_table",
                                                     "forecast_probability")}
        return dataclasses.replace(self, **moved)


# ---- the integers on the host ------------------------------------------------------------------------------------------
def _rows_host(members: np.ndarray, truth: np.ndarray, thr: np.ndarray, below: bool) -> np.ndarray:
    """The table of include/aurora_hip.h for (M, n_planes, n_lat, n_lon) members, (n_planes, n_lat, n_lon) truth and (n_planes,
    T) float32 thresholds, in numpy integers (one bincount per plane and threshold): (n_planes, n_lat, T, 2, M + 1) int32."""
    members, truth = members.astype(np.float32, copy=False), truth.astype(np.float32, copy=False)
    M, (n_planes, n_lat, n_lon) = members.shape[0], truth.shape
    T, per_row = thr.shape[1], 2 * (M + 1) + 1                          # (the last bin of a row takes its invalid points)
    rows = np.zeros((n_planes, n_lat, T, 2, M + 1), dtype=np.int32)
    cmp = np.less_equal if below else np.greater_equal
    first = (np.arange(n_lat) * per_row)[:, None]
    for p in range(n_planes):
        x, y = members[:, p], truth[p]
        ok = np.isfinite(y) & np.isfinite(x).all(axis=0)
        for t, th in enumerate(thr[p]):
            with np.errstate(invalid="ignore"):
                k, o = cmp(x, th).sum(axis=0), cmp(y, th)
            index = first + np.where(ok, o * (M + 1) + k, per_row - 1)
            bins = np.bincount(index.reshape(-1), minlength=n_lat * per_row).reshape(n_lat, per_row)
            rows[p, :, t] = bins[:, :-1].reshape(n_lat, 2, M + 1)
    return rows


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
def _finalise(rows: torch.Tensor, w: torch.Tensor, thr: torch.Tensor, M: int):
    """(counts (P, T, 2, M + 1) int64, scores (P, T, 8), bins (P, T, 2, M + 1), roc (P, T, 2, M + 2) fp64, p (M + 1,) fp64)
    from the integer table; elementwise operations and fixed trees on the device of `rows`, no read-back."""
    nan = float("nan")
    counts = rows.sum(dim=1, dtype=torch.int64)
    wr = w[:, None, None, None]
    r = rows.to(torch.float64)                                           # exact: every entry is below 2^31
    # ROC: per row the number of points with k >= c, c = M + 1 .. 0 (sums of integers: exact in fp64 in any order)
    above = torch.cat([torch.zeros_like(r[..., :1]), r.flip(-1).cumsum(dim=-1)], dim=-1)            # (P, n_lat, T, 2, M + 2)
    WA = _tree_sum_rows(torch.cat([r, above], dim=-1) * wr)              # both weighted and added over the rows in one tree
    W, A = WA[..., :M + 1], WA[..., M + 1:]                              # (P, T, 2, M + 1), (P, T, 2, M + 2)
    valid = rows[:, :, 0].sum(dim=(-1, -2), dtype=torch.int64)           # (P, n_lat): the same for every threshold
    N = _tree_sum(valid.to(torch.float64) * w)[:, None]                  # (P, 1)
    k = torch.arange(M + 1, dtype=torch.float64, device=rows.device)
    # (every divisor is a tensor: a division by a Python number is a multiplication by its reciprocal on the GPU and a division
    #  on the CPU, which would part the two paths in the last bit)
    p = k / torch.full_like(k, M)
    W0, W1 = W[:, :, 0], W[:, :, 1]
    n_k = W0 + W1
    some = n_k > 0
    zero = torch.zeros_like(n_k)
    brier = _ratio(_tree_sum(W1 * ((1 - p) * (1 - p)) + W0 * (p * p)), N)
    obar = _ratio(_tree_sum(W1), N)
    unc = obar * (1 - obar)
    obar_k = torch.where(some, W1 / torch.where(some, n_k, torch.ones_like(n_k)), torch.full_like(n_k, nan))
    d_rel, d_res = p - obar_k, obar_k - obar[..., None]
    rel = _ratio(_tree_sum(torch.where(some, n_k * (d_rel * d_rel), zero)), N)
    res = _ratio(_tree_sum(torch.where(some, n_k * (d_res * d_res), zero)), N)
    skill = 1 - _ratio(brier, unc)
    fair = brier - _ratio(_tree_sum(n_k * (k * (M - k) / torch.full_like(k, M * M * (M - 1)))), N)
    rate = _ratio(A, A[..., -1:].expand_as(A))                           # [o = 0: non-events, o = 1: events]
    H, F = rate[:, :, 1], rate[:, :, 0]
    area = _tree_sum((F[..., 1:] - F[..., :-1]) * (H[..., 1:] + H[..., :-1]) / 2)
    scores = torch.stack([brier, fair, skill, rel, res, unc, obar, area], dim=-1)
    bins = torch.stack([obar_k, _ratio(n_k, N[..., None].expand_as(n_k))], dim=2)
    roc = torch.stack([H, F], dim=2)
    padded = torch.isnan(thr)                                            # (P, T)
    scores = torch.where(padded[..., None], torch.full_like(scores, nan), scores)
    bins = torch.where(padded[..., None, None], torch.full_like(bins, nan), bins)
    roc = torch.where(padded[..., None, None], torch.full_like(roc, nan), roc)
    return counts, scores, bins, roc, p


# ---- public function -----------------------------------------------------------------------------------------------------
def probability_scores(members: Union[Batch, Sequence[Batch]], truth: Batch, thresholds: Mapping[str, object],
                       below: bool = False) -> ProbabilityScores:
    """Brier score, its decomposition and skill, reliability diagram and ROC of the fraction of M members over each threshold,
    of the last history entry of the variables named in `thresholds`; see the module's text."""
    if not isinstance(thresholds, Mapping) or not thresholds:
        raise ValueError("probability_scores: thresholds must be a non-empty mapping from variable name to values")
    names, truth_fields, member_fields, layout = _fields.select_members("probability_scores", members, truth, only=thresholds)
    thr = _fields.threshold_table("probability_scores", thresholds, layout) if names else None
    for k in thresholds:
        if k not in names:
            raise ValueError(f"probability_scores: thresholds name the variable {k!r}, which members and truth do not all hold "
                             "as a surface or atmospheric variable")
    M = len(member_fields)
    n_lat, n_lon = truth.metadata.lat.shape[0], truth.metadata.lon.shape[0]

    everything = [("truth", names, truth_fields)] + [(f"members[{m}]", names, fs) for m, fs in enumerate(member_fields)]
    device = _fields.place("probability_scores", everything, n_lat, n_lon, fields="the fields of members and truth")
    lat = _fields._host(truth.metadata.lat)
    if device == "cpu":
        rows = torch.from_numpy(_rows_host(np.stack([_fields.stack(fs, n_lat, n_lon) for fs in member_fields]),
                                           _fields.stack(truth_fields, n_lat, n_lon), thr, bool(below)))
        thr_t, w = torch.from_numpy(thr), torch.from_numpy(latitude_weights(lat))
    else:
        from aurora_amd.engine import lib

        thr_t = _fields.device_thresholds("probability_scores", thr, device)
        rows = lib.probability_rows(member_fields, truth_fields, thr_t, bool(below))
        w = _fields.device_weights("probability_scores", lat, device)
    counts, scores, bins, roc, p = _finalise(rows, w, thr_t, M)
    return ProbabilityScores(rows, counts, scores, bins, roc, p, layout, M, bool(below))
