"""Verifying an ENSEMBLE where it lives: CRPS, the ensemble mean's RMSE / bias / MAE, the spread, their ratio and the rank
histogram per variable and level against truth (WeatherBench 2's probabilistic columns; not in the reference).

    s = aurora_amd.ensemble_scores(members, truth)
    s.crps["z"]          # (B, C) float64 on the members' device; also fair_crps, rmse, bias, mae, spread, spread_skill
    s.rank_hist["2t"]    # (B, M + 1) int64; also count, ties (int64), sums (..., 8), members (M)
    s.cpu()              # the same object with host tensors: the one call that waits for the device

`members` is a sequence of M >= 2 `Batch`es on one grid with the batch size B of `truth` (a lagged ensemble, separate
roll-outs): plane (b, c) of member m is scored against plane (b, c) of `truth`.  Or it is ONE `Batch` of batch size M >= 2
while `truth` has batch size 1: the batch elements are the members (a roll-out from M perturbed initial states) and the
results have B = 1.  M <= 64.  As in `scores`, the last history entry of every surface and atmospheric variable that all
members and `truth` hold is scored.

With the row weight w[i] = cos(lat[i]) / mean_j cos(lat[j]), a point valid where `truth` and ALL M members are finite, and
everything formed in fp64 from the differences to truth d_m = x_m - y (not from the raw values: a pressure of 1e5 Pa with a
spread of 1 Pa must not cost five digits), per valid point

    e = (sum_m d_m) / M  (members in member order)        a = (sum_m |d_m|) / M
    g = (1 / M^2) sum_i sum_j |d_i - d_j| = (2 / M^2) sum_k (2 k - M - 1) d_(k)  with d_(1) <= ... <= d_(M)
    v = sum_m (d_m - e)^2 / (M - 1)

and the sums over the valid points S0 = count, S1 = sum w, S2 = sum w e, S3 = sum w e^2, S4 = sum w |e|, S5 = sum w a,
S6 = sum w g, S7 = sum w v:

    bias = S2 / S1    rmse = sqrt(S3 / S1)    mae = S4 / S1          (of the ensemble mean)
    crps = (S5 - S6 / 2) / S1                  fair_crps = (S5 - (S6 / 2) M / (M - 1)) / S1
    spread = sqrt(S7 / S1)                     spread_skill = sqrt((M + 1) / M) spread / rmse   (NaN where rmse = 0)

A plane without a valid point gives NaN.  Rank histogram: a valid point adds 1 to bin #{m : x_m < y} of M + 1 (the values
compared as they are stored, unweighted); `ties` counts the valid points with some x_m == y, so that bounded variables
(clamped pollutants, wave heights) show when their low bins mean little.  Counts are exact integers.

Fields on one GPU are reduced by ONE aurora_hip_ensemble_scores call (every plane read once, the M values of a point sorted
in registers, a fixed reduction tree: bit-for-bit repeatable, and a plane's results do not depend on what else is scored
with it) and finalised by torch operations on the tiny result, so a roll-out can be scored step by step and read once at the
end.  Fields on the CPU take the same sums in numpy fp64.
"""

from __future__ import annotations

import dataclasses
from typing import Sequence, Union

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._fields import MAX_MEMBERS, latitude_weights
from aurora_amd.batch import Batch

__all__ = ["ensemble_scores", "EnsembleScores", "MAX_MEMBERS"]

_SUMS, _RMSE, _BIAS, _MAE, _CRPS, _FAIR, _SPREAD, _RATIO = slice(0, 8), 8, 9, 10, 11, 12, 13, 14


@dataclasses.dataclass(frozen=True)
class EnsembleScores:
    """Result of `ensemble_scores`: every score is a dict name -> tensor of shape (B,) for a surface variable and (B, C)
    for an atmospheric one, float64 (count, ties: int64), on the device of the members; `rank_hist` has a last dimension
    of M + 1 bins and `sums` one of the eight raw sums."""

    table: torch.Tensor                                  # (n_planes, 15): the eight sums, rmse, bias, mae, crps, fair_crps,
    hist: torch.Tensor                                   #   spread, spread_skill; (n_planes, M + 2) int64: the bins, the ties
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    members: int

    def _column(self, col, of=None) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, (self.table if of is None else of)[:, col])

    crps = property(lambda self: self._column(_CRPS))
    fair_crps = property(lambda self: self._column(_FAIR))
    rmse = property(lambda self: self._column(_RMSE))
    bias = property(lambda self: self._column(_BIAS))
    mae = property(lambda self: self._column(_MAE))
    spread = property(lambda self: self._column(_SPREAD))
    spread_skill = property(lambda self: self._column(_RATIO))
    sums = property(lambda self: self._column(_SUMS))

    @property
    def count(self) -> dict[str, torch.Tensor]:
        return {k: v.to(torch.int64) for k, v in self._column(0).items()}

    @property
    def rank_hist(self) -> dict[str, torch.Tensor]:
        return self._column(slice(0, self.members + 1), self.hist)

    @property
    def ties(self) -> dict[str, torch.Tensor]:
        return self._column(self.members + 1, self.hist)

    def cpu(self) -> "EnsembleScores":
        """The same scores with host tensors (waits for the device)."""
        return dataclasses.replace(self, table=self.table.cpu(), hist=self.hist.cpu())


# ---- the sums on the host ----------------------------------------------------------------------------------
def _ensemble_sums_host(members: np.ndarray, truth: np.ndarray, w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The eight sums and the M + 2 counts of include/aurora_hip.h for (M, n_planes, n_lat, n_lon) members against
    (n_planes, n_lat, n_lon) truth, in numpy fp64 (g in the sorted form): (n_planes, 8) and (n_planes, M + 2)."""
    M, n = members.shape[0], truth.shape[0]
    sums, hist = np.zeros((n, 8)), np.zeros((n, M + 2), dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)[:, None]
    coef = 2.0 * np.arange(1, M + 1) - M - 1
    for k in range(n):
        x, y = members[:, k], truth[k]
        ok = np.isfinite(y) & np.isfinite(x).all(axis=0)
        x, y = x[:, ok], y[ok]
        wk = np.broadcast_to(w, ok.shape)[ok]
        d = x.astype(np.float64) - y.astype(np.float64)
        e = d.sum(axis=0) / M
        a = np.abs(d).sum(axis=0) / M
        g = (2.0 / M ** 2) * (coef[:, None] * np.sort(d, axis=0)).sum(axis=0)
        v = ((d - e) ** 2).sum(axis=0) / (M - 1)
        sums[k] = ok.sum(), wk.sum(), (wk * e).sum(), (wk * e * e).sum(), (wk * np.abs(e)).sum(), (wk * a).sum(), \
            (wk * g).sum(), (wk * v).sum()
        hist[k, :M + 1] = np.bincount((x < y).sum(axis=0), minlength=M + 1)
        hist[k, M + 1] = (x == y).any(axis=0).sum()
    return sums, hist


# ---- public function -----------------------------------------------------------------------------------------
def ensemble_scores(members: Union[Batch, Sequence[Batch]], truth: Batch) -> EnsembleScores:
    """CRPS, fair CRPS, the ensemble mean's RMSE / bias / MAE, spread, spread / skill and the rank histogram of M members
    against `truth`; see the module's text."""
    names, truth_fields, member_fields, layout = _fields.select_members("ensemble_scores", members, truth)
    if not names:
        raise ValueError("ensemble_scores: members and truth have no surface or atmospheric variable in common")
    M = len(member_fields)
    n_lat, n_lon = truth.metadata.lat.shape[0], truth.metadata.lon.shape[0]

    everything = [("truth", names, truth_fields)] + [(f"members[{m}]", names, fs) for m, fs in enumerate(member_fields)]
    device = _fields.place("ensemble_scores", everything, n_lat, n_lon, fields="the fields of members and truth")
    lat = _fields._host(truth.metadata.lat)
    if device == "cpu":
        sums, hist = _ensemble_sums_host(np.stack([_fields.stack(fs, n_lat, n_lon) for fs in member_fields]),
                                         _fields.stack(truth_fields, n_lat, n_lon), latitude_weights(lat))
        sums, hist = torch.from_numpy(sums), torch.from_numpy(hist)
    else:
        from aurora_amd.engine import lib

        sums, hist = lib.ensemble_scores_sums(member_fields, truth_fields, _fields.device_weights("ensemble_scores", lat, device))
    return EnsembleScores(_finalise(sums, M), hist, layout, M)


def _finalise(sums: torch.Tensor, M: int) -> torch.Tensor:
    """(n_planes, 8) sums -> (n_planes, 15) table; elementwise torch operations on the device of `sums`, no read-back."""
    nan = torch.full_like(sums[:, 0], float("nan"))
    s1 = sums[:, 1]
    some = sums[:, 0] > 0
    rmse = torch.where(some, torch.sqrt(sums[:, 3] / s1), nan)
    bias = torch.where(some, sums[:, 2] / s1, nan)
    mae = torch.where(some, sums[:, 4] / s1, nan)
    crps = torch.where(some, (sums[:, 5] - sums[:, 6] / 2) / s1, nan)
    fair = torch.where(some, (sums[:, 5] - (sums[:, 6] / 2) * (M / (M - 1))) / s1, nan)
    spread = torch.where(some, torch.sqrt(sums[:, 7] / s1), nan)
    ratio = torch.where(some & (rmse > 0), float(np.sqrt((M + 1) / M)) * spread / rmse, nan)
    return torch.cat([sums, torch.stack([rmse, bias, mae, crps, fair, spread, ratio], dim=1)], dim=1)
