"""Verifying a forecast where it lives: latitude-weighted RMSE / bias / MAE per variable and level against truth, and the
anomaly correlation (ACC) against a climatology (not in the reference, which has no scoring function).

    s = aurora_amd.scores(pred, truth, climatology=None)
    s.rmse["2t"]    # (B,)   float64, on pred's device
    s.rmse["z"]     # (B, C) one value per pressure level
    s.bias, s.mae, s.acc, s.count, s.sums
    s.cpu()         # the same object with host tensors: the one call that waits for the device

With the row weight w[i] = cos(lat[i]) / mean_j cos(lat[j]) and the sums S over the points where the prediction, the
truth and (if given) the climatology are all finite -- S1 = sum w, S2 = sum w d, S3 = sum w d^2, S4 = sum w |d| with
d = pred - truth; S5 = sum w p' t', S6 = sum w p'^2, S7 = sum w t'^2 with p' = pred - clim, t' = truth - clim --

    bias = S2 / S1    rmse = sqrt(S3 / S1)    mae = S4 / S1    acc = S5 / sqrt(S6 S7)

A plane without a valid point, and an ACC with a zero denominator, give NaN.  Fields on one GPU are reduced by ONE
aurora_hip_scores call (fp64 differences and accumulation, a fixed reduction tree: bit-for-bit repeatable, and a plane's
sums do not depend on what else is scored with it) and finalised by torch operations on the tiny fp64 result, so a
roll-out can be scored step by step and read once at the end.  Fields on the CPU take the same sums in numpy fp64.
"""

from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._fields import latitude_weights
from aurora_amd.batch import Batch

__all__ = ["scores", "Scores", "latitude_weights"]

_SUMS, _RMSE, _BIAS, _MAE, _ACC, _COLS = slice(0, 8), 8, 9, 10, 11, 12


@dataclasses.dataclass(frozen=True)
class Scores:
    """Result of `scores`: every property is a dict name -> tensor of shape (B,) for a surface variable and (B, C) for an
    atmospheric one, float64 (count: int64), on the device of the prediction.  `acc` is None without a climatology;
    `sums` holds the eight raw sums in a last dimension."""

    table: torch.Tensor                                  # (n_planes, 12): the eight sums, rmse, bias, mae, acc
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    has_climatology: bool

    def _column(self, col) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, self.table[:, col])

    @property
    def rmse(self) -> dict[str, torch.Tensor]:
        return self._column(_RMSE)

    @property
    def bias(self) -> dict[str, torch.Tensor]:
        return self._column(_BIAS)

    @property
    def mae(self) -> dict[str, torch.Tensor]:
        return self._column(_MAE)

    @property
    def acc(self) -> Optional[dict[str, torch.Tensor]]:
        return self._column(_ACC) if self.has_climatology else None

    @property
    def count(self) -> dict[str, torch.Tensor]:
        return {k: v.to(torch.int64) for k, v in self._column(0).items()}

    @property
    def sums(self) -> dict[str, torch.Tensor]:
        return self._column(_SUMS)

    def cpu(self) -> "Scores":
        """The same scores with host tensors (one copy; waits for the device)."""
        return dataclasses.replace(self, table=self.table.cpu())


# ---- the sums on the host ----------------------------------------------------------------------------------
def _sums_host(pred: np.ndarray, truth: np.ndarray, clim: Optional[np.ndarray], w: np.ndarray) -> np.ndarray:
    """The eight sums of include/aurora_hip.h for (n_planes, n_lat, n_lon) arrays, in numpy fp64: (n_planes, 8)."""
    out = np.zeros((pred.shape[0], 8))
    w = np.asarray(w, dtype=np.float64)[:, None]
    for k in range(pred.shape[0]):
        p, t = pred[k].astype(np.float64), truth[k].astype(np.float64)
        ok = np.isfinite(p) & np.isfinite(t)
        c = None
        if clim is not None:
            c = clim[k].astype(np.float64)
            ok &= np.isfinite(c)
        wk = np.broadcast_to(w, p.shape)[ok]
        d = p[ok] - t[ok]
        out[k, :5] = ok.sum(), wk.sum(), (wk * d).sum(), (wk * d * d).sum(), (wk * np.abs(d)).sum()
        if c is not None:
            pa, ta = p[ok] - c[ok], t[ok] - c[ok]
            out[k, 5:] = (wk * pa * ta).sum(), (wk * pa * pa).sum(), (wk * ta * ta).sum()
    return out


# ---- public function -----------------------------------------------------------------------------------------
def scores(pred: Batch, truth: Batch, climatology: Optional[Batch] = None) -> Scores:
    """Latitude-weighted RMSE, bias, MAE (and ACC with a `climatology`) of the last history entry of every surface and
    atmospheric variable that both `pred` and `truth` hold; see the module's text."""
    others = [("truth", truth)] + ([("climatology", climatology)] if climatology is not None else [])
    for what, b in others:
        _fields.check_same_grid("scores", pred, b, "pred", what, "the prediction")
    n_lat, n_lon = pred.metadata.lat.shape[0], pred.metadata.lon.shape[0]
    names, fields, layout = _fields.select_pair("scores", pred, others)
    if not names:
        raise ValueError("scores: pred and truth have no surface or atmospheric variable in common")

    device = _fields.place("scores", [(what, names, fs) for what, fs in zip(("pred", "truth", "climatology"), fields)], n_lat, n_lon)
    lat = _fields._host(pred.metadata.lat)
    if device == "cpu":
        p, t, *c = (_fields.stack(fs, n_lat, n_lon) for fs in fields)
        sums = torch.from_numpy(_sums_host(p, t, c[0] if c else None, latitude_weights(lat)))
    else:
        from aurora_amd.engine import lib

        sums = lib.scores_sums(fields[0], fields[1], fields[2] if climatology is not None else None,
                               _fields.device_weights("scores", lat, device))
    return Scores(_finalise(sums, climatology is not None), layout, climatology is not None)


def _finalise(sums: torch.Tensor, has_clim: bool) -> torch.Tensor:
    """(n_planes, 8) sums -> (n_planes, 12) table; elementwise torch operations on the device of `sums`, no read-back."""
    nan = torch.full_like(sums[:, 0], float("nan"))
    s1 = sums[:, 1]
    some = sums[:, 0] > 0
    rmse = torch.where(some, torch.sqrt(sums[:, 3] / s1), nan)
    bias = torch.where(some, sums[:, 2] / s1, nan)
    mae = torch.where(some, sums[:, 4] / s1, nan)
    acc = nan
    if has_clim:
        den = torch.sqrt(sums[:, 6]) * torch.sqrt(sums[:, 7])
        acc = torch.where(den > 0, sums[:, 5] / den, nan)
    return torch.cat([sums, torch.stack([rmse, bias, mae, acc], dim=1)], dim=1)
