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
import threading
import weakref
from typing import Optional

import numpy as np
import torch

from aurora_amd.batch import BandBatch, Batch

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
        out = {}
        for name, first, shape in self.layout:
            n = int(np.prod(shape))
            v = self.table[first:first + n, col]
            out[name] = v.reshape(*shape, *v.shape[1:])
        return out

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


# ---- coordinates and weights -------------------------------------------------------------------------------
_lock = threading.Lock()
_host_coords: dict[int, tuple] = {}        # id(tensor) -> (weak reference, version, fp64 host copy)
_weights: dict[tuple, torch.Tensor] = {}   # (latitude bytes, device) -> device weights


def _version(t: torch.Tensor) -> int:
    return 0 if t.is_inference() else t._version   # (inference tensors keep no version counter)


def _host(t: torch.Tensor) -> np.ndarray:
    """fp64 host copy of a coordinate tensor, remembered per tensor object: the first call for a device tensor waits for
    the device, later calls (every step of a roll-out carries the same coordinates) do not."""
    with _lock:
        hit = _host_coords.get(id(t))
        if hit is not None and hit[0]() is t and hit[1] == _version(t):
            return hit[2]
    a = t.detach().to(torch.float64).cpu().numpy()
    a.setflags(write=False)
    key = id(t)

    def forget(_ref, key=key):
        with _lock:
            cur = _host_coords.get(key)
            if cur is not None and cur[0] is _ref:
                del _host_coords[key]

    with _lock:
        _host_coords[key] = (weakref.ref(t, forget), _version(t), a)
    return a


def latitude_weights(lat) -> np.ndarray:
    """w[i] = cos(lat[i]) / mean_j cos(lat[j]) in fp64 (latitudes in degrees, a vector within [-90, 90])."""
    lat = np.asarray(lat, dtype=np.float64)
    if lat.ndim != 1 or lat.size == 0:
        raise ValueError("scores: latitudes must be a non-empty vector")
    if not np.all(np.isfinite(lat)) or lat.max() > 90 or lat.min() < -90:
        raise ValueError("scores: latitudes must be in the range [-90, 90]")
    c = np.maximum(np.cos(np.deg2rad(lat)), 0.0)
    mean = c.mean()
    if not mean > 0:
        raise ValueError("scores: the latitudes carry no weight (every row is a pole)")
    return c / mean


def _device_weights(lat: np.ndarray, device: torch.device) -> torch.Tensor:
    key = (lat.tobytes(), str(device))
    with _lock:
        hit = _weights.get(key)
    if hit is None:
        hit = torch.from_numpy(latitude_weights(lat)).to(device)
        with _lock:
            if len(_weights) >= 64:
                _weights.clear()
            _weights[key] = hit
    return hit


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
def _check_same_grid(pred: Batch, other: Batch, what: str) -> None:
    for b, name in ((pred, "pred"), (other, what)):
        if isinstance(b, BandBatch):
            raise ValueError(f"scores: {name} is a latitude band (BandBatch); gather the forecast first, band scores are "
                             "not supported")
        if b.metadata.lat.dim() != 1 or b.metadata.lon.dim() != 1:
            raise ValueError(f"scores: {name} has matrices for latitudes / longitudes; vector coordinates are needed")
    for c in ("lat", "lon"):
        a, o = getattr(pred.metadata, c), getattr(other.metadata, c)
        if a.shape != o.shape:
            hint = ""
            if c == "lat" and o.shape[0] == a.shape[0] + 1:
                hint = f"; the prediction was cropped to the model's patch size: use {what}.crop(model.patch_size)"
            raise ValueError(f"scores: pred and {what} differ in {c}: {a.shape[0]} against {o.shape[0]} values{hint}")
        if a is not o and not np.array_equal(_host(a), _host(o)):
            raise ValueError(f"scores: pred and {what} differ in {c} (same length, different values)")
    if tuple(pred.metadata.atmos_levels) != tuple(other.metadata.atmos_levels):
        raise ValueError(f"scores: pred and {what} differ in atmos_levels: {tuple(pred.metadata.atmos_levels)} against "
                         f"{tuple(other.metadata.atmos_levels)}")


def scores(pred: Batch, truth: Batch, climatology: Optional[Batch] = None) -> Scores:
    """Latitude-weighted RMSE, bias, MAE (and ACC with a `climatology`) of the last history entry of every surface and
    atmospheric variable that both `pred` and `truth` hold; see the module's text."""
    batches = [("truth", truth)] + ([("climatology", climatology)] if climatology is not None else [])
    for what, b in batches:
        _check_same_grid(pred, b, what)
    n_lat, n_lon = pred.metadata.lat.shape[0], pred.metadata.lon.shape[0]

    names, fields = [], [[] for _ in range(1 + len(batches))]
    for group in ("surf_vars", "atmos_vars"):
        for k, v in getattr(pred, group).items():
            if k not in getattr(truth, group):
                continue
            if climatology is not None and k not in getattr(climatology, group):
                raise ValueError(f"scores: the climatology has no {group[:-5]} variable {k!r}")
            if k in names:
                raise ValueError(f"scores: {k!r} is both a surface and an atmospheric variable")
            names.append(k)
            for slot, (what, b) in enumerate([("pred", pred)] + batches):
                f = getattr(b, group)[k]
                want = 4 if group == "surf_vars" else 5
                if f.dim() != want or tuple(f.shape[-2:]) != (n_lat, n_lon):
                    raise ValueError(f"scores: {what}.{group}[{k!r}] has shape {tuple(f.shape)}, which does not fit a "
                                     f"{n_lat} x {n_lon} grid")
                f = f[:, -1]
                if slot and f.shape != fields[0][-1].shape:
                    p_shape = fields[0][-1].shape
                    what_differs = "batch size" if f.shape[0] != p_shape[0] else "shape"
                    raise ValueError(f"scores: pred and {what} differ in {what_differs} for {k!r}: {tuple(p_shape)} against "
                                     f"{tuple(f.shape)}")
                fields[slot].append(f)
    if not names:
        raise ValueError("scores: pred and truth have no surface or atmospheric variable in common")

    layout, first = [], 0
    for name, f in zip(names, fields[0]):
        shape = tuple(f.shape[:-2])
        layout.append((name, first, shape))
        first += int(np.prod(shape))

    devices = {f.device for fs in fields for f in fs}
    lat = _host(pred.metadata.lat)
    if all(d.type == "cpu" for d in devices):
        stack = lambda fs: np.concatenate([f.detach().reshape(-1, n_lat, n_lon).numpy() for f in fs])  # noqa: E731
        sums = torch.from_numpy(_sums_host(stack(fields[0]), stack(fields[1]),
                                           stack(fields[2]) if climatology is not None else None, latitude_weights(lat)))
    elif len(devices) == 1 and next(iter(devices)).type == "cuda":
        from aurora_amd.engine import lib

        dev = next(iter(devices))
        for what, fs in zip(("pred", "truth", "climatology"), fields):
            for name, f in zip(names, fs):
                if f.dtype != torch.float32:
                    raise TypeError(f"scores: {what} variable {name!r} is {f.dtype}; the device path scores float32 fields "
                                    "(move the batches to the CPU to score other precisions)")
                if (n_lon > 1 and f.stride(-1) != 1) or (n_lat > 1 and f.stride(-2) != n_lon):
                    raise ValueError(f"scores: the planes of {what} variable {name!r} are not row-major contiguous; "
                                     "call .contiguous() on it first")
        sums = lib.scores_sums(fields[0], fields[1], fields[2] if climatology is not None else None,
                               _device_weights(lat, dev))
    else:
        raise ValueError(f"scores: the fields are on {sorted(map(str, devices))}; move the batches to the CPU or to one GPU "
                         "first")
    return Scores(_finalise(sums, climatology is not None), tuple(layout), climatology is not None)


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
