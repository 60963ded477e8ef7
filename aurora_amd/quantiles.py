"""The ensemble products a forecaster looks at first, where the members live: per-point QUANTILE maps -- the median, the
10 % and 90 % maps, the interquartile range -- and the map of where the truth fell among the members (not in the reference).

    eq = aurora_amd.ensemble_quantiles(members, q=(0.1, 0.5, 0.9), truth=None)
    eq.quantile["2t"]     # (B, Q, H, W) float32; atmospheric: (B, C, Q, H, W); on the members' device
    eq.as_batch(0.5)      # a float32 Batch, one history entry, of one requested q
    eq.rank["2t"]         # with a truth: (B, H, W) / (B, C, H, W) int8 = #{m : x_m < y}, -1 where not defined
    eq.q, eq.members      # the q values as given (fp64 tuple), M
    eq.cpu()              # the same object with host tensors: the one call that waits for the device

`members` is as in `ensemble_scores`: a sequence of 2 to 64 `Batch`es on one grid (results of their batch size), or ONE
`Batch` whose batch elements are the members (results of B = 1).  Any 2 to 64 batches are valid samples: the steps of a
roll-out give the per-point median over time.  The last history entry of every surface and atmospheric variable that all
members (and `truth`, if given) hold is used.  `q` is 1 to 8 finite values in [0, 1], in any order, repeats allowed.
`as_batch` carries the metadata and the static variables of the first member, so every scorer, `FieldStats.update`,
`diagnostics`, `regrid` and `to_netcdf` take it unchanged.

THE RULE, which the kernel and the numpy path both implement, bit for bit:

    validity   a point is valid where all M members are finite; at an invalid point every quantile is NaN
    order      the M fp32 values are put in ascending order of the integer key bits ^ ((bits >> 31) & 0x7fffffff): the
               order of the floats with -0 below +0 (`np.sort` would leave +-0 in input order)
    index      for each q: h = (M - 1) q in fp64, j = min(floor(h), M - 1), g = h - j, hi = min(j + 1, M - 1)
    value      (float32)(a + g (b - a)) with a = (double)x_(j), b = (double)x_(hi): three fp64 operations, each rounded on
               its own (no fused multiply-add), then one rounding to fp32.  With g = 0 the value is x_(j): q = 0 is the
               minimum and q = 1 the maximum.  (This is numpy's method="linear", which takes b - (b - a)(1 - g) for g >= 0.5
               instead: at most one fp32 unit in the last place apart.)
    rank       with a truth y: #{m : x_m < y}, the values compared as stored (the rule of `ensemble_scores`' rank histogram:
               its bins count this map's values); -1 where y or any member is not finite.  The quantiles do not depend on
               the truth.

Fields on one GPU take ONE aurora_hip_ensemble_quantiles call (`aurora_amd/csrc/ensemble_quantiles.hip`): one launch, every
member plane read once, a point's M values sorted in registers, nothing allocated but the maps, nothing read back.  Fields on
the CPU take the rule in numpy (after a conversion to float32).  Neither depends on the order of the members.

Not offered: NaN-skipping quantiles, other interpolation types, weighted members, more than 64 samples, latitude bands
(`BandBatch`).
"""

from __future__ import annotations

import copy
import dataclasses
from typing import Optional, Sequence, Union

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._fields import MAX_MEMBERS
from aurora_amd.batch import Batch, Metadata

__all__ = ["ensemble_quantiles", "EnsembleQuantiles", "MAX_MEMBERS", "MAX_QUANTILES"]

MAX_QUANTILES = 8


@dataclasses.dataclass(frozen=True)
class EnsembleQuantiles:
    """Result of `ensemble_quantiles`; see the module's text."""

    maps: torch.Tensor                                   # (n_planes, Q, H, W) float32
    ranks: Optional[torch.Tensor]                        # (n_planes, H, W) int8, or None without a truth
    layout: _fields.Layout                               # (name, first plane, shape) per variable
    q: tuple[float, ...]
    members: int
    like: tuple[Metadata, dict]                          # the metadata (of the results' batch size) and static variables
                                                         #   of the first member

    @property
    def quantile(self) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, self.maps)

    @property
    def rank(self) -> dict[str, torch.Tensor]:
        if self.ranks is None:
            raise ValueError("ensemble_quantiles: no truth was given, so there is no rank map")
        return _fields.by_variable(self.layout, self.ranks)

    def as_batch(self, q: float) -> Batch:
        """The map of one requested q as a float32 `Batch` (one history entry)."""
        if float(q) not in self.q:
            raise ValueError(f"ensemble_quantiles: as_batch offers the requested q {self.q}, got {q!r}")
        maps = _fields.by_variable(self.layout, self.maps[:, self.q.index(float(q))])
        surf = {name: maps[name][:, None] for name, _, shape in self.layout if len(shape) == 1}
        atmos = {name: maps[name][:, None] for name, _, shape in self.layout if len(shape) == 2}
        md, static = self.like
        return Batch(surf, dict(static), atmos, md)

    def cpu(self) -> "EnsembleQuantiles":
        """The same maps with host tensors (waits for the device)."""
        return dataclasses.replace(self, maps=self.maps.cpu(), ranks=None if self.ranks is None else self.ranks.cpu())


# ---- the rule on the host -------------------------------------------------------------------------------------
def quantile_index(M: int, q: Sequence[float]) -> tuple[np.ndarray, np.ndarray]:
    """(j, g) of the rule for every q: int64 and fp64 arrays."""
    h = (M - 1) * np.asarray(q, dtype=np.float64)
    j = np.minimum(np.floor(h), M - 1)
    return j.astype(np.int64), h - j


def _quantiles_host(members: np.ndarray, truth: Optional[np.ndarray], q: Sequence[float]):
    """The rule for (M, n_planes, n_lat, n_lon) float32 members and (n_planes, n_lat, n_lon) truth or None, in numpy:
    (n_planes, Q, n_lat, n_lon) float32 and (n_planes, n_lat, n_lon) int8 or None."""
    M = members.shape[0]
    x = np.ascontiguousarray(members, dtype=np.float32)
    bits = x.view(np.int32)
    key = bits ^ ((bits >> 31) & 0x7fffffff)
    s = np.take_along_axis(x, np.argsort(key, axis=0, kind="stable"), axis=0).astype(np.float64)
    valid = np.isfinite(x).all(axis=0)
    out = np.empty((len(q), *x.shape[1:]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (j, g) in enumerate(zip(*quantile_index(M, q))):
            a, b = s[j], s[min(j + 1, M - 1)]
            d = b - a
            t = g * d
            out[i] = np.where(valid, a + t, np.nan).astype(np.float32)
        rank = None
        if truth is not None:
            rank = np.where(valid & np.isfinite(truth), (x < truth).sum(axis=0), -1).astype(np.int8)
    return np.ascontiguousarray(np.moveaxis(out, 0, 1)), rank


# ---- public function -----------------------------------------------------------------------------------------
def ensemble_quantiles(members: Union[Batch, Sequence[Batch]], q: Sequence[float] = (0.1, 0.5, 0.9),
                       truth: Optional[Batch] = None) -> EnsembleQuantiles:
    """Per-point quantile maps of M members and, with `truth`, the map of its rank among them; see the module's text."""
    try:
        qs = tuple(float(v) for v in (q if np.ndim(q) else (q,)))
    except (TypeError, ValueError):
        raise ValueError("ensemble_quantiles: q must be numbers") from None
    if not 1 <= len(qs) <= MAX_QUANTILES:
        raise ValueError(f"ensemble_quantiles: 1 to {MAX_QUANTILES} values of q, got {len(qs)}")
    if not all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in qs):
        raise ValueError(f"ensemble_quantiles: q must be finite values in [0, 1], got {qs}")
    names, truth_fields, member_fields, layout = _fields.select_samples("ensemble_quantiles", members, truth)
    if not names:
        raise ValueError("ensemble_quantiles: the members" + (" and truth" if truth is not None else "") +
                         " have no surface or atmospheric variable in common")
    M = len(member_fields)
    first = members if isinstance(members, Batch) else members[0]
    md = first.metadata
    n_lat, n_lon = md.lat.shape[0], md.lon.shape[0]
    B = member_fields[0][0].shape[0]
    if len(md.time) != B:                                  # ONE Batch of members: the first member's time (a copy: building a
        md = copy.copy(md)                                 #   Metadata checks its coordinates, which waits for the device)
        md.time = tuple(md.time[:B])
    like = (md, dict(first.static_vars))

    everything = [(f"members[{m}]", names, fs) for m, fs in enumerate(member_fields)]
    if truth is not None:
        everything.append(("truth", names, truth_fields))
    device = _fields.place("ensemble_quantiles", everything, n_lat, n_lon, task=_fields.TAKES_TASK,
                           fields="the fields of members and truth" if truth is not None else "the fields of members")
    if device == "cpu":
        host = lambda fs: _fields.stack([f.to(torch.float32) for f in fs], n_lat, n_lon)  # noqa: E731
        maps, ranks = _quantiles_host(np.stack([host(fs) for fs in member_fields]), None if truth is None else host(truth_fields), qs)
        maps, ranks = torch.from_numpy(maps), None if ranks is None else torch.from_numpy(ranks)
    else:
        from aurora_amd.engine import lib

        maps, ranks = lib.ensemble_quantiles(member_fields, truth_fields, qs)
    return EnsembleQuantiles(maps, ranks, layout, qs, M, like)
