"""Inputs that the two conservative_regrid test modules share: the grids of the issue and seeded batches on them."""
from datetime import datetime

import numpy as np
import torch

from aurora_amd import Batch, Metadata
from aurora_amd.batch import derive_metadata

LEVELS = (100, 500, 850)


def lin(a, b, n):
    return np.linspace(a, b, n)


def circle(n):
    return np.linspace(0, 360, n, endpoint=False)


# name -> (source lat, source lon, target lat, target lon)
GRIDS = {
    "poles 19x36 -> 8x14": (lin(90, -90, 19), circle(36), lin(90, -90, 8), circle(14)),
    "ascending 13x24 -> descending 5x9": (lin(-90, 90, 13), circle(24), lin(90, -90, 5), circle(9)),
    "no poles 12x20 -> 7x12": (lin(82.5, -82.5, 12), circle(20), 90.0 - (np.arange(7) + 0.5) * (180.0 / 7), circle(12)),
    "regional 13x13 -> overhanging 6x6": (lin(60, 30, 13), lin(10, 40, 13), lin(64.5, 25.5, 6), lin(5.5, 44.5, 6)),
    "finer 8x14 -> 19x36": (lin(90, -90, 8), circle(14), lin(90, -90, 19), circle(36)),
}
GLOBAL = [k for k in GRIDS if not k.startswith("regional")]

_BASE = Metadata(lat=torch.tensor([1.0, 0.0], dtype=torch.float64), lon=torch.tensor([0.0, 1.0], dtype=torch.float64),
                 time=(datetime(2023, 1, 1, 6),), atmos_levels=LEVELS)


def metadata(lat, lon, B=1, levels=LEVELS, rollout_step=3) -> Metadata:
    """Unvalidated, so that ascending latitudes pass (the rule takes both directions)."""
    return derive_metadata(_BASE, lat=torch.from_numpy(np.array(lat, dtype=np.float64)), lon=torch.from_numpy(np.array(lon, dtype=np.float64)),
                           time=tuple(datetime(2023, 1, 1 + b, 6) for b in range(B)), atmos_levels=tuple(levels), rollout_step=rollout_step)


def field(shape, seed, land=0.0, dtype=np.float32) -> np.ndarray:
    """280 + 20 N(0, 1) rounded to `dtype`, about `land` of the points NaN."""
    g = np.random.default_rng(seed)
    x = (280.0 + 20.0 * g.standard_normal(shape)).astype(dtype)
    if land:
        x[g.random(shape) < land] = np.nan
    return x


def batch(lat, lon, seed=0, B=1, T=2, land=0.0, dtype=torch.float32, levels=LEVELS) -> Batch:
    """2 surface variables, 1 static one and 1 atmospheric one on len(levels) levels: B T (2 + levels) + 1 planes."""
    n = (len(lat), len(lon))
    f = lambda k, *lead: torch.from_numpy(field((*lead, *n), 10 * seed + k, land, np.float64)).to(dtype)  # noqa: E731
    return Batch({"2t": f(0, B, T), "msl": f(1, B, T)}, {"lsm": f(2)}, {"z": f(3, B, T, len(levels))}, metadata(lat, lon, B, levels))


def every_field(b: Batch):
    for group in ("surf_vars", "static_vars", "atmos_vars"):
        for k, v in getattr(b, group).items():
            yield group, k, v


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
