"""The scores of `aurora_amd.scores` by region: latitude bands, longitude boxes and masks, as published scorecards report
them (not in the reference, which has no scoring function).

    regs = Regions({
        "global":        Region(),
        "tropics":       Region(lat=(-20, 20)),
        "extratropics":  Region(lat=[(-90, -20), (20, 90)]),
        "europe":        Region(lat=(35, 75), lon=(-12.5, 42.5)),
        "land":          Region(mask=batch.static_vars["lsm"] >= 0.5),
        "tropical land": Region(lat=(-20, 20), mask=batch.static_vars["lsm"] >= 0.5),
    })
    s = aurora_amd.region_scores(pred, truth, regs, climatology=None)
    s.regions           # ("global", "tropics", ...)
    s.rmse["2t"]        # (B, R) float64, on pred's device;  s.rmse["z"]: (B, C, R)
    s.bias, s.mae, s.acc, s.count, s.sums      # sums: (B[, C], R, 8), the eight sums of `scores`
    s["tropics"]        # an aurora_amd.Scores of that region
    s.cpu()             # the same object with host tensors: the one call that waits for the device

THE RULE, the same on both devices.  A point belongs to a region where its row, its column and its mask all say so:

    lat   a pair (lo, hi) of degrees or a sequence of pairs (their union); closed: row i belongs where lo <= lat[i] <= hi in
          float64 for some pair.  None: every row.
    lon   a pair (west, east) or a sequence of pairs.  Both ends and the grid's longitudes are reduced mod 360 into [0, 360);
          column j belongs where west <= lon[j] <= east, and where west > east after the reduction the box wraps:
          lon[j] >= west or lon[j] <= east.  None: every column.
    mask  a BOOL tensor or numpy array of shape (n_lat, n_lon), on the host or on the device of the fields.  None: every point.

Regions may overlap.  A latitude or longitude selection that holds no row or column of the grid is a ValueError (known on the
host); an all-False mask is not: it gives count 0 and NaN scores, and nothing is read back to find out.  A call takes 1 to 32
regions.  The weights are those of `scores` (`latitude_weights` over ALL rows of the grid), so a region's eight sums are the
sums of `scores` restricted to its points, validity is that of `scores`, and the finalisation is `scores`' own, per region.

Fields on one GPU are reduced by ONE aurora_hip_region_scores call per 8 regions (every input read once -- rows that belong
to no region of the call are not read at all -- fp64 throughout, the fixed reduction tree of `scores`: repeatable bit for bit,
and a region's sums depend on its own points alone, not on the other planes and not on which other regions, or how many, are
scored with it, so the grouping by eights does not show).  Fields on the CPU take the same sums in numpy fp64.

A `Regions` object keeps what a call needs: the row and column memberships per grid, their uint8 bit tables on the device
(bit r for region r of a launch; through the shared cache of small device tables, keyed by content), and the uint8 mask-bit
plane per grid and device (formed once by elementwise torch operations, without a synchronisation; masks are read at that
moment, so a mask changed afterwards needs a new `Regions`).  A second call with the same object uploads nothing, and after
one eager call the call can be captured in a hipGraph.  A dict is accepted in place of a `Regions`; one is then made for the
call, and its mask plane with it.
"""

from __future__ import annotations

import dataclasses
import threading
from typing import Mapping, Optional, Union

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._fields import latitude_weights
from aurora_amd.batch import Batch
from aurora_amd.scores import Scores, _finalise

__all__ = ["region_scores", "Region", "Regions", "RegionScores", "SCORECARD"]

MAX_REGIONS = 32
PER_LAUNCH = 8                                  # regions of one aurora_hip_region_scores call: the bits of a byte
_RMSE, _BIAS, _MAE, _ACC = 8, 9, 10, 11         # the columns of `Scores.table`


def _pairs(what: str, value) -> Optional[tuple[tuple[float, float], ...]]:
    """None, a pair or a sequence of pairs -> a tuple of (float, float)."""
    if value is None:
        return None
    try:
        a = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"Region: {what} must be a pair of degrees or a sequence of pairs, got {value!r}") from None
    if a.shape == (2,):
        a = a[None]
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] == 0 or not np.all(np.isfinite(a)):
        raise ValueError(f"Region: {what} must be a pair of degrees or a sequence of pairs, got {value!r}")
    return tuple((float(lo), float(hi)) for lo, hi in a)


@dataclasses.dataclass(frozen=True, eq=False)
class Region:
    """Where to score: see the module's text.  `lat` and `lon` are kept as tuples of pairs."""

    lat: Optional[tuple[tuple[float, float], ...]] = None
    lon: Optional[tuple[tuple[float, float], ...]] = None
    mask: Optional[Union[torch.Tensor, np.ndarray]] = None

    def __post_init__(self):
        object.__setattr__(self, "lat", _pairs("lat", self.lat))
        object.__setattr__(self, "lon", _pairs("lon", self.lon))
        for lo, hi in self.lat or ():
            if lo > hi:
                raise ValueError(f"Region: a latitude interval must ascend, got ({lo}, {hi})")
        m = self.mask
        if m is not None:
            if not isinstance(m, (torch.Tensor, np.ndarray)):
                raise TypeError(f"Region: mask must be a bool tensor or numpy array of shape (n_lat, n_lon), got {type(m).__name__}")
            if m.dtype not in (torch.bool, np.dtype(bool)) or m.ndim != 2:
                raise TypeError(f"Region: mask must be a bool tensor or numpy array of shape (n_lat, n_lon), got {m.dtype} of "
                                f"shape {tuple(m.shape)}")

    def rows(self, lat: np.ndarray) -> np.ndarray:
        """(n_lat,) bool: the rows of the region."""
        if self.lat is None:
            return np.ones(lat.shape, dtype=bool)
        out = np.zeros(lat.shape, dtype=bool)
        for lo, hi in self.lat:
            out |= (lat >= lo) & (lat <= hi)
        return out

    def cols(self, lon: np.ndarray) -> np.ndarray:
        """(n_lon,) bool: the columns of the region."""
        if self.lon is None:
            return np.ones(lon.shape, dtype=bool)
        x = _mod360(lon)
        out = np.zeros(lon.shape, dtype=bool)
        for west, east in self.lon:
            west, east = float(_mod360(np.float64(west))), float(_mod360(np.float64(east)))
            out |= ((x >= west) & (x <= east)) if west <= east else ((x >= west) | (x <= east))
        return out


def _mod360(x):
    r = np.mod(x, 360.0)
    return np.where(r >= 360.0, 0.0, r)          # (a tiny negative value rounds up to 360.0)


SCORECARD: dict[str, Region] = {
    "global": Region(),
    "tropics": Region(lat=(-20, 20)),
    "extratropics": Region(lat=[(-90, -20), (20, 90)]),
    "n.hem": Region(lat=(20, 90)),
    "s.hem": Region(lat=(-90, -20)),
    "arctic": Region(lat=(60, 90)),
    "antarctic": Region(lat=(-90, -60)),
    "europe": Region(lat=(35, 75), lon=(-12.5, 42.5)),
    "n.america": Region(lat=(25, 60), lon=(-120, -75)),
    "n.atlantic": Region(lat=(25, 65), lon=(-70, -10)),
    "n.pacific": Region(lat=(25, 60), lon=(145, -130)),
    "e.asia": Region(lat=(25, 60), lon=(102.5, 150)),
    "ausnz": Region(lat=(-45, -12.5), lon=(120, 175)),
}

_ON_CAPTURE = ("region_scores: call once with these regions on this grid before capturing a graph (the region tables are "
               "uploaded on the first call, which a captured graph cannot replay)")


class Regions:
    """1 to 32 named `Region`s and the tables a call needs of them, memoised (see the module's text).  `tables`: the cache
    of small device tables to use, the package's shared one by default."""

    def __init__(self, regions: Mapping[str, Region], tables: Optional[_fields.DeviceTables] = None):
        if isinstance(regions, Regions):
            regions = dict(zip(regions.names, regions.values))
        if not isinstance(regions, Mapping):
            raise TypeError(f"region_scores: regions must be a Regions object or a dict name -> Region, got {type(regions).__name__}")
        if not 1 <= len(regions) <= MAX_REGIONS:
            raise ValueError(f"region_scores: 1 to {MAX_REGIONS} regions per call, got {len(regions)}")
        for name, r in regions.items():
            if not isinstance(name, str):
                raise TypeError(f"region_scores: the names of the regions must be strings, got {name!r}")
            if not isinstance(r, Region):
                raise TypeError(f"region_scores: region {name!r} must be a Region, got {type(r).__name__}")
        self.names: tuple[str, ...] = tuple(regions)
        self.values: tuple[Region, ...] = tuple(regions.values())
        self._tables = _fields.tables if tables is None else tables
        self._members: dict[tuple, tuple[np.ndarray, np.ndarray]] = {}   # grid -> (R, n_lat) and (R, n_lon) bool
        self._mask_planes: dict[tuple, tuple] = {}                        # (grid, device) -> a plane or None per launch
        self._lock = threading.Lock()

    def __len__(self) -> int:
        return len(self.names)

    def launches(self) -> list[range]:
        """The regions of every launch: at most 8 each, in order."""
        return [range(a, min(a + PER_LAUNCH, len(self))) for a in range(0, len(self), PER_LAUNCH)]

    # ---- on the host ---------------------------------------------------------------------------------------------------
    def members(self, lat: np.ndarray, lon: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """The row and the column membership of every region on a grid, (R, n_lat) and (R, n_lon) bool; a selection that
        holds no row or column of the grid raises."""
        key = (lat.tobytes(), lon.tobytes())
        with self._lock:
            hit = self._members.get(key)
        if hit is not None:
            return hit
        rows, cols = np.stack([r.rows(lat) for r in self.values]), np.stack([r.cols(lon) for r in self.values])
        for name, r, in_rows, in_cols in zip(self.names, self.values, rows, cols):
            if not in_rows.any():
                raise ValueError(f"region_scores: the latitudes {r.lat} of region {name!r} hold no row of the grid")
            if not in_cols.any():
                raise ValueError(f"region_scores: the longitudes {r.lon} of region {name!r} hold no column of the grid")
        with self._lock:
            self._members[key] = (rows, cols)
        return rows, cols

    def check_masks(self, n_lat: int, n_lon: int, device) -> None:
        """Every mask fits the grid, and one that lives on a GPU lives on the device of the fields."""
        for name, r in zip(self.names, self.values):
            if r.mask is None:
                continue
            if tuple(r.mask.shape) != (n_lat, n_lon):
                raise ValueError(f"region_scores: the mask of region {name!r} has shape {tuple(r.mask.shape)}, which does not "
                                 f"fit a {n_lat} x {n_lon} grid")
            where = r.mask.device if isinstance(r.mask, torch.Tensor) else torch.device("cpu")
            if where.type != "cpu" and where != device:
                raise ValueError(f"region_scores: the mask of region {name!r} is on {where} but the fields are on {device}; move "
                                 "the mask to the device of the fields or to the CPU first")

    def host_masks(self) -> list[Optional[np.ndarray]]:
        return [None if r.mask is None else torch.as_tensor(r.mask).numpy() for r in self.values]

    # ---- on the device -------------------------------------------------------------------------------------------------
    def device_tables(self, lat: np.ndarray, lon: np.ndarray, device: torch.device) -> list[tuple]:
        """(row bits, column bits, mask-bit plane or None, number of regions) per launch, on `device`."""
        rows, cols = self.members(lat, lon)
        planes = self._mask_bits(lat, lon, device)
        out = []
        for idx, plane in zip(self.launches(), planes):
            bit = (1 << np.arange(len(idx), dtype=np.uint8))[:, None]
            tabs = []
            for what, member in (("region row bits", rows), ("region column bits", cols)):
                bits = np.bitwise_or.reduce(np.where(member[idx.start:idx.stop], bit, np.uint8(0)), axis=0).astype(np.uint8)
                tabs.append(self._tables.get((what, bits.tobytes()), device, bits.copy, _ON_CAPTURE))
            out.append((tabs[0], tabs[1], plane, len(idx)))
        return out

    def _mask_bits(self, lat: np.ndarray, lon: np.ndarray, device: torch.device) -> tuple:
        key = (lat.tobytes(), lon.tobytes(), str(device))
        with self._lock:
            hit = self._mask_planes.get(key)
        if hit is not None:
            return hit
        if all(r.mask is None for r in self.values):
            planes = tuple(None for _ in self.launches())
        elif torch.cuda.is_current_stream_capturing():
            raise RuntimeError(_ON_CAPTURE)
        else:
            planes = tuple(self._mask_plane(idx, lat.shape[0], lon.shape[0], device) for idx in self.launches())
        with self._lock:
            self._mask_planes[key] = planes
        return planes

    def _mask_plane(self, idx: range, n_lat: int, n_lon: int, device: torch.device) -> Optional[torch.Tensor]:
        """(n_lat, n_lon) uint8: bit b set where region idx[b] has no mask or its mask is True; None where none has a mask."""
        masks = [self.values[i].mask for i in idx]
        if all(m is None for m in masks):
            return None
        free = sum(1 << b for b, m in enumerate(masks) if m is None)
        plane = torch.full((n_lat, n_lon), free, dtype=torch.uint8, device=device)
        for b, m in enumerate(masks):
            if m is None:
                continue
            if not (isinstance(m, torch.Tensor) and m.is_cuda):
                m = _fields._upload(torch.as_tensor(m).numpy(), device)          # pinned, no synchronisation
            plane.bitwise_or_(m.to(torch.uint8) * (1 << b))
        return plane


@dataclasses.dataclass(frozen=True)
class RegionScores:
    """Result of `region_scores`: every property is a dict name -> tensor of shape (B, R) for a surface variable and (B, C, R)
    for an atmospheric one, float64 (count: int64), on the device of the prediction; R follows `regions`.  `acc` is None
    without a climatology; `sums` holds the eight raw sums in a last dimension.  `s[name]` is the `Scores` of one region."""

    table: torch.Tensor                                  # (n_planes, R, 12): the eight sums, rmse, bias, mae, acc
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    has_climatology: bool
    regions: tuple[str, ...]

    def _column(self, col) -> dict[str, torch.Tensor]:
        return _fields.by_variable(self.layout, self.table[:, :, col])

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
        return self._column(slice(0, 8))

    def __getitem__(self, region: str) -> Scores:
        if region not in self.regions:
            raise KeyError(f"region_scores: no region {region!r}; the regions are {self.regions}")
        return Scores(self.table[:, self.regions.index(region)], self.layout, self.has_climatology)

    def cpu(self) -> "RegionScores":
        """The same scores with host tensors (one copy; waits for the device)."""
        return dataclasses.replace(self, table=self.table.cpu())


# ---- the sums on the host --------------------------------------------------------------------------------------------------
def _sums_host(pred: np.ndarray, truth: np.ndarray, clim: Optional[np.ndarray], w: np.ndarray, rows: np.ndarray,
               cols: np.ndarray, masks: list) -> np.ndarray:
    """The table of include/aurora_hip.h for (n_planes, n_lat, n_lon) arrays and the memberships of R regions, in numpy fp64:
    (n_planes, R, 8).  Boolean indexing per region."""
    R = rows.shape[0]
    out = np.zeros((pred.shape[0], R, 8))
    W = np.broadcast_to(np.asarray(w, dtype=np.float64)[:, None], pred.shape[1:])
    inside = []
    for r in range(R):
        m = rows[r][:, None] & cols[r][None, :]
        inside.append(m if masks[r] is None else m & masks[r])
    for k in range(pred.shape[0]):
        p, t = pred[k].astype(np.float64), truth[k].astype(np.float64)
        ok = np.isfinite(p) & np.isfinite(t)
        c = None
        if clim is not None:
            c = clim[k].astype(np.float64)
            ok &= np.isfinite(c)
        for r in range(R):
            m = ok & inside[r]
            wk, d = W[m], p[m] - t[m]
            out[k, r, :5] = m.sum(), wk.sum(), (wk * d).sum(), (wk * d * d).sum(), (wk * np.abs(d)).sum()
            if c is not None:
                pa, ta = p[m] - c[m], t[m] - c[m]
                out[k, r, 5:] = (wk * pa * ta).sum(), (wk * pa * pa).sum(), (wk * ta * ta).sum()
    return out


# ---- public function -------------------------------------------------------------------------------------------------------
def region_scores(pred: Batch, truth: Batch, regions: Union[Regions, Mapping[str, Region]],
                  climatology: Optional[Batch] = None) -> RegionScores:
    """Latitude-weighted RMSE, bias, MAE (and ACC with a `climatology`) per region of the last history entry of every
    surface and atmospheric variable that both `pred` and `truth` hold; see the module's text."""
    regs = regions if isinstance(regions, Regions) else Regions(regions)
    others = [("truth", truth)] + ([("climatology", climatology)] if climatology is not None else [])
    for what, b in others:
        _fields.check_same_grid("region_scores", pred, b, "pred", what, "the prediction")
    n_lat, n_lon = pred.metadata.lat.shape[0], pred.metadata.lon.shape[0]
    names, fields, layout = _fields.select_pair("region_scores", pred, others)
    if not names:
        raise ValueError("region_scores: pred and truth have no surface or atmospheric variable in common")

    device = _fields.place("region_scores", [(what, names, fs) for what, fs in zip(("pred", "truth", "climatology"), fields)],
                           n_lat, n_lon)
    lat, lon = _fields._host(pred.metadata.lat), _fields._host(pred.metadata.lon)
    regs.check_masks(n_lat, n_lon, device)
    if device == "cpu":
        p, t, *c = (_fields.stack(fs, n_lat, n_lon) for fs in fields)
        rows, cols = regs.members(lat, lon)
        sums = torch.from_numpy(_sums_host(p, t, c[0] if c else None, latitude_weights(lat), rows, cols, regs.host_masks()))
    else:
        from aurora_amd.engine import lib

        w = _fields.device_weights("region_scores", lat, device)
        clim = fields[2] if climatology is not None else None
        parts = [lib.region_sums(fields[0], fields[1], clim, row_bits, col_bits, mask_bits, n, w)
                 for row_bits, col_bits, mask_bits, n in regs.device_tables(lat, lon, device)]
        sums = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)   # (the grouping does not show: see the text)
    R = len(regs)
    table = _finalise(sums.reshape(-1, 8), climatology is not None).reshape(-1, R, 12)
    return RegionScores(table, layout, climatology is not None, regs.names)
