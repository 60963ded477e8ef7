"""Where are the lows and the highs of a field, how deep are they and how many are there (not in the reference): a point is a
candidate where it is the minimum (or maximum) of the field over all points within R kilometres -- the DetectNodes step of
cyclone detection, storm counts, jet-streak and heat-dome centres -- on the device, for every plane of a batch at once, where
`Tracker` follows one known low on the host in a box counted in grid points.

    e = aurora_amd.extrema(batch, 500.0, kind="min", only=["msl"], max_points=4096)
    e.index["msl"]        # (B, H, W) int32 on the batch's device: the flat index k W + c of the disc's extreme point, -1 for none
    e.filtered["msl"]     # (B, H, W) float32: the value there, bit for bit -- the minimum (maximum) filter over the disc; NaN for none
    e.is_extremum["msl"]  # (B, H, W) bool: the point is valid and index is its own flat index
    e.count["msl"]        # (B,) int32: the number of extrema -- the true number, also beyond max_points
    e.table["msl"]        # (B, max_points, 2) int64: index, key of the extrema in ascending flat index; zero past min(count, max_points)
    e.truncated["msl"]    # count > max_points
    e.value, e.lat, e.lon, e.row, e.col    # (B, max_points): NaN (float) or -1 (integer) past the rows of the table
    e.as_batch()          # `filtered` as a float32 Batch in the layout `smooth` returns: `objects`, the scorers, `to_netcdf` take it
    e.cpu()               # the same object with host tensors: the one call that waits for the device

An atmospheric variable has (B, C, ...) in place of (B, ...).  The last history entry of every surface and atmospheric variable
is used, or of those named in `only`.  Fields of another precision (CPU batches only) are rounded to float32 first.

THE RULE (both paths follow it; include/aurora_hip.h has it for the device).

    MEMBERSHIP  the table of `aurora_amd.smooth.disc_table(lat, dlambda, n_lon, wrap, radius_km)` and nothing else: source row k
                = row_lo[i] + r, r < row_count[i], belongs to target row i, and in it the columns j - n .. j + n, n = half[i, r]
                (none where n = -1).  On a full circle the columns are taken mod W, and the window is the whole row once
                2 n + 1 >= W; on a regional grid they are clipped into the row.  One addition: the target point is always a
                member of its own disc -- in its own row n counts as max(n, 0).
    VALIDITY    a point is valid where it is finite.  NaN and +-Inf are never members and never extrema.
    ORDER       K(v) is the integer key of `objects` (`aurora_amd.objects.value_keys`: ascending with v, -0 below +0); for
                kind="max" the key is ~K(v), so that both kinds take a minimum.  The COMPOSITE of a valid point is the uint64
                (key << 32) | flat index.  The disc's extreme point is the minimum composite over its valid members: the
                extreme value and, among equal values, the smallest flat index.
    EXTREMUM    a valid point is an extremum where the disc's minimum composite is its own.  (A constant plane therefore has
                exactly one extremum on a connected grid.)
    RESULT      index, filtered, table (index, K(v) -- K, not ~K, for either kind -- in ascending flat index) and count.
                Everything is an integer or a copied float32: the two paths agree in every byte, and nothing here has a tolerance.
    LIMITS      radius_km finite and > 0; at most 255 source rows per target row (`disc_table` refuses); 1 to 4096 longitudes;
                max_points 1 to 65536.

The grid is checked by THE GRID RULE of aurora_amd/_sphere.py, which also says when it wraps.

Fields on one GPU are filtered by ONE aurora_hip_extrema call (aurora_amd/csrc/extrema.hip, extrema_window.h): per source row
the composites are staged in LDS and doubled, m[l + 1][c] = min(m[l][c], m[l][c + 2^l]), and a window is answered from two
entries of the level floor(log2(2 n + 1)) -- an exact range-minimum query whose cost does not grow with the width of the
window.  Nothing is read back; the workspace holds 16 bytes per row, not per point.  The disc table on the device is the one
`smooth` uploads for the same grid and radius.  Fields on the CPU take the same rule in numpy, with the same doubling tables
per source row.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Optional, Sequence

import numpy as np
import torch

from aurora_amd import _fields, _sphere
from aurora_amd._fields import _host
from aurora_amd.batch import Batch
from aurora_amd.objects import Result, final_properties, value_keys
from aurora_amd.smooth import _packed, _table

__all__ = ["extrema", "Extrema", "COLUMNS", "MAX_POINTS"]

COLUMNS = ("index", "key")
MAX_POINTS = 65536
_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
_ON_CAPTURE = ("extrema: call once on this grid with this radius before capturing a graph (the disc table and the coordinates "
               "are uploaded on the first call, which a captured graph cannot replay)")


# ---- the rule on the host ---------------------------------------------------------------------------------------------------
def _log2(v):
    """floor(log2(v)) for whole numbers v >= 1 (exact: no floating point)."""
    v = np.asarray(v, dtype=np.int64)
    out = np.zeros(v.shape, dtype=np.int64)
    for s in (16, 8, 4, 2, 1):
        big = (v >> (out + s)) != 0
        out = np.where(big, out + s, out)
    return out


def _window(n: int, W: int, wrap: bool):
    """(level of every column, a, b) of the windows of half width n that are not the whole row: the minimum over the window
    is min(m[level][a], m[level][b]); aurora_amd/csrc/extrema_window.h in numpy."""
    j = np.arange(W)
    if wrap:
        level = np.full(W, int(_log2(2 * n + 1)))
        return level, (j - n) % W, (j + n + 1 - (1 << level)) % W
    lo, hi = np.clip(j - n, 0, W - 1), np.clip(j + n, 0, W - 1)
    level = _log2(hi - lo + 1)
    return level, lo, hi + 1 - (1 << level)


def _double(m: np.ndarray, l: int, wrap: bool) -> np.ndarray:
    """Level l + 1 from level l, (..., W): m[l + 1][c] = min(m[l][c], m[l][c + 2^l]), around the circle or up to the row's end."""
    step = 1 << l
    if wrap:
        return np.minimum(m, np.roll(m, -step, axis=-1))
    out = m.copy()
    if step < m.shape[-1]:
        np.minimum(m[..., :-step], m[..., step:], out=out[..., :-step])
    return out


def composites(x: np.ndarray, is_max: bool) -> np.ndarray:
    """The composites of THE RULE for float32 planes (..., H, W): uint64, all ones where a point is not finite."""
    H, W = x.shape[-2:]
    flat = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    comp = (value_keys(x, is_max).astype(np.uint64) << np.uint64(32)) | flat
    return np.where(np.isfinite(x), comp, _NONE)


def _extrema_host(x: np.ndarray, table, wrap: bool, is_max: bool, max_points: int):
    """x: (n, H, W) float32 -> index (n, H, W) int32, filtered (n, H, W) float32, table (n, max_points, 2) int64, count (n,) int32
    by THE RULE."""
    row_lo, row_count, half, _ = table
    n_planes, H, W = x.shape
    comp = composites(x, is_max)
    levels: dict[int, list[np.ndarray]] = {}                  # source row -> its doubling tables, each (n_planes, W)
    windows: dict = {}
    best = np.full((n_planes, H, W), _NONE, dtype=np.uint64)
    planes = np.arange(n_planes)[:, None]
    for i in range(H):
        reach = int(row_lo[i:].min())
        for k in [k for k in levels if k < reach]:             # (rows that no later target row reaches)
            del levels[k]
        for r in range(row_count[i]):                          # ascending source rows
            n, k = int(half[i, r]), int(row_lo[i]) + r
            if k == i:
                n = max(n, 0)                                  # a point is a member of its own disc
            if n < 0:
                continue
            if (2 * n + 1 >= W) if wrap else (n >= W - 1):     # the whole row
                np.minimum(best[:, i], comp[:, k].min(axis=-1, keepdims=True), out=best[:, i])
                continue
            if n not in windows:
                windows[n] = _window(n, W, wrap)
            level, a, b = windows[n]
            m = levels.setdefault(k, [comp[:, k]])
            while len(m) <= int(level.max()):
                m.append(_double(m[-1], len(m) - 1, wrap))
            if wrap:                                           # one level for every column
                t = m[int(level[0])]
                q = np.minimum(t[:, a], t[:, b])
            else:
                t = np.stack(m[:int(level.max()) + 1])         # (levels, n_planes, W)
                q = np.minimum(t[level, planes, a], t[level, planes, b])
            np.minimum(best[:, i], q, out=best[:, i])
    found = best != _NONE
    index = np.where(found, best & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    values = np.take_along_axis(x.reshape(n_planes, -1), index.reshape(n_planes, -1), axis=1).reshape(x.shape)
    filtered = np.where(found, values, np.float32("nan")).astype(np.float32)
    index = np.where(found, index, -1).astype(np.int32)
    own = index == np.arange(H * W, dtype=np.int64).reshape(H, W)
    out_table = np.zeros((n_planes, max_points, len(COLUMNS)), dtype=np.int64)
    count = np.zeros(n_planes, dtype=np.int32)
    for p in range(n_planes):
        at = np.flatnonzero(own[p])
        count[p] = at.shape[0]
        at = at[:max_points]
        out_table[p, :at.shape[0], 0] = at
        out_table[p, :at.shape[0], 1] = value_keys(x[p].reshape(-1)[at], False)
    return index, filtered, out_table, count


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
def _finalise(table: torch.Tensor, count: torch.Tensor, lat: torch.Tensor, lon: torch.Tensor) -> dict[str, torch.Tensor]:
    """The properties of every extremum from the integer table; elementwise, no read-back."""
    W, M = lon.shape[0], table.shape[-2]
    live = torch.arange(M, device=table.device) < count[..., None]
    real = lambda x: torch.where(live, x, torch.full_like(x, float("nan")))           # noqa: E731
    whole = lambda x: torch.where(live, x, torch.full_like(x, -1))                    # noqa: E731
    at, key = table[..., 0], table[..., 1]
    u = torch.where(key >= 0x80000000, key ^ 0x80000000, key ^ 0xffffffff)            # undo K of THE RULE
    value = torch.where(u >= 0x80000000, u - 2 ** 32, u).to(torch.int32).view(torch.float32)
    row, col = at // W, at % W
    return {"value": real(value), "row": whole(row), "col": whole(col), "lat": real(lat[row]), "lon": real(lon[col])}


@dataclasses.dataclass(eq=False)
class Extrema(Result):
    """Result of `extrema`: every property is a dict name -> tensor with the leading shape (B,) for a surface variable and
    (B, C) for an atmospheric one, on the device of the batch."""

    index_table: torch.Tensor                              # (n_planes, H, W) int32
    filtered_table: torch.Tensor                           # (n_planes, H, W) float32
    table_table: torch.Tensor                              # (n_planes, max_points, 2) int64
    count_table: torch.Tensor                              # (n_planes,) int32
    grid_lat: torch.Tensor                                 # (H,) fp64, on the device of the tables
    grid_lon: torch.Tensor                                 # (W,) fp64
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    kind: str
    radius_km: float
    wrap: bool
    max_points: int
    source: Batch = dataclasses.field(repr=False)          # the batch: its metadata, static variables and variable groups

    def _finalise(self) -> dict[str, torch.Tensor]:
        return _finalise(self.table_table, self.count_table, self.grid_lat, self.grid_lon)

    @property
    def index(self) -> dict[str, torch.Tensor]:
        return self._field(self.index_table)

    @property
    def filtered(self) -> dict[str, torch.Tensor]:
        return self._field(self.filtered_table)

    @property
    def is_extremum(self) -> dict[str, torch.Tensor]:
        H, W = self.index_table.shape[-2:]
        own = torch.arange(H * W, dtype=torch.int32, device=self.index_table.device).view(H, W)
        return self._field(self.index_table == own)

    @property
    def table(self) -> dict[str, torch.Tensor]:
        return self._field(self.table_table)

    @property
    def count(self) -> dict[str, torch.Tensor]:
        return self._field(self.count_table)

    @property
    def truncated(self) -> dict[str, torch.Tensor]:
        return self._field(self.count_table > self.max_points)

    def as_batch(self) -> Batch:
        """`filtered` as a float32 `Batch` in the layout `smooth` returns: (B, 1, H, W) and (B, 1, C, H, W), with the metadata
        and the static variables of the input."""
        by_name = self.filtered
        surf = {k: by_name[k][:, None] for k in self.source.surf_vars if k in by_name}
        atmos = {k: by_name[k][:, None] for k in self.source.atmos_vars if k in by_name}
        return Batch(surf, dict(self.source.static_vars), atmos, self.source.metadata)

    def cpu(self) -> "Extrema":
        """The same extrema with host tensors (waits for the device)."""
        moved = {f: getattr(self, f).cpu() for f in ("index_table", "filtered_table", "table_table", "count_table", "grid_lat",
                                                     "grid_lon")}
        return dataclasses.replace(self, **moved)


final_properties(Extrema, ("value", "lat", "lon", "row", "col"), "of every extremum; see the module's text.")


# ---- public function ------------------------------------------------------------------------------------------------------
def extrema(batch: Batch, radius_km: float, *, kind: str = "min", only: Optional[Sequence[str]] = None,
            max_points: int = 4096) -> Extrema:
    """The extreme point of the great-circle disc of `radius_km` around every point, and the local extrema, of the last history
    entry of every surface and atmospheric variable of `batch` (or of those named in `only`); see the module's text."""
    if not isinstance(batch, Batch):
        raise TypeError(f"extrema: batch must be a Batch, got {type(batch).__name__}")
    _fields.check_vector_grid("extrema", batch, "batch", band="fields")
    try:
        radius_km = float(radius_km)
    except (TypeError, ValueError):
        raise ValueError(f"extrema: radius_km must be a finite number above 0, got {radius_km!r}") from None
    if not (math.isfinite(radius_km) and radius_km > 0):
        raise ValueError(f"extrema: radius_km must be a finite number above 0, got {radius_km!r}")
    if kind not in ("min", "max"):
        raise ValueError(f"extrema: kind must be 'min' or 'max', got {kind!r}")
    if isinstance(max_points, bool) or not isinstance(max_points, (int, np.integer)) or not 1 <= max_points <= MAX_POINTS:
        raise ValueError(f"extrema: max_points must be a whole number in 1..{MAX_POINTS}, got {max_points!r}")
    if isinstance(only, str):
        only = (only,)
    md = batch.metadata
    lat, lon = _host(md.lat), _host(md.lon)
    n_lat, n_lon = lat.shape[0], lon.shape[0]
    if not 1 <= n_lon <= _sphere.MAX_LON:
        raise ValueError(f"extrema: the grid has {n_lon} longitudes; 1 to {_sphere.MAX_LON} are supported")
    step, wrap = _sphere.regular_grid("extrema", lat, lon, least=1, in_range=True)     # (a single row or column passes)
    dlambda = float(np.deg2rad(step))
    names, fields, layout = _fields.select_one("extrema", batch, "batch", only)
    if not names:
        raise ValueError("extrema: batch holds no surface or atmospheric variable")
    dev = _fields.device_of("extrema", fields, batches="batch")
    table = _table(lat.tobytes(), dlambda, n_lon, wrap, radius_km)     # (more than 255 rows: the refusal of `disc_table`)
    is_max, max_points = kind == "max", int(max_points)

    if dev == "cpu":
        with np.errstate(over="ignore", invalid="ignore"):
            x = np.ascontiguousarray(_fields.stack(fields, n_lat, n_lon), dtype=np.float32)
        index, filtered, rows, count = (torch.from_numpy(a) for a in _extrema_host(x, table, wrap, is_max, max_points))
        lat_t, lon_t = torch.from_numpy(np.array(lat)), torch.from_numpy(np.array(lon))
    else:
        from aurora_amd.engine import lib

        _fields.check_planes("extrema", [("batch", names, fields)], n_lat, n_lon, _fields.TAKES_TASK)
        key = (lat.tobytes(), dlambda, n_lon, wrap, radius_km)
        packed = _fields.tables.get(("smooth rows", *key), dev, lambda: _packed(table), _ON_CAPTURE)     # (the table of `smooth`)
        lat_t = _fields.tables.get(("coordinate", lat.tobytes()), dev, lambda: np.array(lat), _ON_CAPTURE)
        lon_t = _fields.tables.get(("coordinate", lon.tobytes()), dev, lambda: np.array(lon), _ON_CAPTURE)
        index, filtered, rows, count = lib.extrema_planes(fields, packed, wrap, is_max, max_points)
    return Extrema(index, filtered, rows, count, lat_t, lon_t, layout, kind, radius_km, wrap, max_points, batch)
