"""First-order conservative (area-weighted) regridding where the predictions live (not in the reference, whose only route
between grids is the bilinear `Batch.regrid`): the step that brings a fine forecast to the coarser grid of its truth without
aliasing its small scales and without changing its area mean.

    coarse = aurora_amd.conservative_regrid(pred_hres, 0.25)            # the grid of Batch.regrid(0.25)
    coarse = aurora_amd.conservative_regrid(pred, lat=lat, lon=lon)     # any lat / lon vectors
    aurora_amd.scores(coarse, truth)

Every surface, static and atmospheric variable is regridded, with all history entries and all batch elements, into float32
fields; the metadata is the input's with the new coordinates, on the input's device.  `Batch.regrid` stays bilinear.

THE RULE (the numpy path below and csrc/conservative_regrid.hip implement it operation for operation).

Latitude cells.  Latitudes are strictly monotonic, ascending or descending (source and target may differ), |lat| <= 90, at
least two.  Interior cell edges are the midpoints 0.5 (lat[k] + lat[k+1]); the outer edges are lat[0] - 0.5 (lat[1] - lat[0])
and lat[-1] + 0.5 (lat[-1] - lat[-2]), clipped to [-90, 90] (a row at a pole is a half cell).  The measure of an edge is
sin(edge in radians), with +-90 mapped to exactly +-1; a cell is [lo, hi] with lo < hi in that measure.

Longitude cells.  Longitudes are strictly increasing in [0, 360), at least two.  A grid is a full circle where
`_sphere.full_circle` says so: then the west edge of the first cell is 0.5 ((lon[-1] - 360) + lon[0]) and the east edge
of the last cell is that plus 360.  Otherwise it is regional, with outer edges half the adjacent spacing beyond the end
columns.  Interior edges are midpoints; the measure is degrees.

Overlaps.  The overlap of a target cell [tl, th] and a source cell [sl, sh] is min(th, sh) - max(tl, sl); the cells that
overlap a target cell are those with sh > tl and sl < th, and only they are taps.  The source longitude cells of a
full-circle source are taken at -360, 0 and +360, so a target cell may straddle the seam: with e its n + 1 edges, the 3 n cells
lie between the consecutive values of (e[0 .. n-1] - 360, e[0 .. n-1], e[0 .. n] + 360), neighbours sharing their edge across
the seam too, so that the overlaps of a covered target cell add up to its measure.  The row taps of a target row are
consecutive source rows in ascending row index; the column taps are consecutive modulo n_lon, eastward from the westernmost
overlapping source cell.  More than 64 taps of a target cell on either axis is a ValueError; a cell with no tap gives NaN.
A_i and B_j are the measures th - tl of the target row and column cells (not the tap sums).

Arithmetic: fp64, each operation rounded on its own (no fused multiply-add).  For target row i and every source column c,
over the row taps (a, r) in order, from cn[c] = cd[c] = 0:  if x[r, c] is finite, cn[c] += a * x[r, c] and cd[c] += a.  For
target column j, over the column taps (b, c) in order, from n = d = 0:  n += b * cn[c];  d += b * cd[c].  The value is
(float)(n / d) where d > 0 and d >= min_valid * (A_i * B_j), and NaN otherwise.

So a NaN or an infinity of the source drops out and the rest is renormalised (the land points of a wave field), a target cell
that hangs out of a regional source counts the uncovered part as invalid, and `min_valid` in (0, 1] is the covered, valid
fraction of its measure a target cell needs.  Sources in fp32 and fp64 are read as they are, bf16 / fp16 are widened to fp32
first (lossless), other dtypes go through fp64.

Tables (made here and nowhere else, `plan`; include/aurora_hip.h has the format): per target row and column a first source
index, the offset of its first weight, a count and the fp64 weights, plus A and B.  A CPU batch takes the numpy path.  A batch
whose fields and coordinates live on one GPU takes ONE aurora_hip_conservative_regrid launch per source dtype and stays there:
no workspace, nothing read back; the device copies of the tables and of the new coordinates are kept in `_fields.tables` by the
content of the four coordinate vectors, so a second call uploads nothing, and after one eager call the call can be captured in
a hipGraph (fp32 / fp64 fields with contiguous planes: a widened copy would be a new tensor in every call).

Not offered: latitude bands (`BandBatch`), matrix coordinates, second-order remapping, masks other than NaN / Inf.
"""

from __future__ import annotations

import threading
from collections import OrderedDict
from typing import NamedTuple, Optional

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._sphere import check_latitudes, full_circle
from aurora_amd._fields import _host
from aurora_amd.batch import Batch, derive_metadata

__all__ = ["conservative_regrid", "MAX_TAPS"]

FN = "conservative_regrid"
MAX_TAPS = 64


class Axis(NamedTuple):
    """The taps of every target cell of one axis: source index of the first tap (longitudes of a full-circle source:
    unwrapped, the column is the index mod n), offset of its first weight in `w`, count, the weights, the cell measures."""
    first: np.ndarray     # (n_out, 2) int32: first source index, offset into w
    count: np.ndarray     # (n_out,) int32
    w: np.ndarray         # (sum of counts, at least 1) float64
    measure: np.ndarray   # (n_out,) float64


class Plan(NamedTuple):
    lat: np.ndarray       # the target coordinates, float64
    lon: np.ndarray
    n_lat: int            # the source grid
    n_lon: int
    rows: Axis
    cols: Axis


# ---- cells ---------------------------------------------------------------------------------------------------------------
def _check_lat(lat: np.ndarray, what: str) -> None:
    if lat.ndim != 1 or lat.shape[0] < 2:
        raise ValueError(f"{FN}: the latitudes of {what} must be a vector of at least 2 values")
    check_latitudes(FN, lat, of=f" of {what}")


def _check_lon(lon: np.ndarray, what: str) -> None:
    if lon.ndim != 1 or lon.shape[0] < 2:
        raise ValueError(f"{FN}: the longitudes of {what} must be a vector of at least 2 values")
    if not np.all(np.isfinite(lon)) or lon.min() < 0 or lon.max() >= 360:
        raise ValueError(f"{FN}: the longitudes of {what} must be in the range [0, 360)")
    if not np.all(np.diff(lon) > 0):
        raise ValueError(f"{FN}: the longitudes of {what} must be strictly increasing")


def lat_cells(lat: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(lo, hi) of every row's cell in sin(lat), in the order of `lat`."""
    e = np.empty(lat.shape[0] + 1)
    e[1:-1] = 0.5 * (lat[:-1] + lat[1:])
    e[0] = lat[0] - 0.5 * (lat[1] - lat[0])
    e[-1] = lat[-1] + 0.5 * (lat[-1] - lat[-2])
    e = np.clip(e, -90.0, 90.0)
    m = np.sin(np.deg2rad(e))
    m[e == 90.0], m[e == -90.0] = 1.0, -1.0
    return np.minimum(m[:-1], m[1:]), np.maximum(m[:-1], m[1:])


def lon_cells(lon: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(west, east) of every column's cell in degrees."""
    e = np.empty(lon.shape[0] + 1)
    e[1:-1] = 0.5 * (lon[:-1] + lon[1:])
    if full_circle(lon):
        e[0] = 0.5 * ((lon[-1] - 360.0) + lon[0])
        e[-1] = e[0] + 360.0
    else:
        e[0] = lon[0] - 0.5 * (lon[1] - lon[0])
        e[-1] = lon[-1] + 0.5 * (lon[-1] - lon[-2])
    return e[:-1].copy(), e[1:].copy()


def _taps(tl: np.ndarray, th: np.ndarray, sl: np.ndarray, sh: np.ndarray, what: str):
    """Source cells [sl, sh] in ascending position; per target cell the index of the first overlapping one, the count, and
    all the overlaps one target cell after the other."""
    k_lo = np.searchsorted(sh, tl, side="right")            # the first cell with sh > tl
    k_hi = np.searchsorted(sl, th, side="left")             # one past the last cell with sl < th
    count = np.maximum(k_hi - k_lo, 0)
    if count.max(initial=0) > MAX_TAPS:
        raise ValueError(f"{FN}: a target cell overlaps {int(count.max())} source {what}; at most {MAX_TAPS} are supported")
    offset = np.concatenate([[0], np.cumsum(count)[:-1]])
    cell = np.repeat(np.arange(tl.shape[0]), count)
    k = np.repeat(k_lo - offset, count) + np.arange(cell.shape[0])
    w = np.minimum(th[cell], sh[k]) - np.maximum(tl[cell], sl[k])
    return k_lo, count, offset, w


def _axis(first, count, offset, w, measure) -> Axis:
    # A cell without taps takes the index where its neighbours' taps end, so that along the cells neither the first index
    # nor the end (first + count) ever decreases: the kernel takes a tile's span of source columns from its end cells.
    first = first.astype(np.int64)
    if np.any(count > 0):
        end = np.maximum.accumulate(np.where(count > 0, first + count, 0))
        first = np.where(count > 0, first, np.maximum(end, first[count > 0][0]))
    else:
        first = np.zeros_like(first)
    table = np.stack([first, offset], axis=1).astype(np.int32)
    return Axis(table, count.astype(np.int32), np.ascontiguousarray(w if w.shape[0] else np.zeros(1)), measure)


def row_axis(src: np.ndarray, dst: np.ndarray) -> Axis:
    sl, sh = lat_cells(src)
    tl, th = lat_cells(dst)
    n = src.shape[0]
    if src[0] > src[-1]:                                     # descending rows: position k is row n - 1 - k
        sl, sh = sl[::-1], sh[::-1]
    k_lo, count, offset, w = _taps(tl, th, sl, sh, "rows")
    first = k_lo
    if src[0] > src[-1]:                                     # ascending row index: the taps of a cell are reversed
        first = n - k_lo - count
        at = np.repeat(offset + count - 1, count) - (np.arange(w.shape[0]) - np.repeat(offset, count))
        w = w[at]
    return _axis(first, count, offset, w, th - tl)


def col_axis(src: np.ndarray, dst: np.ndarray) -> Axis:
    sl, sh = lon_cells(src)
    tl, th = lon_cells(dst)
    if full_circle(src):                                     # images at -360, 0, +360: index n + k is column k
        e = np.concatenate([sl, sh[-1:]])
        u = np.concatenate([e[:-1] - 360.0, e[:-1], e + 360.0])
        sl, sh = u[:-1], u[1:]
    k_lo, count, offset, w = _taps(tl, th, sl, sh, "columns")
    return _axis(k_lo, count, offset, w, th - tl)


_plans: "OrderedDict[tuple, Plan]" = OrderedDict()
_plans_lock = threading.Lock()


def plan(src_lat, src_lon, lat, lon) -> Plan:
    """The tables from a checked source grid to the target (float64 vectors), remembered by content."""
    src_lat, src_lon, lat, lon = (np.ascontiguousarray(a, dtype=np.float64) for a in (src_lat, src_lon, lat, lon))
    key = tuple(a.tobytes() for a in (src_lat, src_lon, lat, lon))
    with _plans_lock:
        hit = _plans.get(key)
        if hit is not None:
            _plans.move_to_end(key)
            return hit
    _check_lat(src_lat, "the batch"), _check_lon(src_lon, "the batch")
    _check_lat(lat, "the target"), _check_lon(lon, "the target")
    lat, lon = lat.copy(), lon.copy()                        # (kept, and never the caller's arrays)
    made = Plan(lat, lon, src_lat.shape[0], src_lon.shape[0], row_axis(src_lat, lat), col_axis(src_lon, lon))
    for a in (lat, lon, *made.rows, *made.cols):
        a.setflags(write=False)
    with _plans_lock:
        _plans[key] = made
        while len(_plans) > 16:
            _plans.popitem(last=False)
    return made


# ---- the rule on the host ------------------------------------------------------------------------------------------------
def regrid_planes(x: np.ndarray, p: Plan, min_valid: float) -> np.ndarray:
    """x: (n_planes, n_lat, n_lon) float32 or float64 -> (n_planes, target rows, target columns) float32."""
    rows, cols = p.rows, p.cols
    n_lon = x.shape[-1]
    out = np.empty((x.shape[0], rows.count.shape[0], cols.count.shape[0]), dtype=np.float32)
    c_first, c_off, c_count = cols.first[:, 0].astype(np.int64), cols.first[:, 1].astype(np.int64), cols.count
    nan = np.float64("nan")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(out.shape[1]):
            cn = np.zeros((x.shape[0], n_lon))
            cd = np.zeros((x.shape[0], n_lon))
            for t in range(rows.count[i]):
                a = rows.w[rows.first[i, 1] + t]
                xr = x[:, rows.first[i, 0] + t, :].astype(np.float64)
                fin = np.isfinite(xr)
                cn = np.where(fin, cn + a * np.where(fin, xr, 0.0), cn)
                cd = np.where(fin, cd + a, cd)
            n = np.zeros((x.shape[0], out.shape[2]))
            d = np.zeros((x.shape[0], out.shape[2]))
            for t in range(int(c_count.max(initial=0))):
                live = t < c_count
                c = (c_first + t) % n_lon
                b = cols.w[np.where(live, c_off + t, 0)]
                n = np.where(live, n + b * cn[:, c], n)
                d = np.where(live, d + b * cd[:, c], d)
            ok = (d > 0.0) & (d >= min_valid * (rows.measure[i] * cols.measure))
            out[:, i, :] = np.where(ok, n / np.where(ok, d, 1.0), nan).astype(np.float32)
    return out


# ---- the tables on the device ----------------------------------------------------------------------------------------------
_ON_CAPTURE = (f"{FN}: call once on this pair of grids before capturing a graph (the overlap tables and the new coordinates "
               "are uploaded on the first call, which a captured graph cannot replay)")


def _packed(p: Plan) -> np.ndarray:
    """The eight tables in one byte array, each at a multiple of 16 bytes."""
    tables = (*p.rows, *p.cols)
    blob = np.zeros(sum(-(-a.nbytes // 16) * 16 for a in tables), dtype=np.uint8)
    at = 0
    for a in tables:
        blob[at:at + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        at += -(-a.nbytes // 16) * 16
    return blob


_TORCH = {np.dtype(np.int32): torch.int32, np.dtype(np.float64): torch.float64}


def device_tables(p: Plan, key: tuple, device: torch.device) -> list[torch.Tensor]:
    """Device copies of the eight tables of `p` (row first, count, weights, measures; the same of the columns): views of ONE
    uploaded array, kept in `_fields.tables`."""
    blob = _fields.tables.get(("conservative tables", *key), device, lambda: _packed(p), _ON_CAPTURE)
    at, views = 0, []
    for a in (*p.rows, *p.cols):
        views.append(blob[at:at + a.nbytes].view(_TORCH[a.dtype]).view(a.shape))
        at += -(-a.nbytes // 16) * 16
    return views


def _coordinate(given, values: np.ndarray, device) -> torch.Tensor:
    """The new coordinate on `device`: the caller's tensor where it is there already, else a copy (on a GPU a kept one)."""
    if isinstance(given, torch.Tensor) and given.dtype == torch.float64 and given.device == torch.device(device):
        return given
    if device == "cpu":
        return torch.from_numpy(values.copy())
    return _fields.tables.get(("coordinate", values.tobytes()), device, values.copy, _ON_CAPTURE)


# ---- public function -------------------------------------------------------------------------------------------------------
def _vector(value, name: str) -> np.ndarray:
    if isinstance(value, torch.Tensor):
        if value.dim() != 1:
            raise ValueError(f"{FN}: {name} must be a vector, got shape {tuple(value.shape)}")
        return _host(value)
    a = np.asarray(value, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{FN}: {name} must be a vector, got shape {a.shape}")
    return a


def _source_dtype(dt: torch.dtype) -> torch.dtype:
    if dt in (torch.float32, torch.float64):
        return dt
    return torch.float32 if dt in (torch.bfloat16, torch.float16) else torch.float64


def conservative_regrid(batch: Batch, res: Optional[float] = None, *, lat=None, lon=None, min_valid: float = 0.5) -> Batch:
    """`batch` on the `res`-degree grid of `Batch.regrid`, or on the grid of the vectors `lat` / `lon` (float64 on the host, or
    tensors), by first-order conservative remapping: a float32 `Batch` on the device of the input; see the module's text."""
    if not isinstance(batch, Batch):
        raise TypeError(f"{FN}: batch must be a Batch, got {type(batch).__name__}")
    _fields.check_vector_grid(FN, batch, "batch", band="regrids")
    if res is not None and (lat is not None or lon is not None):
        raise ValueError(f"{FN}: give either res or lat / lon, not both")
    if res is None and (lat is None or lon is None):
        raise ValueError(f"{FN}: give the target grid: res, or both lat and lon")
    try:
        min_valid = float(min_valid)
    except (TypeError, ValueError):
        raise ValueError(f"{FN}: min_valid must be a number in (0, 1], got {min_valid!r}") from None
    if not 0.0 < min_valid <= 1.0:
        raise ValueError(f"{FN}: min_valid must be in (0, 1], got {min_valid!r}")
    if res is not None:
        if not (isinstance(res, (int, float)) and 0.0 < res <= 90.0):
            raise ValueError(f"{FN}: res must be a spacing in degrees in (0, 90], got {res!r}")
        lat_new = np.linspace(90, -90, round(180 / res) + 1)
        lon_new = np.linspace(0, 360, round(360 / res), endpoint=False)
    else:
        lat_new, lon_new = _vector(lat, "lat"), _vector(lon, "lon")
    md = batch.metadata
    src_lat, src_lon = _host(md.lat), _host(md.lon)
    p = plan(src_lat, src_lon, lat_new, lon_new)
    n_lat, n_lon = p.n_lat, p.n_lon
    n_rows, n_cols = p.lat.shape[0], p.lon.shape[0]

    groups = (("surf_vars", batch.surf_vars), ("static_vars", batch.static_vars), ("atmos_vars", batch.atmos_vars))
    for group, fields in groups:
        for k, f in fields.items():
            if group == "static_vars":
                if f.dim() != 2 or tuple(f.shape) != (n_lat, n_lon):
                    raise ValueError(f"{FN}: batch.static_vars[{k!r}] has shape {tuple(f.shape)}, which does not fit a "
                                     f"{n_lat} x {n_lon} grid")
            else:
                _fields.check_field(FN, f, "batch", group, k, n_lat, n_lon)
    every = [f for _, fields in groups for f in fields.values()]
    dev = _fields.device_of(FN, [*every, md.lat, md.lon], "the fields and coordinates", "whole batch")

    if dev == "cpu":
        def f(v: torch.Tensor) -> torch.Tensor:
            x = v.detach().to(_source_dtype(v.dtype)).reshape(-1, n_lat, n_lon).numpy()
            return torch.from_numpy(regrid_planes(x, p, min_valid)).reshape(*v.shape[:-2], n_rows, n_cols)

        out = [{k: f(v) for k, v in fields.items()} for _, fields in groups]
        new_lat, new_lon = _coordinate(lat, p.lat, "cpu"), _coordinate(lon, p.lon, "cpu")
    else:
        from aurora_amd.engine import lib

        key = tuple(a.tobytes() for a in (src_lat, src_lon, p.lat, p.lon))
        with torch.cuda.device(dev):
            tables = device_tables(p, key, dev)
            new_lat, new_lon = _coordinate(lat, p.lat, dev), _coordinate(lon, p.lon, dev)
            # one output array per source dtype: its planes follow each other, and the fields are views of it
            work: dict[torch.dtype, list] = {}
            for _, fields in groups:
                for v in fields.values():
                    w = v.detach().to(_source_dtype(v.dtype))
                    work.setdefault(w.dtype, []).append(w.contiguous())
            flat = {}
            for dt, src in work.items():
                flat[dt] = [torch.empty(sum(s.numel() for s in src) // (n_lat * n_lon), n_rows, n_cols, dtype=torch.float32,
                                        device=dev), 0]
                lib.conservative_regrid(src, flat[dt][0], tables, min_valid)

            def f(v: torch.Tensor) -> torch.Tensor:
                pair = flat[_source_dtype(v.dtype)]
                n = v.numel() // (n_lat * n_lon)
                planes = pair[0][pair[1]:pair[1] + n]
                pair[1] += n
                return planes.view(*v.shape[:-2], n_rows, n_cols)

            out = [{k: f(v) for k, v in fields.items()} for _, fields in groups]
    return Batch(out[0], out[1], out[2], derive_metadata(md, lat=new_lat, lon=new_lon))
