"""Fields smoothed over a great-circle disc where the predictions live (not in the reference): object-based verification
(MODE, atmospheric-river and storm catalogues) takes the mean of a field over all points within R kilometres before it
thresholds, or `objects` labels grid-scale noise.  `smooth` returns a `Batch`, so that every scorer, `objects`, `field_quantiles`
and `to_netcdf` take the result unchanged:

    ivt = aurora_amd.diagnostics(pred, "ivt")
    smoothed = aurora_amd.smooth(ivt, 150.0)
    found = aurora_amd.objects(smoothed, aurora_amd.field_quantiles(smoothed, [0.95]).thresholds())

The last history entry of the inputs is used, like in every scorer here.  The outputs are float32, (B, 1, H, W) for a surface
variable and (B, 1, C, H, W) for an atmospheric one; the returned batch carries the metadata of the input and its static
variables.  The disc has the same size in kilometres everywhere: towards the poles it spans more and more columns.

THE RULE (both paths follow it; include/aurora_hip.h has it for the device).

    MEMBERSHIP  rho = radius_km / 6371.229.  Source row k belongs to target row i where |phi_k - phi_i| <= rho, and in it the
                columns with gap |d| <= n(i, k), n(i, k) the largest d with  s_i s_k + c_i c_k cos(d dlambda) >= cos(rho)
                (s = sin(phi), c = cos(phi)), -1 where no d does.  On a full circle d is at most floor(W / 2), and the window is the
                whole row once 2 n + 1 >= W; on a regional grid d is at most W - 1 (and pi / dlambda).  `disc_table` evaluates
                this on the host in fp64 into an integer table -- row_lo[i], row_count[i], half[i, r] as int32 -- and both paths
                read only that table, so membership is never decided twice.
    WEIGHTS     w_k = cos(lat_k), exactly 0 for pole rows (|lat| >= 90 - 1e-9, the rule of `diagnostics`).
    VALIDITY    a source point is valid where it is finite; an invalid point enters as 0 with count 0.
    ROW SUMS    from exclusive prefix tables per row, P[0 .. W] (fp64 sums of the valid values) and N[0 .. W] (int32 counts).
                With lo = j - n and hi = j + n + 1 the window sum S is  P[W] if 2 n + 1 >= W;  (P[W] - P[lo + W]) + P[hi] if lo < 0;
                (P[W] - P[lo]) + P[hi - W] if hi > W;  P[hi] - P[lo] otherwise; the count C takes the same cases in integers.  A
                regional grid clips lo and hi into the row instead.
    VALUE       num = sum_k w_k S_k and den = sum_k w_k C_k over k in ascending row order in fp64; value = (float)(num / den); a
                result that is not finite is NaN.
    COVERAGE    full = sum_k w_k F_k with F = 2 n + 1, on a full circle at most W; columns clipped off a regional grid count as
                invalid.  The target is NaN where den <= 0 and where den / full < min_valid; with keep_mask=True also where the
                centre point itself is not finite, so the land of the wave model stays land.
    LIMITS      radius_km finite and > 0; min_valid in [0, 1]; at most 255 source rows per target row.

The grid is checked by THE GRID RULE of aurora_amd/_sphere.py, which also says when it wraps.

Fields on one GPU are smoothed by aurora_hip_smooth (aurora_amd/csrc/smooth.hip): a prefix launch (a wavefront scans a row)
and a gather launch (a lane reads the prefix tables at the ends of its windows); nothing is read back.  The workspace is
PLANE-SIZED -- 12 bytes per point of the planes in flight, plus one entry per row -- so the binding takes the planes in chunks
that keep it under 128 MiB.  A plane's result does not depend on the chunking.  Fields on the CPU take the rule in numpy
(`np.cumsum` for the prefixes, after a conversion to float32).

Not offered: Gaussian or other kernels, latitude bands (`BandBatch`).  Minimum / maximum filters over the same disc: `extrema`.
"""

from __future__ import annotations

import functools
import math
from typing import Optional, Sequence

import numpy as np
import torch

from aurora_amd import _fields, _sphere
from aurora_amd._fields import _host
from aurora_amd.batch import Batch

__all__ = ["smooth", "disc_table", "EARTH_RADIUS_KM", "MAX_ROWS"]

EARTH_RADIUS_KM = _sphere.EARTH_RADIUS / 1000.0
MAX_ROWS = 255


# ---- the table ---------------------------------------------------------------------------------------------------------------
def disc_table(lat, dlambda: float, n_lon: int, wrap: bool, radius_km: float):
    """THE RULE's membership as a table: (row_lo (H,), row_count (H,), half (H, max_rows) int32 -- -1 where a row has no column
    or past row_count -- and w (H,) fp64) for latitudes in degrees, the longitude step in radians and the radius."""
    lat = np.asarray(lat, dtype=np.float64)
    H, W = lat.shape[0], int(n_lon)
    phi = np.deg2rad(lat)
    rho = float(radius_km) / EARTH_RADIUS_KM
    s, c, cos_rho = np.sin(phi), np.cos(phi), math.cos(rho)
    cap = W // 2 if wrap else (min(W - 1, int(math.floor(math.pi / dlambda))) if W > 1 else 0)
    cos_d = np.cos(np.arange(cap + 1, dtype=np.float64) * dlambda)
    member = np.abs(phi[None, :] - phi[:, None]) <= rho                       # (target, source); contiguous in a monotonic grid
    row_count = member.sum(axis=1).astype(np.int32)
    row_lo = member.argmax(axis=1).astype(np.int32)
    if row_count.max() > MAX_ROWS:
        gaps = np.sort(np.abs(phi[None, :] - phi[:, None]), axis=1)[:, MAX_ROWS]   # the gap to the first row too many
        limit = float(gaps.min()) * EARTH_RADIUS_KM
        raise ValueError(f"smooth: a radius of {float(radius_km):g} km spans {int(row_count.max())} latitude rows of this grid; at "
                         f"most {MAX_ROWS} are supported, which allows any radius below {limit:.3f} km")
    half = np.full((H, int(row_count.max())), -1, dtype=np.int32)
    for i in range(H):
        ks = np.arange(row_lo[i], row_lo[i] + row_count[i])
        inside = (s[i] * s[ks])[:, None] + (c[i] * c[ks])[:, None] * cos_d[None, :] >= cos_rho     # (rows, cap + 1)
        half[i, :ks.shape[0]] = np.where(inside.any(axis=1), cap - np.argmax(inside[:, ::-1], axis=1), -1)
    w = np.where(np.abs(lat) >= 90.0 - 1e-9, 0.0, np.maximum(c, 0.0))
    return row_lo, row_count, half, w


@functools.lru_cache(maxsize=8)
def _table(lat_bytes: bytes, dlambda: float, n_lon: int, wrap: bool, radius_km: float):
    return disc_table(np.frombuffer(lat_bytes, dtype=np.float64), dlambda, n_lon, wrap, radius_km)


def _packed(table) -> np.ndarray:
    """[row_lo | row_count | half] as one int32 vector: what `lib.smooth_planes` takes."""
    row_lo, row_count, half, _ = table
    return np.concatenate([row_lo, row_count, half.reshape(-1)]).astype(np.int32)


# ---- the rule on the host ---------------------------------------------------------------------------------------------------
def _window(n: int, W: int, wrap: bool):
    """The entries (e0, e1, e2) of every column's window, sum = (P[e1] - P[e0]) + P[e2] with P[0] = 0, and its full width:
    aurora_amd/csrc/smooth_window.h in numpy."""
    j = np.arange(W)
    lo, hi = j - n, j + n + 1
    zero = np.zeros(W, dtype=np.int64)
    if not wrap:
        return np.clip(lo, 0, W), np.clip(hi, 0, W), zero, 2 * n + 1
    if 2 * n + 1 >= W:
        return zero, np.full(W, W), zero, W
    west, east = lo < 0, hi > W
    e0 = np.where(west, lo + W, lo)
    e1 = np.where(west | east, W, hi)
    e2 = np.where(west, hi, np.where(east, hi - W, 0))
    return e0, e1, e2, 2 * n + 1


def _smooth_host(x: np.ndarray, table, wrap: bool, min_valid: float, keep_mask: bool) -> np.ndarray:
    """x: (n, H, W) float32 -> (n, H, W) float32 by THE RULE."""
    row_lo, row_count, half, w = table
    n_planes, H, W = x.shape
    valid = np.isfinite(x)
    P = np.zeros((n_planes, H, W + 1))
    N = np.zeros((n_planes, H, W + 1), dtype=np.int64)
    np.cumsum(np.where(valid, x.astype(np.float64), 0.0), axis=-1, out=P[..., 1:])
    np.cumsum(valid, axis=-1, out=N[..., 1:])
    windows: dict = {}
    out = np.empty((n_planes, H, W), dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(H):
            num, den, full = np.zeros((n_planes, W)), np.zeros((n_planes, W)), np.zeros(W)
            for r in range(row_count[i]):                                  # ascending source rows
                n = int(half[i, r])
                if n < 0:
                    continue
                k = row_lo[i] + r
                if n not in windows:
                    windows[n] = _window(n, W, wrap)
                e0, e1, e2, width = windows[n]
                S = (P[:, k, e1] - P[:, k, e0]) + P[:, k, e2]
                C = (N[:, k, e1] - N[:, k, e0]) + N[:, k, e2]
                num += w[k] * S
                den += w[k] * C.astype(np.float64)
                full += w[k] * float(width)
            value = (num / den).astype(np.float32)
            keep = (den > 0.0) & ~(den / full < min_valid) & np.isfinite(value)
            if keep_mask:
                keep &= valid[:, i]
            out[:, i] = np.where(keep, value, np.float32("nan"))
    return out


# ---- public function ------------------------------------------------------------------------------------------------------
_ON_CAPTURE = ("smooth: call once on this grid with this radius before capturing a graph (the disc table is uploaded on the "
               "first call, which a captured graph cannot replay)")


def smooth(batch: Batch, radius_km: float, *, only: Optional[Sequence[str]] = None, min_valid: float = 0.5,
           keep_mask: bool = True) -> Batch:
    """The mean over the great-circle disc of `radius_km` of the last history entry of every surface and atmospheric variable
    of `batch` (or of those named in `only`), as a float32 `Batch` on the device of the inputs; see the module's text."""
    if not isinstance(batch, Batch):
        raise TypeError(f"smooth: batch must be a Batch, got {type(batch).__name__}")
    _fields.check_vector_grid("smooth", batch, "batch", band="fields")
    try:
        radius_km = float(radius_km)
    except (TypeError, ValueError):
        raise ValueError(f"smooth: radius_km must be a finite number above 0, got {radius_km!r}") from None
    if not (math.isfinite(radius_km) and radius_km > 0):
        raise ValueError(f"smooth: radius_km must be a finite number above 0, got {radius_km!r}")
    if isinstance(min_valid, bool) or not isinstance(min_valid, (int, float, np.integer, np.floating)) or not 0 <= min_valid <= 1:
        raise ValueError(f"smooth: min_valid must be a number in [0, 1], got {min_valid!r}")
    if isinstance(only, str):
        only = (only,)
    md = batch.metadata
    lat, lon = _host(md.lat), _host(md.lon)
    n_lat, n_lon = lat.shape[0], lon.shape[0]
    step, wrap = _sphere.regular_grid("smooth", lat, lon, least=1, in_range=True)      # (a single row or column passes)
    dlambda = float(np.deg2rad(step))
    names, fields, layout = _fields.select_one("smooth", batch, "batch", only)
    if not names:
        raise ValueError("smooth: batch holds no surface or atmospheric variable to smooth")
    dev = _fields.device_of("smooth", fields, batches="batch")
    table = _table(lat.tobytes(), dlambda, n_lon, wrap, radius_km)
    min_valid, keep_mask = float(min_valid), bool(keep_mask)

    if dev == "cpu":
        by_name = {}
        for name, f in zip(names, fields):
            x = f.detach().to(torch.float32).contiguous().numpy().reshape(-1, n_lat, n_lon)
            by_name[name] = torch.from_numpy(_smooth_host(x, table, wrap, min_valid, keep_mask).reshape(tuple(f.shape)))
    else:
        from aurora_amd.engine import lib

        _fields.check_planes("smooth", [("batch", names, fields)], n_lat, n_lon, _fields.TAKES_TASK)
        key = (lat.tobytes(), dlambda, n_lon, wrap, radius_km)
        rows = _fields.tables.get(("smooth rows", *key), dev, lambda: _packed(table), _ON_CAPTURE)
        w = _fields.tables.get(("smooth weights", lat.tobytes()), dev, lambda: table[3], _ON_CAPTURE)
        # (ONE output tensor, so that the plane-pointer table names the inputs alone and a captured graph finds it again)
        by_name = _fields.by_variable(layout, lib.smooth_planes(fields, rows, w, wrap, min_valid, keep_mask))

    surf = {k: by_name[k][:, None] for k in batch.surf_vars if k in by_name}
    atmos = {k: by_name[k][:, None] for k in batch.atmos_vars if k in by_name}
    return Batch(surf, dict(batch.static_vars), atmos, md)
