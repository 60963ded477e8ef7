"""Which of the lows is a storm (not in the reference): a candidate of `extrema` is kept where the field rises (for maxima: falls)
by at least delta on every path from it to the rim of a disc of R kilometres -- the closed-contour criterion of DetectNodes-type
cyclone detection, the step between "every local minimum of red noise" and a storm count -- on the device, for every candidate of
every plane at once, from the integer table that `extrema` left there.

    lows = aurora_amd.extrema(aurora_amd.smooth(pred, 100.0), 300.0, only=["msl"])
    c = aurora_amd.closed_contours(lows, {"msl": [100.0, 200.0, 400.0]}, 600.0, connectivity=8)
    c.table["msl"]         # (B, T, max_points, 2) int32 on the device of `lows`: points, exits; (B, C, T, ...) for an atmospheric variable
    c.points, c.exits      # (B[, C], T, max_points) int32: the two columns
    c.closed["msl"]        # (B[, C], T, max_points) bool: the row is live and has no exit
    c.depth["msl"]         # (B[, C], max_points) float32: the largest delta that closes; 0 where none does, NaN past the live rows
    c.count_closed["msl"]  # (B[, C], T) int64: the number of closed contours -- the storm count
    c.value, c.lat, c.lon, c.row, c.col    # (B[, C], max_points): those of `lows`, for the variables tested
    c.cpu()                # the same object with host tensors: the one call that waits for the device

`e` is an `Extrema`, on the CPU or on one GPU: its `source` batch supplies the field (the last history entry of the same
variables), its `kind`, `wrap`, table, count and `max_points` the candidates; nothing is read back to build the call.  `delta`
follows the thresholds of `objects`: a variable of `e` -> 1 to 8 values (or a (C, T_v) array for an atmospheric variable), or
ONE sequence for every variable of `e`; finite, above 0, strictly ascending; ROUNDED TO FLOAT32 ONCE; a shorter list is padded
with NaN, and NaN means "no test"; only the variables named are tested.  `radius_km` is the radius of the contour's disc,
independent of `e.radius_km`; it goes through the cached `disc_table` of `smooth`, and on the device the table is the one that
`smooth` and `extrema` upload for the same grid and radius.

THE RULE (both paths and the tests refer to this text; include/aurora_hip.h has it for the device).  In one line: flood the
disc from the candidate through every point that is less than delta above it (or not finite), and count the filled points
that touch a passable point outside the disc.

    CANDIDATE   row s < min(count, max_points) of a plane's extrema table: the flat index p0 = i0 W + j0 and the value
                v0 = x[p0], which is finite by the rule of `extrema`.
    DOMAIN      the MEMBERS of the disc of row i0 around column j0, by the integer table of `disc_table(radius_km)` and nothing
                else; the wrap, clip and whole-row cases are those of `extrema`; p0 is always a member.
    PASSABLE    a point q is passable for delta where x[q] is not finite, and where (double)x[q] - (double)v0 < (double)delta
                (kind "max": (double)v0 - (double)x[q] < (double)delta): one fp64 subtraction and one comparison, the same bits
                on both paths.  A non-finite point can never hold a contour: the land of the wave model is open water here.
    NEIGHBOURS  those of `objects`: 4 or 8, none across rows 0 and H - 1, column W - 1 joins column 0 where `e.wrap`.
    FILL        F is the smallest set that holds p0 and every passable member adjacent to a point of F.  (The fixed point is
                unique, so nothing depends on the order in which it is reached.)
    EXIT        a point of F is an exit where a neighbour of it is passable and not a member; and, where `e.wrap` is false (a
                regional grid: every edge is open), where it lies in row 0, row H - 1, column 0 or column W - 1.  On a wrapping
                grid the first and the last row are walls.
    RESULT      table (n_planes, T, max_points, 2) int32: points = |F|, exits = the number of exits.  Rows past min(count,
                max_points) are zero; padded deltas give zero rows.  The contour is CLOSED where the row is live and exits == 0.
                Everything is an integer: the two paths agree in every byte, and nothing here has a tolerance.  (Closed at a
                delta implies closed at every smaller one: F only shrinks, and an exit of the smaller F is one of the larger.)
    LIMITS      radius_km as in `smooth` (finite, > 0, at most 255 source rows per target row); 1 to 4096 longitudes; and the
                largest WINDOW of the grid -- the source rows of a disc plus a ring row above and below, times the 64-column words
                of its widest row plus a ring column on either side (`window_words`) -- must fit the kernel's LDS budget in three
                bitmaps: 24 (max_rows + 2) max_words <= 159744 bytes (156 KiB).  A larger window is refused here, on either
                device, and again in the C entry point, before any launch.  The budget admits 721 x 1440 at 1000 km (73 rows x
                23 words: 40 KiB) and, by this arithmetic, 1801 x 3600 at 600 km (109 rows x 57 words: 146 KiB).

Fields on one GPU are tested by ONE aurora_hip_closed_contours call (aurora_amd/csrc/contours.hip, contour_fill.h): a workgroup
per (plane, table row) builds the window's bitmaps in LDS by ballot and repeats R |= A & dilate(R) until a sweep changes nothing;
no workspace, nothing read back.  Fields on the CPU take the rule in numpy per candidate: the window as boolean arrays, the
fill as the component of the candidate under `objects.label_events`.  Finalisation is torch code shared by both devices.

Not offered: testing ANOTHER variable around the candidate (a warm-core test); latitude bands of a full circle whose first or
last row should be open; prominence as a continuous value (`depth` is the largest of the <= 8 deltas given); `BandBatch`.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Mapping

import numpy as np
import torch

from aurora_amd import _fields, _sphere
from aurora_amd._fields import _host
from aurora_amd.extrema import Extrema
from aurora_amd.extrema import _finalise as _finalise_extrema
from aurora_amd.objects import Result, final_properties, label_events
from aurora_amd.smooth import _packed, _table

__all__ = ["closed_contours", "ClosedContours", "COLUMNS", "LDS_BUDGET", "window_words"]

COLUMNS = ("points", "exits")
LDS_BUDGET = 156 * 1024          # bytes of a workgroup's three bitmaps: kContourLdsBudget of aurora_amd/csrc/contour_fill.h
_ON_CAPTURE = ("closed_contours: call once on this grid with this radius before capturing a graph (the disc table is uploaded on "
               "the first call, which a captured graph cannot replay)")


# ---- the window ----------------------------------------------------------------------------------------------------------
def _widest(table) -> np.ndarray:
    """The widest half width of every target row's disc, its own row counted as max(n, 0): (H,) int."""
    row_lo, row_count, half, _ = table
    H = row_lo.shape[0]
    own = np.arange(H) - row_lo
    n = half.copy()
    inside = (own >= 0) & (own < row_count)
    n[np.flatnonzero(inside), own[inside]] = np.maximum(n[np.flatnonzero(inside), own[inside]], 0)
    return n.max(axis=1) if n.shape[1] else np.full(H, -1)


def window_words(table, n_lon: int, wrap: bool) -> np.ndarray:
    """The 64-column words of the widest window row of every target row, whatever the candidate's column ((H,) int;
    contour_row_words of aurora_amd/csrc/contour_fill.h): on a full circle the whole row where a disc row is the whole row, else
    2 n + 3 columns; on a regional grid at most W + 2."""
    n, W = np.minimum(_widest(table).astype(np.int64), n_lon), int(n_lon)
    if wrap:
        width = np.where(2 * n + 1 >= W, W, 2 * n + 3)
    else:
        width = np.minimum(2 * n + 3, W + 2)
    return (width + 63) // 64


def _check_budget(table, n_lon: int, wrap: bool, radius_km: float) -> int:
    """max_words of the grid, after THE RULE's LIMITS."""
    words = window_words(table, n_lon, wrap)
    max_rows = int(table[2].shape[1])
    need = 24 * (max_rows + 2) * words
    over = np.flatnonzero(need > LDS_BUDGET)
    if over.size:
        fits = LDS_BUDGET // (24 * (max_rows + 2))
        raise ValueError(f"closed_contours: a radius of {float(radius_km):g} km gives windows of {max_rows + 2} rows x "
                         f"{int(words.max())} words of 64 columns on this grid, {int(need.max())} bytes of LDS in three bitmaps; the "
                         f"budget is {LDS_BUDGET} bytes, which allows {fits} words at this many rows, and {over.size} target rows "
                         f"({int(over[0])} to {int(over[-1])}) exceed it")
    return int(words.max())


# ---- the rule on the host ---------------------------------------------------------------------------------------------------
def _dilate(m: np.ndarray, eight: bool, cyclic: bool) -> np.ndarray:
    """The points of a (rows, width) mask or next to one: the four or eight neighbours, around the circle where `cyclic`."""
    def sideways(a):
        out = a.copy()
        if cyclic:
            return out | np.roll(a, 1, axis=1) | np.roll(a, -1, axis=1)
        out[:, 1:] |= a[:, :-1]
        out[:, :-1] |= a[:, 1:]
        return out

    up, down = np.zeros_like(m), np.zeros_like(m)
    up[1:], down[:-1] = m[:-1], m[1:]
    if eight:
        return sideways(m) | sideways(up) | sideways(down)
    return sideways(m) | up | down


def _contours_host(x: np.ndarray, rows: np.ndarray, count: np.ndarray, deltas: np.ndarray, table, wrap: bool, is_max: bool,
                   connectivity: int) -> np.ndarray:
    """x: (n, H, W) float32, rows: (n, max_points, 2) int64, count: (n,), deltas: (n, T) float32 -> (n, T, max_points, 2) int32
    by THE RULE."""
    row_lo, row_count, half, _ = table
    n_planes, H, W = x.shape
    T, max_points = deltas.shape[1], rows.shape[1]
    out = np.zeros((n_planes, T, max_points, len(COLUMNS)), dtype=np.int32)
    eight = connectivity == 8
    for p in range(n_planes):
        for s in range(min(int(count[p]), max_points)):
            p0 = int(rows[p, s, 0])
            i0, j0 = divmod(p0, W)
            k_lo, cnt = int(row_lo[i0]), int(row_count[i0])
            n = np.full(cnt + 2, -1, dtype=np.int64)                    # the ring rows hold no member
            n[1:-1] = half[i0, :cnt]
            n[i0 - k_lo + 1] = max(n[i0 - k_lo + 1], 0)
            n_max = int(n.max())
            cyclic = wrap and 2 * n_max + 1 >= W
            if cyclic:                                                  # the window is the whole circle
                first, cols = 0, np.arange(W)
                gap = np.abs(cols - j0)
                gap, in_row = np.minimum(gap, W - gap), np.ones(W, dtype=bool)
            else:                                                       # the disc's columns and a ring column on either side
                first, last = j0 - n_max - 1, j0 + n_max + 1
                if not wrap:
                    first, last = max(first, -1), min(last, W)
                cols = np.arange(first, last + 1)
                gap = np.abs(cols - j0)
                in_row = np.ones(cols.shape[0], dtype=bool) if wrap else (cols >= 0) & (cols < W)
                cols = cols % W if wrap else np.clip(cols, 0, W - 1)
            k = np.arange(k_lo - 1, k_lo + cnt + 1)
            exists = ((k >= 0) & (k < H))[:, None] & in_row[None, :]
            v = x[p][np.clip(k, 0, H - 1)[:, None], cols[None, :]]
            member = exists & (gap[None, :] <= n[:, None])
            v0 = np.float64(x[p, i0, j0])
            with np.errstate(invalid="ignore", over="ignore"):
                rise = (v0 - v.astype(np.float64)) if is_max else (v.astype(np.float64) - v0)
            edge = np.zeros_like(exists)
            if not wrap:
                edge = exists & (((k == 0) | (k == H - 1))[:, None] | ((cols == 0) | (cols == W - 1))[None, :])
            seed = (i0 - k_lo + 1, j0 - first)
            for t in range(T):
                d = deltas[p, t]
                if not d > 0:
                    continue
                with np.errstate(invalid="ignore"):
                    passable = exists & (~np.isfinite(v) | (rise < np.float64(d)))
                labels, _ = label_events(passable & member, connectivity, cyclic)
                F = labels == labels[seed]
                open_ = _dilate(passable & ~member, eight, cyclic) | edge
                out[p, t, s] = int(F.sum()), int((F & open_).sum())
    return out


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
def _finalise(table: torch.Tensor, count: torch.Tensor, deltas: torch.Tensor, rows: torch.Tensor, lat: torch.Tensor,
              lon: torch.Tensor) -> dict[str, torch.Tensor]:
    """The properties of every candidate from the integer tables; elementwise and sums of integers, no read-back."""
    M = table.shape[-2]
    live = torch.arange(M, device=table.device) < count[..., None]                   # (n, M)
    tested = ~torch.isnan(deltas)                                                     # (n, T)
    points, exits = table[..., 0], table[..., 1]
    closed = live[:, None, :] & tested[:, :, None] & (exits == 0)
    zero = torch.zeros((), dtype=torch.float32, device=table.device)
    depth = torch.where(closed, deltas[:, :, None], zero).amax(dim=1)                 # (closed at a delta: at every smaller one)
    depth = torch.where(live, depth, torch.full_like(depth, float("nan")))
    out = {"points": points, "exits": exits, "closed": closed, "depth": depth, "count_closed": closed.sum(dim=-1)}
    out.update(_finalise_extrema(rows, count, lat, lon))
    return out


@dataclasses.dataclass(eq=False)
class ClosedContours(Result):
    """Result of `closed_contours`: every property is a dict name -> tensor with the leading shape (B,) for a surface variable
    and (B, C) for an atmospheric one, on the device of the extrema."""

    table_table: torch.Tensor                              # (n_planes, T, max_points, 2) int32
    deltas_table: torch.Tensor                             # (n_planes, T) float32, NaN: none
    rows_table: torch.Tensor                               # (n_planes, max_points, 2) int64: the extrema table of these planes
    count_table: torch.Tensor                              # (n_planes,) int32: their numbers of extrema
    grid_lat: torch.Tensor                                 # (H,) fp64, on the device of the tables
    grid_lon: torch.Tensor                                 # (W,) fp64
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable tested
    kind: str
    radius_km: float
    connectivity: int
    wrap: bool
    max_points: int

    def _finalise(self) -> dict[str, torch.Tensor]:
        return _finalise(self.table_table, self.count_table, self.deltas_table, self.rows_table, self.grid_lat, self.grid_lon)

    @property
    def table(self) -> dict[str, torch.Tensor]:
        return self._field(self.table_table)

    @property
    def deltas(self) -> dict[str, torch.Tensor]:
        return self._field(self.deltas_table)

    @property
    def count(self) -> dict[str, torch.Tensor]:
        """The number of extrema of every plane: that of the `Extrema`."""
        return self._field(self.count_table)

    def cpu(self) -> "ClosedContours":
        """The same result with host tensors (waits for the device)."""
        moved = {f: getattr(self, f).cpu() for f in ("table_table", "deltas_table", "rows_table", "count_table", "grid_lat",
                                                     "grid_lon")}
        return dataclasses.replace(self, **moved)


final_properties(ClosedContours, ("points", "exits", "closed", "depth", "count_closed", "value", "lat", "lon", "row", "col"),
                 "of every candidate; see the module's text.")


# ---- public function ------------------------------------------------------------------------------------------------------
def _planes_of(e, names) -> tuple:
    """The extrema table and count of the planes of `names`, in that order: views where they are one run of planes."""
    first = {name: (at, math.prod(shape)) for name, at, shape in e.layout}
    runs = [first[name] for name in names]
    if all(a + n == b for (a, n), (b, _) in zip(runs, runs[1:])):
        lo, hi = runs[0][0], runs[-1][0] + runs[-1][1]
        return e.table_table[lo:hi], e.count_table[lo:hi]
    return (torch.cat([e.table_table[a:a + n] for a, n in runs]), torch.cat([e.count_table[a:a + n] for a, n in runs]))


def closed_contours(e, delta, radius_km: float, *, connectivity: int = 8) -> ClosedContours:
    """The closed-contour test of the candidates of `e` (an `Extrema`) at the deltas of `delta` within `radius_km`; see the
    module's text for THE RULE."""
    if not isinstance(e, Extrema):
        raise TypeError(f"closed_contours: e must be an Extrema, got {type(e).__name__}")
    try:
        radius_km = float(radius_km)
    except (TypeError, ValueError):
        raise ValueError(f"closed_contours: radius_km must be a finite number above 0, got {radius_km!r}") from None
    if not (math.isfinite(radius_km) and radius_km > 0):
        raise ValueError(f"closed_contours: radius_km must be a finite number above 0, got {radius_km!r}")
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"closed_contours: connectivity must be 4 or 8, got {connectivity!r}")
    held = [name for name, _, _ in e.layout]
    if not isinstance(delta, Mapping):
        delta = {name: delta for name in held}
    if not delta:
        raise ValueError("closed_contours: delta must be a non-empty mapping from variable name to values, or one sequence")
    for k in delta:
        if k not in held:
            raise ValueError(f"closed_contours: delta names the variable {k!r}, which e does not hold; its variables are {tuple(held)}")
    batch = e.source
    _fields.check_vector_grid("closed_contours", batch, "e.source", band="fields")
    names, fields, layout = _fields.select_one("closed_contours", batch, "e.source", [k for k in held if k in delta])
    deltas = _fields.threshold_table("closed_contours", delta, layout, "deltas")
    for k, v in delta.items():
        f = np.asarray(v, dtype=np.float64).astype(np.float32)
        if not np.all(np.isfinite(f) & (f > 0)):
            raise ValueError(f"closed_contours: the deltas of {k!r} must be finite and above 0 (as float32), got {f.reshape(-1).tolist()}")
    _fields.check_ascending("closed_contours", deltas, layout, "deltas")
    rows, count = _planes_of(e, names)
    dev = _fields.device_of("closed_contours", [*fields, e.table_table, e.count_table], "the tables of e and the fields of e.source",
                            "Extrema and its source batch")
    md = batch.metadata
    lat, lon = _host(md.lat), _host(md.lon)
    n_lat, n_lon = lat.shape[0], lon.shape[0]
    if tuple(e.index_table.shape[-2:]) != (n_lat, n_lon):
        raise ValueError(f"closed_contours: e was made on a grid of {tuple(e.index_table.shape[-2:])} points, e.source has {(n_lat, n_lon)}")
    step, wrap = _sphere.regular_grid("closed_contours", lat, lon, least=1, in_range=True)
    if wrap != e.wrap:
        raise ValueError(f"closed_contours: e.wrap is {e.wrap}, but the grid of e.source {'wraps' if wrap else 'does not wrap'}")
    dlambda = float(np.deg2rad(step))
    table = _table(lat.tobytes(), dlambda, n_lon, wrap, radius_km)     # (more than 255 rows: the refusal of `disc_table`)
    max_words = _check_budget(table, n_lon, wrap, radius_km)           # (on either device: the paths accept the same calls)
    is_max, connectivity = e.kind == "max", int(connectivity)

    if dev == "cpu":
        with np.errstate(over="ignore", invalid="ignore"):
            x = np.ascontiguousarray(_fields.stack(fields, n_lat, n_lon), dtype=np.float32)
        out = torch.from_numpy(_contours_host(x, rows.numpy(), count.numpy(), deltas, table, wrap, is_max, connectivity))
        deltas_t = torch.from_numpy(deltas)
    else:
        from aurora_amd.engine import lib

        _fields.check_planes("closed_contours", [("e.source", names, fields)], n_lat, n_lon, _fields.TAKES_TASK)
        key = (lat.tobytes(), dlambda, n_lon, wrap, radius_km)
        packed = _fields.tables.get(("smooth rows", *key), dev, lambda: _packed(table), _ON_CAPTURE)     # (the table of `smooth`)
        deltas_t = _fields.device_thresholds("closed_contours", deltas, dev)
        out = lib.closed_contours_planes(fields, rows.contiguous(), count.contiguous(), deltas_t, packed, max_words, wrap, is_max,
                                         connectivity)
    return ClosedContours(out, deltas_t, rows, count, e.grid_lat, e.grid_lon, layout, e.kind, radius_km, connectivity, wrap,
                          e.max_points)
