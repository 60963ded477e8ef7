"""Which storm is this, where is it and how large: the connected regions of `field >= threshold` on the sphere, per variable
and level, with their sizes, positions and peaks (not in the reference).  The primitive of object-based verification (MODE, SAL,
atmospheric-river catalogues, storm counts).

    o = aurora_amd.objects(batch, {"ivt": [250., 500.], "10ws": [15.]}, below=False, connectivity=8, wrap=None, max_objects=4096)
    o.labels["ivt"]     # (B, T, H, W) int32 on the batch's device, 0 for background; (B, C, T, H, W) for an atmospheric variable
    o.count["ivt"]      # (B[, C], T) int32: the number of objects -- the true number, also beyond max_objects
    o.table["ivt"]      # (B[, C], T, max_objects, 10) int64: one row per object, the columns of THE RULE
    o.truncated["ivt"]  # count > max_objects
    o.points, o.area, o.centroid_row, o.centroid_col, o.centroid_lat, o.centroid_lon, o.peak, o.peak_row, o.peak_col,
    o.peak_lat, o.peak_lon          # (B[, C], T, max_objects): NaN (float) or -1 (integer) past `count`
    o.bbox              # (B[, C], T, max_objects, 4) int64: row_min, row_max, col_min, col_max (col_min > col_max across the seam)
    o.mask("ivt", 3)    # labels["ivt"] == 3
    o.cpu()             # the same object with host tensors: the one call that waits for the device

`thresholds` follows `event_scores`: a variable name -> 1 to 8 values, or a (C, T_v) array for an atmospheric variable; ROUNDED TO
FLOAT32 ONCE; a shorter list is padded with NaN, and NaN means "no event"; only the variables named are labelled, on their last
history entry.  Fields of another precision (CPU batches only) are rounded to float32 first.

THE RULE (both paths and the tests refer to this text)

 1. A point is an EVENT where its value v is finite and v >= t (`below=True`: v <= t).  NaN, +-Inf and non-events are background.
    Neighbours are grid neighbours: 4 (rows and columns) or 8 (diagonals too, `connectivity`).  There are none across the poles:
    rows 0 and H - 1 have none beyond them.  On a WRAPPING grid column W - 1 and column 0 are neighbours (diagonally too with 8).
    `wrap=None` takes the grid as wrapping where THE GRID RULE does (`_sphere.full_circle`); `wrap=True` / `False` overrides
    that.
    An OBJECT is a maximal connected set of events of one plane and one threshold.
 2. Its FIRST POINT is its smallest row-major flat index i W + j.
 3. Objects are numbered 1, 2, ... in ascending order of their first points.
 4. `labels` holds the number of every point's object and 0 for background: on a grid that does not wrap the numbering of
    `scipy.ndimage.label`; on a wrapping grid objects that meet across the seam are one.
 5. `count` is the number of objects, also when it exceeds `max_objects`.
 6. `table` has one row per object k <= max_objects, at index k - 1; rows past `count` are zero.  An object numbered above
    `max_objects` keeps its label in the map but has no row; `truncated` says that this happened.
 7. The columns, all exact integers:
      0 points        the number of points
      1 area_units    sum of unit[i] over the points, unit[i] = llrint(w_i 2^32) made once on the host from w =
                      `_fields.latitude_weights(lat)`: the area in "grid points at mean latitude" is area_units / 2^32, with an
                      absolute error of at most points 2^-33 (each unit is off by at most 2^-33 of a point).  (The sum stays
                      within int64 for objects of up to 2^30 points.)
      2 first         the flat index of the first point
      3 row_min  4 row_max   the smallest and largest row
      5 row_sum       sum of i over the points
      6 col_off_min  7 col_off_max  8 col_off_sum   of d = j - j_first, where j_first = first mod W; on a wrapping grid d is
                      reduced into [-floor(W / 2), W - floor(W / 2)).  An object wider than half the circle has an ambiguous
                      centre (its offsets may fold onto each other); that is not an error.
      9 peak_key      the unsigned 64-bit MAXIMUM over the points of  (K(v) << 32) | (0xffffffff - flat index),  stored as the
                      int64 of the same bits, where for the float32 bits u of v:  K = ~u where u has the sign bit, else
                      u | 0x80000000  (ascending with v; -0 sorts below +0, as the integer key of ensemble_scores.hip), and
                      with `below=True` ~K in its place.  So the peak is the largest value (`below`: the smallest), and among
                      equal values the smallest flat index.

Finalisation is torch code shared by both devices, elementwise on these integers, so `area`, the centroids (row_sum / points
and j_first + col_off_sum / points, the column taken mod W on a wrapping grid; latitude and longitude by linear interpolation of
the coordinate vectors at the fractional row and column, across the seam -- lon[0] + 360 follows lon[W - 1] -- on a wrapping
grid), the peak and the bounding box have the same bits on either device.

Fields on one GPU are labelled by ONE aurora_hip_objects call (union-find over planes: aurora_amd/csrc/objects.hip) with nothing
read back; unlike the other verification modules it needs a plane-sized workspace, 4 bytes per point and threshold.  Fields on
the CPU are labelled in numpy: runs per row, a union-find over the runs that touch, the table by np.add.at / minimum.at /
maximum.at.  `labels`, `count` and `table` agree bit for bit between the two.
"""

from __future__ import annotations

import dataclasses
import functools
from typing import Mapping, Optional

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._sphere import full_circle
from aurora_amd.batch import Batch

__all__ = ["objects", "Objects", "COLUMNS"]

COLUMNS = ("points", "area_units", "first", "row_min", "row_max", "row_sum", "col_off_min", "col_off_max", "col_off_sum",
           "peak_key")
MAX_POINTS = 2 ** 31 - 2
_POINTS, _AREA, _FIRST, _ROW_MIN, _ROW_MAX, _ROW_SUM, _OFF_MIN, _OFF_MAX, _OFF_SUM, _PEAK = range(10)
_ON_CAPTURE = ("objects: call once on this grid before capturing a graph (the area units and the coordinates are uploaded on "
               "the first call, which a captured graph cannot replay)")


def area_units(lat) -> np.ndarray:
    """unit[i] = llrint(w_i 2^32) of THE RULE, int64."""
    return np.rint(_fields.latitude_weights(lat) * 2.0 ** 32).astype(np.int64)


def device_units(lat: np.ndarray, device: torch.device, on_capture: str) -> torch.Tensor:
    """`area_units(lat)` on `device`: one table per grid, which `objects` uploads and `object_matches` finds again."""
    return _fields.tables.get(("object units", lat.tobytes()), device, lambda: area_units(lat), on_capture)


# ---- the CPU path ----------------------------------------------------------------------------------------------------------
def label_events(ev: np.ndarray, connectivity: int = 8, wrap: bool = False) -> tuple[np.ndarray, int]:
    """(labels (H, W) int32, count) of an (H, W) bool event mask by THE RULE: the runs of every row, the pairs of runs that touch
    (the row above, the seam), a union-find over the runs that hangs the later run under the earlier, numbers by first point."""
    H, W = ev.shape
    labels = np.zeros((H, W), dtype=np.int32)
    pad = np.zeros((H, W + 2), dtype=np.int8)
    pad[:, 1:-1] = ev
    step = np.diff(pad, axis=1)
    row, s = np.nonzero(step == 1)                 # the runs in row-major order: row, first column
    e = np.nonzero(step == -1)[1] - 1              # last column
    n = s.shape[0]
    if n == 0:
        return labels, 0
    # the runs of the row above that a run touches are consecutive: those that end at or after s - k and start at or before e + k
    k, K = (1 if connectivity == 8 else 0), W + 2
    lo = np.searchsorted(row * K + e + 1, (row - 1) * K + s + 1 - k, "left")
    hi = np.searchsorted(row * K + s + 1, (row - 1) * K + e + 1 + k, "right")
    cnt = np.maximum(hi - lo, 0)
    a = np.repeat(np.arange(n), cnt)
    b = np.repeat(lo, cnt) + np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    if wrap and W > 1:
        at_first, at_last = np.full(H, -1), np.full(H, -1)      # the run of a row at column 0 and at column W - 1
        at_first[row[s == 0]] = np.flatnonzero(s == 0)
        at_last[row[e == W - 1]] = np.flatnonzero(e == W - 1)
        seams = [(at_last, at_first)]
        if connectivity == 8:
            seams += [(at_first[1:], at_last[:-1]), (at_last[1:], at_first[:-1])]
        for x, y in seams:
            both = (x >= 0) & (y >= 0)
            a, b = np.concatenate([a, x[both]]), np.concatenate([b, y[both]])
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(a.tolist(), b.tolist()):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)
    root = np.fromiter((find(x) for x in range(n)), dtype=np.int64, count=n)
    firsts = np.unique(root)                       # ascending run index = ascending first point
    labels[ev] = np.repeat(np.searchsorted(firsts, root) + 1, e - s + 1).astype(np.int32)
    return labels, int(firsts.shape[0])


def value_keys(v: np.ndarray, below: bool) -> np.ndarray:
    """K(v) (`below`: ~K) of THE RULE for float32 values, uint32."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ~key if below else key


def tabulate(values: np.ndarray, labels: np.ndarray, count: int, unit: np.ndarray, max_objects: int, below: bool,
             wrap: bool) -> np.ndarray:
    """The (max_objects, 10) int64 table of one float32 plane and its label map."""
    table = np.zeros((max_objects, len(COLUMNS)), dtype=np.int64)
    n = min(count, max_objects)
    if n == 0:
        return table
    H, W = labels.shape
    flat = labels.reshape(-1)
    idx = np.flatnonzero((flat > 0) & (flat <= max_objects)).astype(np.int64)
    k = flat[idx].astype(np.int64) - 1
    i, j = idx // W, idx % W
    t = table[:n]
    first = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(first, k, idx)
    d = j - (first % W)[k]
    if wrap:
        half = W // 2
        d = np.where(d < -half, d + W, np.where(d >= W - half, d - W, d))
    t[:, _FIRST] = first
    np.add.at(t[:, _POINTS], k, 1)
    np.add.at(t[:, _AREA], k, unit[i])
    t[:, _ROW_MIN] = np.iinfo(np.int64).max
    np.minimum.at(t[:, _ROW_MIN], k, i)
    np.maximum.at(t[:, _ROW_MAX], k, i)
    np.add.at(t[:, _ROW_SUM], k, i)
    np.minimum.at(t[:, _OFF_MIN], k, d)            # the first point has d = 0, so 0 is a sound start for both
    np.maximum.at(t[:, _OFF_MAX], k, d)
    np.add.at(t[:, _OFF_SUM], k, d)
    key = (value_keys(values.reshape(-1)[idx], below).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - idx.astype(np.uint64))
    peak = np.zeros(n, dtype=np.uint64)
    np.maximum.at(peak, k, key)
    t[:, _PEAK] = peak.view(np.int64)
    return table


def _objects_host(planes: np.ndarray, thr: np.ndarray, unit: np.ndarray, below: bool, connectivity: int, wrap: bool,
                  max_objects: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    n_planes, H, W = planes.shape
    T = thr.shape[1]
    labels = np.zeros((n_planes, T, H, W), dtype=np.int32)
    count = np.zeros((n_planes, T), dtype=np.int32)
    table = np.zeros((n_planes, T, max_objects, len(COLUMNS)), dtype=np.int64)
    cmp = np.less_equal if below else np.greater_equal
    for p in range(n_planes):
        with np.errstate(over="ignore", invalid="ignore"):
            v = planes[p].astype(np.float32)
        finite = np.isfinite(v)
        for t in range(T):
            with np.errstate(invalid="ignore"):
                ev = finite & cmp(v, thr[p, t])
            labels[p, t], count[p, t] = label_events(ev, connectivity, wrap)
            table[p, t] = tabulate(v, labels[p, t], int(count[p, t]), unit, max_objects, below, wrap)
    return labels, count, table


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
def _finalise(table: torch.Tensor, count: torch.Tensor, lat: torch.Tensor, lon: torch.Tensor, wrap: bool,
              below: bool) -> dict[str, torch.Tensor]:
    """The properties of every object from the integer table; elementwise, no read-back."""
    H, W, M = lat.shape[0], lon.shape[0], table.shape[-2]
    live = torch.arange(M, device=table.device) < count[..., None]
    col = lambda c: table[..., c]                                                     # noqa: E731
    real = lambda x: torch.where(live, x, torch.full_like(x, float("nan")))           # noqa: E731
    whole = lambda x: torch.where(live, x, torch.full_like(x, -1))                    # noqa: E731
    n = col(_POINTS).to(torch.float64)
    j_first = col(_FIRST) % W
    c_row = col(_ROW_SUM).to(torch.float64) / n
    c_col = j_first.to(torch.float64) + col(_OFF_SUM).to(torch.float64) / n
    if wrap:
        c_col = torch.where(c_col < 0, c_col + W, torch.where(c_col >= W, c_col - W, c_col))
    # the coordinates at the fractional row and column
    r = torch.where(live, c_row, torch.zeros_like(c_row))
    i0 = torch.floor(r).clamp(0, max(H - 2, 0)).to(torch.int64)
    i1 = (i0 + 1).clamp(max=H - 1)
    c_lat = lat[i0] + (r - i0.to(torch.float64)) * (lat[i1] - lat[i0])
    c = torch.where(live, c_col, torch.zeros_like(c_col))
    j0 = torch.floor(c).clamp(0, W - 1).to(torch.int64)
    j1 = j0 + 1
    past = lon[0] + 360.0 if wrap else lon[W - 1]
    lon1 = torch.where(j1 < W, lon[j1.clamp(max=W - 1)], past)
    c_lon = lon[j0] + (c - j0.to(torch.float64)) * (lon1 - lon[j0])
    # the peak: undo the packing of THE RULE
    key = col(_PEAK)
    hi, lo = (key >> 32) & 0xffffffff, key & 0xffffffff
    if below:
        hi = hi ^ 0xffffffff
    u = torch.where(hi >= 0x80000000, hi ^ 0x80000000, hi ^ 0xffffffff)
    peak = torch.where(u >= 0x80000000, u - 2 ** 32, u).to(torch.int32).view(torch.float32)
    at = torch.where(live, 0xffffffff - lo, torch.zeros_like(lo))
    p_row, p_col = at // W, at % W
    cols = [j_first + col(_OFF_MIN), j_first + col(_OFF_MAX)]
    if wrap:
        cols = [x % W for x in cols]
    return {"points": whole(col(_POINTS)), "area": real(col(_AREA).to(torch.float64) / 2.0 ** 32),
            "centroid_row": real(c_row), "centroid_col": real(c_col), "centroid_lat": real(c_lat), "centroid_lon": real(c_lon),
            "peak": real(peak), "peak_row": whole(p_row), "peak_col": whole(p_col), "peak_lat": real(lat[p_row]),
            "peak_lon": real(lon[p_col]),
            "bbox": torch.where(live[..., None], torch.stack([col(_ROW_MIN), col(_ROW_MAX), *cols], dim=-1),
                                torch.full((), -1, dtype=torch.int64, device=table.device))}


class Result:
    """What `Objects`, `ObjectMatches`, `NearestEvent` and `ObjectSeparations` share: a property is a dict name -> tensor, cut
    from a table by the layout of the `Objects` that the field named `_owner` holds (None: the result itself); the finalised
    ones are made once, by the class's `_finalise()`, and looked up by `final_properties`."""

    _owner = None

    def _field(self, t: torch.Tensor) -> dict[str, torch.Tensor]:
        return _fields.by_variable((getattr(self, self._owner) if self._owner else self).layout, t)

    @functools.cached_property
    def _final(self) -> dict[str, torch.Tensor]:
        return self._finalise()


def _final_property(name: str, doc: str) -> property:
    return property(lambda self: self._field(self._final[name]), doc=f"`{name}` {doc}")


def final_properties(cls: type, names: tuple[str, ...], doc: str) -> None:
    """Give `cls` one property per name of its `_final`; `doc`: what follows the name in the property's text."""
    for name in names:
        setattr(cls, name, _final_property(name, doc))


def check_pair(fn: str, a: "Objects", b: "Objects") -> None:
    """`a` and `b` have the same layout, number of thresholds, grid and device, and bit-equal coordinates."""
    if a.layout != b.layout:
        raise ValueError(f"{fn}: a and b differ in layout (variable, first plane, shape): {a.layout} against {b.layout}")
    sa, sb = tuple(a.labels_table.shape), tuple(b.labels_table.shape)
    if sa[1] != sb[1]:
        raise ValueError(f"{fn}: a and b differ in the number of thresholds: {sa[1]} against {sb[1]}")
    if sa[2:] != sb[2:]:
        raise ValueError(f"{fn}: a and b differ in grid: {sa[2]} x {sa[3]} against {sb[2]} x {sb[3]} points; regrid first")
    da, db = a.labels_table.device, b.labels_table.device
    if da != db:
        raise ValueError(f"{fn}: a is on {da} and b on {db}; move both to the CPU (.cpu()) or label both on one GPU")
    for c in ("lat", "lon"):
        if not _same_values(getattr(a, c), getattr(b, c)):
            raise ValueError(f"{fn}: a and b differ in {c} (same length, different values); regrid first")


def _same_values(x: torch.Tensor, y: torch.Tensor) -> bool:
    """Bit-equal coordinates; `objects` keeps one device copy per content, so on a device this is `x is y` and waits for nothing."""
    return x is y or (x.shape == y.shape and torch.equal(x.view(torch.int64), y.view(torch.int64)))


@dataclasses.dataclass(eq=False)
class Objects(Result):
    """Result of `objects`: every property is a dict name -> tensor with the leading shape (B,) for a surface variable and
    (B, C) for an atmospheric one, on the device of the batch."""

    labels_table: torch.Tensor                            # (n_planes, T, H, W) int32
    count_table: torch.Tensor                             # (n_planes, T) int32
    table_table: torch.Tensor                             # (n_planes, T, max_objects, 10) int64
    thresholds_table: torch.Tensor                        # (n_planes, T) float32
    lat: torch.Tensor                                     # (H,) fp64, on the device of the tables
    lon: torch.Tensor                                     # (W,) fp64
    layout: tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable
    below: bool
    connectivity: int
    wrap: bool
    max_objects: int

    def _finalise(self) -> dict[str, torch.Tensor]:
        return _finalise(self.table_table, self.count_table, self.lat, self.lon, self.wrap, self.below)

    @property
    def labels(self) -> dict[str, torch.Tensor]:
        return self._field(self.labels_table)

    @property
    def count(self) -> dict[str, torch.Tensor]:
        return self._field(self.count_table)

    @property
    def table(self) -> dict[str, torch.Tensor]:
        return self._field(self.table_table)

    @property
    def truncated(self) -> dict[str, torch.Tensor]:
        return self._field(self.count_table > self.max_objects)

    @property
    def thresholds(self) -> dict[str, torch.Tensor]:
        return self._field(self.thresholds_table)

    def mask(self, name: str, k: int) -> torch.Tensor:
        """labels[name] == k: the points of object k of every plane and threshold of the variable."""
        labels = self.labels
        if name not in labels:
            raise KeyError(f"objects: no variable {name!r}; the variables are {tuple(labels)}")
        return labels[name] == k

    def cpu(self) -> "Objects":
        """The same objects with host tensors (waits for the device)."""
        moved = {f: getattr(self, f).cpu() for f in ("labels_table", "count_table", "table_table", "thresholds_table", "lat", "lon")}
        return dataclasses.replace(self, **moved)


final_properties(Objects, ("points", "area", "centroid_row", "centroid_col", "centroid_lat", "centroid_lon", "peak", "peak_row",
                           "peak_col", "peak_lat", "peak_lon", "bbox"), "of every object; see the module's text.")


# ---- public function -----------------------------------------------------------------------------------------------------
def objects(batch: Batch, thresholds: Mapping[str, object], below: bool = False, connectivity: int = 8,
            wrap: Optional[bool] = None, max_objects: int = 4096) -> Objects:
    """The objects of the last history entry of the variables named in `thresholds`; see the module's text for THE RULE."""
    if not isinstance(batch, Batch):
        raise TypeError(f"objects: batch must be a Batch, got {type(batch).__name__}")
    _fields.check_vector_grid("objects", batch, "batch", band="objects")
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"objects: connectivity must be 4 or 8, got {connectivity!r}")
    if wrap is not None and not isinstance(wrap, (bool, np.bool_)):
        raise ValueError(f"objects: wrap must be None, True or False, got {wrap!r}")
    if isinstance(max_objects, bool) or not isinstance(max_objects, (int, np.integer)) or max_objects < 1:
        raise ValueError(f"objects: max_objects must be a whole number of at least 1, got {max_objects!r}")
    n_lat, n_lon = batch.metadata.lat.shape[0], batch.metadata.lon.shape[0]
    if not 1 <= n_lon <= _fields.MAX_LON:
        raise ValueError(f"objects: the grid has {n_lon} longitudes; 1 to {_fields.MAX_LON} are supported")
    if n_lat < 1 or n_lat * n_lon > MAX_POINTS:
        raise ValueError(f"objects: the grid has {n_lat} x {n_lon} points; 1 to 2^31 - 2 fit an int32 label map")
    if not isinstance(thresholds, Mapping) or not thresholds:
        raise ValueError("objects: thresholds must be a non-empty mapping from variable name to values")
    names, fields, layout = _fields.select_pair("objects", batch, [], only=thresholds)
    for k in thresholds:
        if k not in names:
            raise ValueError(f"objects: thresholds name the variable {k!r}, which batch does not hold as a surface or "
                             "atmospheric variable")
    thr = _fields.threshold_table("objects", thresholds, layout)
    device = _fields.place("objects", [("batch", names, fields[0])], n_lat, n_lon, _fields.TAKES_TASK)
    lat, lon = _fields._host(batch.metadata.lat), _fields._host(batch.metadata.lon)
    wrap = full_circle(lon) if wrap is None else bool(wrap)
    below, connectivity, max_objects = bool(below), int(connectivity), int(max_objects)
    if device == "cpu":
        labels, count, table = (torch.from_numpy(x) for x in _objects_host(
            _fields.stack(fields[0], n_lat, n_lon), thr, area_units(lat), below, connectivity, wrap, max_objects))
        thr_t, lat_t, lon_t = torch.from_numpy(thr), torch.from_numpy(np.array(lat)), torch.from_numpy(np.array(lon))
    else:
        from aurora_amd.engine import lib

        thr_t = _fields.device_thresholds("objects", thr, device)
        unit = device_units(lat, device, _ON_CAPTURE)
        lat_t = _fields.tables.get(("coordinate", lat.tobytes()), device, lambda: np.array(lat), _ON_CAPTURE)
        lon_t = _fields.tables.get(("coordinate", lon.tobytes()), device, lambda: np.array(lon), _ON_CAPTURE)
        labels, count, table = lib.object_labels(fields[0], thr_t, unit, below, connectivity, wrap, max_objects)
    return Objects(labels, count, table, thr_t, lat_t, lon_t, layout, below, connectivity, wrap, max_objects)
