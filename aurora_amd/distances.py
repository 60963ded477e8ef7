"""How far is it to the nearest storm, and how far apart are two objects that do not touch: for every grid point the great-circle
distance to the nearest EVENT of a label map and which point that is -- a feature transform on the sphere -- and, from it, the
separations of the objects of two `Objects` (not in the reference).  `object_matches` pairs objects that share grid points; a
forecast storm displaced by two of its own widths shares none.  These are the quantities that say how far off it was: MODE's
minimum boundary separation, the directed and the symmetric Hausdorff distance, "nearest observed object within 300 km".

    n = aurora_amd.nearest_event(o, max_km=None)            # o: Objects
    n.index["ivt"]      # (B, T, H, W) int32: the flat index i W + j of the nearest event, -1 for none; (B, C, T, H, W) for an atmospheric variable
    n.key["ivt"]        # the same shape, fp64: 1 - cos(angle) by THE RULE; +inf where index is -1
    n.label, n.distance_km                                  # labels gathered at index (0 for none); kilometres (NaN for none)
    n.cpu()

    s = aurora_amd.object_separations(a, b, max_km=None)    # a, b: Objects on one grid (forecast, truth)
    s.table["ivt"]      # (B[, C], T, a.max_objects, 3) int64: key_bits, a_point, b_point per object of a
    s.hausdorff_bits["ivt"]                                 # (B[, C], T) int64: the largest key over all events of a, as bits
    s.distance_km, s.nearest_b, s.a_lat, s.a_lon, s.b_lat, s.b_lon             # (B[, C], T, a.max_objects)
    s.hausdorff_km                                          # (B[, C], T): the DIRECTED Hausdorff distance from a to b
    s.matched(max_km)                                       # distance_km <= max_km, bool per object of a
    s.nearest                                               # the NearestEvent of b that the table was made from
    s.cpu()

THE RULE (both paths, aurora_amd/csrc/nearest_event_search.h and the tests refer to this text)

 1. Tables, made once on the host in numpy fp64 from the coordinates of the `Objects`: s[i] = sin(rad(lat_i)),
    c[i] = max(cos(rad(lat_i)), 0), cd[d] = cos(rad(d dlon)) for d = 0 .. W - 1 with cd[0] = 1 exactly.  dlon is the longitude step:
    360 / W on a wrapping grid (`o.wrap`), (lon[W - 1] - lon[0]) / (W - 1) otherwise.  Longitudes must be equally spaced by that
    step and latitudes strictly monotone within [-90, 90], both by THE GRID RULE of aurora_amd/_sphere.py; otherwise ValueError.
 2. An EVENT is a point with label > 0; that includes objects numbered above `max_objects`.  The GAP of columns j and j' is
    d = |j - j'|, on a wrapping grid min(d, W - d).
 3. The ROW CANDIDATE of target column j in source row k is the event of row k with the smallest gap, of two at the same gap the
    one with the smaller column.  A row without events has no candidate.
 4. key(i, k, d) = 1 - (s_i s_k + (c_i c_k) cd[d]): the products, the sum and the difference in fp64, each rounded on its own,
    never a fused multiply-add; negative results become 0.  Where the point (i, j) is itself an event its candidate in row i is
    itself and that key is exactly 0.
 5. The NEAREST EVENT of (i, j) is the row candidate with the smallest key, of equal keys the one with the smallest flat index
    k W + j'.  `index` is that flat index and `key` its key; -1 and +inf where there is no candidate.
 6. `max_km`, if given, is a positive finite number, converted once on the host to key_max = 1 - cos(min(max_km 1000 /
    EARTH_RADIUS, pi)) in fp64; candidates with key > key_max are ignored.
 7. label = labels at index, 0 for none.  distance_km = EARTH_RADIUS / 1000 * 2 asin(sqrt(key / 2)) with the `_sqrt` and `_asin`
    of aurora_amd/_sphere.py, torch code shared by both devices; NaN for none.

The nearest is defined through row candidates on purpose.  For equally spaced longitudes the candidate is the nearest point of
its row -- for two fixed rows the distance grows with the gap -- so this is the true nearest point; and it stays well defined
to the bit where rounding makes two keys of one row equal or reorders two keys an ulp apart.

 8. `object_separations(a, b, max_km)`: a and b must pass the checks of `object_matches` (layout, thresholds, grid, device,
    bit-equal coordinates).  With n = nearest_event(b, max_km), for every object k <= a.max_objects of a, over its points:
    key_bits = the smallest n.key, as the int64 of its fp64 bits (keys are not negative, so they order like their bits);
    a_point = the smallest flat index among the object's points that attain it; b_point = n.index at a_point.  Rows at or past
    min(a.count, a.max_objects) are zero.  An object with no event of b in reach (or, in a hand-made label map, a number
    without points) has the bits of +inf and -1 in both point columns.
 9. hausdorff_bits = the largest n.key over ALL events of a (objects above a.max_objects too), as bits; the bits of 0 where a has
    no event, of +inf where some event of a has no event of b in reach.
10. Finalised in torch on either device from these integers: distance_km (+inf for an object with nothing in reach, NaN past
    count), nearest_b (the label of b at b_point, 0 for none or past count), a_lat / a_lon / b_lat / b_lon (the coordinates of
    the two points, NaN for none), hausdorff_km, matched(max_km) = distance_km <= max_km.

`Objects` on one GPU take ONE aurora_hip_nearest_event call (aurora_amd/csrc/nearest_event.hip: the candidates of every row, then
an exact search in which every point walks the rows outward from its own and provably stops) and ONE
aurora_hip_object_separations call, with nothing read back; the tables are uploaded on the first call on a grid.  `Objects` on the
CPU take the same rule in numpy.  index, key, table and hausdorff_bits agree bit for bit between the two, and so does everything
finalised from them.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from aurora_amd import _fields, _sphere
from aurora_amd._sphere import EARTH_RADIUS, _km
from aurora_amd.objects import Objects, Result, check_pair, final_properties

__all__ = ["nearest_event", "NearestEvent", "object_separations", "ObjectSeparations", "COLUMNS", "MARGIN"]

COLUMNS = ("key_bits", "a_point", "b_point")
_KEY, _A, _B = range(3)
MARGIN = 2.0 ** -46          # of the stop test; derived in aurora_amd/csrc/nearest_event_search.h, which holds the same number
_INF_BITS = 0x7FF0000000000000
_ON_CAPTURE = ("nearest_event: call once on this grid before capturing a graph (the sine and cosine tables are uploaded on the "
               "first call, which a captured graph cannot replay)")


# ---- the tables and key_max ------------------------------------------------------------------------------------------------
def tables_of(lat: np.ndarray, lon: np.ndarray, wrap: bool) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(s, c, cd) of THE RULE, point 1."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    W = lon.shape[0]
    _sphere.check_latitudes("nearest_event", lat, monotonic="monotone (the row walk relies on rows farther away in index being "
                            "farther away in latitude)")
    if not 1 <= W <= _fields.MAX_LON:
        raise ValueError(f"nearest_event: the grid has {W} longitudes; 1 to {_fields.MAX_LON} are supported")
    step = 0.0
    if W > 1:
        step = 360.0 / W if wrap else float(lon[-1] - lon[0]) / (W - 1)
        if not np.all(np.isfinite(lon)) or step == 0 or not _sphere.equally_spaced(lon, step):
            how = "and cover the full circle on a wrapping grid" if wrap else "(the nearest event of a row is found by its column gap)"
            raise ValueError(f"nearest_event: the longitudes must be equally spaced {how}")
    s = np.sin(np.deg2rad(lat))
    c = np.maximum(np.cos(np.deg2rad(lat)), 0.0)
    cd = np.cos(np.deg2rad(np.arange(W, dtype=np.float64) * step))
    cd[0] = 1.0
    return s, c, cd


def key_max_of(max_km) -> float:
    """key_max of THE RULE, point 6; +inf for None."""
    if max_km is None:
        return math.inf
    if isinstance(max_km, (bool, np.bool_)) or not isinstance(max_km, (int, float, np.integer, np.floating)) \
            or not math.isfinite(max_km) or not max_km > 0:
        raise ValueError(f"nearest_event: max_km must be None or a positive finite number of kilometres, got {max_km!r}")
    return float(1.0 - np.cos(min(float(max_km) * 1000.0 / EARTH_RADIUS, math.pi)))


# ---- the CPU path ----------------------------------------------------------------------------------------------------------
def row_candidates(ev: np.ndarray, wrap: bool) -> np.ndarray:
    """(H, W) int32: the row candidate of every column in every row of an (H, W) bool event mask, -1 in a row without events."""
    H, W = ev.shape
    far = 4 * W + 4
    reps = 3 if wrap else 1
    col = np.arange(reps * W, dtype=np.int64) - (W if wrap else 0)               # columns of the unrolled row
    e = np.tile(ev, (1, reps))
    west = np.maximum.accumulate(np.where(e, col, -far), axis=1)                  # the last event at or before a column
    east = np.minimum.accumulate(np.where(e, col, far)[:, ::-1], axis=1)[:, ::-1]
    mid = slice(W, 2 * W) if wrap else slice(0, W)
    west, east, j = west[:, mid], east[:, mid], np.arange(W, dtype=np.int64)
    dw, de = j - west, east - j
    wc, ec = west % W, east % W
    cand = np.where(dw < de, wc, np.where(de < dw, ec, np.minimum(wc, ec)))
    return np.where((west > -far) | (east < far), cand, -1).astype(np.int32)


def _keys(si, ci, sk, ck, cd):
    """key of THE RULE, point 4, elementwise: numpy rounds every operation on its own."""
    m1 = si * sk
    m2 = ci * ck
    m3 = m2 * cd
    a = m1 + m3
    return np.maximum(1.0 - a, 0.0)


def nearest_of(labels: np.ndarray, s: np.ndarray, c: np.ndarray, cd: np.ndarray, wrap: bool, key_max: float = math.inf
               ) -> tuple[np.ndarray, np.ndarray]:
    """(index (H, W) int32, key (H, W) fp64) of one (H, W) label map by THE RULE.  The rows are taken by their offset from the
    target row, 0, -1, +1, -2, ..., all target rows at once; a target row leaves a direction by the stop test of
    nearest_event_search.h applied to the largest bound of its points (a visit too many changes nothing: the result is the
    minimum over all candidates)."""
    H, W = labels.shape
    cand = row_candidates(labels > 0, wrap)
    has = cand[:, 0] >= 0
    index = np.full((H, W), -1, dtype=np.int32)
    key = np.full((H, W), np.inf)
    if not has.any():
        return index, key
    cols = np.arange(W, dtype=np.int64)
    bound = np.full(H, key_max)                                                   # per target row: max over its points of min(best, key_max)
    walking = {-1: np.ones(H, dtype=bool), 1: np.ones(H, dtype=bool)}
    for r in range(H):
        for sign in ((-1,) if r == 0 else (-1, 1)):
            act = walking[sign]
            rows = np.flatnonzero(act)
            k = rows + sign * r
            inside = (k >= 0) & (k < H)
            act[rows[~inside]] = False
            rows, k = rows[inside], k[inside]
            stop = _keys(s[rows], c[rows], s[k], c[k], 1.0) - MARGIN > bound[rows]
            act[rows[stop]] = False
            keep = ~stop & has[k]
            rows, k = rows[keep], k[keep]
            if rows.size == 0:
                continue
            cnd = cand[k].astype(np.int64)
            d = np.abs(cols[None] - cnd)
            if wrap:
                d = np.minimum(d, W - d)
            kk = _keys(s[rows, None], c[rows, None], s[k, None], c[k, None], cd[d])
            if r == 0:
                kk = np.where(cnd == cols[None], 0.0, kk)
            kk = np.where(kk > key_max, np.inf, kk)
            idx = (k[:, None] * W + cnd).astype(np.int32)
            old_key, old_idx = key[rows], index[rows]
            better = (kk < old_key) | ((kk == old_key) & np.isfinite(kk) & (idx < old_idx))
            key[rows], index[rows] = np.where(better, kk, old_key), np.where(better, idx, old_idx)
            bound[rows] = np.minimum(key[rows].max(axis=1), key_max)
        if not walking[-1].any() and not walking[1].any():
            break
    return index, key


def _nearest_host(labels: np.ndarray, s, c, cd, wrap: bool, key_max: float) -> tuple[np.ndarray, np.ndarray]:
    """`nearest_of` over (*lead, H, W) stacks."""
    index, key = np.empty(labels.shape, dtype=np.int32), np.empty(labels.shape, dtype=np.float64)
    for at in np.ndindex(*labels.shape[:-2]):
        index[at], key[at] = nearest_of(labels[at], s, c, cd, wrap, key_max)
    return index, key


def separations_of(la: np.ndarray, key: np.ndarray, index: np.ndarray, count: int, max_objects: int) -> tuple[np.ndarray, int]:
    """(rows (max_objects, 3) int64, hausdorff bits) of one item by THE RULE, points 8 and 9."""
    rows = np.zeros((max_objects, len(COLUMNS)), dtype=np.int64)
    fa, bits, fi = la.reshape(-1), np.ascontiguousarray(key).reshape(-1).view(np.int64), index.reshape(-1)
    hausdorff = int(bits[fa > 0].max(initial=0))
    n = min(int(count), max_objects)
    if n <= 0:
        return rows, hausdorff
    at = np.flatnonzero((fa >= 1) & (fa <= max_objects)).astype(np.int64)
    k = fa[at].astype(np.int64) - 1
    least = np.full(max_objects, _INF_BITS, dtype=np.int64)
    np.minimum.at(least, k, bits[at])
    attains = (bits[at] == least[k]) & (bits[at] != _INF_BITS)
    first = np.full(max_objects, np.iinfo(np.int64).max)
    np.minimum.at(first, k[attains], at[attains])
    found = first != np.iinfo(np.int64).max
    a_point = np.where(found, first, -1)
    b_point = np.where(found, fi[np.where(found, first, 0)].astype(np.int64), -1)
    rows[:n] = np.stack([np.where(found, least, _INF_BITS), a_point, b_point], axis=1)[:n]
    return rows, hausdorff


def _separations_host(la: np.ndarray, key: np.ndarray, index: np.ndarray, count: np.ndarray, max_objects: int
                      ) -> tuple[np.ndarray, np.ndarray]:
    lead = la.shape[:-2]
    table = np.zeros((*lead, max_objects, len(COLUMNS)), dtype=np.int64)
    hausdorff = np.zeros(lead, dtype=np.int64)
    for at in np.ndindex(*lead):
        table[at], hausdorff[at] = separations_of(la[at], key[at], index[at], int(count[at]), max_objects)
    return table, hausdorff


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
def _gather_points(values: torch.Tensor, point: torch.Tensor) -> torch.Tensor:
    """values (*lead, H, W) at the flat indices point (*lead, M); where point is -1, at 0 (the caller masks)."""
    return values.reshape(*values.shape[:-2], -1).gather(-1, point.clamp(min=0).to(torch.int64))


@dataclasses.dataclass(eq=False)
class NearestEvent(Result):
    """Result of `nearest_event`: every property is a dict name -> tensor with the leading shape (B,) for a surface variable and
    (B, C) for an atmospheric one, on the device of the `Objects`."""

    index_table: torch.Tensor                             # (n_planes, T, H, W) int32
    key_table: torch.Tensor                               # (n_planes, T, H, W) fp64
    objects: Objects
    max_km: Optional[float]
    _owner = "objects"

    def _finalise(self) -> dict[str, torch.Tensor]:
        none = self.index_table < 0
        flat = self.index_table.reshape(*self.index_table.shape[:-2], -1)
        label = _gather_points(self.objects.labels_table, flat).reshape(self.index_table.shape)
        km = _km(self.key_table)
        return {"label": torch.where(none, torch.zeros_like(label), label),
                "distance_km": torch.where(none, torch.full_like(km, float("nan")), km)}

    @property
    def index(self) -> dict[str, torch.Tensor]:
        return self._field(self.index_table)

    @property
    def key(self) -> dict[str, torch.Tensor]:
        return self._field(self.key_table)

    @property
    def label(self) -> dict[str, torch.Tensor]:
        """The label of the nearest event (THE RULE, point 7), int32, 0 for none."""
        return self._field(self._final["label"])

    @property
    def distance_km(self) -> dict[str, torch.Tensor]:
        """The great-circle distance to the nearest event in kilometres (THE RULE, point 7), NaN for none."""
        return self._field(self._final["distance_km"])

    def cpu(self) -> "NearestEvent":
        """The same result with host tensors (waits for the device)."""
        return dataclasses.replace(self, index_table=self.index_table.cpu(), key_table=self.key_table.cpu(), objects=self.objects.cpu())


def _finalise(table: torch.Tensor, hausdorff: torch.Tensor, a: Objects, b: Objects) -> dict[str, torch.Tensor]:
    """THE RULE, point 10, from the integer tables; elementwise and gathers, no read-back."""
    M, W = table.shape[-2], a.lon.shape[0]
    live = torch.arange(M, device=table.device) < a.count_table[..., None]
    a_point, b_point = table[..., _A], table[..., _B]
    some = live & (b_point >= 0)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=table.device)
    where = lambda p, coord, per: torch.where(some, coord[(p.clamp(min=0) // W) if per == "row" else (p.clamp(min=0) % W)], nan)  # noqa: E731
    key = table[..., _KEY].contiguous().view(torch.float64)
    nearest_b = _gather_points(b.labels_table, b_point)
    return {"distance_km": torch.where(live, _km(key), nan),
            "nearest_b": torch.where(some, nearest_b, torch.zeros_like(nearest_b)),
            "a_lat": where(a_point, a.lat, "row"), "a_lon": where(a_point, a.lon, "col"),
            "b_lat": where(b_point, a.lat, "row"), "b_lon": where(b_point, a.lon, "col"),
            "hausdorff_km": _km(hausdorff.view(torch.float64))}


@dataclasses.dataclass(eq=False)
class ObjectSeparations(Result):
    """Result of `object_separations`: every property is a dict name -> tensor with the leading shape (B,) for a surface
    variable and (B, C) for an atmospheric one, on the device of the two `Objects`."""

    table_table: torch.Tensor                             # (n_planes, T, a.max_objects, 3) int64
    hausdorff_table: torch.Tensor                         # (n_planes, T) int64
    a: Objects
    b: Objects
    nearest: NearestEvent                                 # of b
    max_km: Optional[float]
    _owner = "a"

    def _finalise(self) -> dict[str, torch.Tensor]:
        return _finalise(self.table_table, self.hausdorff_table, self.a, self.b)

    @property
    def table(self) -> dict[str, torch.Tensor]:
        return self._field(self.table_table)

    @property
    def hausdorff_bits(self) -> dict[str, torch.Tensor]:
        return self._field(self.hausdorff_table)

    def matched(self, max_km: float) -> dict[str, torch.Tensor]:
        """Per object of a: is an event of b within `max_km` kilometres of it (distance_km <= max_km)?  With 0.0: do they touch."""
        return self._field(self._final["distance_km"] <= float(max_km))       # NaN (past count): False

    def cpu(self) -> "ObjectSeparations":
        """The same separations with host tensors (waits for the device)."""
        nearest = self.nearest.cpu()
        return dataclasses.replace(self, table_table=self.table_table.cpu(), hausdorff_table=self.hausdorff_table.cpu(), a=self.a.cpu(),
                                   b=nearest.objects, nearest=nearest)


final_properties(ObjectSeparations, ("distance_km", "nearest_b", "a_lat", "a_lon", "b_lat", "b_lon", "hausdorff_km"),
                 "of THE RULE, point 10; see the module's text.")


# ---- public functions ------------------------------------------------------------------------------------------------------
def _device_tables(o: Objects, device) -> torch.Tensor:
    lat, lon = _fields._host(o.lat), _fields._host(o.lon)   # remembered per tensor: `objects` hands out one copy per grid
    return _fields.tables.get(("nearest event tables", lat.tobytes(), lon.tobytes(), bool(o.wrap)), device,
                              lambda: np.concatenate(tables_of(lat, lon, o.wrap)), _ON_CAPTURE)


def nearest_event(o: Objects, max_km: Optional[float] = None) -> NearestEvent:
    """For every grid point the nearest point with `labels > 0` of its plane and threshold, and 1 - cos of the angle between
    them; see the module's text for THE RULE.  `max_km`: events farther away than that are ignored."""
    if not isinstance(o, Objects):
        raise TypeError(f"nearest_event: o must be an Objects (the result of aurora_amd.objects), got {type(o).__name__}")
    key_max = key_max_of(max_km)
    device = o.labels_table.device
    if device.type == "cpu":
        tables = tables_of(o.lat.numpy(), o.lon.numpy(), o.wrap)
        index, key = (torch.from_numpy(x) for x in _nearest_host(o.labels_table.numpy(), *tables, bool(o.wrap), key_max))
    else:
        from aurora_amd.engine import lib

        if not 1 <= o.lon.shape[0] <= _fields.MAX_LON:
            raise ValueError(f"nearest_event: the grid has {o.lon.shape[0]} longitudes; 1 to {_fields.MAX_LON} are supported")
        index, key = lib.nearest_event_maps(o.labels_table, _device_tables(o, device), bool(o.wrap), key_max)
    return NearestEvent(index, key, o, None if max_km is None else float(max_km))


def object_separations(a: Objects, b: Objects, max_km: Optional[float] = None) -> ObjectSeparations:
    """How far every object of `a` is from the nearest event of `b`, between which two points, and the directed Hausdorff
    distance from a to b; see the module's text for THE RULE.

    The SYMMETRIC Hausdorff distance is max(object_separations(a, b).hausdorff_km, object_separations(b, a).hausdorff_km).
    Two objects that overlap have a distance of exactly 0, so for objects that have table rows on both sides
    `matched(0.0)` equals `object_matches(a, b).matched_a()` (which also asks for an overlap of non-zero area: rows at a pole
    carry none, and all points of a pole row are one point of the sphere)."""
    for name, o in (("a", a), ("b", b)):
        if not isinstance(o, Objects):
            raise TypeError(f"object_separations: {name} must be an Objects (the result of aurora_amd.objects), got {type(o).__name__}")
    check_pair("object_separations", a, b)
    n = nearest_event(b, max_km)
    if a.labels_table.device.type == "cpu":
        table, hausdorff = (torch.from_numpy(x) for x in _separations_host(
            a.labels_table.numpy(), n.key_table.numpy(), n.index_table.numpy(), a.count_table.numpy(), a.max_objects))
    else:
        from aurora_amd.engine import lib

        table, hausdorff = lib.object_separation_table(a.labels_table, n.key_table, n.index_table, a.count_table, a.max_objects)
    return ObjectSeparations(table, hausdorff, a, b, n, n.max_km)
