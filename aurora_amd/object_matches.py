"""Which forecast object is which observed object, how much do they overlap, which were missed -- and which object of step t is
which object of step t + 1: the overlap PAIR TABLE of two `Objects` on the same grid, and what follows from it (not in the
reference).  The step from `objects`, the primitive, to object-based verification: intersection over union, best match per
object, object POD / FAR / CSI, centroid displacement of matched pairs, the links of a track.

    m = aurora_amd.object_matches(a, b, max_pairs=4096)     # a, b: Objects (forecast, truth; or step t, step t + 1)
    m.pairs["ivt"]      # (B, T, max_pairs, 4) int64: ka, kb, points, area_units; (B, C, T, max_pairs, 4) for an atmospheric variable
    m.count["ivt"]      # (B[, C], T) int32: the number of pairs; -1 where the item overflows
    m.overflow, m.truncated                     # truncated = overflow | a.truncated | b.truncated
    m.intersection, m.iou, m.fraction_of_a, m.fraction_of_b, m.distance_km      # (B[, C], T, max_pairs) fp64, NaN past count
    m.best_b, m.best_b_fraction                 # (B[, C], T, a.max_objects): per a-object; -1 / NaN without a partner or past a.count
    m.best_a, m.best_a_fraction                 # (B[, C], T, b.max_objects): per b-object
    m.matched_a(min_fraction=0.0), m.matched_b(min_fraction=0.0)               # bool per object
    m.summary(min_fraction=0.0)                 # name -> variable -> (B[, C], T): n_a, n_b, n_a_matched, n_b_matched, pod, far, csi
    m.cpu()                                     # the same object with host tensors: the one call that waits for the device

THE RULE (both paths, aurora_amd/csrc/pairs_hash.h and the tests refer to this text)

 1. `a` and `b` must have the same layout (variable names and planes), the same number of thresholds T, the same (H, W),
    bit-equal `lat` and `lon`, and the same device.  `below`, `connectivity`, `wrap`, the threshold values and `max_objects` may
    differ (the percentile thresholds of two fields differ by nature).  Anything else raises; mixed devices raise.
 2. An ITEM is one plane and one threshold.  A point x of an item CONTRIBUTES where 1 <= la(x) <= a.max_objects and
    1 <= lb(x) <= b.max_objects.  Every other label value is ignored: background, negatives, and labels past the tables, which
    have no row to join to.
 3. A pair row is [ka, kb, points, area_units]: the number of contributing points with (la, lb) = (ka, kb) and the sum of
    `objects.area_units(lat)[row]` over them -- the integer units of column 1 of the object table, so that
    iou = inter / (area_a + area_b - inter) is formed from exact integers.
 4. Rows are in ascending (ka, kb) order.  `count` is their number.  Rows past `count` are zero.
 5. An item with more than `max_pairs` pairs OVERFLOWS: count = -1 and all its rows are zero -- never a partial table, whose
    contents would depend on the order of insertion.  1 <= max_pairs <= 8192.
 6. Finalisation is torch code shared by both devices, on these integers and on a.table_table / b.table_table, with no
    read-back.  Past `count` (and everywhere in an item that overflows) the fp64 properties are NaN.
      intersection    area_units / 2^32: grid points at mean latitude, as `Objects.area`
      iou             area_units / (area_a + area_b - area_units), the denominator an exact integer
      fraction_of_a   area_units / area_a;  fraction_of_b likewise
      best_b          of an a-object: the kb of its pair with the largest area_units, among equal ones the smallest kb (a scatter
                      amax, then a scatter amin over the rows that attain it); -1 without a pair or past a.count
      best_b_fraction that intersection over the a-object's own area; NaN where best_b is -1 (and where the area is 0)
      matched_a(f)    best_b_fraction > f: with f = 0 any overlap of non-zero area counts (rows at a pole carry none)
      summary(f)      with `a` the forecast and `b` the observed: n_a, n_b = the objects that have a table row
                      (min(count, max_objects)); pod = n_b_matched / n_b, far = 1 - n_a_matched / n_a,
                      csi = n_b_matched / (n_b + n_a - n_a_matched), NaN where the denominator is 0; in an item that overflows
                      the matched counts are -1 and the three scores NaN
      distance_km     the great-circle distance between the two objects' `centroid_lat` / `centroid_lon` as `Objects`
                      finalises them: `haversine_km` of aurora_amd/_sphere.py, whose sine, arcsine and square root are
                      elementwise fp64 products, sums and quotients of tensors alone (a library sin or asin may round differently
                      on the GPU than on the CPU, and torch's fp64 sqrt does), so this too has the same bits on either device;
                      they agree with the correctly rounded functions to a few ulps.

`Objects` on one GPU are matched by ONE aurora_hip_object_matches call (a bounded, lock-free hash aggregation over planes:
aurora_amd/csrc/object_matches.hip) with nothing read back; the area units come from the table that `objects` uploaded.  `Objects`
on the CPU are matched in numpy: np.unique on la.astype(int64) << 32 | lb over the contributing points, np.add.at for the units.
`pairs` and `count` agree bit for bit between the two, and so does everything finalised from them.
"""

from __future__ import annotations

import dataclasses

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._sphere import haversine_km
from aurora_amd.objects import _AREA, Objects, Result, area_units, check_pair, device_units, final_properties

__all__ = ["object_matches", "ObjectMatches", "COLUMNS", "MAX_PAIRS"]

COLUMNS = ("ka", "kb", "points", "area_units")
MAX_PAIRS = 8192
_KA, _KB, _POINTS, _UNITS = range(4)
_ON_CAPTURE = ("object_matches: call once on this grid before capturing a graph (the area units are uploaded on the first call, "
               "which a captured graph cannot replay)")


# ---- the CPU path ----------------------------------------------------------------------------------------------------------
def pairs_of(la: np.ndarray, lb: np.ndarray, unit: np.ndarray, max_objects_a: int, max_objects_b: int,
             max_pairs: int) -> tuple[np.ndarray, int]:
    """(rows (max_pairs, 4) int64, count) of one item by THE RULE: two (H, W) int32 label maps and the (H,) int64 row units."""
    rows = np.zeros((max_pairs, len(COLUMNS)), dtype=np.int64)
    W = la.shape[1]
    fa, fb = la.reshape(-1), lb.reshape(-1)
    idx = np.flatnonzero((fa >= 1) & (fa <= max_objects_a) & (fb >= 1) & (fb <= max_objects_b))
    key = (fa[idx].astype(np.int64) << 32) | fb[idx].astype(np.int64)
    keys, inverse, points = np.unique(key, return_inverse=True, return_counts=True)
    n = keys.shape[0]
    if n > max_pairs:
        return rows, -1
    units = np.zeros(n, dtype=np.int64)
    np.add.at(units, inverse.reshape(-1), unit[idx // W])
    rows[:n] = np.stack([keys >> 32, keys & 0xffffffff, points, units], axis=1)
    return rows, n


def _pairs_host(labels_a: np.ndarray, labels_b: np.ndarray, unit: np.ndarray, max_objects_a: int, max_objects_b: int,
                max_pairs: int) -> tuple[np.ndarray, np.ndarray]:
    """`pairs_of` over (*lead, H, W) stacks: pairs (*lead, max_pairs, 4) int64 and count (*lead) int32."""
    lead = labels_a.shape[:-2]
    pairs = np.zeros((*lead, max_pairs, len(COLUMNS)), dtype=np.int64)
    count = np.zeros(lead, dtype=np.int32)
    for at in np.ndindex(*lead):
        pairs[at], count[at] = pairs_of(labels_a[at], labels_b[at], unit, max_objects_a, max_objects_b, max_pairs)
    return pairs, count


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
def _best(idx: torch.Tensor, other: torch.Tensor, units: torch.Tensor, live: torch.Tensor, own_area: torch.Tensor,
          own_count: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Per object of one side (rows idx = k - 1 of its (..., M) table): the partner `other` of its pair with the most units,
    the smallest among equal ones, and that intersection over the object's own area."""
    M = own_area.shape[-1]
    none = torch.iinfo(torch.int64).max
    most = torch.full_like(own_area, -1).scatter_reduce(-1, idx, torch.where(live, units, torch.full_like(units, -1)), "amax")
    attains = live & (units == most.gather(-1, idx))
    partner = torch.full_like(own_area, none).scatter_reduce(-1, idx, torch.where(attains, other, torch.full_like(other, none)), "amin")
    has = (partner != none) & (torch.arange(M, device=idx.device) < own_count[..., None])
    fraction = torch.where(has, most.to(torch.float64) / own_area.to(torch.float64), torch.full((), float("nan"), dtype=torch.float64, device=idx.device))
    return torch.where(has, partner, torch.full_like(partner, -1)), fraction


def _finalise(pairs: torch.Tensor, count: torch.Tensor, a: Objects, b: Objects) -> dict[str, torch.Tensor]:
    """Everything of THE RULE, point 6, from the integer tables; elementwise, gathers and scatters, no read-back."""
    P = pairs.shape[-2]
    live = torch.arange(P, device=pairs.device) < count[..., None]
    real = lambda x: torch.where(live, x, torch.full_like(x, float("nan")))           # noqa: E731
    ia, ib = (pairs[..., _KA] - 1).clamp(min=0), (pairs[..., _KB] - 1).clamp(min=0)      # dead rows point at row 0, unused
    units = pairs[..., _UNITS]
    area_a, area_b = a.table_table[..., _AREA], b.table_table[..., _AREA]
    of_a, of_b = area_a.gather(-1, ia), area_b.gather(-1, ib)
    inter = units.to(torch.float64)
    fa, fb = a._final, b._final
    distance = haversine_km(fa["centroid_lat"].gather(-1, ia), fa["centroid_lon"].gather(-1, ia),
                            fb["centroid_lat"].gather(-1, ib), fb["centroid_lon"].gather(-1, ib))
    best_b, best_b_fraction = _best(ia, pairs[..., _KB], units, live, area_a, a.count_table)
    best_a, best_a_fraction = _best(ib, pairs[..., _KA], units, live, area_b, b.count_table)
    return {"intersection": real(inter / 2.0 ** 32), "iou": real(inter / (of_a + of_b - units).to(torch.float64)),
            "fraction_of_a": real(inter / of_a.to(torch.float64)), "fraction_of_b": real(inter / of_b.to(torch.float64)),
            "distance_km": real(distance), "best_b": best_b, "best_b_fraction": best_b_fraction, "best_a": best_a,
            "best_a_fraction": best_a_fraction}


@dataclasses.dataclass(eq=False)
class ObjectMatches(Result):
    """Result of `object_matches`: every property is a dict name -> tensor with the leading shape (B,) for a surface variable
    and (B, C) for an atmospheric one, on the device of the two `Objects`."""

    pairs_table: torch.Tensor                             # (n_planes, T, max_pairs, 4) int64
    count_table: torch.Tensor                             # (n_planes, T) int32
    a: Objects
    b: Objects
    max_pairs: int
    _owner = "a"

    def _finalise(self) -> dict[str, torch.Tensor]:
        return _finalise(self.pairs_table, self.count_table, self.a, self.b)

    @property
    def pairs(self) -> dict[str, torch.Tensor]:
        return self._field(self.pairs_table)

    @property
    def count(self) -> dict[str, torch.Tensor]:
        return self._field(self.count_table)

    @property
    def overflow(self) -> dict[str, torch.Tensor]:
        return self._field(self.count_table < 0)

    @property
    def truncated(self) -> dict[str, torch.Tensor]:
        return self._field((self.count_table < 0) | (self.a.count_table > self.a.max_objects) | (self.b.count_table > self.b.max_objects))

    def _matched(self, side: str, min_fraction: float) -> torch.Tensor:
        return self._final[f"best_{side}_fraction"] > float(min_fraction)              # NaN (no partner): False

    def matched_a(self, min_fraction: float = 0.0) -> dict[str, torch.Tensor]:
        """Per a-object: has it a partner whose intersection is more than `min_fraction` of its own area?"""
        return self._field(self._matched("b", min_fraction))

    def matched_b(self, min_fraction: float = 0.0) -> dict[str, torch.Tensor]:
        return self._field(self._matched("a", min_fraction))

    def summary(self, min_fraction: float = 0.0) -> dict[str, dict[str, torch.Tensor]]:
        """name -> variable -> (B[, C], T): the object counts and scores of THE RULE, `a` as forecast and `b` as observed."""
        lost = self.count_table < 0
        n_a, n_b = self.a.count_table.clamp(max=self.a.max_objects).to(torch.int64), self.b.count_table.clamp(max=self.b.max_objects).to(torch.int64)
        hit_a = torch.where(lost, torch.full_like(n_a, -1), self._matched("b", min_fraction).sum(dim=-1))
        hit_b = torch.where(lost, torch.full_like(n_b, -1), self._matched("a", min_fraction).sum(dim=-1))
        f = lambda x: x.to(torch.float64)                                                # noqa: E731
        nan = torch.full((), float("nan"), dtype=torch.float64, device=lost.device)
        score = lambda num, den: torch.where(lost, nan, _fields.ratio(f(num), f(den)))   # noqa: E731
        out = {"n_a": n_a, "n_b": n_b, "n_a_matched": hit_a, "n_b_matched": hit_b, "pod": score(hit_b, n_b),
               "far": 1.0 - score(hit_a, n_a), "csi": score(hit_b, n_b + n_a - hit_a)}
        return {k: self._field(v) for k, v in out.items()}

    def cpu(self) -> "ObjectMatches":
        """The same matches with host tensors (waits for the device)."""
        return dataclasses.replace(self, pairs_table=self.pairs_table.cpu(), count_table=self.count_table.cpu(), a=self.a.cpu(),
                                   b=self.b.cpu())


final_properties(ObjectMatches, ("intersection", "iou", "fraction_of_a", "fraction_of_b", "distance_km", "best_b", "best_b_fraction",
                                 "best_a", "best_a_fraction"), "of THE RULE, point 6; see the module's text.")


# ---- public function -----------------------------------------------------------------------------------------------------
def object_matches(a: Objects, b: Objects, max_pairs: int = 4096) -> ObjectMatches:
    """The overlap pairs of the objects of `a` and `b` and what follows from them; see the module's text for THE RULE."""
    for name, o in (("a", a), ("b", b)):
        if not isinstance(o, Objects):
            raise TypeError(f"object_matches: {name} must be an Objects (the result of aurora_amd.objects), got {type(o).__name__}")
    if isinstance(max_pairs, bool) or not isinstance(max_pairs, (int, np.integer)) or not 1 <= max_pairs <= MAX_PAIRS:
        raise ValueError(f"object_matches: max_pairs must be a whole number from 1 to {MAX_PAIRS}, got {max_pairs!r}")
    check_pair("object_matches", a, b)
    max_pairs = int(max_pairs)
    da = a.labels_table.device
    if da.type == "cpu":
        pairs, count = (torch.from_numpy(x) for x in _pairs_host(a.labels_table.numpy(), b.labels_table.numpy(),
                                                                 area_units(a.lat.numpy()), a.max_objects, b.max_objects, max_pairs))
    else:
        from aurora_amd.engine import lib

        lat = _fields._host(a.lat)                          # remembered per tensor: `objects` hands out one copy per grid
        unit = device_units(lat, da, _ON_CAPTURE)
        pairs, count = lib.object_pairs(a.labels_table, b.labels_table, unit, a.max_objects, b.max_objects, max_pairs)
    return ObjectMatches(pairs, count, a, b, max_pairs)
