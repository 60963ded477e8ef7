"""Which storm of step t is which storm of step t + 1, where did each one go, how long did it live (not in the reference): the
candidates of two `extrema` results are linked by an all-pairs nearest search on the sphere -- the StitchNodes half of
DetectNodes / StitchNodes -- on the device, for every plane of a batch at once, and `tracks` numbers the chains of links over
the steps of a roll-out, where `Tracker` follows one known low on the host.

    lows = [aurora_amd.extrema(aurora_amd.smooth(p, 100.0), 300.0, only=["msl"]) for p in predictions]
    keep = [{"msl": aurora_amd.closed_contours(e, {"msl": [200.0]}, 600.0).closed["msl"][:, 0]} for e in lows]
    l = aurora_amd.link_extrema(lows[0], lows[1], 500.0, keep_a=keep[0], keep_b=keep[1])
    l.forward["msl"]       # (B, Ma, 2) int64 on the device of the tables: key_bits, row of b; (B, C, Ma, 2) for an atmospheric variable
    l.backward["msl"]      # (B, Mb, 2) int64: key_bits, row of a
    l.next["msl"]          # (B, Ma) int64: the row of b that a row of a is MUTUALLY linked to, -1 for none; l.prev: (B, Mb)
    l.distance_km["msl"]   # (B, Ma) fp64: the length of that link in kilometres, NaN for none
    l.nearest_next, l.nearest_prev          # the raw rows of forward and backward
    l.ends, l.starts       # (B, Ma) / (B, Mb) bool: a live row of a without next / a live row of b without prev
    l.live_a, l.live_b     # the live rows of the two sides
    l.cpu()                # the same object with host tensors: the one call that waits for the device

    t = aurora_amd.tracks(lows, 500.0, keep=keep)
    t.track_id["msl"]      # (S, B, M) int32: the number of the track a node belongs to, -1 where the row is not live
    t.n_tracks["msl"]      # (B,) int32
    t.length, t.first_step                  # (S, B, M) int32: the nodes of the node's track, the step of its first node
    t.value, t.lat, t.lon, t.row, t.col     # (S, B, M): those of the steps, stacked
    t.links                # the S - 1 `Links`
    t.cpu().tracks_of("msl", b=0, min_length=3)      # a list of dicts of numpy arrays, one per track, in id order

`a` and `b` are `Extrema` of two steps (or of forecast and truth) with the same `layout` (names and plane shapes), `kind`,
`wrap`, bit-equal `grid_lat` / `grid_lon` and device; `radius_km` and `max_points` may differ (Ma and Mb).  `max_km` is
required: a positive finite number of kilometres.  `keep_a` / `keep_b` is None or a dict variable name -> bool tensor of shape
(B[, C], max_points) on the tables' device, typically one delta's slice of `ClosedContours.closed`; a name that is not in the
dict keeps all of its rows.

THE RULE (both paths, include/aurora_hip.h and the tests refer to this text)

 1. (s, c, cd) = `distances.tables_of(lat, lon, wrap)`.  The point of table row r is (i, j) = divmod(table[r, 0], W); a flat
    index outside the grid (no `extrema` writes one) is clamped into it.
 2. Row r of a side is LIVE where r < min(count, max_points) and its keep bit is set.
 3. For two points with the same flat index key(p, q) = 0 exactly.  Otherwise key(p, q) = key_of(s[ia], c[ia], s[ib], c[ib],
    cd[gap(ja, jb)]): point 4 of the rule of aurora_amd/distances.py with the gap of its point 2, 1 - (s s' + (c c') cd[gap]),
    every fp64 operation rounded on its own, never a fused multiply-add, negative results 0.  The expression is symmetric in
    its two points bit for bit (products and the gap commute).
 4. key_max = `distances.key_max_of(max_km)`.  forward[p] is the live q with the smallest (key, q) among keys <= key_max;
    backward[q] is the live p with the smallest (key, p).
 5. The outputs are forward (n_planes, Ma, 2) and backward (n_planes, Mb, 2), int64 with the columns key_bits -- the bits of the
    fp64 key -- and row.  A row that is not live holds the bits of +inf and -1; a live row with nothing in reach the same.
 6. Finalised in torch from these integers, with the same bits on either device: next (..., Ma) = the forward row where
    backward[forward[p]] == p, a MUTUAL link, else -1; prev (..., Mb) the same in the other direction; distance_km of the mutual
    link by `_sphere._km`, NaN for none; nearest_next / nearest_prev the raw rows; ends = live a without next; starts = live b
    without prev.

Tables on one GPU take ONE aurora_hip_link_extrema call (aurora_amd/csrc/links.hip, links_scan.h: a thread owns one row and
scans the other side, staged through LDS in tiles of gathered points, with cd in LDS); nothing is read back, and (s, c, cd) on
the device are the tables `nearest_event` uploads for the same grid, on the first call.  Tables on the CPU take the same rule
in numpy, the key matrix in blocks of rows.  forward and backward agree in every byte between the two, and so does everything
finalised from them.  The call is capturable in a hipGraph after one eager call on the grid; during capture `a` and `b` must hold
the SAME coordinate tensors (those of `extrema` on one grid and device are), since comparing two tensors would wait for the device.

`tracks(steps, max_km, keep=None)`: 2 to 256 `Extrema`, pairwise compatible as above and with EQUAL max_points M; `keep` is None
or a sequence of the same length of dicts as above (or None).  Consecutive steps are linked by `link_extrema`; a track is a chain
of mutual links.  Per plane, tracks are numbered from 0 in the order (step, row) of their first node: at step 0
id = cumsum(live) - 1; at step t + 1 id[q] = id_t[prev[q]] where prev[q] >= 0, else n_t + the rank of q among the live rows
without prev, in row order, n_t being the number of tracks started up to step t; a row that is not live has -1.  It is torch
code alone, the same on either device with the same bits, and reads nothing back; `length` is formed by a scatter_add over
M S slots a plane.

Not offered: bridging a missing step (gaps: a track ends where a step has no mutual partner), speed or direction criteria,
merging and splitting (a link is one to one), `BandBatch`.
"""

from __future__ import annotations

import dataclasses
import math
import types
from typing import Mapping, Optional, Sequence

import numpy as np
import torch

from aurora_amd import distances
from aurora_amd._sphere import _km
from aurora_amd.distances import _keys
from aurora_amd.extrema import Extrema
from aurora_amd.objects import Result, _same_values, final_properties

__all__ = ["link_extrema", "Links", "tracks", "Tracks", "COLUMNS", "MAX_STEPS"]

COLUMNS = ("key_bits", "row")
MAX_STEPS = 256
_INF_BITS = 0x7FF0000000000000
_BLOCK_BYTES = 32 << 20          # of one fp64 block of the key matrix on the host: 1024 rows at 4096 partners


# ---- the checks ------------------------------------------------------------------------------------------------------------
def check_pair(fn: str, a: Extrema, b: Extrema, na: str = "a", nb: str = "b") -> None:
    """`a` and `b` have the same layout, kind, wrap, grid and device, and bit-equal coordinates."""
    if a.layout != b.layout:
        raise ValueError(f"{fn}: {na} and {nb} differ in layout (variable, first plane, shape): {a.layout} against {b.layout}")
    if a.kind != b.kind:
        raise ValueError(f"{fn}: {na} and {nb} differ in kind: {a.kind!r} against {b.kind!r}")
    if bool(a.wrap) != bool(b.wrap):
        raise ValueError(f"{fn}: {na} and {nb} differ in wrap: {a.wrap} against {b.wrap}")
    ga, gb = (a.grid_lat.shape[0], a.grid_lon.shape[0]), (b.grid_lat.shape[0], b.grid_lon.shape[0])
    if ga != gb:
        raise ValueError(f"{fn}: {na} and {nb} differ in grid: {ga[0]} x {ga[1]} against {gb[0]} x {gb[1]} points; regrid first")
    da, db = a.table_table.device, b.table_table.device
    if da != db:
        raise ValueError(f"{fn}: {na} is on {da} and {nb} on {db}; move both to the CPU (.cpu()) or find both on one GPU")
    for c in ("grid_lat", "grid_lon"):
        if not _same_values(getattr(a, c), getattr(b, c)):
            raise ValueError(f"{fn}: {na} and {nb} differ in {c} (same length, different values); regrid first")


def _keep_table(fn: str, what: str, keep, e: Extrema) -> Optional[torch.Tensor]:
    """(n_planes, max_points) bool on the device of `e` from the dict of `keep`, or None where every row is kept."""
    if keep is None:
        return None
    if not isinstance(keep, Mapping):
        raise TypeError(f"{fn}: {what} must be None or a dict from variable name to a bool tensor, got {type(keep).__name__}")
    held = {name: (first, shape) for name, first, shape in e.layout}
    for k in keep:
        if k not in held:
            raise ValueError(f"{fn}: {what} names the variable {k!r}, which the extrema do not hold; their variables are {tuple(held)}")
    if not keep:
        return None
    dev, M = e.table_table.device, e.max_points
    out = torch.ones((e.table_table.shape[0], M), dtype=torch.bool, device=dev)
    for name, t in keep.items():
        first, shape = held[name]
        if not isinstance(t, torch.Tensor) or t.dtype != torch.bool:
            raise TypeError(f"{fn}: {what}[{name!r}] must be a bool tensor, got "
                            f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if tuple(t.shape) != (*shape, M):
            raise ValueError(f"{fn}: {what}[{name!r}] has shape {tuple(t.shape)}, not {(*shape, M)} (the variable's planes x max_points)")
        if t.device != dev:
            raise ValueError(f"{fn}: {what}[{name!r}] is on {t.device} and the tables on {dev}")
        out[first:first + math.prod(shape)] = t.reshape(-1, M)
    return out


def _live(e: Extrema, keep: Optional[torch.Tensor]) -> torch.Tensor:
    """THE RULE, point 2: (n_planes, max_points) bool."""
    live = torch.arange(e.max_points, device=e.table_table.device) < e.count_table[:, None]
    return live if keep is None else live & keep


# ---- the rule on the host ---------------------------------------------------------------------------------------------------
def _nearest_rows(fa: np.ndarray, la: np.ndarray, fb: np.ndarray, lb: np.ndarray, s, c, cd, W: int, wrap: bool, key_max: float
                  ) -> np.ndarray:
    """(len(fa), 2) int64 by THE RULE, points 3 to 5: for every row of flat indices `fa` (live where `la`) the live row of `fb`
    with the smallest (key, row).  The key matrix is formed in blocks of rows of a."""
    out = np.empty((fa.shape[0], len(COLUMNS)), dtype=np.int64)
    out[:, 0], out[:, 1] = _INF_BITS, -1
    rows, cols = np.flatnonzero(la), np.flatnonzero(lb)
    if rows.size == 0 or cols.size == 0:
        return out
    ib, jb = np.divmod(fb[cols], W)
    sb, cb = s[ib], c[ib]
    block = max(1, _BLOCK_BYTES // (8 * cols.size))
    for first in range(0, rows.size, block):
        r = rows[first:first + block]
        ia, ja = np.divmod(fa[r], W)
        gap = np.abs(ja[:, None] - jb[None, :])
        if wrap:
            gap = np.minimum(gap, W - gap)
        key = _keys(s[ia][:, None], c[ia][:, None], sb[None, :], cb[None, :], cd[gap])
        key[fa[r][:, None] == fb[cols][None, :]] = 0.0
        key[key > key_max] = np.inf
        at = key.argmin(axis=1)                                  # the first of equal keys: the smallest row
        best = key[np.arange(r.size), at]
        found = np.isfinite(best)
        out[r[found], 0] = best[found].view(np.int64)
        out[r[found], 1] = cols[at[found]]
    return out


def _links_host(table_a, count_a, keep_a, table_b, count_b, keep_b, s, c, cd, n_lat: int, n_lon: int, wrap: bool, key_max: float
                ) -> tuple[np.ndarray, np.ndarray]:
    """forward (n, Ma, 2) and backward (n, Mb, 2) int64 by THE RULE."""
    n, ma, mb = table_a.shape[0], table_a.shape[1], table_b.shape[1]
    forward = np.empty((n, ma, len(COLUMNS)), dtype=np.int64)
    backward = np.empty((n, mb, len(COLUMNS)), dtype=np.int64)
    last = n_lat * n_lon - 1
    for p in range(n):
        fa, fb = np.clip(table_a[p, :, 0], 0, last), np.clip(table_b[p, :, 0], 0, last)
        la = np.arange(ma) < min(max(int(count_a[p]), 0), ma)
        lb = np.arange(mb) < min(max(int(count_b[p]), 0), mb)
        if keep_a is not None:
            la &= keep_a[p]
        if keep_b is not None:
            lb &= keep_b[p]
        forward[p] = _nearest_rows(fa, la, fb, lb, s, c, cd, n_lon, wrap, key_max)
        backward[p] = _nearest_rows(fb, lb, fa, la, s, c, cd, n_lon, wrap, key_max)
    return forward, backward


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
def _mutual(there: torch.Tensor, back: torch.Tensor) -> torch.Tensor:
    """The row of `there` (n, M) where the row of `back` (n, M') at it points back, else -1."""
    rows = torch.arange(there.shape[-1], device=there.device)
    returned = back.gather(-1, there.clamp(min=0))
    return torch.where((there >= 0) & (returned == rows), there, torch.full_like(there, -1))


def _finalise(forward: torch.Tensor, backward: torch.Tensor, live_a: torch.Tensor, live_b: torch.Tensor) -> dict[str, torch.Tensor]:
    """THE RULE, point 6, from the integer tables; elementwise and gathers, no read-back."""
    nearest_next, nearest_prev = forward[..., 1], backward[..., 1]
    nxt, prv = _mutual(nearest_next, nearest_prev), _mutual(nearest_prev, nearest_next)
    km = _km(forward[..., 0].contiguous().view(torch.float64))
    return {"next": nxt, "prev": prv, "nearest_next": nearest_next, "nearest_prev": nearest_prev,
            "distance_km": torch.where(nxt >= 0, km, torch.full_like(km, float("nan"))),
            "ends": live_a & (nxt < 0), "starts": live_b & (prv < 0), "live_a": live_a, "live_b": live_b}


@dataclasses.dataclass(eq=False)
class Links(Result):
    """Result of `link_extrema`: every property is a dict name -> tensor with the leading shape (B,) for a surface variable and
    (B, C) for an atmospheric one, on the device of the two `Extrema`."""

    forward_table: torch.Tensor                            # (n_planes, Ma, 2) int64
    backward_table: torch.Tensor                           # (n_planes, Mb, 2) int64
    live_a_table: torch.Tensor                             # (n_planes, Ma) bool
    live_b_table: torch.Tensor                             # (n_planes, Mb) bool
    a: Extrema
    b: Extrema
    max_km: float
    _owner = "a"

    def _finalise(self) -> dict[str, torch.Tensor]:
        return _finalise(self.forward_table, self.backward_table, self.live_a_table, self.live_b_table)

    @property
    def forward(self) -> dict[str, torch.Tensor]:
        return self._field(self.forward_table)

    @property
    def backward(self) -> dict[str, torch.Tensor]:
        return self._field(self.backward_table)

    def cpu(self) -> "Links":
        """The same links with host tensors (waits for the device)."""
        moved = {f: getattr(self, f).cpu() for f in ("forward_table", "backward_table", "live_a_table", "live_b_table")}
        return dataclasses.replace(self, a=self.a.cpu(), b=self.b.cpu(), **moved)


final_properties(Links, ("next", "prev", "nearest_next", "nearest_prev", "distance_km", "ends", "starts", "live_a", "live_b"),
                 "of THE RULE, point 6; see the module's text.")


# ---- public functions ------------------------------------------------------------------------------------------------------
def link_extrema(a: Extrema, b: Extrema, max_km: float, *, keep_a=None, keep_b=None) -> Links:
    """For every candidate of `a` the nearest candidate of `b` within `max_km` kilometres, and the reverse; see the module's
    text for THE RULE."""
    for name, e in (("a", a), ("b", b)):
        if not isinstance(e, Extrema):
            raise TypeError(f"link_extrema: {name} must be an Extrema (the result of aurora_amd.extrema), got {type(e).__name__}")
    check_pair("link_extrema", a, b)
    if max_km is None:
        raise ValueError("link_extrema: max_km is required: a positive finite number of kilometres, got None")
    try:
        key_max = distances.key_max_of(max_km)
    except ValueError:
        raise ValueError(f"link_extrema: max_km must be a positive finite number of kilometres, got {max_km!r}") from None
    ka, kb = _keep_table("link_extrema", "keep_a", keep_a, a), _keep_table("link_extrema", "keep_b", keep_b, b)
    n_lat, n_lon, wrap = a.grid_lat.shape[0], a.grid_lon.shape[0], bool(a.wrap)
    device = a.table_table.device
    grid = types.SimpleNamespace(lat=a.grid_lat, lon=a.grid_lon, wrap=wrap)          # (what `distances` reads of an `Objects`)
    try:                                                                             # (a grid that `tables_of` refuses, on either device)
        tables = distances.tables_of(a.grid_lat.numpy(), a.grid_lon.numpy(), wrap) if device.type == "cpu" else \
            distances._device_tables(grid, device)
    except ValueError as e:
        raise ValueError(str(e).replace("nearest_event:", "link_extrema:", 1)) from None
    if device.type == "cpu":
        forward, backward = (torch.from_numpy(x) for x in _links_host(
            a.table_table.numpy(), a.count_table.numpy(), None if ka is None else ka.numpy(),
            b.table_table.numpy(), b.count_table.numpy(), None if kb is None else kb.numpy(), *tables, n_lat, n_lon, wrap, key_max))
    else:
        from aurora_amd.engine import lib

        forward, backward = lib.link_extrema_tables(a.table_table.contiguous(), a.count_table.contiguous(), ka,
                                                    b.table_table.contiguous(), b.count_table.contiguous(), kb,
                                                    tables, n_lat, n_lon, wrap, key_max)
    return Links(forward, backward, _live(a, ka), _live(b, kb), a, b, float(max_km))


@dataclasses.dataclass(eq=False)
class Tracks(Result):
    """Result of `tracks`: every property is a dict name -> tensor with the leading shape (S, B) for a surface variable and
    (S, B, C) for an atmospheric one (`n_tracks`: (B[, C])), on the device of the steps."""

    track_id_table: torch.Tensor                           # (n_planes, S, M) int32
    n_tracks_table: torch.Tensor                           # (n_planes,) int32
    length_table: torch.Tensor                             # (n_planes, S, M) int32
    first_step_table: torch.Tensor                         # (n_planes, S, M) int32
    steps: tuple                                           # the S `Extrema`
    links: tuple                                           # the S - 1 `Links`
    max_km: float

    @property
    def layout(self):
        return self.steps[0].layout

    def _by_step(self, t: torch.Tensor) -> dict[str, torch.Tensor]:
        """(n_planes, S, ...) -> name -> (S, *shape, ...)."""
        return {name: v.movedim(v.dim() - t.dim() + 1, 0) for name, v in self._field(t).items()}

    def _finalise(self) -> dict[str, torch.Tensor]:
        return {name: torch.stack([e._final[name] for e in self.steps], dim=1) for name in ("value", "lat", "lon", "row", "col")}

    @property
    def track_id(self) -> dict[str, torch.Tensor]:
        return self._by_step(self.track_id_table)

    @property
    def n_tracks(self) -> dict[str, torch.Tensor]:
        return self._field(self.n_tracks_table)

    @property
    def length(self) -> dict[str, torch.Tensor]:
        return self._by_step(self.length_table)

    @property
    def first_step(self) -> dict[str, torch.Tensor]:
        return self._by_step(self.first_step_table)

    def cpu(self) -> "Tracks":
        """The same tracks with host tensors (waits for the device)."""
        steps = tuple(e.cpu() for e in self.steps)                  # every step once: links[t].b IS links[t + 1].a
        tables = ("forward_table", "backward_table", "live_a_table", "live_b_table")
        links = tuple(dataclasses.replace(l, a=steps[t], b=steps[t + 1], **{f: getattr(l, f).cpu() for f in tables})
                      for t, l in enumerate(self.links))
        moved = {f: getattr(self, f).cpu() for f in ("track_id_table", "n_tracks_table", "length_table", "first_step_table")}
        return dataclasses.replace(self, steps=steps, links=links, **moved)

    def tracks_of(self, name: str, b: int = 0, c: Optional[int] = None, min_length: int = 1) -> list[dict[str, np.ndarray]]:
        """The tracks of one plane of a `.cpu()`ed result with at least `min_length` nodes, in id order: per track a dict of numpy
        arrays over its nodes -- step, row, lat, lon, value, and distance_km, the length of the link that led to the node (NaN
        for the first)."""
        if self.track_id_table.device.type != "cpu":
            raise ValueError("tracks_of: the result is on a device; call .cpu() first (the one call that waits for it)")
        held = {n: (first, shape) for n, first, shape in self.layout}
        if name not in held:
            raise ValueError(f"tracks_of: no variable {name!r}; the variables are {tuple(held)}")
        first, shape = held[name]
        at = (b,) if len(shape) == 1 else (b, c)
        if len(shape) == 2 and c is None:
            raise ValueError(f"tracks_of: {name!r} is an atmospheric variable; name its level with c")
        if len(shape) == 1 and c is not None:
            raise ValueError(f"tracks_of: {name!r} is a surface variable and has no level c")
        if not all(isinstance(i, (int, np.integer)) and 0 <= i < n for i, n in zip(at, shape)):
            raise ValueError(f"tracks_of: {name!r} has the planes {tuple(shape)}, got {at}")
        plane = first + int(np.ravel_multi_index(at, shape))
        ids = self.track_id_table[plane].numpy()                                     # (S, M)
        S, M = ids.shape
        final = {k: v[plane].numpy() for k, v in self._final.items()}
        km = np.full((S, M), np.nan)
        for t, l in enumerate(self.links):                                           # the link that arrives at (t + 1, q)
            prev = l._final["prev"][plane].numpy()
            dist = l._final["distance_km"][plane].numpy()
            km[t + 1] = np.where(prev >= 0, dist[np.maximum(prev, 0)], np.nan)
        step, row = np.nonzero(ids >= 0)                                             # in (step, row) order
        order = np.argsort(ids[step, row], kind="stable")
        step, row = step[order], row[order]
        cuts = np.flatnonzero(np.diff(ids[step, row])) + 1
        out = []
        for s_, r_ in zip(np.split(step, cuts), np.split(row, cuts)):
            if s_.size >= max(int(min_length), 1):
                out.append({"step": s_, "row": r_, "lat": final["lat"][s_, r_], "lon": final["lon"][s_, r_],
                            "value": final["value"][s_, r_], "distance_km": km[s_, r_]})
        return out


for _name in ("value", "lat", "lon", "row", "col"):
    setattr(Tracks, _name, property(lambda self, _n=_name: self._by_step(self._final[_n]),
                                    doc=f"`{_name}` of every node: that of the steps, stacked; see the module's text."))


def tracks(steps: Sequence[Extrema], max_km: float, *, keep: Optional[Sequence] = None) -> Tracks:
    """The tracks through the candidates of 2 to 256 steps: consecutive steps linked by `link_extrema`, the chains of mutual
    links numbered per plane; see the module's text."""
    if isinstance(steps, Extrema) or not isinstance(steps, Sequence):
        raise TypeError(f"tracks: steps must be a sequence of Extrema, got {type(steps).__name__}")
    steps = tuple(steps)
    if not 2 <= len(steps) <= MAX_STEPS:
        raise ValueError(f"tracks: 2 to {MAX_STEPS} steps are linked, got {len(steps)}")
    for t, e in enumerate(steps):
        if not isinstance(e, Extrema):
            raise TypeError(f"tracks: steps[{t}] must be an Extrema (the result of aurora_amd.extrema), got {type(e).__name__}")
    for t, e in enumerate(steps[1:], 1):
        check_pair("tracks", steps[0], e, "steps[0]", f"steps[{t}]")
        if e.max_points != steps[0].max_points:
            raise ValueError(f"tracks: steps[0] and steps[{t}] differ in max_points: {steps[0].max_points} against {e.max_points}")
    if keep is None:
        keep = (None,) * len(steps)
    elif isinstance(keep, Mapping) or not isinstance(keep, Sequence):
        raise TypeError(f"tracks: keep must be None or a sequence of one dict (or None) per step, got {type(keep).__name__}")
    elif len(keep) != len(steps):
        raise ValueError(f"tracks: keep holds {len(keep)} entries for {len(steps)} steps")
    links = tuple(link_extrema(steps[t], steps[t + 1], max_km, keep_a=keep[t], keep_b=keep[t + 1]) for t in range(len(steps) - 1))

    S, M = len(steps), steps[0].max_points
    none = torch.full((), -1, dtype=torch.int64, device=links[0].forward_table.device)
    live = links[0].live_a_table
    ids = [torch.where(live, live.cumsum(-1) - 1, none)]
    firsts = [torch.where(live, torch.zeros_like(none), none)]
    n = live.sum(-1, keepdim=True)                                                   # (n_planes, 1): stays on the device
    for t, l in enumerate(links):
        prev, live = l._final["prev"], l.live_b_table
        has, new = prev >= 0, l._final["starts"]
        at = prev.clamp(min=0)
        ids.append(torch.where(has, ids[-1].gather(-1, at), torch.where(new, n + new.cumsum(-1) - 1, none)))
        firsts.append(torch.where(has, firsts[-1].gather(-1, at), torch.where(new, torch.full_like(none, t + 1), none)))
        n = n + new.sum(-1, keepdim=True)
    track_id = torch.stack(ids, dim=1)                                               # (n_planes, S, M)
    flat, node = track_id.reshape(-1, S * M), (track_id >= 0).reshape(-1, S * M)
    nodes = torch.zeros_like(flat).scatter_add_(-1, flat.clamp(min=0), node.to(torch.int64))   # per track: its number of nodes
    length = torch.where(node, nodes.gather(-1, flat.clamp(min=0)), torch.zeros_like(flat)).reshape(-1, S, M)
    return Tracks(track_id.to(torch.int32), n[:, 0].to(torch.int32), length.to(torch.int32),
                  torch.stack(firsts, dim=1).to(torch.int32), steps, links, float(max_km))
