"""What the verification front ends (`scores`, `ensemble_scores`, `ensemble_quantiles`, `event_scores`, `probability_scores`,
`spectra`, `FieldStats`, `diagnostics`, `field_quantiles`) share: coordinates and grid checks, the selection of the fields of a call, the
decision where they are reduced, the layout accessor, threshold tables, the fixed summation trees and the cache of small
device tables.

Plain functions.  The name a message starts with (`fn`) and the words for the operands are arguments, so every module's
messages are made here with its own wording; tests/test_verification_messages.py pins them."""

from __future__ import annotations

import math
import threading
import weakref
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from aurora_amd import _sphere
from aurora_amd._sphere import MAX_LON
from aurora_amd.batch import BandBatch, Batch
from aurora_amd.engine.tables import DeviceTables, _upload  # noqa: F401  (tests wrap `_fields._upload` to count uploads)

GROUPS = ("surf_vars", "atmos_vars")
MAX_MEMBERS, MAX_THRESHOLDS = 64, 8
Layout = tuple[tuple[str, int, tuple[int, ...]], ...]   # (name, first plane, shape) per variable


# ---- coordinates and grids -----------------------------------------------------------------------------------------
_lock = threading.Lock()
_host_coords: dict[int, tuple] = {}        # id(tensor) -> (weak reference, version, fp64 host copy)


def _version(t: torch.Tensor) -> int:
    return 0 if t.is_inference() else t._version   # (inference tensors keep no version counter)


def _host(t: torch.Tensor) -> np.ndarray:
    """fp64 host copy of a coordinate tensor, remembered per tensor object: the first call for a device tensor waits for
    the device, later calls (every step of a roll-out carries the same coordinates) do not."""
    with _lock:
        hit = _host_coords.get(id(t))
        if hit is not None and hit[0]() is t and hit[1] == _version(t):
            return hit[2]
    a = t.detach().to(torch.float64).cpu().numpy()
    a.setflags(write=False)
    key = id(t)

    def forget(_ref, key=key):
        with _lock:
            cur = _host_coords.get(key)
            if cur is not None and cur[0] is _ref:
                del _host_coords[key]

    with _lock:
        _host_coords[key] = (weakref.ref(t, forget), _version(t), a)
    return a


def latitude_weights(lat) -> np.ndarray:
    """w[i] = cos(lat[i]) / mean_j cos(lat[j]) in fp64 (latitudes in degrees, a vector within [-90, 90])."""
    lat = np.asarray(lat, dtype=np.float64)
    if lat.ndim != 1 or lat.size == 0:
        raise ValueError("scores: latitudes must be a non-empty vector")
    _sphere.check_latitudes("scores", lat, monotonic=None)
    c = np.maximum(np.cos(np.deg2rad(lat)), 0.0)
    mean = c.mean()
    if not mean > 0:
        raise ValueError("scores: the latitudes carry no weight (every row is a pole)")
    return c / mean


def check_vector_grid(fn: str, b: Batch, name: str, band: str = "scores") -> None:
    """`b` is a whole grid with vector coordinates."""
    if isinstance(b, BandBatch):
        raise ValueError(f"{fn}: {name} is a latitude band (BandBatch); gather the forecast first, band {band} are "
                         "not supported")
    if b.metadata.lat.dim() != 1 or b.metadata.lon.dim() != 1:
        raise ValueError(f"{fn}: {name} has matrices for latitudes / longitudes; vector coordinates are needed")


def check_same_coordinates(fn: str, a: Batch, b: Batch, a_name: str, b_name: str, cropped: str) -> None:
    """`a` and `b` have the same latitudes, longitudes and levels; `cropped`: how the hint speaks of `a`."""
    for c in ("lat", "lon"):
        x, o = getattr(a.metadata, c), getattr(b.metadata, c)
        if x.shape != o.shape:
            hint = ""
            if c == "lat" and o.shape[0] == x.shape[0] + 1:
                hint = f"; {cropped} was cropped to the model's patch size: use {b_name}.crop(model.patch_size)"
            raise ValueError(f"{fn}: {a_name} and {b_name} differ in {c}: {x.shape[0]} against {o.shape[0]} values{hint}")
        if x is not o and not np.array_equal(_host(x), _host(o)):
            raise ValueError(f"{fn}: {a_name} and {b_name} differ in {c} (same length, different values)")
    if tuple(a.metadata.atmos_levels) != tuple(b.metadata.atmos_levels):
        raise ValueError(f"{fn}: {a_name} and {b_name} differ in atmos_levels: {tuple(a.metadata.atmos_levels)} against "
                         f"{tuple(b.metadata.atmos_levels)}")


def check_same_grid(fn: str, a: Batch, b: Batch, a_name: str, b_name: str, cropped: str) -> None:
    check_vector_grid(fn, a, a_name)
    check_vector_grid(fn, b, b_name)
    check_same_coordinates(fn, a, b, a_name, b_name, cropped)


def check_longitudes(lon: np.ndarray) -> None:
    """spectra's refusal of a grid that is no `_sphere.full_circle`."""
    n = lon.shape[0]
    if not 2 <= n <= MAX_LON:
        raise ValueError(f"spectra: the grid has {n} longitudes; 2 to {MAX_LON} are supported")
    if not _sphere.full_circle(lon):
        raise ValueError("spectra: the longitudes must be equally spaced and cover the full circle (a zonal spectrum of a "
                         "regional or irregular grid is not defined)")


# ---- the selection ---------------------------------------------------------------------------------------------------
def check_field(fn: str, f: torch.Tensor, what: str, group: str, k: str, n_lat: int, n_lon: int) -> None:
    """`f` is (B, T, n_lat, n_lon) in surf_vars and (B, T, C, n_lat, n_lon) in atmos_vars."""
    if f.dim() != (4 if group == "surf_vars" else 5) or tuple(f.shape[-2:]) != (n_lat, n_lon):
        raise ValueError(f"{fn}: {what}.{group}[{k!r}] has shape {tuple(f.shape)}, which does not fit a {n_lat} x {n_lon} grid")


def _differ(fn: str, a_name: str, b_name: str, k: str, a_shape, b_shape) -> ValueError:
    what_differs = "batch size" if a_shape[0] != b_shape[0] else "shape"
    return ValueError(f"{fn}: {a_name} and {b_name} differ in {what_differs} for {k!r}: {tuple(a_shape)} against "
                      f"{tuple(b_shape)}")


def layout_of(names: Sequence[str], fields: Sequence[torch.Tensor]) -> Layout:
    layout, first = [], 0
    for name, f in zip(names, fields):
        shape = tuple(f.shape[:-2])
        layout.append((name, first, shape))
        first += math.prod(shape)
    return tuple(layout)


def select_pair(fn: str, pred: Batch, others: Sequence[tuple[str, Batch]], only=None, repeated: Sequence[str] = ()):
    """The last history entry of every variable (of `only`, if given) that `pred` and the first of `others` hold, which
    every further one must hold too, for the deterministic front ends: (names, one list of fields per batch, pred's first,
    and the layout).  The batches are on one checked grid.  An operand named in `repeated` may have batch size 1 against a
    larger `pred`: its field is then expanded, a view whose batch elements are the one plane (nothing is copied)."""
    n_lat, n_lon = pred.metadata.lat.shape[0], pred.metadata.lon.shape[0]
    batches = [("pred", pred), *others]
    names, fields = [], [[] for _ in batches]
    for group in GROUPS:
        for k in getattr(pred, group):
            if (only is not None and k not in only) or (others and k not in getattr(others[0][1], group)):
                continue
            for what, b in others[1:]:
                if k not in getattr(b, group):
                    raise ValueError(f"{fn}: the {what} has no {group[:-5]} variable {k!r}")
            if k in names:
                raise ValueError(f"{fn}: {k!r} is both a surface and an atmospheric variable")
            names.append(k)
            for slot, (what, b) in enumerate(batches):
                f = getattr(b, group)[k]
                check_field(fn, f, what, group, k, n_lat, n_lon)
                f = f[:, -1]
                if what in repeated and f.shape[0] == 1 and f.shape[1:] == fields[0][-1].shape[1:]:
                    f = f.expand_as(fields[0][-1])
                if slot and f.shape != fields[0][-1].shape:
                    raise _differ(fn, "pred", what, k, fields[0][-1].shape, f.shape)
                fields[slot].append(f)
    return names, fields, layout_of(names, fields[0])


def select_one(fn: str, b: Batch, what: str = "batch", only=None):
    """The last history entry of every variable (of `only`, if given, all of which `b` must hold) of ONE batch on a checked
    grid, for the front ends that look at a field on its own: (names, fields, the layout)."""
    n_lat, n_lon = b.metadata.lat.shape[0], b.metadata.lon.shape[0]
    names, fields = [], []
    for group in GROUPS:
        for k, f in getattr(b, group).items():
            if only is not None and k not in only:
                continue
            if k in names:
                raise ValueError(f"{fn}: {k!r} is both a surface and an atmospheric variable")
            check_field(fn, f, what, group, k, n_lat, n_lon)
            names.append(k)
            fields.append(f[:, -1])
    for k in (only if only is not None else ()):
        if k not in names:
            raise ValueError(f"{fn}: only names the variable {k!r}, which {what} does not hold as a surface or atmospheric "
                             "variable")
    return names, fields, layout_of(names, fields)


def select_members(fn: str, members, truth: Batch, only=None):
    """The same for M members against `truth`: `members` is a sequence of 2 to 64 batches with the batch size of `truth`, or
    ONE batch whose batch elements are the members while `truth` has batch size 1.  (names, truth's fields, M lists of
    member fields, the layout)."""
    if not isinstance(truth, Batch):
        raise TypeError(f"{fn}: truth must be a Batch, got {type(truth).__name__}")
    if isinstance(truth, BandBatch):
        check_vector_grid(fn, truth, "truth")
    one_batch = isinstance(members, Batch)
    batches = [members] if one_batch else list(members)
    for m, b in enumerate(batches):
        if not isinstance(b, Batch):
            raise TypeError(f"{fn}: members[{m}] must be a Batch, got {type(b).__name__}")
    who = ["members"] if one_batch else [f"members[{m}]" for m in range(len(batches))]
    if not one_batch and not 2 <= len(batches) <= MAX_MEMBERS:
        raise ValueError(f"{fn}: members must hold 2 to {MAX_MEMBERS} batches, got {len(batches)}")
    for b, w in zip(batches, who):
        # (a message that names the member has always come out with "ensemble_" in front of the function's name; kept as it
        #  is, and pinned by tests/test_verification_messages.py, until a change of its own rewords it)
        check_vector_grid("ensemble_" + fn, b, w)
        check_vector_grid(fn, truth, "truth")
        check_same_coordinates("ensemble_" + fn, b, truth, w, "truth", w)
    n_lat, n_lon = truth.metadata.lat.shape[0], truth.metadata.lon.shape[0]

    names, truth_fields, member_fields = [], [], [[] for _ in batches]
    for group in GROUPS:
        for k, t in getattr(truth, group).items():
            if (only is not None and k not in only) or not all(k in getattr(b, group) for b in batches):
                continue
            if k in names:
                raise ValueError(f"{fn}: {k!r} is both a surface and an atmospheric variable")
            names.append(k)
            check_field(fn, t, "truth", group, k, n_lat, n_lon)
            for b, w in zip(batches, who):
                check_field(fn, getattr(b, group)[k], w, group, k, n_lat, n_lon)
            t = t[:, -1]
            truth_fields.append(t)
            for m, b in enumerate(batches):
                f = getattr(b, group)[k][:, -1]
                if one_batch:
                    if t.shape[0] != 1:
                        raise ValueError(f"{fn}: members is ONE Batch (its batch elements are the members), so truth must "
                                         f"have batch size 1, got {t.shape[0]} for {k!r}; pass a sequence of Batches to score "
                                         "a batch of ensembles")
                    if f.shape[1:] != t.shape[1:]:
                        raise ValueError(f"{fn}: members and truth differ in shape for {k!r}: {tuple(f.shape)} against "
                                         f"{tuple(t.shape)}")
                elif f.shape != t.shape:
                    raise _differ(fn, who[m], "truth", k, f.shape, t.shape)
                member_fields[m].append(f)
    if one_batch and names:                                # the batch elements of the one Batch are the members
        sizes = {f.shape[0] for f in member_fields[0]}
        M = sizes.pop()
        if sizes or not 2 <= M <= MAX_MEMBERS:
            raise ValueError(f"{fn}: members is ONE Batch, whose batch size is the number of members: it must be 2 to "
                             f"{MAX_MEMBERS}, got {sorted(sizes | {M})}")
        member_fields = [[f[m:m + 1] for f in member_fields[0]] for m in range(M)]
    return names, truth_fields, member_fields, layout_of(names, truth_fields)


def select_samples(fn: str, members, truth: Optional[Batch] = None):
    """M members as in `select_members`, with or WITHOUT a truth (`ensemble_quantiles`): without one the grid and the shapes
    of members[0] are what the others must match, and with one `truth` is one more operand of the same shapes.  (names, truth's
    fields or None, M lists of member fields, the layout)."""
    if truth is not None and not isinstance(truth, Batch):
        raise TypeError(f"{fn}: truth must be a Batch or None, got {type(truth).__name__}")
    one_batch = isinstance(members, Batch)
    batches = [members] if one_batch else list(members)
    for m, b in enumerate(batches):
        if not isinstance(b, Batch):
            raise TypeError(f"{fn}: members[{m}] must be a Batch, got {type(b).__name__}")
    who = ["members"] if one_batch else [f"members[{m}]" for m in range(len(batches))]
    if not one_batch and not 2 <= len(batches) <= MAX_MEMBERS:
        raise ValueError(f"{fn}: members must hold 2 to {MAX_MEMBERS} batches, got {len(batches)}")
    operands = list(zip(who, batches)) + ([("truth", truth)] if truth is not None else [])
    first_name, first = operands[0]
    for w, b in operands:
        check_vector_grid(fn, b, w, band="quantiles")
    for w, b in operands[1:]:
        check_same_coordinates(fn, b, first, w, first_name, w)
    n_lat, n_lon = first.metadata.lat.shape[0], first.metadata.lon.shape[0]

    names, fields = [], [[] for _ in operands]
    for group in GROUPS:
        for k in getattr(first, group):
            if not all(k in getattr(b, group) for _, b in operands):
                continue
            if k in names:
                raise ValueError(f"{fn}: {k!r} is both a surface and an atmospheric variable")
            names.append(k)
            for slot, (w, b) in enumerate(operands):
                f = getattr(b, group)[k]
                check_field(fn, f, w, group, k, n_lat, n_lon)
                f = f[:, -1]
                if w == "truth" and one_batch:
                    if f.shape[0] != 1:
                        raise ValueError(f"{fn}: members is ONE Batch (its batch elements are the members), so truth must "
                                         f"have batch size 1, got {f.shape[0]} for {k!r}; pass a sequence of Batches for a "
                                         "batch of ensembles")
                    if f.shape[1:] != fields[0][-1].shape[1:]:
                        raise ValueError(f"{fn}: members and truth differ in shape for {k!r}: {tuple(fields[0][-1].shape)} "
                                         f"against {tuple(f.shape)}")
                elif slot and f.shape != fields[0][-1].shape:
                    raise _differ(fn, w, first_name, k, f.shape, fields[0][-1].shape)
                fields[slot].append(f)
    member_fields = fields[:len(batches)]
    truth_fields = fields[-1] if truth is not None else None
    if one_batch and names:                                # the batch elements of the one Batch are the members
        sizes = {f.shape[0] for f in member_fields[0]}
        M = sizes.pop()
        if sizes or not 2 <= M <= MAX_MEMBERS:
            raise ValueError(f"{fn}: members is ONE Batch, whose batch size is the number of members: it must be 2 to "
                             f"{MAX_MEMBERS}, got {sorted(sizes | {M})}")
        member_fields = [[f[m:m + 1] for f in member_fields[0]] for m in range(M)]
    return names, truth_fields, member_fields, layout_of(names, member_fields[0])


def by_variable(layout: Layout, t: torch.Tensor) -> dict[str, torch.Tensor]:
    """(n_planes, ...) -> name -> (*shape, ...): what every result's properties return."""
    out = {}
    for name, first, shape in layout:
        n = math.prod(shape)
        v = t[first:first + n]
        out[name] = v.reshape(*shape, *v.shape[1:])
    return out


class PowerViews:
    """The views that `Spectra` and `SphereSpectra` share, over the result's `table` ((n_planes, 1 or 3, ...): pred, truth,
    error) and `layout`.  No fields of its own."""

    def _field(self, t: torch.Tensor) -> dict[str, torch.Tensor]:
        return by_variable(self.layout, t)

    @property
    def has_truth(self) -> bool:
        return self.table.shape[1] == 3

    @property
    def power(self) -> dict[str, torch.Tensor]:
        return self._field(self.table[:, 0])

    @property
    def truth_power(self) -> Optional[dict[str, torch.Tensor]]:
        return self._field(self.table[:, 1]) if self.has_truth else None

    @property
    def error_power(self) -> Optional[dict[str, torch.Tensor]]:
        return self._field(self.table[:, 2]) if self.has_truth else None

    @property
    def ratio(self) -> Optional[dict[str, torch.Tensor]]:
        return self._field(self.table[:, 0] / self.table[:, 1]) if self.has_truth else None


# ---- where the fields are reduced ------------------------------------------------------------------------------------
def stack(fs: Sequence[torch.Tensor], n_lat: int, n_lon: int) -> np.ndarray:
    """Host fields as one (n_planes, n_lat, n_lon) array."""
    return np.concatenate([f.detach().reshape(-1, n_lat, n_lon).numpy() for f in fs])


def _variable(what: str, name: str) -> str:
    return f"{what} variable {name!r}"


def device_of(fn: str, tensors, fields: str = "the fields", batches: str = "batches"):
    """"cpu" where every tensor is on the host, the device where all are on one GPU; anything else is an error."""
    devices = {f.device for f in tensors}
    if all(d.type == "cpu" for d in devices):
        return "cpu"
    if len(devices) == 1 and next(iter(devices)).type == "cuda":
        return next(iter(devices))
    raise ValueError(f"{fn}: {fields} are on {sorted(map(str, devices))}; move the {batches} to the CPU or to one GPU first")


def check_planes(fn: str, labelled, n_lat: int, n_lon: int, task: str, noun: Callable[[str, str], str] = _variable) -> None:
    """What the device path needs of every field of `labelled`, [(what, names, fields)]: float32 and row-major planes."""
    for what, names, fs in labelled:
        for name, f in zip(names, fs):
            if f.dtype != torch.float32:
                raise TypeError(f"{fn}: {noun(what, name)} is {f.dtype}; the device path {task}")
            if (n_lon > 1 and f.stride(-1) != 1) or (n_lat > 1 and f.stride(-2) != n_lon):
                raise ValueError(f"{fn}: the planes of {noun(what, name)} are not row-major contiguous; call .contiguous() "
                                 "on it first")


SCORES_TASK = "scores float32 fields (move the batches to the CPU to score other precisions)"
TAKES_TASK = "takes float32 fields (move the batches to the CPU for other precisions)"


def place(fn: str, labelled, n_lat: int, n_lon: int, task: str = SCORES_TASK, fields: str = "the fields"):
    """`device_of` the fields of `labelled`; on a device they have passed `check_planes`."""
    device = device_of(fn, [f for _, _, fs in labelled for f in fs], fields)
    if device != "cpu":
        check_planes(fn, labelled, n_lat, n_lon, task)
    return device


# ---- thresholds --------------------------------------------------------------------------------------------------------
def threshold_rows(fn: str, name: str, value, levels: Optional[int], noun: str = "thresholds") -> np.ndarray:
    """(1 or C, T_v) float32 thresholds of one variable; `noun` is what the messages call them."""
    try:
        a = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: the {noun} of {name!r} must be numbers") from None
    if a.ndim == 1:
        a = a[None]
    elif a.ndim == 2 and levels is not None:
        if a.shape[0] != levels:
            raise ValueError(f"{fn}: the {noun} of {name!r} have shape {a.shape}; a (C, T) array needs C = {levels} "
                             "levels")
    else:
        want = "a sequence" if levels is None else f"a sequence or a ({levels}, T) array"
        raise ValueError(f"{fn}: the {noun} of {name!r} have shape {a.shape}; {want} is needed")
    if not 1 <= a.shape[1] <= MAX_THRESHOLDS:
        raise ValueError(f"{fn}: 1 to {MAX_THRESHOLDS} {noun} per variable, {name!r} has {a.shape[1]}")
    return a.astype(np.float32)


def pad_thresholds(rows: Sequence[np.ndarray]) -> np.ndarray:
    """Per-variable (n, T_v) rows -> (n_planes, max T_v) float32, the shorter ones padded with NaN."""
    T = max(r.shape[1] for r in rows)
    return np.concatenate([np.pad(r, ((0, 0), (0, T - r.shape[1])), constant_values=np.nan) for r in rows]).astype(np.float32)


def threshold_table(fn: str, thresholds, layout: Layout, noun: str = "thresholds") -> np.ndarray:
    """(n_planes, T) float32: the thresholds of every variable of `layout`, one row per plane in (B, [C]) order."""
    rows = []
    for name, _, lead in layout:
        r = threshold_rows(fn, name, thresholds[name], lead[1] if len(lead) == 2 else None, noun)
        if len(lead) == 2:
            r = np.broadcast_to(r, (lead[1], r.shape[1]))
        rows.append(np.broadcast_to(r, (lead[0], *r.shape)).reshape(-1, r.shape[1]))
    return pad_thresholds(rows)


def check_ascending(fn: str, table: np.ndarray, layout: Layout, noun: str = "edges") -> None:
    """The values of every row of `table` ((n_planes, T), NaN: none) that are not NaN ascend strictly."""
    for name, first, lead in layout:
        for row in table[first:first + math.prod(lead)]:
            v = row[~np.isnan(row)]
            if not np.all(v[1:] > v[:-1]):
                raise ValueError(f"{fn}: the {noun} of {name!r} must be strictly ascending, got {v.tolist()}")


# ---- finalisation: the same torch code on either device ----------------------------------------------------------------
# `tree_sum` and `tree_sum_rows` add the same pairs in the same order, one over the last dimension and one over dimension 1:
# `probability_scores` and `event_scores` rely on a sum taken by either over the same numbers having the same bits.
def tree_sum(x: torch.Tensor) -> torch.Tensor:
    """Sum over the last dimension as a fixed pairwise tree of elementwise additions: the same roundings on every device
    (a library reduction may add in another order on the GPU than on the CPU)."""
    n = x.shape[-1]
    size = 1
    while size < n:
        size *= 2
    if size != n:
        x = torch.cat([x, x.new_zeros(*x.shape[:-1], size - n)], dim=-1)
    while size > 1:
        size //= 2
        x = x[..., :size] + x[..., size:]
    return x[..., 0]


def tree_sum_rows(x: torch.Tensor) -> torch.Tensor:
    """`tree_sum` over dimension 1, the rows, on slices that stay contiguous in the bins."""
    n = x.shape[1]
    size = 1
    while size < n:
        size *= 2
    if size != n:
        x = torch.cat([x, x.new_zeros(x.shape[0], size - n, *x.shape[2:])], dim=1)
    while size > 1:
        size //= 2
        x = x[:, :size] + x[:, size:]
    return x[:, 0]


def ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    return torch.where(den != 0, num / den, torch.full_like(num, float("nan")))


# ---- small tables on the device ----------------------------------------------------------------------------------------
tables = DeviceTables()


def device_weights(fn: str, lat: np.ndarray, device: torch.device) -> torch.Tensor:
    return tables.get(("latitude weights", lat.tobytes()), device, lambda: latitude_weights(lat),
                      f"{fn}: call once on this grid before capturing a graph (the latitude weights are uploaded on the first "
                      "call, which a captured graph cannot replay)")


def device_thresholds(fn: str, thr: np.ndarray, device: torch.device) -> torch.Tensor:
    return tables.get(("thresholds", thr.tobytes(), thr.shape), device, thr.copy,
                      f"{fn}: call once with these thresholds before capturing a graph (the threshold table is uploaded on "
                      "the first call, which a captured graph cannot replay)")
