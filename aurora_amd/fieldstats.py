"""Per-point statistics over the steps of a roll-out, the members of an ensemble or many forecast - truth pairs, kept as MAPS
where the predictions live (not in the reference).  `scores`, `ensemble_scores`, `spectra` and `event_scores` reduce a
prediction over space; `FieldStats` reduces a sequence of them over its length and keeps the grid:

    acc = aurora_amd.FieldStats(thresholds={"2t": [303.15, 308.15], "10ws": [17.2, 32.7]}, below=False, derived=("10ws",))
    for pred in rollout(model, batch, 40):
        acc.update(pred)                  # one sample: the last history entry of every surface and atmospheric variable
    acc.update(members, over="batch")     # the B = 2..64 batch elements are B samples of a B = 1 state
    acc.update(pred, minus=truth)         # the sample is pred - truth: mean-error and RMSE maps
    acc.mean["2t"]                        # (B, H, W) float64 on the device of the samples; atmospheric: (B, C, H, W)
    acc.std(ddof=1)["z"], acc.var(), acc.rms, acc.min, acc.max            # float64; NaN where no sample was valid
    acc.argmin, acc.argmax, acc.count     # int32: the sample (counted from 0 over all updates) of the extreme, -1 if none
    acc.exceed_count["2t"]                # (B, T, H, W) int32; atmospheric (B, T, C, H, W); also longest_run (int32),
    acc.exceed_fraction["2t"]             #   exceed_fraction (float64, count / valid samples)
    acc.as_batch("mean")                  # a float32 Batch with the metadata of the last update: scores(), regrid, to_netcdf
    acc.reset(); acc.cpu()

`derived` adds "10ws" = sqrt(10u^2 + 10v^2) (a surface variable) and / or "ws" = sqrt(u^2 + v^2) (an atmospheric one), formed
per sample in fp64 and rounded to fp32 once; with `minus=` the reference of a derived variable is the variable of that name
in `minus`.  `thresholds` maps a variable to up to 8 values (an atmospheric one: a sequence for every level or a (C, T) array),
rounded to float32 once and compared in float32: the event is value >= threshold (`below=True`: <=); a shorter list is padded
with NaN, which is never exceeded.  The first `update` fixes the variables, the grid, the levels, the batch size and the
device; later ones must match.

Per point and sample, v = (double)x (or (double)x - (double)r with `minus`) and w = fp32(v).  A sample is SKIPPED at a point
where an input is not finite (a land mask, a missing value): nothing of that point's state changes, and a run of exceedances
is neither extended nor broken.  The state keeps n, origin = w of the first valid sample, the SHIFTED sums s1 = sum d and
s2 = sum d^2 with d = v - origin (differences, never raw values: a pressure of 1e5 Pa that varies by a few hundred keeps its
digits), the minimum and maximum of w with the index of the first sample that reached them, and per threshold the count, the
current run and the longest run.  On demand, as elementwise torch on the state's device and without a read-back:

    mean = origin + s1 / n     var = max(0, s2 - s1^2 / n) / (n - ddof)     rms = sqrt((s2 + 2 origin s1 + n origin^2) / n)

The state costs 36 + 12 T bytes per point: 2.6 GB for the 69 planes of a 0.25-degree state (721 x 1440) without thresholds,
4.3 GB with T = 2.  Fields on one GPU are accumulated by ONE aurora_hip_field_stats_update call per `update` (a point's state
is read once, updated by the call's samples in order in registers, and written once; no temporary, no atomics, nothing read
back, capturable in a hipGraph after one warm call on the same buffers; the sample counter lives on the device).  Nothing is
reduced across threads, so the result is repeatable bit for bit and does not depend on how the samples were grouped into
`update` calls.  Fields on the CPU take the same recurrence in numpy (after a conversion to float32).

Not offered: merging two accumulators, latitude bands (`BandBatch`), windows inside one object (use one `FieldStats` per
window).
"""

from __future__ import annotations

import copy
from typing import Mapping, Optional, Sequence

import numpy as np
import torch

from aurora_amd import _fields
from aurora_amd._fields import MAX_THRESHOLDS, _host
from aurora_amd.batch import Batch, derive_metadata

__all__ = ["FieldStats", "MAX_SAMPLES", "MAX_THRESHOLDS"]

MAX_SAMPLES = 64
DERIVED = {"10ws": ("surf_vars", "10u", "10v"), "ws": ("atmos_vars", "u", "v")}
# state array -> (dtype, per threshold); include/aurora_hip.h has the meanings
_STATE = {"n": (torch.int32, False), "origin": (torch.float32, False), "s1": (torch.float64, False),
          "s2": (torch.float64, False), "vmin": (torch.float32, False), "vmax": (torch.float32, False),
          "argmin": (torch.int32, False), "argmax": (torch.int32, False), "exceed": (torch.int32, True),
          "run": (torch.int32, True), "longest": (torch.int32, True)}
_MAPS = ("mean", "std", "var", "rms", "min", "max")


def _update_host(state: dict, x: np.ndarray, b: Optional[np.ndarray], has_b: np.ndarray, r: Optional[np.ndarray],
                 thr: Optional[np.ndarray], below: bool, index: int) -> None:
    """One sample of every plane into the numpy views of the state: the recurrence of include/aurora_hip.h.  x, b, r:
    (n_planes, n_points) float32; has_b: (n_planes,) bool; thr: (n_planes, T) float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(x)
        if b is not None:
            ws = np.sqrt(x.astype(np.float64) ** 2 + b.astype(np.float64) ** 2).astype(np.float32)
            ok &= np.isfinite(b) | ~has_b[:, None]
            x = np.where(has_b[:, None], ws, x)
            ok &= np.isfinite(x)
        v = x.astype(np.float64)
        if r is not None:
            ok &= np.isfinite(r)
            v = v - r.astype(np.float64)
        w = v.astype(np.float32)
        first = ok & (state["n"] == 0)
        state["origin"][first] = w[first]
        d = np.where(ok, v - state["origin"].astype(np.float64), 0.0)
        state["s1"] += d
        state["s2"] += d * d
        for ext, arg, cmp in (("vmin", "argmin", np.less), ("vmax", "argmax", np.greater)):
            new = first | (ok & cmp(w, state[ext]))
            state[ext][new] = w[new]
            state[arg][new] = index
        if thr is not None:
            ev = (np.less_equal if below else np.greater_equal)(w[:, None, :], thr[:, :, None]) & ok[:, None, :]
            state["exceed"] += ev
            state["run"][...] = np.where(ok[:, None, :], np.where(ev, state["run"] + 1, 0), state["run"])
            np.maximum(state["longest"], state["run"], out=state["longest"])
        state["n"] += ok


class FieldStats:
    """Streaming per-point statistics over samples; see the module's text."""

    def __init__(self, thresholds: Optional[Mapping[str, object]] = None, below: bool = False, derived: Sequence[str] = ()):
        if thresholds is not None and not isinstance(thresholds, Mapping):
            raise ValueError("FieldStats: thresholds must be a mapping from variable name to values")
        derived = (derived,) if isinstance(derived, str) else tuple(derived)
        for d in derived:
            if d not in DERIVED:
                raise ValueError(f"FieldStats: derived offers {sorted(DERIVED)}, got {d!r}")
        self._thresholds = dict(thresholds or {})
        self._below = bool(below)
        self._derived = tuple(dict.fromkeys(derived))
        self._state: Optional[dict[str, torch.Tensor]] = None

    # ---- the samples of an update -------------------------------------------------------------------------------------
    def _fields(self, batch: Batch, what: str, reference: bool = False):
        """[(name, group, field (B, [C,] H, W), second operand or None)] of a batch, derived variables last in each group."""
        n_lat, n_lon = batch.metadata.lat.shape[0], batch.metadata.lon.shape[0]
        out = []
        for group in ("surf_vars", "atmos_vars"):
            vars_ = getattr(batch, group)
            for k, f in vars_.items():
                _fields.check_field("FieldStats", f, what, group, k, n_lat, n_lon)
                if k in DERIVED and k in self._derived and not reference:
                    raise ValueError(f"FieldStats: {what} holds {k!r}, which is also a derived variable")
                if not (reference and k in DERIVED and k not in self._derived):
                    out.append((k, group, f[:, -1], None))
            for d in self._derived:
                g, a, b = DERIVED[d]
                if g != group:
                    continue
                if reference:
                    if d not in vars_:
                        raise ValueError(f"FieldStats: with minus=, the reference of the derived variable {d!r} is "
                                         f"minus.{group}[{d!r}], which is missing")
                    continue
                if a not in vars_ or b not in vars_:
                    raise ValueError(f"FieldStats: the derived variable {d!r} needs {a!r} and {b!r} in {what}.{group}")
                out.append((d, group, vars_[a][:, -1], vars_[b][:, -1]))
        names = [k for k, *_ in out]
        if len(set(names)) != len(names):
            dup = sorted({k for k in names if names.count(k) > 1})
            raise ValueError(f"FieldStats: {dup[0]!r} is both a surface and an atmospheric variable")
        if not out:
            raise ValueError(f"FieldStats: {what} has no surface or atmospheric variable")
        return out

    def _start(self, batch: Batch, fields, B: int, device: torch.device) -> None:
        n_lat, n_lon = batch.metadata.lat.shape[0], batch.metadata.lon.shape[0]
        layout, first, thr_rows = [], 0, []
        for name, group, f, _ in fields:
            shape = (B, *f.shape[1:-2])
            layout.append((name, group, first, shape))
            n = int(np.prod(shape))
            first += n
            rows = np.full((1, 1), np.nan, dtype=np.float32)
            if name in self._thresholds:
                rows = _fields.threshold_rows("FieldStats", name, self._thresholds[name], None if group == "surf_vars" else shape[1])
            # (1 or C, T_v) -> one row per plane, planes in (B, [C]) order
            thr_rows.append(np.broadcast_to(rows, (B, n // B, rows.shape[1])).reshape(n, rows.shape[1]))
        known = {name for name, *_ in layout}
        for k in self._thresholds:
            if k not in known:
                raise ValueError(f"FieldStats: thresholds name the variable {k!r}, which the batch does not hold as a surface, "
                                 "atmospheric or derived variable")
        T = max(r.shape[1] for r in thr_rows) if self._thresholds else 0
        thr = None
        if T:
            thr = torch.from_numpy(_fields.pad_thresholds(thr_rows)).to(device)
        self._layout, self._n_planes, self._T, self._thr = tuple(layout), first, T, thr
        self._grid = (n_lat, n_lon)
        self._lat, self._lon = _host(batch.metadata.lat), _host(batch.metadata.lon)
        self._levels, self._B, self._device = tuple(batch.metadata.atmos_levels), B, device
        P = n_lat * n_lon
        self._state = {k: torch.zeros((first, T, P) if per_thr else (first, P), dtype=dt, device=device)
                       for k, (dt, per_thr) in _STATE.items() if T or not per_thr}
        self._index = torch.zeros(1, dtype=torch.int64, device=device)
        self._last = None

    def _check_grid(self, batch: Batch, what: str) -> None:
        """The comparison and wording of `_fields.check_same_coordinates`, against the grid of the first update."""
        for c, mine in (("lat", self._lat), ("lon", self._lon)):
            o = getattr(batch.metadata, c)
            if o.shape[0] != mine.shape[0]:
                raise ValueError(f"FieldStats: {what} and the first update differ in {c}: {o.shape[0]} against {mine.shape[0]} "
                                 "values")
            if not np.array_equal(_host(o), mine):
                raise ValueError(f"FieldStats: {what} and the first update differ in {c} (same length, different values)")
        if tuple(batch.metadata.atmos_levels) != self._levels:
            raise ValueError(f"FieldStats: {what} and the first update differ in atmos_levels: "
                             f"{tuple(batch.metadata.atmos_levels)} against {self._levels}")

    def update(self, batch: Batch, over: Optional[str] = None, minus: Optional[Batch] = None) -> "FieldStats":
        """Adds one sample (the last history entry of every variable of `batch`), or with over="batch" one sample per batch
        element; with `minus` the sample is batch - minus.  Returns self."""
        if over not in (None, "batch"):
            raise ValueError(f"FieldStats: over must be None or 'batch', got {over!r}")
        for what, b in (("batch", batch), ("minus", minus)):
            if b is None:
                continue
            if not isinstance(b, Batch):
                raise TypeError(f"FieldStats: {what} must be a Batch, got {type(b).__name__}")
            _fields.check_vector_grid("FieldStats", b, what, band="statistics")
        if minus is not None:
            _fields.check_same_coordinates("FieldStats", batch, minus, "batch", "minus", "batch")
        fields = self._fields(batch, "batch")
        sizes = {f.shape[0] for _, _, f, _ in fields}
        if len(sizes) != 1:
            raise ValueError(f"FieldStats: the variables of batch differ in batch size: {sorted(sizes)}")
        Bb = sizes.pop()
        if over == "batch" and not 2 <= Bb <= MAX_SAMPLES:
            raise ValueError(f"FieldStats: with over='batch' the batch size is the number of samples: it must be 2 to "
                             f"{MAX_SAMPLES}, got {Bb}")
        B = 1 if over == "batch" else Bb
        refs = None
        if minus is not None:
            by_name = {k: f for k, _, f, _ in self._fields(minus, "minus", reference=True)}
            for d in self._derived:
                by_name[d] = getattr(minus, DERIVED[d][0])[d][:, -1]
            refs = []
            for name, _, f, _ in fields:
                if name not in by_name:
                    raise ValueError(f"FieldStats: minus has no variable {name!r}")
                r = by_name[name]
                if tuple(r.shape) != (B, *f.shape[1:]):
                    what_differs = "batch size" if r.shape[0] != B else "shape"
                    raise ValueError(f"FieldStats: batch and minus differ in {what_differs} for {name!r}: "
                                     f"{(B, *f.shape[1:])} against {tuple(r.shape)}")
                refs.append(r)

        everything = [f for _, _, f, b in fields for f in ((f,) if b is None else (f, b))] + (refs or [])
        device = torch.device(_fields.device_of("FieldStats", everything))
        if self._state is None:
            self._start(batch, fields, B, device)
        else:
            self._check_grid(batch, "batch")
            got = tuple((name, group, (B, *f.shape[1:-2])) for name, group, f, _ in fields)
            want = tuple((name, group, shape) for name, group, _, shape in self._layout)
            if got != want:
                if [g[:2] for g in got] != [w[:2] for w in want]:
                    raise ValueError(f"FieldStats: batch holds the variables {[g[0] for g in got]}, the first update held "
                                     f"{[w[0] for w in want]}")
                bad = next((g, w) for g, w in zip(got, want) if g != w)
                what_differs = "batch size" if bad[0][2][0] != bad[1][2][0] else "shape"
                raise ValueError(f"FieldStats: batch and the first update differ in {what_differs} for {bad[0][0]!r}: "
                                 f"{bad[0][2]} against {bad[1][2]}")
            if device != self._device:
                raise ValueError(f"FieldStats: the fields are on {device}, the state of the first update is on {self._device}; "
                                 "move the batches there, or use .cpu()")

        S = Bb if over == "batch" else 1
        pick = (lambda f, m: f[m:m + 1]) if over == "batch" else (lambda f, m: f)
        samples = [[pick(f, m) for _, _, f, _ in fields] for m in range(S)]
        any_second = any(b is not None for *_, b in fields)
        second = [[None if b is None else pick(b, m) for *_, b in fields] for m in range(S)] if any_second else None
        if device.type == "cuda":
            from aurora_amd.engine import lib

            n_lat, n_lon = self._grid
            of_batch = [f for fs in samples for f in fs] + [b for bs in (second or []) for b in bs if b is not None]
            _fields.check_planes("FieldStats", [("batch", of_batch, of_batch), ("minus", refs or [], refs or [])], n_lat, n_lon,
                                 _fields.TAKES_TASK, noun=lambda what, _: f"a variable of {what}")
            lib.field_stats_update(samples, refs, second, self._thr, self._below, self._index, self._state)
        else:
            self._update_host(samples, refs, second)
        md = batch.metadata
        if over == "batch":
            md = derive_metadata(md, time=tuple(md.time[:1]))
        self._last = (md, batch.static_vars)
        return self

    def _update_host(self, samples, refs, second) -> None:
        P = self._grid[0] * self._grid[1]
        stack = lambda fs: np.concatenate([f.detach().to(torch.float32).reshape(-1, P).numpy() for f in fs])  # noqa: E731
        state = {k: v.numpy() for k, v in self._state.items()}
        r = stack(refs) if refs is not None else None
        thr = self._thr.numpy() if self._T else None
        index = int(self._index)
        for m, fs in enumerate(samples):
            x, b, has_b = stack(fs), None, np.zeros(self._n_planes, dtype=bool)
            if second is not None:
                b = stack([torch.zeros_like(f) if s is None else s for f, s in zip(fs, second[m])])
                has_b = np.concatenate([np.full(f.numel() // P, s is not None) for f, s in zip(fs, second[m])])
            _update_host(state, x, b, has_b, r, thr, self._below, index + m)
        self._index += len(samples)

    # ---- results --------------------------------------------------------------------------------------------------------
    @property
    def state(self) -> dict[str, torch.Tensor]:
        """The raw arrays of include/aurora_hip.h, (n_planes, n_points) -- per threshold (n_planes, T, n_points) --, planes
        in the order of `layout`; not copies."""
        return self._need_state()

    @property
    def layout(self) -> tuple[tuple[str, str, int, tuple[int, ...]], ...]:
        """(name, group, first plane, leading shape) per variable."""
        self._need_state()
        return self._layout

    def _need_state(self) -> dict[str, torch.Tensor]:
        if self._state is None:
            raise ValueError("FieldStats: no update yet")
        return self._state

    def _maps(self, t: torch.Tensor, only: Optional[set] = None) -> dict[str, torch.Tensor]:
        """(n_planes, [T,] n_points) -> name -> (B, [T,] [C,] H, W)."""
        out = {}
        for name, _, first, shape in self._layout:
            if only is not None and name not in only:
                continue
            n = int(np.prod(shape))
            v = t[first:first + n]
            v = v.reshape(*shape, *v.shape[1:-1], *self._grid)
            out[name] = v.movedim(len(shape), 1) if t.dim() == 3 else v
        return out

    def _table(self, what: str, ddof: int = 0) -> torch.Tensor:
        s = self._need_state()
        n = s["n"].to(torch.float64)
        nan = torch.full_like(n, float("nan"))
        some = s["n"] > 0
        o = s["origin"].to(torch.float64)
        if what == "mean":
            return torch.where(some, o + s["s1"] / n, nan)
        if what in ("var", "std"):
            var = torch.clamp(s["s2"] - s["s1"] * s["s1"] / n, min=0.0) / (n - ddof)
            var = torch.where(s["n"] > ddof, var, nan)
            return torch.sqrt(var) if what == "std" else var
        if what == "rms":
            return torch.where(some, torch.sqrt((s["s2"] + 2.0 * o * s["s1"] + n * o * o) / n), nan)
        if what in ("min", "max"):
            return torch.where(some, s["v" + what].to(torch.float64), nan)
        raise ValueError(f"FieldStats: unknown quantity {what!r}; one of {_MAPS}")

    mean = property(lambda self: self._maps(self._table("mean")))
    rms = property(lambda self: self._maps(self._table("rms")))
    min = property(lambda self: self._maps(self._table("min")))
    max = property(lambda self: self._maps(self._table("max")))
    count = property(lambda self: self._maps(self._need_state()["n"]))

    def var(self, ddof: int = 0) -> dict[str, torch.Tensor]:
        return self._maps(self._table("var", ddof))

    def std(self, ddof: int = 0) -> dict[str, torch.Tensor]:
        return self._maps(self._table("std", ddof))

    def _arg(self, which: str) -> dict[str, torch.Tensor]:
        s = self._need_state()
        return self._maps(torch.where(s["n"] > 0, s[which], torch.full_like(s[which], -1)))

    argmin = property(lambda self: self._arg("argmin"))
    argmax = property(lambda self: self._arg("argmax"))

    def _per_threshold(self, which: str) -> dict[str, torch.Tensor]:
        s = self._need_state()
        if not self._T:
            raise ValueError("FieldStats: no thresholds were given")
        return self._maps(s[which], only=set(self._thresholds))

    exceed_count = property(lambda self: self._per_threshold("exceed"))
    longest_run = property(lambda self: self._per_threshold("longest"))

    @property
    def exceed_fraction(self) -> dict[str, torch.Tensor]:
        """exceed_count / count in float64; NaN where no sample was valid and for a padded threshold slot."""
        s = self._need_state()
        if not self._T:
            raise ValueError("FieldStats: no thresholds were given")
        n = s["n"].to(torch.float64)[:, None, :]
        frac = torch.where(n > 0, s["exceed"].to(torch.float64) / n, torch.full_like(n, float("nan")))
        frac = torch.where(torch.isnan(self._thr)[:, :, None], torch.full_like(frac, float("nan")), frac)
        return self._maps(frac, only=set(self._thresholds))

    def as_batch(self, what: str = "mean", ddof: int = 0) -> Batch:
        """One of mean, std, var, rms, min, max as a float32 `Batch` (one history entry) with the metadata and the static
        variables of the last update; a derived variable goes where its components are."""
        if what not in _MAPS:
            raise ValueError(f"FieldStats: as_batch offers {_MAPS}, got {what!r}")
        maps = self._maps(self._table(what, ddof).to(torch.float32))
        md, static = self._last
        out = {"surf_vars": {}, "atmos_vars": {}}
        for name, group, _, _ in self._layout:
            out[group][name] = maps[name][:, None]
        return Batch(out["surf_vars"], dict(static), out["atmos_vars"], md)

    # ---- housekeeping ---------------------------------------------------------------------------------------------------
    def reset(self) -> "FieldStats":
        """Forgets every sample (in place, no allocation); the variables, grid and device stay fixed."""
        if self._state is not None:
            for v in self._state.values():
                v.zero_()
            self._index.zero_()
        return self

    def cpu(self) -> "FieldStats":
        """A copy with the state on the host (waits for the device)."""
        new = copy.copy(self)
        if self._state is not None:
            new._state = {k: v.cpu().clone() for k, v in self._state.items()}
            new._index = self._index.cpu().clone()
            new._thr = None if self._thr is None else self._thr.cpu()
            new._device = torch.device("cpu")
            md, static = self._last
            md = derive_metadata(md, lat=md.lat.cpu(), lon=md.lon.cpu())
            new._last = (md, {k: v.cpu() for k, v in static.items()})
        return new
