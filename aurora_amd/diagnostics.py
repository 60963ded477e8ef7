"""Derived fields where the predictions live (not in the reference): what forecasters threshold and verify is rarely a
variable the model emits.  `diagnostics` forms them from a batch and returns a `Batch`, so that every scorer, `FieldStats`,
`regrid` and `to_netcdf` take them unchanged:

    d = aurora_amd.diagnostics(pred, ("vo", "ivt", "10ws"))
    acc.update(d)
    aurora_amd.event_scores(d, aurora_amd.diagnostics(truth, ("vo", "ivt", "10ws")), {"ivt": [250.0, 500.0]})

    name                 group   from          definition
    ws                   atmos   u, v          sqrt(u^2 + v^2)
    vo                   atmos   u, v          relative vorticity, s^-1
    d                    atmos   u, v          horizontal divergence, s^-1
    10ws, 10vo, 10d      surf    10u, 10v      the same from the 10 m wind
    tcwv                 surf    q             (1 / g) integral q dp, kg m^-2
    ivtu, ivtv           surf    q, u, v       (1 / g) integral q u dp and (1 / g) integral q v dp, kg m^-1 s^-1
    ivt                  surf    q, u, v       sqrt(ivtu^2 + ivtv^2)

The last history entry of the inputs is used, like in every scorer here.  The outputs are float32, (B, 1, H, W) for a surface
name and (B, 1, C, H, W) for an atmospheric one; the returned batch carries the metadata of the input (the time unchanged)
and its static variables, and with `keep=True` also the last history entry of the input's own variables.

Arithmetic (include/aurora_hip.h has it in full): inputs fp32, every expression in fp64, one rounding to fp32; a result that
is not finite is NaN.  Horizontal derivatives are centred differences on the sphere (a = 6 371 229 m) with the three-point
formula for unequal latitude spacing, one-sided in the first and last row; the true latitudes enter, so ascending and
descending grids need no flag.  Pole rows (|lat| >= 90 - 1e-9) are NaN -- every scorer here skips them -- and there is no
polar-cap formula.  Longitudes follow THE GRID RULE of aurora_amd/_sphere.py: a grid that wraps by it takes its differences
across the seam, a regional one uses one-sided differences in its first and last column.  Vertical integrals are trapezoids over the batch's
pressure levels (2 to 64, any order, distinct; g = 9.80665 m s^-2); nothing is extrapolated to the surface or to the top,
and no level is masked below the ground (the model has no surface pressure).  A NaN or an infinity that a formula reads
makes that point NaN and no other.

Fields on one GPU are formed by ONE aurora_hip_diagnostics call: one launch for every wind-derived plane (u and v are read
once for vorticity, divergence and speed) and one for the columns; nothing is read back and no temporary of plane size
exists beside the outputs.  Fields on the CPU take the same formulas in numpy (after a conversion to float32).

Not offered: latitude bands (`BandBatch`), humidity or thermodynamic quantities, spherical-harmonic derivatives
(`sphere_spectra` has the analysis half of the transform: spectra, no synthesis).
"""

from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np
import torch

from aurora_amd import _fields, _sphere
from aurora_amd._fields import _host
from aurora_amd._sphere import EARTH_RADIUS
from aurora_amd.batch import Batch

__all__ = ["diagnostics", "EARTH_RADIUS", "GRAVITY", "MAX_LEVELS", "NAMES"]

GRAVITY = 9.80665
MAX_LEVELS = 64
# name -> (group, kind, components)
NAMES = {"ws": ("atmos_vars", "ws", ("u", "v")), "vo": ("atmos_vars", "vo", ("u", "v")), "d": ("atmos_vars", "div", ("u", "v")),
         "10ws": ("surf_vars", "ws", ("10u", "10v")), "10vo": ("surf_vars", "vo", ("10u", "10v")),
         "10d": ("surf_vars", "div", ("10u", "10v")), "tcwv": ("surf_vars", "tcwv", ("q",)),
         "ivtu": ("surf_vars", "ivtu", ("q", "u")), "ivtv": ("surf_vars", "ivtv", ("q", "v")),
         "ivt": ("surf_vars", "ivt", ("q", "u", "v"))}
_WIND, _COLUMN = ("vo", "div", "ws"), ("tcwv", "ivtu", "ivtv", "ivt")


# ---- the caller's tables ------------------------------------------------------------------------------------------------
def row_table(lat) -> np.ndarray:
    """(n_lat, 4) fp64 (A, m0, m1, m2) per latitude row (degrees, strictly monotonic, at least 2): include/aurora_hip.h."""
    lat = np.asarray(lat, dtype=np.float64)
    phi = np.deg2rad(lat)
    cos = np.cos(phi)
    n = lat.shape[0]
    h = np.diff(phi)
    c = np.zeros((n, 3))
    h1, h2 = h[:-1], h[1:]
    c[1:-1, 0] = -h2 / (h1 * (h1 + h2))
    c[1:-1, 1] = (h2 - h1) / (h1 * h2)
    c[1:-1, 2] = h1 / (h2 * (h1 + h2))
    c[0] = 0.0, -1.0 / h[0], 1.0 / h[0]
    c[-1] = -1.0 / h[-1], 1.0 / h[-1], 0.0
    at = np.arange(n)
    out = np.empty((n, 4))
    out[:, 0] = np.where(np.abs(lat) >= 90.0 - 1e-9, np.nan, 1.0 / (EARTH_RADIUS * cos))
    out[:, 1] = c[:, 0] * cos[np.maximum(at - 1, 0)]
    out[:, 2] = c[:, 1] * cos
    out[:, 3] = c[:, 2] * cos[np.minimum(at + 1, n - 1)]
    return out


def level_weights(levels) -> np.ndarray:
    """w_c = 100 (p_next - p_prev) / (2 g) in the order of `levels` (hPa), the neighbours taken in the sorted pressures; an end
    level takes half its one interval."""
    p = np.asarray(levels, dtype=np.float64)
    order = np.argsort(p)
    s = p[order]
    span = np.empty_like(s)
    span[1:-1] = s[2:] - s[:-2]
    span[0], span[-1] = s[1] - s[0], s[-1] - s[-2]
    w = np.empty_like(s)
    w[order] = 100.0 * span / (2.0 * GRAVITY)
    return w


def _grid(lat: np.ndarray, lon: np.ndarray) -> tuple[float, bool]:
    """(L = 1 / (2 dlambda), wrap) of a grid checked by THE GRID RULE (aurora_amd/_sphere.py); the range of the latitudes is left unchecked."""
    step, wrap = _sphere.regular_grid("diagnostics", lat, lon, least=2, in_range=False)
    return 1.0 / (2.0 * np.deg2rad(step)), wrap


# ---- the formulas on the host ---------------------------------------------------------------------------------------------
def _result(x: np.ndarray) -> np.ndarray:
    """Rounded to fp32 once; a result that is not finite is NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = x.astype(np.float32)
    r[~np.isfinite(r)] = np.nan
    return r


def _wind_host(u: np.ndarray, v: np.ndarray, rows: np.ndarray, L: float, wrap: bool, kinds) -> dict[str, np.ndarray]:
    """u, v: (..., n_lat, n_lon) float32 -> kind -> float32."""
    u, v = u.astype(np.float64), v.astype(np.float64)
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        if "ws" in kinds:
            out["ws"] = _result(np.sqrt(u * u + v * v))
        if "vo" in kinds or "div" in kinds:
            n_lat, n_lon = u.shape[-2:]
            north, south = np.maximum(np.arange(n_lat) - 1, 0), np.minimum(np.arange(n_lat) + 1, n_lat - 1)
            A, m0, m1, m2 = (rows[:, k][:, None] for k in range(4))

            def d_lon(f):
                if wrap:
                    return (np.roll(f, -1, axis=-1) - np.roll(f, 1, axis=-1)) * L
                east, west = np.minimum(np.arange(n_lon) + 1, n_lon - 1), np.maximum(np.arange(n_lon) - 1, 0)
                factor = np.full(n_lon, L)
                factor[[0, -1]] = 2.0 * L
                return (f[..., east] - f[..., west]) * factor

            def d_lat(f):
                return m0 * f[..., north, :] + m1 * f + m2 * f[..., south, :]

            if "vo" in kinds:
                out["vo"] = _result(A * (d_lon(v) - d_lat(u)))
            if "div" in kinds:
                out["div"] = _result(A * (d_lon(u) + d_lat(v)))
    return out


def _column_host(q: np.ndarray, u: Optional[np.ndarray], v: Optional[np.ndarray], w: np.ndarray, kinds) -> dict[str, np.ndarray]:
    """q, u, v: (B, C, n_lat, n_lon) float32 -> kind -> (B, n_lat, n_lon) float32; the levels added in level order."""
    sums = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for kind, f in (("tcwv", None), ("ivtu", u), ("ivtv", v)):
            if kind in kinds or (kind != "tcwv" and "ivt" in kinds):
                s = np.zeros(q.shape[:1] + q.shape[2:])
                for c in range(q.shape[1]):
                    wq = w[c] * q[:, c].astype(np.float64)
                    s += wq if f is None else wq * f[:, c].astype(np.float64)
                sums[kind] = s
        out = {kind: _result(sums[kind]) for kind in ("tcwv", "ivtu", "ivtv") if kind in kinds}
        if "ivt" in kinds:
            out["ivt"] = _result(np.sqrt(sums["ivtu"] * sums["ivtu"] + sums["ivtv"] * sums["ivtv"]))
    return out


# ---- public function ------------------------------------------------------------------------------------------------------
def diagnostics(batch: Batch, which: Union[str, Sequence[str]], keep: bool = False) -> Batch:
    """The derived fields named in `which` (a name or a sequence of `NAMES`) of the last history entry of `batch`, as a
    float32 `Batch` on the device of the inputs; see the module's text."""
    if not isinstance(batch, Batch):
        raise TypeError(f"diagnostics: batch must be a Batch, got {type(batch).__name__}")
    _fields.check_vector_grid("diagnostics", batch, "batch", band="diagnostics")
    md = batch.metadata
    which = (which,) if isinstance(which, str) else tuple(dict.fromkeys(which))
    for name in which:
        if name not in NAMES:
            raise ValueError(f"diagnostics: which offers {sorted(NAMES)}, got {name!r}")
    if not which:
        raise ValueError(f"diagnostics: which names no field; it offers {sorted(NAMES)}")
    lat, lon = _host(md.lat), _host(md.lon)
    n_lat, n_lon = lat.shape[0], lon.shape[0]
    L, wrap = _grid(lat, lon)

    # the components: the last history entry, checked
    fields: dict[str, torch.Tensor] = {}
    for name in which:
        group, _, parts = NAMES[name]
        if name in getattr(batch, group):
            raise ValueError(f"diagnostics: batch.{group} already holds {name!r}")
        for part in parts:
            part_group = "surf_vars" if part.startswith("10") else "atmos_vars"
            if part not in getattr(batch, part_group):
                raise ValueError(f"diagnostics: {name!r} needs {part!r} in batch.{part_group}, which is missing")
            f = getattr(batch, part_group)[part]
            _fields.check_field("diagnostics", f, "batch", part_group, part, n_lat, n_lon)
            fields[part] = f[:, -1]
    shapes = {tuple(f.shape[:-2]) for k, f in fields.items() if not k.startswith("10")}
    sizes = {f.shape[0] for f in fields.values()}
    if len(sizes) != 1 or len(shapes) > 1:
        raise ValueError(f"diagnostics: the variables of batch differ in batch size or levels: "
                         f"{sorted(tuple(f.shape[:-2]) for f in fields.values())}")
    B = sizes.pop()
    kinds = {group: [NAMES[n][1] for n in which if NAMES[n][0] == group and NAMES[n][1] in _WIND] for group in ("atmos_vars", "surf_vars")}
    column = [NAMES[n][1] for n in which if NAMES[n][1] in _COLUMN]
    levels = np.asarray(md.atmos_levels, dtype=np.float64)
    if column:
        C = fields["q"].shape[1]
        if levels.shape[0] != C:
            raise ValueError(f"diagnostics: batch.atmos_vars['q'] has {C} levels, the metadata names {levels.shape[0]}")
        if not 2 <= C <= MAX_LEVELS:
            raise ValueError(f"diagnostics: a vertical integral takes 2 to {MAX_LEVELS} pressure levels, the batch has {C}")
        if not np.all(np.isfinite(levels)) or np.unique(levels).shape[0] != C:
            raise ValueError(f"diagnostics: a vertical integral needs distinct pressure levels, got {tuple(md.atmos_levels)}")

    dev = _fields.device_of("diagnostics", fields.values(), batches="batch")
    out: dict[str, dict[str, torch.Tensor]] = {"surf_vars": {}, "atmos_vars": {}}
    name_of = {(NAMES[n][0], NAMES[n][1]): n for n in which}
    if dev == "cpu":
        host = {k: f.detach().to(torch.float32).numpy() for k, f in fields.items()}
        rows = row_table(lat)
        for group, (a, b) in (("atmos_vars", ("u", "v")), ("surf_vars", ("10u", "10v"))):
            if kinds[group]:
                for kind, r in _wind_host(host[a], host[b], rows, L, wrap, kinds[group]).items():
                    out[group][name_of[group, kind]] = torch.from_numpy(r)[:, None]
        if column:
            for kind, r in _column_host(host["q"], host.get("u"), host.get("v"), level_weights(levels), column).items():
                out["surf_vars"][name_of["surf_vars", kind]] = torch.from_numpy(r)[:, None]
    else:
        from aurora_amd.engine import lib

        _fields.check_planes("diagnostics", [("batch", fields, fields.values())], n_lat, n_lon, _fields.TAKES_TASK,
                             noun=lambda what, _: f"a variable of {what}")
        on_capture = ("diagnostics: call once on this grid before capturing a graph (the row and level tables are "
                      "uploaded on the first call, which a captured graph cannot replay)")
        args: dict = {}
        wind_in, wind_out = ([], []), {k: [] for k in _WIND}
        for group, (a, b) in (("atmos_vars", ("u", "v")), ("surf_vars", ("10u", "10v"))):
            if not kinds[group]:
                continue
            wind_in[0].append(fields[a]), wind_in[1].append(fields[b])
            for kind in _WIND:
                if kind in kinds[group]:
                    t = torch.empty(fields[a].shape, dtype=torch.float32, device=dev)
                    out[group][name_of[group, kind]] = t[:, None]
                    wind_out[kind].append(t)
                elif any(kind in ks for ks in kinds.values()):      # asked of the other group only: NULL entries for this one
                    wind_out[kind].append(None)
        if wind_in[0]:
            args.update(u=wind_in[0], v=wind_in[1], L=L, wrap=wrap)
            stencil = any(k in ks for ks in kinds.values() for k in ("vo", "div"))
            if stencil:
                args["row_table"] = _fields.tables.get(("rows", lat.tobytes()), dev, lambda: row_table(lat), on_capture)
            args.update({kind: ts for kind, ts in zip(("vo", "div", "ws"), (wind_out[k] for k in _WIND)) if ts})
        if column:
            args.update(q=[fields["q"]], level_w=_fields.tables.get(("levels", levels.tobytes()), dev,
                                                                      lambda: level_weights(levels), on_capture))
            if "u" in fields and any(k in column for k in ("ivtu", "ivt")):
                args["col_u"] = [fields["u"]]
            if "v" in fields and any(k in column for k in ("ivtv", "ivt")):
                args["col_v"] = [fields["v"]]
            for kind in column:
                t = torch.empty((B, n_lat, n_lon), dtype=torch.float32, device=dev)
                out["surf_vars"][name_of["surf_vars", kind]] = t[:, None]
                args[kind] = [t]
        lib.diagnostics(n_lat, n_lon, **args)

    surf = {k: v[:, -1:] for k, v in batch.surf_vars.items()} if keep else {}
    atmos = {k: v[:, -1:] for k, v in batch.atmos_vars.items()} if keep else {}
    for name in which:                                           # in the order asked for
        group = NAMES[name][0]
        (surf if group == "surf_vars" else atmos)[name] = out[group][name]
    return Batch(surf, dict(batch.static_vars), atmos, md)
