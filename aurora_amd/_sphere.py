"""The sphere of the verification modules (`diagnostics`, `objects`, `object_matches`, `nearest_event`, `smooth`, `extrema`,
`conservative_regrid`, `spectra`): the Earth radius, THE GRID RULE -- when longitudes are equally spaced, when they cover the full
circle, what latitudes may be -- on the host in numpy fp64, and the great-circle arithmetic in torch that gives the same bits on
every device.  The rule is stated here and nowhere else; the modules' own texts point to it.

(`tracker` and `engine/encodings` carry the radii of the reference model: another contract.)"""

from __future__ import annotations

import math

import numpy as np
import torch

EARTH_RADIUS = 6371229.0      # metres
MAX_LON = 4096                # the longitudes the kernels take


# ---- THE GRID RULE -----------------------------------------------------------------------------------------------------
def equally_spaced(lon: np.ndarray, step: float) -> bool:
    """Is lon[j] = lon[0] + j step to a millionth of a step?  (`step` may be negative: a descending axis.)"""
    return bool(np.all(np.abs(lon - lon[0] - np.arange(lon.shape[0], dtype=np.float64) * step) <= 1e-6 * abs(step)))


def full_circle(lon: np.ndarray) -> bool:
    """Does the grid WRAP in longitude: 2 to `MAX_LON` longitudes, equally spaced at a step of 360 / n?  Raises nothing.

    The limit is part of the predicate: a grid of more than `MAX_LON` equally spaced longitudes around the circle does NOT count
    as one, so `diagnostics`, `smooth` and `conservative_regrid` take it as regional (one-sided differences, clipped windows and
    uncovered cells at the seam) without saying so, while `spectra` and `objects` refuse it."""
    n = lon.shape[0]
    return 2 <= n <= MAX_LON and equally_spaced(lon, 360.0 / n)


def check_latitudes(fn: str, lat: np.ndarray, of: str = "", in_range: bool = True, monotonic: str = "monotonic") -> None:
    """Latitudes are finite and within [-90, 90] (`in_range`) and strictly ascending or strictly descending (`monotonic`: the
    module's word for it, or None where any order will do).  `of`: whose they are, where the message says so."""
    if in_range and (not np.all(np.isfinite(lat)) or lat.max() > 90 or lat.min() < -90):
        raise ValueError(f"{fn}: {'the latitudes' + of if of else 'latitudes'} must be in the range [-90, 90]")
    if monotonic and not (np.all(np.diff(lat) > 0) or np.all(np.diff(lat) < 0)):
        raise ValueError(f"{fn}: the latitudes{of} must be strictly {monotonic}")


def regular_grid(fn: str, lat: np.ndarray, lon: np.ndarray, least: int, in_range: bool) -> tuple[float, bool]:
    """(longitude step in degrees, wrap) of a grid with at least `least` rows and columns, checked latitudes and equally spaced
    ascending longitudes: one that is a `full_circle` wraps, any other is regional.  A single column has step 0."""
    n_lat, n_lon = lat.shape[0], lon.shape[0]
    if n_lat < least or n_lon < least:
        raise ValueError(f"{fn}: the grid has {n_lat} latitudes and {n_lon} longitudes; at least {least} of each "
                         f"{'is' if least == 1 else 'are'} needed")
    check_latitudes(fn, lat, in_range=in_range)
    if n_lon == 1:
        return 0.0, False
    if full_circle(lon):
        return 360.0 / n_lon, True
    step = (lon[-1] - lon[0]) / (n_lon - 1)
    if not step > 0 or not equally_spaced(lon, step):
        raise ValueError(f"{fn}: the longitudes must be equally spaced")
    return step, False


# ---- great-circle arithmetic: the same torch code, and the same bits, on either device -------------------------------------
def _sin(x: torch.Tensor) -> torch.Tensor:
    """sin x for |x| <= pi / 2 (fp64): the Taylor polynomial to x^27 by Horner's rule in x^2 -- products and sums only, so the
    same bits on every device; the first term left out is below 2e-23."""
    x2 = x * x
    s = torch.full_like(x, -1.0 / math.factorial(27))
    sign = 1.0
    for k in range(25, 0, -2):
        s = s * x2 + sign / math.factorial(k)
        sign = -sign
    return s * x


def _sqrt(x: torch.Tensor) -> torch.Tensor:
    """sqrt x for x >= 0 (fp64, normal numbers or 0) to an ulp or two, from integer operations, products and sums alone:
    `torch.sqrt` of an fp64 tensor is correctly rounded on the CPU and not on the GPU (measured on an MI355X: one value in 70
    differs in the last bit).  The reciprocal root starts from the shifted bit pattern (off by at most 3.5 %), takes five Newton
    steps r <- r (3/2 - x/2 r^2), which square the error each time, and one correction of x r with the residual."""
    safe = torch.where(x > 0, x, torch.ones_like(x))
    r = (0x5FE6EB50C7B537A9 - (safe.view(torch.int64) >> 1)).view(torch.float64)
    half = 0.5 * safe
    for _ in range(5):
        r = r * (1.5 - half * (r * r))
    root = safe * r
    root = root + (0.5 * r) * (safe - root * root)
    return torch.where(x > 0, root, torch.zeros_like(x))


def _asin(s: torch.Tensor) -> torch.Tensor:
    """asin s for 0 <= s <= 1 (fp64): the angle is halved twice, sin(y / 2) = s / sqrt(2 (1 + sqrt(1 - s^2))), which brings the
    argument below sin(pi / 8) = 0.383; there the Maclaurin series to t^61 (the first term left out is below 1e-28); products,
    sums, quotients of tensors and `_sqrt` only, so the same bits on every device."""
    t = s
    for _ in range(2):
        t = t / _sqrt(2.0 * (1.0 + _sqrt((1.0 - t * t).clamp(min=0.0))))
    t2 = t * t
    coefficient = [1.0]                                    # of t^(2 k + 1): prod (2 i - 1) / (2 i) over i <= k, over 2 k + 1
    for k in range(1, 31):
        coefficient.append(coefficient[-1] * (2 * k - 1) / (2 * k))
    coefficient = [c / (2 * k + 1) for k, c in enumerate(coefficient)]
    y = torch.full_like(t, coefficient[-1])
    for c in reversed(coefficient[:-1]):
        y = y * t2 + c
    return 4.0 * (y * t)


def haversine_km(lat1: torch.Tensor, lon1: torch.Tensor, lat2: torch.Tensor, lon2: torch.Tensor) -> torch.Tensor:
    """The great-circle distance by the haversine formula, degrees in, kilometres out."""
    rad = math.pi / 180.0
    dlon = lon2 - lon1
    dlon = dlon - 360.0 * torch.round(dlon * (1.0 / 360.0))   # into [-180, 180]; (a tensor divided by a number is multiplied by
    #                                                            the number's reciprocal on the GPU and divided on the CPU)
    cos = lambda x: 1.0 - 2.0 * _sin(0.5 * x) ** 2         # noqa: E731
    sa, sb = _sin(0.5 * rad * (lat2 - lat1)), _sin(0.5 * rad * dlon)
    h = sa * sa + cos(rad * lat1) * cos(rad * lat2) * (sb * sb)
    return (2.0 * EARTH_RADIUS / 1000.0) * _asin(_sqrt(h.clamp(0.0, 1.0)))


def _km(key: torch.Tensor) -> torch.Tensor:
    """EARTH_RADIUS / 1000 * 2 asin(sqrt(key / 2)) for keys 1 - cos(angle), finite in [0, 2]; +inf for +inf; products, sums and
    quotients of tensors alone (`_sqrt`, `_asin`), so the same bits on either device.  (key * 0.5 is exact.)"""
    finite = torch.isfinite(key)
    half = torch.where(finite, key, torch.zeros_like(key)) * 0.5
    km = (2.0 * EARTH_RADIUS / 1000.0) * _asin(_sqrt(half.clamp(0.0, 1.0)))
    return torch.where(finite, km, torch.full_like(km, float("inf")))
