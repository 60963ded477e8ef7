"""Inputs that more than one verification test module (scores, ensemble_scores, spectra, event_scores, probability_scores,
field_stats, diagnostics, conditional_scores) uses: seeded fields and batches, latitude weights, thresholds, and the device
copy that reaches the unaligned path of the kernels.  The fp64 yardsticks and the bounds stay with the module they judge."""
from datetime import datetime

import numpy as np
import torch

from aurora_amd import Batch, Metadata

DEV = torch.device("cuda:0")
LEVELS = (100, 500, 850)


def carve(values, offset_floats=0, fill=0.0) -> torch.Tensor:
    """A device copy of `values` (a numpy array or a tensor of any float dtype) as fp32, carved out of a flat buffer filled
    with `fill`, `offset_floats` past its 256-byte-aligned start; the planes follow each other unpadded.  The kernels read
    four floats at a time where every plane pointer is 16-byte aligned and n_lon % 4 == 0, and one at a time otherwise: with
    an offset of 1 no plane pointer is 16-byte aligned, so the same values go down the other path."""
    values = torch.as_tensor(values)
    flat = torch.full((offset_floats + values.numel(),), fill, dtype=torch.float32)
    flat[offset_floats:] = values.reshape(-1).float()
    return flat.to(DEV)[offset_floats:].view(values.shape)


def cos_weights(lat_deg) -> np.ndarray:
    """The tests' own weights: cos(lat) / mean cos(lat)."""
    c = np.cos(np.deg2rad(np.asarray(lat_deg, dtype=np.float64)))
    return c / c.mean()


def weights(n_lat) -> np.ndarray:
    return cos_weights(np.linspace(90, -90, n_lat)) if n_lat > 1 else np.ones(1)


def red_noise(shape, seed, mean=5e4, amp=500.0):
    """Rows with a realistic offset and tail: `mean` plus noise with a k^-3 amplitude spectrum, rounded to fp32."""
    g = np.random.default_rng(seed)
    N = shape[-1]
    K = N // 2 + 1
    a = np.zeros(K)
    a[1:] = amp * np.arange(1, K, dtype=np.float64) ** -3.0
    X = a * np.exp(2j * np.pi * g.random((*shape[:-1], K))) * N / 2
    return (mean + np.fft.irfft(X, n=N, axis=-1)).astype(np.float32)


def randn_batch(n_lat, n_lon, seed=0, B=2, T=2, offset=0.0, scale=1.0, dtype=torch.float32, levels=LEVELS):
    """White noise: 2 surface variables + 1 three-level variable, B = 2, two history entries (only the last one is scored)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (offset + scale * torch.randn(*s, n_lat, n_lon, generator=g, dtype=torch.float64)).to(dtype)  # noqa: E731
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1)[:-1],
                  time=tuple(datetime(2023, 1, 1, 6) for _ in range(B)), atmos_levels=tuple(levels))
    return Batch({"2t": r(B, T), "msl": r(B, T)}, {"lsm": r()}, {"z": r(B, T, len(levels))}, md)


def red_noise_batch(n_lat, n_lon, seed=0, B=2, T=2, levels=LEVELS, mean=5e4, dtype=torch.float32):
    """`red_noise` in the layout of `randn_batch`; a single row sits on the equator."""
    r = lambda k, *s: torch.from_numpy(red_noise((*s, n_lat, n_lon), seed * 10 + k, mean=mean)).to(dtype)  # noqa: E731
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64) if n_lat > 1 else torch.zeros(1, dtype=torch.float64),
                  lon=torch.linspace(0, 360, n_lon + 1, dtype=torch.float64)[:-1],
                  time=tuple(datetime(2023, 1, 1, 6) for _ in range(B)), atmos_levels=tuple(levels))
    return Batch({"2t": r(0, B, T), "msl": r(1, B, T)}, {"lsm": r(2)}, {"z": r(3, B, T, len(levels))}, md)


def shifted(b: Batch, f) -> Batch:
    return Batch({k: f(v.clone()) for k, v in b.surf_vars.items()}, b.static_vars,
                 {k: f(v.clone()) for k, v in b.atmos_vars.items()}, b.metadata)


def every(d: dict) -> np.ndarray:
    return np.concatenate([v.numpy().reshape(-1) for v in d.values()])


def planes_of(b: Batch):
    """(name, index, plane) of every scored plane of a batch, in the order of the result's layout."""
    for grp in ("surf_vars", "atmos_vars"):
        for k, v in getattr(b, grp).items():
            last = v[:, -1].cpu().numpy()
            for idx in np.ndindex(*last.shape[:-2]):
                yield k, idx, last[idx]


def quantile_thresholds(x, extra=()):
    """About the 0.5, 0.9 and 0.99 quantiles of the finite values, as float32, plus `extra`."""
    v = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.quantile(v[np.isfinite(v)], [0.5, 0.9, 0.99]), np.asarray(extra, dtype=np.float64)]).astype(np.float32)


def thresholds_of(t: np.ndarray, T: int) -> np.ndarray:
    """(n_planes, T) float32 from each truth plane: T = 5: three quantiles, above the maximum, NaN; T = 4: quantiles and NaN;
    T = 8: the five, then three more quantiles."""
    rows = []
    for x in t:
        v = x[np.isfinite(x)] if np.isfinite(x).any() else np.zeros(1, dtype=np.float32)
        q = quantile_thresholds(v)
        five = [*q, np.float32(v.max() + 1000), np.float32("nan")]
        rows.append({4: [*q, np.float32("nan")], 5: five,
                     8: five + list(np.quantile(v.astype(np.float64), [0.1, 0.75, 0.999]).astype(np.float32))}[T])
    return np.asarray(rows, dtype=np.float32)
