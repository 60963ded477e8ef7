"""`aurora_amd.spectra` on the device for one 0.25-degree state (721 x 1440; 4 surface + 5 x 13 atmospheric variables =
69 planes), with and without a truth, beside the same quantities as a `torch.fft.rfft` fp64 expression.

    python tools/spectra_bench.py [--calls 20] [--repeats 5]

Kernel: the ONE aurora_hip_spectra call over all 69 planes (`lib.spectra_power`: two launches), --calls of them captured
back to back in a hipGraph and replayed between a HIP event pair after warm-up: device time per call = window / calls;
repeated --repeats times (median and spread).  FLOP of the folded transform = 2 x rows x K x 2 K per field with
K = 721 (rows = 69 x 721; the direct form would be twice that), counted here from the shapes; the fp64 rate is FLOP / that
time.  Also `spectra()` issued eagerly, end to end.  Torch: what a user would write on the same device without this kernel
-- per variable, the fp64 cast, torch.fft.rfft, |X|^2, the band-weighted row mean; the error spectrum from the difference of
the two transforms -- in eager windows (it is device-bound), alternating with the kernel inside each repeat: a yardstick
only.  Check: both against each other on every value (pred and truth relative to the plane's largest; the error field, a
difference of two transforms on both sides, under the derived bound), and the kernel repeatable bit for bit.  The share of a step is `spectra()` issued eagerly over the 124 ms of the 0.25-degree step.
"""
import argparse
import json
import statistics
import sys
from datetime import datetime
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from aurora_amd import Batch, Metadata, spectra  # noqa: E402
from aurora_amd.engine import lib  # noqa: E402
from aurora_amd.spectra import band_weights  # noqa: E402

SURF, ATMOS, LEVELS = ("2t", "10u", "10v", "msl"), ("z", "u", "v", "t", "q"), 13
N_LAT, N_LON = 721, 1440
K = N_LON // 2 + 1
N_PLANES = len(SURF) + len(ATMOS) * LEVELS
STEP_MS = 124.0


def batch(seed: int, base: Batch | None = None, spread: float = 1.0) -> Batch:
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.linspace(90, -90, N_LAT, dtype=torch.float64)
    lon = torch.linspace(0, 360, N_LON + 1, dtype=torch.float64)[:-1]
    r = lambda *s: spread * torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    md = base.metadata if base is not None else Metadata(lat=lat, lon=lon, time=(datetime(2022, 5, 11, 12),),
                                                         atmos_levels=tuple(range(50, 50 + 75 * LEVELS, 75)))
    surf = {k: r(1, 1) + (base.surf_vars[k] if base is not None else 5e4) for k in SURF}
    atmos = {k: r(1, 1, LEVELS) + (base.atmos_vars[k] if base is not None else 5e4) for k in ATMOS}
    return Batch(surf, {}, atmos, md)


def planes(b: Batch) -> list[torch.Tensor]:
    return [v[:, -1] for v in (*b.surf_vars.values(), *b.atmos_vars.values())]


def torch_power(p: torch.Tensor, t: torch.Tensor | None, bw: torch.Tensor, ck: torch.Tensor) -> torch.Tensor:
    """(planes, 1 or 3, n_bands, K) of one variable (..., n_lat, n_lon) as a plain torch expression in fp64."""
    fields = [p.double()] + ([t.double()] if t is not None else [])
    ok = torch.stack([torch.isfinite(f).all(dim=-1) for f in fields]).all(dim=0)              # (..., n_lat)
    X = [torch.fft.rfft(torch.where(ok[..., None], f, 0.0), dim=-1) for f in fields]
    if t is not None:
        X.append(X[0] - X[1])
    w = bw * ok[..., None, :]                                                                  # (..., n_bands, n_lat)
    out = [torch.einsum("...bi,...ik->...bk", w, (x.real ** 2 + x.imag ** 2) * ck) / w.sum(dim=-1, keepdim=True) for x in X]
    return torch.stack(out, dim=-3).reshape(-1, len(X), bw.shape[0], K)


def window_ms(fn, calls: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def case(pred: Batch, truth: Batch | None, calls: int, repeats: int) -> dict:
    bands = ((-90.0, 90.0),)
    bw = torch.from_numpy(band_weights(pred.metadata.lat.numpy(), bands)).cuda()
    ck = torch.full((K,), 2.0, dtype=torch.float64, device="cuda") / (N_LON * N_LON)
    ck[0] /= 2
    ck[-1] /= 2
    P, T = planes(pred), None if truth is None else planes(truth)
    kernel = lambda: lib.spectra_power(P, T, bw)  # noqa: E731
    whole = lambda: spectra(pred, truth, bands=bands)  # noqa: E731
    plain = lambda: torch.cat([torch_power(p, None if T is None else T[i], bw, ck) for i, p in enumerate(P)])  # noqa: E731
    got, again, want = kernel(), kernel(), plain()
    whole()
    torch.cuda.synchronize()
    assert torch.equal(got[0], again[0]), "the kernel's spectra are not repeatable"
    g, y = got[0].cpu().numpy(), want.cpu().numpy()
    worst = float(np.max(np.abs(g - y)[:, :2] / np.abs(y).max(axis=-1, keepdims=True)[:, :2]))
    assert worst <= 1e-11, worst
    if truth is not None:
        # the error field is X_pred - X_truth on both sides: each within E = (N + 8) u (sum|pred| + sum|truth|) of a row, so
        # the powers differ by at most 2 c_k (2 |X| E + E^2) / N^2 (tests/test_gpu_spectra.py), taken at the largest |X|
        E = (N_LON + 8) * 2.0 ** -53 * max(float((p.double().abs().sum(-1) + t.double().abs().sum(-1)).max()) for p, t in zip(P, T))
        X = N_LON * np.sqrt(y[:, 2].max(axis=-1, keepdims=True) / 2)
        assert (np.abs(g - y)[:, 2] <= 4 * (2 * X * E + E * E) / N_LON ** 2).all()
    for f in (kernel, whole, plain):
        window_ms(f, 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            kernel()
    window_ms(graph.replay, 1)
    ms = {"kernel": [], "spectra": [], "torch": []}
    for _ in range(repeats):                                  # alternate the arms inside every repeat
        ms["kernel"].append(window_ms(graph.replay, 1) / calls)
        ms["torch"].append(window_ms(plain, max(3, calls // 4)))
        ms["spectra"].append(window_ms(whole, calls))
    n_fields = 1 if truth is None else 2
    flop = 2.0 * n_fields * N_PLANES * N_LAT * K * (2 * K)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"truth": truth is not None, "planes": N_PLANES, "grid": [N_LAT, N_LON], "folded_GFLOP": flop / 1e9,
            "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"],
            "kernel_ms_min_max": [min(ms["kernel"]), max(ms["kernel"])], "fp64_TFLOPs": flop / med["kernel"] / 1e9,
            "spectra_call_ms": med["spectra"], "torch_ms": med["torch"], "torch_ms_min_max": [min(ms["torch"]), max(ms["torch"])],
            "torch_over_kernel": med["torch"] / med["kernel"], "share_of_step_percent": 100 * med["spectra"] / STEP_MS,
            "worst_difference_over_plane_max": worst}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} per input", flush=True)
    truth = batch(0)
    pred = batch(1, truth, spread=0.02)
    for t in (None, truth):
        rec = case(pred, t, args.calls, args.repeats)
        print(f"truth {'yes' if rec['truth'] else 'no '}: {rec['folded_GFLOP']:.0f} GFLOP (folded): kernel call {rec['kernel_ms']:.3f} ms "
              f"(device time, median of {rec['repeats']} graph replays of {rec['calls_per_window']} calls; "
              f"{rec['kernel_ms_min_max'][0]:.3f}-{rec['kernel_ms_min_max'][1]:.3f}) = {rec['fp64_TFLOPs']:.1f} TFLOP/s fp64; spectra() end to "
              f"end {rec['spectra_call_ms']:.3f} ms = {rec['share_of_step_percent']:.2f} % of a {STEP_MS:.0f} ms step; torch.fft expression "
              f"{rec['torch_ms']:.2f} ms ({rec['torch_ms_min_max'][0]:.2f}-{rec['torch_ms_min_max'][1]:.2f}) = {rec['torch_over_kernel']:.2f} x the "
              f"kernel call; largest difference {rec['worst_difference_over_plane_max']:.1e} of a plane's largest value", flush=True)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
