"""`aurora_amd.spectra` on the device for one 0.25-degree state (721 x 1440; 4 surface + 5 x 13 atmospheric variables =
69 planes), with and without a truth, beside the same quantities as a `torch.fft.rfft` fp64 expression.

    python tools/spectra_bench.py [--calls 20] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arm: the ONE aurora_hip_spectra call over all 69 planes
(`lib.spectra_power`: two launches), --calls of them per graph.  FLOP of the folded transform = 2 x rows x K x 2 K per field
with K = 721 (rows = 69 x 721; the direct form would be twice that), counted here from the shapes; the fp64 rate is FLOP /
that time.  Eager arm: `spectra()` end to end.  Torch: what a user would write on the same device without this kernel
-- per variable, the fp64 cast, torch.fft.rfft, |X|^2, the band-weighted row mean; the error spectrum from the difference of
the two transforms -- in eager windows (it is device-bound): a yardstick only.  Check: both against each other on every value
(pred and truth relative to the plane's largest; the error field, a difference of two transforms on both sides, under the
derived bound), and the kernel repeatable bit for bit.  The share of a step is `spectra()` issued eagerly over the 124 ms of
the 0.25-degree step.
"""
import argparse
import json

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, STEP_MS, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, spectra  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib
from aurora_amd.spectra import band_weights

K = N_LON // 2 + 1


def batch(seed: int, base: Batch | None = None, spread: float = 1.0) -> Batch:
    """Seeded synthetic fields about 5e4; with `base`, base + spread x noise."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: spread * torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    return state(r, base) if base is not None else state(lambda *s: r(*s) + 5e4)


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
        window_ms(f, 3)
    ms = alternate({"kernel": captured(kernel, calls), "torch": lambda: window_ms(plain, max(3, calls // 4)),
                    "spectra": lambda: window_ms(whole, calls)}, repeats)
    n_fields = 1 if truth is None else 2
    flop = 2.0 * n_fields * N_PLANES * N_LAT * K * (2 * K)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    return {"truth": truth is not None, "planes": N_PLANES, "grid": [N_LAT, N_LON], "folded_GFLOP": flop / 1e9,
            "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"],
            "kernel_ms_min_max": span["kernel"], "fp64_TFLOPs": flop / med["kernel"] / 1e9,
            "spectra_call_ms": med["spectra"], "torch_ms": med["torch"], "torch_ms_min_max": span["torch"],
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
