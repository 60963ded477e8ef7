"""`aurora_amd.scores` on the device for one 0.25-degree prediction (721 x 1440; 4 surface + 5 x 13 atmospheric variables =
69 planes, 286 MB per input), with and without a climatology, beside the same metrics as a plain torch expression.

    python tools/scores_bench.py [--calls 30] [--repeats 5]

Kernel: the ONE aurora_hip_scores call over all 69 planes (`lib.scores_sums`: two launches), --calls of them captured back
to back in a hipGraph and replayed between a HIP event pair after warm-up: device time per call = window / calls, free of
the host's enqueue time; repeated --repeats times (median and spread).  Bytes read = planes x 721 x 1440 x 4 x (2 or 3
inputs), counted here from the shapes; TB/s = bytes / that time.  Also the same window issued eagerly, for `lib.scores_sums`
and for `scores()` end to end (checks, cached tables, the call, the finalising torch operations): there the host's enqueue
rate counts too.  Torch: what a user would write on the same device without this kernel -- per variable, fp64 differences
and accumulation, a finite mask -- in eager windows (it is device-bound), alternating with the kernel inside each repeat.
Check: both against each other on every plane (the bound of tests/test_gpu_scores.py), and the kernel repeatable bit for
bit.  The share of a step is `scores()` issued eagerly over the 124 ms of the 0.25-degree step.
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
from aurora_amd import Batch, Metadata, scores  # noqa: E402
from aurora_amd.engine import lib  # noqa: E402
from aurora_amd.scores import latitude_weights  # noqa: E402

SURF, ATMOS, LEVELS = ("2t", "10u", "10v", "msl"), ("z", "u", "v", "t", "q"), 13
N_LAT, N_LON = 721, 1440
N_PLANES = len(SURF) + len(ATMOS) * LEVELS
STEP_MS = 124.0


def batch(seed: int, base: Batch | None = None, spread: float = 1.0) -> Batch:
    """Seeded synthetic fields; with `base`, base + spread x noise (a forecast near its truth)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.linspace(90, -90, N_LAT, dtype=torch.float64)
    lon = torch.linspace(0, 360, N_LON + 1, dtype=torch.float64)[:-1]
    r = lambda *s: spread * torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    md = base.metadata if base is not None else Metadata(lat=lat, lon=lon, time=(datetime(2022, 5, 11, 12),),
                                                         atmos_levels=tuple(range(50, 50 + 75 * LEVELS, 75)))
    surf = {k: r(1, 1) + (base.surf_vars[k] if base is not None else 280.0) for k in SURF}
    atmos = {k: r(1, 1, LEVELS) + (base.atmos_vars[k] if base is not None else 280.0) for k in ATMOS}
    return Batch(surf, {}, atmos, md)


def planes(b: Batch) -> list[torch.Tensor]:
    return [v[:, -1] for v in (*b.surf_vars.values(), *b.atmos_vars.values())]


def torch_sums(p: torch.Tensor, t: torch.Tensor, c: torch.Tensor | None, w: torch.Tensor) -> torch.Tensor:
    """The eight sums of one variable (..., n_lat, n_lon) as a plain torch expression: fp64, masked like nansum."""
    p, t = p.double(), t.double()
    ok = torch.isfinite(p) & torch.isfinite(t)
    if c is not None:
        c = c.double()
        ok &= torch.isfinite(c)
    zero = torch.zeros((), dtype=torch.float64, device=p.device)
    W = torch.where(ok, w[:, None], zero)
    d = torch.where(ok, p - t, zero)
    total = lambda x: x.sum(dim=(-2, -1))  # noqa: E731
    out = [total(ok.double()), total(W), total(W * d), total(W * d * d), total(W * d.abs())]
    if c is not None:
        pa, ta = torch.where(ok, p - c, zero), torch.where(ok, t - c, zero)
        out += [total(W * pa * ta), total(W * pa * pa), total(W * ta * ta)]
    else:
        out += [torch.zeros_like(out[0])] * 3
    return torch.stack(out, dim=-1).reshape(-1, 8)


def window_ms(fn, calls: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def case(pred: Batch, truth: Batch, clim: Batch | None, calls: int, repeats: int) -> dict:
    w = torch.from_numpy(latitude_weights(pred.metadata.lat.numpy())).cuda()
    P, T, C = planes(pred), planes(truth), None if clim is None else planes(clim)
    kernel = lambda: lib.scores_sums(P, T, C, w)  # noqa: E731
    whole = lambda: scores(pred, truth, clim)  # noqa: E731
    plain = lambda: torch.cat([torch_sums(p, t, None if C is None else C[i], w) for i, (p, t) in enumerate(zip(P, T))])  # noqa: E731
    got, again, want = kernel(), kernel(), plain()
    whole()
    torch.cuda.synchronize()
    assert torch.equal(got, again), "the kernel's sums are not repeatable"
    g, y = got.cpu().numpy(), want.cpu().numpy()
    assert g.shape == (N_PLANES, 8) and (g[:, 0] == y[:, 0]).all()
    worst = 0.0
    for s, bound in ((1, y[:, 1]), (2, y[:, 4]), (3, y[:, 3]), (4, y[:, 4])) + (
            ((5, np.sqrt(y[:, 6] * y[:, 7])), (6, y[:, 6]), (7, y[:, 7])) if clim is not None else ()):
        worst = max(worst, float(np.max(np.abs(g[:, s] - y[:, s]) / bound)))
    assert worst <= 1e-9, worst
    for f in (kernel, whole, plain):
        window_ms(f, 3)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            kernel()
    window_ms(graph.replay, 2)
    ms = {"kernel": [], "eager": [], "scores": [], "torch": []}
    for _ in range(repeats):                                  # alternate the arms inside every repeat
        ms["kernel"].append(window_ms(graph.replay, 1) / calls)
        ms["eager"].append(window_ms(kernel, calls))
        ms["torch"].append(window_ms(plain, max(3, calls // 10)))
        ms["scores"].append(window_ms(whole, calls))
    n_in = 2 if clim is None else 3
    read = N_PLANES * N_LAT * N_LON * 4 * n_in
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"climatology": clim is not None, "planes": N_PLANES, "grid": [N_LAT, N_LON], "read_GB": read / 1e9,
            "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"], "kernel_ms_min_max": [min(ms["kernel"]), max(ms["kernel"])],
            "kernel_TBps": read / med["kernel"] / 1e9, "eager_call_ms": med["eager"], "scores_call_ms": med["scores"], "torch_ms": med["torch"],
            "torch_ms_min_max": [min(ms["torch"]), max(ms["torch"])], "torch_over_kernel": med["torch"] / med["kernel"],
            "share_of_step_percent": 100 * med["scores"] / STEP_MS, "worst_error_over_bound_1e-9": worst / 1e-9}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="back-to-back calls per timed window (>= 20)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert args.calls >= 20
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} per input "
          f"({N_PLANES * N_LAT * N_LON * 4 / 1e6:.0f} MB)", flush=True)
    truth = batch(0)
    pred = batch(1, truth, spread=0.02)
    clim = batch(2, truth, spread=0.3)
    for c in (None, clim):
        rec = case(pred, truth, c, args.calls, args.repeats)
        print(f"climatology {'yes' if rec['climatology'] else 'no '}: {rec['read_GB']:.3f} GB read: kernel call "
              f"{rec['kernel_ms']:.3f} ms (device time, median of {rec['repeats']} graph replays of {rec['calls_per_window']} calls; "
              f"{rec['kernel_ms_min_max'][0]:.3f}-{rec['kernel_ms_min_max'][1]:.3f}) = {rec['kernel_TBps']:.2f} TB/s; "
              f"issued eagerly {rec['eager_call_ms']:.3f} ms per call; scores() end to end {rec['scores_call_ms']:.3f} ms = {rec['share_of_step_percent']:.2f} % of a "
              f"{STEP_MS:.0f} ms step; torch expression {rec['torch_ms']:.2f} ms = {rec['torch_over_kernel']:.1f} x the kernel "
              f"call; agreement {rec['worst_error_over_bound_1e-9']:.2e} of the 1e-9 bound", flush=True)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
