"""`aurora_amd.scores` on the device for one 0.25-degree prediction (721 x 1440; 4 surface + 5 x 13 atmospheric variables =
69 planes, 286 MB per input), with and without a climatology, beside the same metrics as a plain torch expression.

    python tools/scores_bench.py [--calls 30] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arm: the ONE aurora_hip_scores call over all 69 planes
(`lib.scores_sums`: two launches), --calls of them per graph.  Bytes read = planes x 721 x 1440 x 4 x (2 or 3 inputs), counted
here from the shapes; TB/s = bytes / that time.  Eager arms: `lib.scores_sums` and `scores()` end to end (checks, cached
tables, the call, the finalising torch operations).  Torch: what a user would write on the same device without this kernel
-- per variable, fp64 differences and accumulation, a finite mask -- in eager windows (it is device-bound).
Check: both against each other on every plane (the bound of tests/test_gpu_scores.py), and the kernel repeatable bit for
bit.  The share of a step is `scores()` issued eagerly over the 124 ms of the 0.25-degree step.
"""
import argparse
import json

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, STEP_MS, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, scores  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib
from aurora_amd.scores import latitude_weights


def batch(seed: int, base: Batch | None = None, spread: float = 1.0) -> Batch:
    """Seeded synthetic fields about 280; with `base`, base + spread x noise (a forecast near its truth)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: spread * torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    return state(r, base) if base is not None else state(lambda *s: r(*s) + 280.0)


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
    ms = alternate({"kernel": captured(kernel, calls), "eager": lambda: window_ms(kernel, calls),
                    "torch": lambda: window_ms(plain, max(3, calls // 10)), "scores": lambda: window_ms(whole, calls)}, repeats)
    n_in = 2 if clim is None else 3
    read = N_PLANES * N_LAT * N_LON * 4 * n_in
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    return {"climatology": clim is not None, "planes": N_PLANES, "grid": [N_LAT, N_LON], "read_GB": read / 1e9,
            "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"], "kernel_ms_min_max": span["kernel"],
            "kernel_TBps": read / med["kernel"] / 1e9, "eager_call_ms": med["eager"], "scores_call_ms": med["scores"], "torch_ms": med["torch"],
            "torch_ms_min_max": span["torch"], "torch_over_kernel": med["torch"] / med["kernel"],
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
