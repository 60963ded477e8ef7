"""`aurora_amd.conditional_scores` on the device for one 0.25-degree prediction (721 x 1440; 4 surface + 5 x 13 atmospheric
variables = 69 planes, 286 MB per input), with E = 4 and E = 8 edges, with and without centre + scale maps, beside
`aurora_hip_scores` as the read-rate yardstick and beside the same sums as a plain torch expression.

    python tools/conditional_scores_bench.py [--calls 30] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arm: the ONE aurora_hip_conditional_scores call over all 69 planes
(`lib.conditional_sums`: two launches), --calls of them per graph.  Bytes read = planes x 721 x 1440 x (8 or 16 per point),
counted here from the shapes.  Yardstick: `lib.scores_sums` without a climatology, a graph arm too; its rate says what one
read of the conditional call's inputs takes, and `x_read` is the conditional call over that time.  Eager arms:
`lib.conditional_sums` and `conditional_scores()` end to end (checks, cached tables, the call, the finalising torch
operations).  Torch: what a user would write on the same device without this kernel -- per variable, fp64, a bin index from
comparisons and one masked sum per bin and slot -- in eager windows.  Check: kernel and torch expression against each other
on every plane and bin (integers equal, the bound of tests/test_gpu_conditional_scores.py), and the kernel repeatable bit
for bit.
"""
import argparse
import json

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, conditional_scores  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib
from aurora_amd.scores import latitude_weights

EDGES = {4: (-1.5, -0.5, 0.5, 1.5), 8: (-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0)}


def batch(seed: int, base: Batch | None = None, spread: float = 1.0) -> Batch:
    """Seeded synthetic fields about 280 (those of tools/scores_bench.py); with `base`, base + spread x noise."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: spread * torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    return state(r, base) if base is not None else state(lambda *s: r(*s) + 280.0)


def torch_sums(p, t, c, s, edges, w) -> torch.Tensor:
    """(planes of the variable, E + 1, 5) as a plain torch expression: fp64, the rule of aurora_amd/conditional.py."""
    p, t = p.double(), t.double()
    ok = torch.isfinite(p) & torch.isfinite(t)
    a = t
    if c is not None:
        c = c.double()
        ok &= torch.isfinite(c)
        a = a - c
    if s is not None:
        s = s.double()
        ok &= torch.isfinite(s) & (s >= 0)
    bins = torch.zeros_like(p, dtype=torch.int32)
    for e in edges:
        bins += a >= (float(np.float32(e)) * s if s is not None else float(np.float32(e)))
    zero = torch.zeros((), dtype=torch.float64, device=p.device)
    d = p - t
    total = lambda x: x.sum(dim=(-2, -1))  # noqa: E731
    out = []
    for b in range(len(edges) + 1):
        m = ok & (bins == b)
        W, db = torch.where(m, w[:, None], zero), torch.where(m, d, zero)
        out.append(torch.stack([total(m.double()), total(W), total(W * db), total(W * db * db), total(W * db.abs())], dim=-1))
    return torch.stack(out, dim=-2).reshape(-1, len(edges) + 1, 5)


def case(pred: Batch, truth: Batch, centre, scale, E: int, calls: int, repeats: int) -> dict:
    w = torch.from_numpy(latitude_weights(pred.metadata.lat.numpy())).cuda()
    P, T = planes(pred), planes(truth)
    C, S = (None if centre is None else planes(centre)), (None if scale is None else planes(scale))
    unit = 1.0 if scale is not None else 0.3
    values = tuple(np.float32(e * unit) for e in EDGES[E])
    table = torch.tensor([values] * N_PLANES, dtype=torch.float32, device="cuda")
    edges = {k: values for k in (*pred.surf_vars, *pred.atmos_vars)}
    kernel = lambda: lib.conditional_sums(P, T, C, S, table, False, w)  # noqa: E731
    yard = lambda: lib.scores_sums(P, T, None, w)  # noqa: E731
    whole = lambda: conditional_scores(pred, truth, edges, centre=centre, scale=scale)  # noqa: E731
    plain = lambda: torch.cat([torch_sums(p, t, None if C is None else C[i], None if S is None else S[i], values, w)  # noqa: E731
                               for i, (p, t) in enumerate(zip(P, T))])
    got, again, want = kernel(), kernel(), plain()
    whole()
    torch.cuda.synchronize()
    assert torch.equal(got, again), "the kernel's sums are not repeatable"
    g, y = got.cpu().numpy(), want.cpu().numpy()
    assert g.shape == (N_PLANES, E + 1, 5) and (g[..., 0] == y[..., 0]).all(), "bin membership differs"
    assert (y[..., 0] >= 0.01 * y[..., 0].sum(axis=1, keepdims=True)).all(), "a bin holds less than 1 % of the points"
    worst = max(float(np.max(np.abs(g[..., s] - y[..., s]) / bound)) for s, bound in ((1, y[..., 1]), (2, y[..., 4]), (3, y[..., 3]), (4, y[..., 4])))
    assert worst <= 1e-9, worst
    for f in (kernel, yard, whole, plain):
        window_ms(f, 3)
    ms = alternate({"kernel": captured(kernel, calls), "yardstick": captured(yard, calls), "eager": lambda: window_ms(kernel, calls),
                    "whole": lambda: window_ms(whole, calls), "torch": lambda: window_ms(plain, max(3, calls // 10))}, repeats)
    n_in = 2 + (centre is not None) + (scale is not None)
    read = N_PLANES * N_LAT * N_LON * 4 * n_in
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    yard_rate = N_PLANES * N_LAT * N_LON * 8 / med["yardstick"] / 1e9                   # TB/s
    one_read_ms = read / yard_rate / 1e9
    return {"edges": E, "maps": centre is not None, "planes": N_PLANES, "grid": [N_LAT, N_LON], "bytes_per_point": 4 * n_in,
            "read_GB": read / 1e9, "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"],
            "kernel_ms_min_max": span["kernel"], "kernel_TBps": read / med["kernel"] / 1e9,
            "scores_ms": med["yardstick"], "scores_ms_min_max": span["yardstick"], "scores_TBps": yard_rate,
            "one_read_ms": one_read_ms, "x_read": med["kernel"] / one_read_ms, "eager_call_ms": med["eager"],
            "conditional_scores_call_ms": med["whole"], "torch_ms": med["torch"], "torch_ms_min_max": span["torch"],
            "torch_over_kernel": med["torch"] / med["kernel"], "worst_error_over_bound_1e-9": worst / 1e-9}


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
    centre = batch(2, truth, spread=0.3)                      # truth - centre ~ N(0, 0.3^2)
    scale = Batch({k: torch.full_like(v, 0.3) for k, v in truth.surf_vars.items()}, {},
                  {k: torch.full_like(v, 0.3) for k, v in truth.atmos_vars.items()}, truth.metadata)
    flat = Batch({k: torch.full_like(v, 280.0) for k, v in truth.surf_vars.items()}, {},
                 {k: torch.full_like(v, 280.0) for k, v in truth.atmos_vars.items()}, truth.metadata)
    for E in (4, 8):
        for maps in (False, True):
            # without maps the edges are raw values: both fields are taken about 0 there, as anomalies would be
            p, t = (pred, truth) if maps else (shift(pred, flat), shift(truth, flat))
            rec = case(p, t, centre if maps else None, scale if maps else None, E, args.calls, args.repeats)
            print(f"E = {E}, centre + scale {'yes' if maps else 'no '}: {rec['bytes_per_point']} B per point, {rec['read_GB']:.3f} GB read: kernel "
                  f"call {rec['kernel_ms']:.3f} ms (device time, median of {rec['repeats']} graph replays of {rec['calls_per_window']} calls; "
                  f"{rec['kernel_ms_min_max'][0]:.3f}-{rec['kernel_ms_min_max'][1]:.3f}) = {rec['kernel_TBps']:.2f} TB/s; aurora_hip_scores "
                  f"{rec['scores_ms']:.3f} ms = {rec['scores_TBps']:.2f} TB/s, so one read of the inputs takes {rec['one_read_ms']:.3f} ms: the "
                  f"call is {rec['x_read']:.2f} x that; issued eagerly {rec['eager_call_ms']:.3f} ms; conditional_scores() end to end "
                  f"{rec['conditional_scores_call_ms']:.3f} ms; torch expression {rec['torch_ms']:.2f} ms = {rec['torch_over_kernel']:.1f} x "
                  f"the kernel call; agreement {rec['worst_error_over_bound_1e-9']:.2e} of the 1e-9 bound", flush=True)
            print(json.dumps(rec), flush=True)


def shift(b: Batch, by: Batch) -> Batch:
    return Batch({k: v - by.surf_vars[k] for k, v in b.surf_vars.items()}, {},
                 {k: v - by.atmos_vars[k] for k, v in b.atmos_vars.items()}, b.metadata)


if __name__ == "__main__":
    main()
