"""`aurora_amd.region_scores` on the device for one 0.25-degree prediction (721 x 1440; 4 surface + 5 x 13 atmospheric
variables = 69 planes, 286 MB per input) in five configurations -- `global` alone; the bands n.hem / tropics / s.hem; eight
`SCORECARD` regions; eight regions of which one is a land mask; the same with a climatology -- beside `aurora_hip_scores` on
the same inputs and beside the same sums as a plain torch expression.

    python tools/region_scores_bench.py [--calls 30] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arm: the ONE aurora_hip_region_scores call over all 69 planes
(`lib.region_sums`: two launches), --calls of them per graph.  Bytes read are counted here from the shapes and the row
table: a row that belongs to no region is not read, a mask plane adds a byte per point.  Yardstick: `lib.scores_sums` on the
same planes (with the climatology where the configuration has one), a graph arm too; `x_scores` is the region call over that
time.  Eager arms: `lib.region_sums` and `region_scores()` end to end (checks, cached tables, the call, the finalising torch
operations).  Torch: what a user would write on the same device without this kernel -- per variable and region, fp64, a
membership mask and one masked sum per slot -- in eager windows.  Check: kernel and torch expression against each other on
every plane and region (counts equal, the bound of tests/test_gpu_region_scores.py), and the kernel repeatable bit for bit.
"""
import argparse
import json

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, Region, Regions, region_scores  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib
from aurora_amd.regions import SCORECARD
from aurora_amd.scores import latitude_weights


def batch(seed: int, base: Batch | None = None, spread: float = 1.0) -> Batch:
    """Seeded synthetic fields about 280 (those of tools/scores_bench.py); with `base`, base + spread x noise."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: spread * torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    return state(r, base) if base is not None else state(lambda *s: r(*s) + 280.0)


def configurations(land: torch.Tensor) -> dict:
    first = lambda n: {k: SCORECARD[k] for k in list(SCORECARD)[:n]}  # noqa: E731
    masked = {**first(7), "land": Region(mask=land)}
    return {"global": ({"global": SCORECARD["global"]}, False),
            "three bands": ({k: SCORECARD[k] for k in ("n.hem", "tropics", "s.hem")}, False),
            "eight regions": (first(8), False),
            "eight, one a land mask": (masked, False),
            "eight, one a land mask, climatology": (masked, True)}


def torch_sums(p, t, c, inside, w) -> torch.Tensor:
    """(planes of the variable, R, 8) as a plain torch expression: fp64, a mask and a weighted sum per region."""
    p, t = p.double(), t.double()
    ok = torch.isfinite(p) & torch.isfinite(t)
    if c is not None:
        c = c.double()
        ok &= torch.isfinite(c)
    zero = torch.zeros((), dtype=torch.float64, device=p.device)
    d = p - t
    total = lambda x: x.sum(dim=(-2, -1))  # noqa: E731
    out = []
    for m in inside:
        m = ok & m
        W, dm = torch.where(m, w[:, None], zero), torch.where(m, d, zero)
        slots = [total(m.double()), total(W), total(W * dm), total(W * dm * dm), total(W * dm.abs())]
        if c is not None:
            pa, ta = torch.where(m, p - c, zero), torch.where(m, t - c, zero)
            slots += [total(W * pa * ta), total(W * pa * pa), total(W * ta * ta)]
        else:
            slots += [torch.zeros_like(slots[0])] * 3
        out.append(torch.stack(slots, dim=-1))
    return torch.stack(out, dim=-2).reshape(-1, len(inside), 8)


def case(name: str, pred: Batch, truth: Batch, clim: Batch | None, regions: dict, calls: int, repeats: int) -> dict:
    lat, lon = pred.metadata.lat.numpy(), pred.metadata.lon.numpy()
    w = torch.from_numpy(latitude_weights(lat)).cuda()
    regs = Regions(regions)
    P, T, C = planes(pred), planes(truth), (None if clim is None else planes(clim))
    (row_bits, col_bits, mask_bits, R), = regs.device_tables(lat, lon, torch.device("cuda", torch.cuda.current_device()))
    rows, cols = regs.members(lat, lon)
    inside = [torch.from_numpy(rows[r][:, None] & cols[r][None, :]).cuda() & (True if v.mask is None else v.mask)
              for r, v in enumerate(regs.values)]
    kernel = lambda: lib.region_sums(P, T, C, row_bits, col_bits, mask_bits, R, w)  # noqa: E731
    yard = lambda: lib.scores_sums(P, T, C, w)  # noqa: E731
    whole = lambda: region_scores(pred, truth, regs, climatology=clim)  # noqa: E731
    plain = lambda: torch.cat([torch_sums(p, t, None if C is None else C[i], inside, w) for i, (p, t) in enumerate(zip(P, T))])  # noqa: E731
    got, again, want = kernel(), kernel(), plain()
    whole()
    torch.cuda.synchronize()
    assert torch.equal(got, again), "the kernel's sums are not repeatable"
    g, y = got.cpu().numpy(), want.cpu().numpy()
    assert g.shape == (N_PLANES, R, 8) and (g[..., 0] == y[..., 0]).all() and (g[..., 0] > 0).all(), "membership differs"
    bounds = [(1, y[..., 1]), (2, y[..., 4]), (3, y[..., 3]), (4, y[..., 4])]
    if clim is not None:
        bounds += [(5, np.sqrt(y[..., 6] * y[..., 7])), (6, y[..., 6]), (7, y[..., 7])]
    worst = max(float(np.max(np.abs(g[..., s] - y[..., s]) / bound)) for s, bound in bounds)
    assert worst <= 1e-9, worst
    for f in (kernel, yard, whole, plain):
        window_ms(f, 3)
    ms = alternate({"kernel": captured(kernel, calls), "yardstick": captured(yard, calls), "eager": lambda: window_ms(kernel, calls),
                    "whole": lambda: window_ms(whole, calls), "torch": lambda: window_ms(plain, max(3, calls // 10))}, repeats)
    n_in = 2 + (clim is not None)
    rows_read = int(rows.any(axis=0).sum())
    read = N_PLANES * rows_read * N_LON * (4 * n_in + (mask_bits is not None))
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    return {"configuration": name, "regions": list(regs.names), "mask": mask_bits is not None, "climatology": clim is not None,
            "planes": N_PLANES, "grid": [N_LAT, N_LON], "rows_read": rows_read, "read_GB": read / 1e9, "calls_per_window": calls,
            "repeats": repeats, "kernel_ms": med["kernel"], "kernel_ms_min_max": span["kernel"],
            "kernel_TBps": read / med["kernel"] / 1e9, "scores_ms": med["yardstick"], "scores_ms_min_max": span["yardstick"],
            "scores_TBps": N_PLANES * N_LAT * N_LON * 4 * n_in / med["yardstick"] / 1e9, "x_scores": med["kernel"] / med["yardstick"],
            "eager_call_ms": med["eager"], "region_scores_call_ms": med["whole"], "torch_ms": med["torch"],
            "torch_ms_min_max": span["torch"], "torch_over_kernel": med["torch"] / med["kernel"],
            "worst_error_over_bound_1e-9": worst / 1e-9}


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
    land = torch.rand(N_LAT, N_LON, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) < 0.3
    for name, (regions, with_clim) in configurations(land).items():
        rec = case(name, pred, truth, clim if with_clim else None, regions, args.calls, args.repeats)
        print(f"{name} (R = {len(rec['regions'])}): {rec['rows_read']} of {N_LAT} rows, {rec['read_GB']:.3f} GB read: kernel call "
              f"{rec['kernel_ms']:.3f} ms (device time, median of {rec['repeats']} graph replays of {rec['calls_per_window']} calls; "
              f"{rec['kernel_ms_min_max'][0]:.3f}-{rec['kernel_ms_min_max'][1]:.3f}) = {rec['kernel_TBps']:.2f} TB/s; aurora_hip_scores "
              f"{rec['scores_ms']:.3f} ms = {rec['scores_TBps']:.2f} TB/s: the call is {rec['x_scores']:.2f} x that; issued eagerly "
              f"{rec['eager_call_ms']:.3f} ms; region_scores() end to end {rec['region_scores_call_ms']:.3f} ms; torch expression "
              f"{rec['torch_ms']:.2f} ms = {rec['torch_over_kernel']:.1f} x the kernel call; agreement "
              f"{rec['worst_error_over_bound_1e-9']:.2e} of the 1e-9 bound", flush=True)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
