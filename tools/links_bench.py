"""`aurora_amd.link_extrema` and `aurora_amd.tracks` on the device for the 69 planes of a 0.25-degree state (721 x 1440): red noise
smoothed at 100 km, its 300 km minima as candidates, linked to those of the same field moved 3 columns east; and a worst case of
4096 live rows on both sides of every plane (distinct random points of the grid).

    python tools/links_bench.py [--calls 10] [--repeats 5]

Grid and timing: tools/verification_bench.py.  Kernel arm: ONE `lib.link_extrema_tables` call over all planes
(aurora_hip_link_extrema, one launch) with the outputs allocated beforehand, captured in a hipGraph.  Measured against, in the same
session: (a) the same rule as a torch expression on the device -- a dense fp64 key matrix of ONE plane over its live rows (their
numbers read back beforehand, which the kernel does not need), `min` / `argmin` in both directions -- captured the same way and
scaled to the 69 planes; (b) the arithmetic floor: live pairs x 2 directions x the 5 fp64 operations of `key_of` (three products, a
sum, a difference) at an fp64 vector rate of 78.6 TFLOP/s, half the 157.3 TFLOP/s fp32 vector peak of the MI355X -- a peak that
counts a fused multiply-add as two operations, which `key_of` may not use, so the floor these operations can reach is about twice
the one reported; (c) the same
call issued eagerly, `link_extrema()` end to end, and `tracks()` over 8 steps end to end.  Before timing, the kernel's rows of
one plane are checked against the torch expression.  Not profiled: no hardware counter was collected, so the LDS bank
conflicts of the cd gather and the issue rate of the inner loop are not known."""
import argparse
import dataclasses
import json
import types

import numpy as np
import torch
from contours_bench import red_noise
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, state, window_ms

from aurora_amd import Batch, distances, extrema, link_extrema, smooth, tracks  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib

MAX_POINTS = 4096
MAX_KM = 500.0
FP64_VECTOR_TFLOPS = 78.6
KEY_FLOPS = 5
INF_BITS = 0x7FF0000000000000


def dense(table_a, na, table_b, nb, tables, key_max):
    """THE RULE of aurora_amd/links.py for one plane as a torch expression over the live rows: (forward, backward) int64 (n, 2)."""
    s, c, cd = tables[:N_LAT], tables[N_LAT:2 * N_LAT], tables[2 * N_LAT:]
    fa, fb = table_a[:na, 0], table_b[:nb, 0]
    ia, ja, ib, jb = fa // N_LON, fa % N_LON, fb // N_LON, fb % N_LON
    gap = (ja[:, None] - jb[None, :]).abs()
    gap = torch.minimum(gap, N_LON - gap)
    key = (1.0 - (s[ia][:, None] * s[ib][None, :] + (c[ia][:, None] * c[ib][None, :]) * cd[gap])).clamp(min=0.0)
    key = torch.where(fa[:, None] == fb[None, :], torch.zeros_like(key), key)
    key = torch.where(key > key_max, torch.full_like(key, float("inf")), key)
    out = []
    for dim in (1, 0):
        best, at = key.min(dim=dim)
        none = torch.isinf(best)
        out.append(torch.stack([torch.where(none, torch.full_like(at, INF_BITS), best.view(torch.int64)),
                                torch.where(none, torch.full_like(at, -1), at)], dim=1))
    return out


def case(name: str, a, b, calls: int, repeats: int) -> dict:
    dev = a.table_table.device
    key_max = distances.key_max_of(MAX_KM)
    link_extrema(a, b, MAX_KM)                                   # the eager call: (s, c, cd) uploaded
    tables = distances._device_tables(distances_grid(a), dev)
    out = (torch.empty(N_PLANES, MAX_POINTS, 2, dtype=torch.int64, device=dev), torch.empty(N_PLANES, MAX_POINTS, 2, dtype=torch.int64, device=dev))
    kernel = lambda: lib.link_extrema_tables(a.table_table, a.count_table, None, b.table_table, b.count_table, None, tables,  # noqa: E731
                                             N_LAT, N_LON, True, key_max, out=out)
    whole = lambda: link_extrema(a, b, MAX_KM)  # noqa: E731
    ca, cb = a.count_table.cpu().numpy().clip(max=MAX_POINTS), b.count_table.cpu().numpy().clip(max=MAX_POINTS)
    na, nb = int(ca[0]), int(cb[0])
    torch_arm = lambda: dense(a.table_table[0], na, b.table_table[0], nb, tables, key_max)  # noqa: E731
    kernel()
    fw, bw = torch_arm()
    # (torch may fuse the product and the sum: the rows are compared, the key bits only where they agree)
    same_rows = float((out[0][0, :na, 1] == fw[:, 1]).double().mean()), float((out[1][0, :nb, 1] == bw[:, 1]).double().mean())
    same_bits = float((out[0][0, :na, 0] == fw[:, 0]).double().mean())
    for f in (kernel, whole, torch_arm):
        window_ms(f, 2)
    arms = {"kernel": captured(kernel, calls), "torch_one_plane": captured(torch_arm, calls),
            "eager": lambda: window_ms(kernel, calls), "whole": lambda: window_ms(whole, calls)}
    ms = alternate(arms, repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    pairs = int((ca.astype(np.int64) * cb.astype(np.int64)).sum())
    floor = pairs * 2 * KEY_FLOPS / (FP64_VECTOR_TFLOPS * 1e12) * 1e3
    plane_share = na * nb / pairs                                # the timed plane's share of all pairs: the scaling of arm (a)
    linked = int((out[0][..., 1] >= 0).sum())
    return {"case": name, "planes": N_PLANES, "grid": [N_LAT, N_LON], "max_points": MAX_POINTS, "max_km": MAX_KM,
            "rows_a_per_plane": [int(ca.min()), int(ca.max())], "rows_b_per_plane": [int(cb.min()), int(cb.max())], "pairs": pairs,
            "forward_links": linked, "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"],
            "kernel_ms_min_max": span["kernel"], "torch_one_plane_ms": med["torch_one_plane"],
            "torch_scaled_ms": med["torch_one_plane"] / plane_share, "torch_over_kernel": med["torch_one_plane"] / plane_share / med["kernel"],
            "floor_ms": floor, "x_floor": med["kernel"] / floor, "fp64_vector_TFLOPS": FP64_VECTOR_TFLOPS,
            "kernel_TFLOPS": pairs * 2 * KEY_FLOPS / med["kernel"] / 1e9, "eager_call_ms": med["eager"],
            "link_extrema_call_ms": med["whole"], "torch_rows_equal": same_rows, "torch_key_bits_equal": same_bits}


def distances_grid(e):
    return types.SimpleNamespace(lat=e.grid_lat, lon=e.grid_lon, wrap=e.wrap)


def worst(e, g: torch.Generator):
    """`e` with 4096 distinct random points of the grid in every plane, in ascending flat index."""
    flat = torch.stack([torch.randperm(N_LAT * N_LON, device="cuda", generator=g)[:MAX_POINTS].sort().values for _ in range(N_PLANES)])
    table = torch.stack([flat, torch.full_like(flat, 0x80000000 + 1000)], dim=-1).contiguous()
    return dataclasses.replace(e, table_table=table, count_table=torch.full_like(e.count_table, MAX_POINTS))


def report(rec: dict) -> None:
    print(f"{rec['case']}: {rec['rows_a_per_plane']} rows a plane in a, {rec['rows_b_per_plane']} in b, {rec['pairs']} live pairs, "
          f"{rec['forward_links']} forward links within {rec['max_km']:g} km; all planes {rec['kernel_ms']:.4f} ms (device time, median "
          f"of {rec['repeats']} graph replays of {rec['calls_per_window']} calls; min, max {rec['kernel_ms_min_max']}) = "
          f"{rec['kernel_TFLOPS']:.2f} TFLOP/s of key arithmetic; the arithmetic floor at {rec['fp64_vector_TFLOPS']} TFLOP/s fp64 is "
          f"{rec['floor_ms']:.5f} ms: the call is {rec['x_floor']:.1f} x that floor; the torch expression on one plane "
          f"{rec['torch_one_plane_ms']:.4f} ms, scaled by pairs to all planes {rec['torch_scaled_ms']:.3f} ms = "
          f"{rec['torch_over_kernel']:.1f} x the kernel call (its rows equal the kernel's on {rec['torch_rows_equal']} of the rows); "
          f"issued eagerly {rec['eager_call_ms']:.4f} ms; link_extrema() end to end {rec['link_extrema_call_ms']:.3f} ms", flush=True)
    print(json.dumps(rec), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8, help="steps of the tracks() arm")
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON}", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    noise = state(lambda *lead: red_noise(g, *lead))
    steps = []
    for t in range(args.steps):                                  # the field moved 3 columns east a step
        moved = Batch({k: torch.roll(v, 3 * t, -1) for k, v in noise.surf_vars.items()}, {},
                      {k: torch.roll(v, 3 * t, -1) for k, v in noise.atmos_vars.items()}, noise.metadata)
        steps.append(extrema(smooth(moved, 100.0), 300.0, kind="min", max_points=MAX_POINTS))
    report(case("red noise, b = a moved 3 columns east", steps[0], steps[1], args.calls, args.repeats))
    wa, wb = worst(steps[0], g), worst(steps[1], g)
    report(case("4096 live rows on both sides", wa, wb, args.calls, args.repeats))
    follow = lambda: tracks(steps, MAX_KM)  # noqa: E731
    t = follow()
    window_ms(follow, 2)
    ms = [window_ms(follow, 3) for _ in range(args.repeats)]
    med, span = med_min_max(ms)
    rec = {"case": f"tracks over {args.steps} steps", "steps": args.steps, "tracks_call_ms": med, "tracks_call_ms_min_max": span,
           "n_tracks": int(t.n_tracks_table.sum()), "full_length": int((t.length_table[:, 0] == args.steps).sum()),
           "nodes_step_0": int((t.track_id_table[:, 0] >= 0).sum())}
    print(f"tracks() over {args.steps} steps of {N_PLANES} planes end to end (eager, {args.steps - 1} link_extrema calls and the numbering "
          f"in torch): {med:.3f} ms a call (median of {args.repeats} windows of 3; min, max {span}); {rec['n_tracks']} tracks, "
          f"{rec['full_length']} of the {rec['nodes_step_0']} nodes of step 0 are followed through every step", flush=True)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
