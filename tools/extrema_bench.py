"""`aurora_amd.extrema` on the device for the 69 planes of a 0.25-degree state (721 x 1440), at radii of 50, 150 and 500 km and
for both kinds.

    python tools/extrema_bench.py [--calls 10] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arm: ONE `lib.extrema_planes` call over all planes (aurora_hip_extrema,
four launches) with the outputs and the workspace allocated beforehand, captured in a hipGraph.  Measured against, in the same
session: (a) `lib.smooth_planes` at the same radius (the mean over the same disc: a prefix scan and a gather), captured the same
way; (b) the time one read of the planes plus one write of the two maps (12 bytes per point) would take at the rate
aurora_hip_scores reaches on the same planes: the floor; (c) the same rule as a torch expression on the device -- signed 64-bit
composites, the doubling levels by `torch.minimum` of a plane and its roll, then per source-row offset a `gather` at the two
entries of the window -- ONE plane timed and scaled to the 69; (d) the same call issued eagerly, and `extrema()` end to end.
The growth from 150 km to 500 km is printed beside the growth of the number of source rows and of rows x width: it should
follow the first.  Before timing, one plane is checked against the CPU path byte for byte, and the torch expression too.  Not
profiled: no hardware counters were collected, so the LDS bank conflicts, the share of the four launches and the occupancy are
not known."""
import argparse
import importlib
import json

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import extrema  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib

mod = importlib.import_module("aurora_amd.extrema")       # (the package's attributes of these names are the functions)
smooth_mod = importlib.import_module("aurora_amd.smooth")
SIGN = 1 << 31


def torch_plan(table, W: int, device) -> list:
    """Per source-row offset (k = i + off) the index tensors of `torch_rule` on a full circle, made once outside the timed region."""
    row_lo, row_count, half, _ = table
    H, i = row_lo.shape[0], np.arange(row_lo.shape[0])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    plan = []
    for off in range(-half.shape[1], half.shape[1] + 1):
        k = i + off
        r = k - row_lo
        ok = (k >= 0) & (k < H) & (r >= 0) & (r < row_count)
        n = np.where(ok, half[i, np.clip(r, 0, half.shape[1] - 1)], -1)
        if off == 0:
            n = np.maximum(n, 0)
        if not (n >= 0).any():
            continue
        whole = (n >= 0) & (2 * n + 1 >= W)
        windowed = (n >= 0) & ~whole
        level, a, b = (np.stack(t) for t in zip(*(mod._window(int(v) if w else 0, W, True) for v, w in zip(n, windowed))))
        plan.append((to(np.clip(k, 0, H - 1)), to(level[:, 0]), to(a), to(b), to(whole)[:, None], to(windowed)[:, None]))
    return plan


def torch_rule(x: torch.Tensor, plan: list, is_max: bool) -> torch.Tensor:
    """THE RULE of aurora_amd/extrema.py for ONE plane (H, W) on a full circle as torch operations on its device: the index map."""
    H, W = x.shape
    u = x.view(torch.int32).to(torch.int64) & 0xffffffff
    key = torch.where(u >= SIGN, u ^ 0xffffffff, u | SIGN)
    if is_max:
        key = key ^ 0xffffffff
    flat = torch.arange(H * W, device=x.device).view(H, W)
    none = torch.full((), 2 ** 63 - 1, dtype=torch.int64, device=x.device)
    comp = torch.where(torch.isfinite(x), ((key - SIGN) << 32) | flat, none)         # (signed: the order of the uint64 composites)
    levels = [comp]
    while (2 << (len(levels) - 1)) <= W:
        levels.append(torch.minimum(levels[-1], torch.roll(levels[-1], -(1 << (len(levels) - 1)), dims=1)))
    m = torch.stack(levels)
    row_min = comp.min(dim=1, keepdim=True).values
    best = none.expand(H, W).clone()
    for kk, level, a, b, whole, windowed in plan:
        t = m[level, kk]
        q = torch.minimum(t.gather(1, a), t.gather(1, b))
        q = torch.where(windowed, q, torch.where(whole, row_min[kk], none))
        best = torch.minimum(best, q)
    return torch.where(best == none, torch.full_like(best, -1), best & 0xffffffff).to(torch.int32)


def case(radius: float, kind: str, batch, calls: int, repeats: int) -> dict:
    fields = planes(batch)
    lat = batch.metadata.lat.numpy()
    dlam = 2 * np.pi / N_LON
    table = smooth_mod.disc_table(lat, dlam, N_LON, True, radius)
    rows, w = torch.from_numpy(smooth_mod._packed(table)).cuda(), torch.from_numpy(table[3]).cuda()
    is_max, max_points = kind == "max", 4096
    out = (torch.empty(N_PLANES, N_LAT, N_LON, dtype=torch.int32, device="cuda"), torch.empty(N_PLANES, N_LAT, N_LON, device="cuda"),
           torch.empty(N_PLANES, max_points, 2, dtype=torch.int64, device="cuda"), torch.empty(N_PLANES, dtype=torch.int32, device="cuda"))
    ws = torch.empty(lib.extrema_workspace_bytes(N_PLANES, N_LAT, N_LON), dtype=torch.uint8, device="cuda")
    kernel = lambda: lib.extrema_planes(fields, rows, True, is_max, max_points, out=out, workspace=ws)  # noqa: E731
    s_out = torch.empty(N_PLANES, N_LAT, N_LON, device="cuda")
    one = lib.smooth_workspace_bytes(1, N_LAT, N_LON)
    s_ws = torch.empty(lib.SMOOTH_WORKSPACE_CAP // one * one, dtype=torch.uint8, device="cuda")
    mean = lambda: lib.smooth_planes(fields, rows, w, True, out=s_out, workspace=s_ws)  # noqa: E731
    weights = torch.from_numpy(smooth_mod._fields.latitude_weights(lat)).cuda()
    yard = lambda: lib.scores_sums(fields, fields, None, weights)  # noqa: E731
    whole = lambda: extrema(batch, radius, kind=kind)  # noqa: E731
    x0 = fields[0][0]
    plan = torch_plan(table, N_LON, x0.device)
    expr = lambda: torch_rule(x0, plan, is_max)  # noqa: E731
    got = [t[0].cpu().numpy() for t in kernel()]
    want = [t[0] for t in mod._extrema_host(x0.cpu().numpy()[None], table, True, is_max, max_points)]
    assert all(g.tobytes() == h.tobytes() for g, h in zip(got, want)), "the device differs from the CPU path"
    assert expr().cpu().numpy().tobytes() == want[0].tobytes(), "the torch expression differs from the CPU path"
    counts = out[3].cpu().numpy()
    whole()
    for f in (kernel, mean, yard, whole, expr):
        window_ms(f, 2)
    arms = {"kernel": captured(kernel, calls), "smooth": captured(mean, calls), "scores": captured(yard, calls),
            "eager": lambda: window_ms(kernel, calls), "whole": lambda: window_ms(whole, calls), "torch": lambda: window_ms(expr, 2)}
    ms = alternate(arms, repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    n = N_LAT * N_LON
    rate = N_PLANES * n * 4 * 2 / med["scores"] / 1e9                               # TB/s of aurora_hip_scores on these planes
    floor = N_PLANES * n * 12 / rate / 1e9
    live = table[2] >= 0
    return {"radius_km": radius, "kind": kind, "planes": N_PLANES, "grid": [N_LAT, N_LON], "max_rows": int(table[2].shape[1]),
            "widest_half": int(table[2].max()), "mean_rows": float(live.sum(axis=1).mean()),
            "mean_rows_x_width": float(np.where(live, np.minimum(2 * table[2] + 1, N_LON), 0).sum(axis=1).mean()),
            "extrema_per_plane": [int(counts.min()), int(counts.max())], "workspace_MB": ws.numel() / 1e6,
            "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"], "kernel_ms_min_max": span["kernel"],
            "smooth_ms": med["smooth"], "x_smooth": med["kernel"] / med["smooth"], "scores_ms": med["scores"], "scores_TBps": rate,
            "floor_ms": floor, "x_floor": med["kernel"] / floor, "eager_call_ms": med["eager"], "extrema_call_ms": med["whole"],
            "torch_one_plane_ms": med["torch"], "torch_scaled_ms": med["torch"] * N_PLANES,
            "torch_over_kernel": med["torch"] * N_PLANES / med["kernel"]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} ({N_PLANES * N_LAT * N_LON * 4 / 1e6:.0f} MB)",
          flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    batch = state(lambda *lead: 280.0 + 10.0 * torch.randn(*lead, N_LAT, N_LON, device="cuda", generator=g))
    recs = {}
    for kind in ("min", "max"):
        for radius in (50.0, 150.0, 500.0):
            rec = recs[kind, radius] = case(radius, kind, batch, args.calls, args.repeats)
            print(f"kind {kind}, R = {radius:g} km (up to {rec['max_rows']} source rows, {rec['mean_rows']:.1f} on average): all planes "
                  f"{rec['kernel_ms']:.3f} ms (device time, median of {rec['repeats']} graph replays of {rec['calls_per_window']} calls) = "
                  f"{rec['x_smooth']:.2f} x aurora_hip_smooth at this radius ({rec['smooth_ms']:.3f} ms); aurora_hip_scores on the same "
                  f"planes {rec['scores_ms']:.3f} ms = {rec['scores_TBps']:.2f} TB/s, at which one read of the planes and one write of the "
                  f"two maps take {rec['floor_ms']:.3f} ms: the call is {rec['x_floor']:.1f} x that floor; issued eagerly "
                  f"{rec['eager_call_ms']:.3f} ms; extrema() end to end {rec['extrema_call_ms']:.3f} ms; the torch expression "
                  f"{rec['torch_one_plane_ms']:.2f} ms for one plane = {rec['torch_scaled_ms']:.0f} ms for {N_PLANES} = "
                  f"{rec['torch_over_kernel']:.0f} x the kernel call; {rec['extrema_per_plane']} extrema per plane", flush=True)
            print(json.dumps(rec), flush=True)
        a, b = recs[kind, 150.0], recs[kind, 500.0]
        print(f"kind {kind}, 150 km -> 500 km: the call grows {b['kernel_ms'] / a['kernel_ms']:.2f} x; the source rows grow "
              f"{b['mean_rows'] / a['mean_rows']:.2f} x, rows x width {b['mean_rows_x_width'] / a['mean_rows_x_width']:.2f} x", flush=True)


if __name__ == "__main__":
    main()
