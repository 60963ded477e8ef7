"""`aurora_amd.smooth` on the device for the 69 planes of a 0.25-degree state (721 x 1440), at radii of 50, 150 and 500 km.

    python tools/smooth_bench.py [--calls 10] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arm: `lib.smooth_planes` over all planes (aurora_hip_smooth calls of two
launches each, the planes divided so that the prefix tables stay under the workspace cap) with the output and the workspace
allocated beforehand, captured in a hipGraph -- once with the default cap of 128 MiB (inside the 256 MiB Infinity Cache: 10
planes of prefix tables in flight) and once with a cap that takes all 69 planes in ONE call (861 MB of tables).  Measured
against, in the same session: (a) the time one read plus one write of the planes would take at the rate aurora_hip_scores
reaches on the same planes (a streaming floor: the call also writes its 12-byte-per-point tables once and reads them two to
three entries per source row and point); (b) the same rule as a torch expression on the device: fp64 `cumsum` of the valid
values and counts, then per source-row offset a `gather` at the window ends, ONE plane timed and scaled to the 69 (it keeps
fp64 temporaries of plane size per offset); (c) `smooth()` end to end, issued eagerly.  Before timing, one plane is checked
against the CPU path bit for bit, and two calls against each other.  Not profiled: no hardware counters were collected, so
cache hit rates, the share of the two launches and the occupancy are not known; a fused single-launch variant that keeps the
prefixes in LDS was not built or measured."""
import argparse
import importlib
import json

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import smooth  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib

mod = importlib.import_module("aurora_amd.smooth")       # (the package's attribute of this name is the function)


def torch_plan(table, wrap: bool, W: int, device) -> list:
    """Per source-row offset (k = i + off) the index tensors of `torch_rule`, made once outside the timed region."""
    row_lo, row_count, half, w = table
    H, i = row_lo.shape[0], np.arange(row_lo.shape[0])
    plan = []
    for off in range(-half.shape[1], half.shape[1] + 1):
        k = i + off
        r = k - row_lo
        ok = (k >= 0) & (k < H) & (r >= 0) & (r < row_count)
        n = np.where(ok, half[i, np.clip(r, 0, half.shape[1] - 1)], -1)
        if not (n >= 0).any():
            continue
        e = np.stack([np.stack(mod._window(max(int(v), 0), W, wrap)[:3]) for v in n])   # (H, 3, W)
        width = np.where(n >= 0, np.minimum(2 * n + 1, W) if wrap else 2 * n + 1, 0).astype(np.float64)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        plan.append((to(np.clip(k, 0, H - 1)), to(e[:, 0]), to(e[:, 1]), to(e[:, 2]), to(np.where(n >= 0, w[np.clip(k, 0, H - 1)], 0.0))[:, None],
                     to(width)[:, None], to(n >= 0)[:, None]))
    return plan


def torch_rule(x: torch.Tensor, plan: list, min_valid: float) -> torch.Tensor:
    """THE RULE of aurora_amd/smooth.py for ONE plane (H, W) as torch operations on its device (keep_mask=True): fp64 cumsum for
    the prefixes, then per source-row offset a gather at the window ends, in ascending source rows."""
    H, W = x.shape
    valid = torch.isfinite(x)
    zero = torch.zeros(H, 1, dtype=torch.float64, device=x.device)
    P = torch.cat([zero, torch.cumsum(torch.where(valid, x.double(), 0.0), dim=1)], dim=1)
    N = torch.cat([zero.long(), torch.cumsum(valid.long(), dim=1)], dim=1)
    num, den, full = (torch.zeros(H, W, dtype=torch.float64, device=x.device) for _ in range(3))
    for kk, e0, e1, e2, wk, width, live in plan:
        Pk, Nk = P[kk], N[kk]
        S = (Pk.gather(1, e1) - Pk.gather(1, e0)) + Pk.gather(1, e2)
        C = (Nk.gather(1, e1) - Nk.gather(1, e0)) + Nk.gather(1, e2)
        num += torch.where(live, wk * S, 0.0)
        den += torch.where(live, wk * C.double(), 0.0)
        full += wk * width
    value = (num / den).float()
    keep = (den > 0) & ~(den / full < min_valid) & torch.isfinite(value) & valid
    return torch.where(keep, value, torch.full_like(value, float("nan")))


def case(radius: float, batch, calls: int, repeats: int) -> dict:
    fields = planes(batch)
    lat = batch.metadata.lat.numpy()
    dlam = 2 * np.pi / N_LON
    table = mod.disc_table(lat, dlam, N_LON, True, radius)
    rows, w = torch.from_numpy(mod._packed(table)).cuda(), torch.from_numpy(table[3]).cuda()
    out = torch.empty(N_PLANES, N_LAT, N_LON, device="cuda")
    one = lib.smooth_workspace_bytes(1, N_LAT, N_LON)
    ws = {"cap 128 MiB": torch.empty(lib.SMOOTH_WORKSPACE_CAP // one * one, dtype=torch.uint8, device="cuda"),
          "one call": torch.empty(N_PLANES * one, dtype=torch.uint8, device="cuda")}
    kernel = {k: (lambda t=t: lib.smooth_planes(fields, rows, w, True, out=out, workspace=t)) for k, t in ws.items()}
    weights = torch.from_numpy(mod._fields.latitude_weights(lat)).cuda()
    yard = lambda: lib.scores_sums(fields, fields, None, weights)  # noqa: E731
    whole = lambda: smooth(batch, radius)  # noqa: E731
    x0 = fields[0][0]
    plan = torch_plan(table, True, N_LON, x0.device)
    expr = lambda: torch_rule(x0, plan, 0.5)  # noqa: E731
    first = kernel["cap 128 MiB"]().clone()
    again = kernel["one call"]()
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), again.view(torch.int32)), "the two workspace caps differ"
    want = mod._smooth_host(x0.cpu().numpy()[None], table, True, 0.5, True)[0]
    assert np.array_equal(first[0].cpu().numpy().view(np.uint32), want.view(np.uint32)), "the device differs from the CPU path"
    assert np.array_equal(expr().cpu().numpy().view(np.uint32), want.view(np.uint32)), "the torch expression differs from the CPU path"
    whole()
    for f in (*kernel.values(), yard, whole, expr):
        window_ms(f, 2)
    arms = {k: captured(f, calls) for k, f in kernel.items()}
    arms.update({"scores": captured(yard, calls), "eager": lambda: window_ms(kernel["cap 128 MiB"], calls),
                 "whole": lambda: window_ms(whole, calls), "torch": lambda: window_ms(expr, 2)})
    ms = alternate(arms, repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    n = N_LAT * N_LON
    rate = N_PLANES * n * 4 * 2 / med["scores"] / 1e9                               # TB/s of aurora_hip_scores on these planes
    floor = N_PLANES * n * 4 * 2 / rate / 1e9
    return {"radius_km": radius, "planes": N_PLANES, "grid": [N_LAT, N_LON], "max_rows": int(table[2].shape[1]),
            "widest_half": int(table[2].max()), "workspace_MB": {k: t.numel() / 1e6 for k, t in ws.items()},
            "calls_per_window": calls, "repeats": repeats, "kernel_ms": {k: med[k] for k in ws}, "kernel_ms_min_max": {k: span[k] for k in ws},
            "scores_ms": med["scores"], "scores_TBps": rate, "streaming_floor_ms": floor, "x_floor": med["cap 128 MiB"] / floor,
            "eager_call_ms": med["eager"], "smooth_call_ms": med["whole"], "torch_one_plane_ms": med["torch"],
            "torch_scaled_ms": med["torch"] * N_PLANES, "torch_over_kernel": med["torch"] * N_PLANES / med["cap 128 MiB"]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} ({N_PLANES * N_LAT * N_LON * 4 / 1e6:.0f} MB)",
          flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    batch = state(lambda *lead: 280.0 + 10.0 * torch.randn(*lead, N_LAT, N_LON, device="cuda", generator=g))
    for radius in (50.0, 150.0, 500.0):
        rec = case(radius, batch, args.calls, args.repeats)
        k = rec["kernel_ms"]
        print(f"R = {radius:g} km (up to {rec['max_rows']} source rows): all planes {k['cap 128 MiB']:.3f} ms with the 128 MiB cap, "
              f"{k['one call']:.3f} ms in one call (device time, median of {rec['repeats']} graph replays of {rec['calls_per_window']} calls); "
              f"aurora_hip_scores on the same planes {rec['scores_ms']:.3f} ms = {rec['scores_TBps']:.2f} TB/s, at which one read and one "
              f"write of the planes take {rec['streaming_floor_ms']:.3f} ms: the call is {rec['x_floor']:.1f} x that; issued eagerly "
              f"{rec['eager_call_ms']:.3f} ms; smooth() end to end {rec['smooth_call_ms']:.3f} ms; the torch cumsum + gather expression "
              f"{rec['torch_one_plane_ms']:.2f} ms for one plane = {rec['torch_scaled_ms']:.0f} ms for {N_PLANES} = "
              f"{rec['torch_over_kernel']:.0f} x the kernel call", flush=True)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
