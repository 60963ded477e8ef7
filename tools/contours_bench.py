"""`aurora_amd.closed_contours` on the device for the 69 planes of a 0.25-degree state (721 x 1440): red noise smoothed at 100 km,
its 300 km minima as candidates, contour radii of 300 and 600 km, one delta and three.

    python tools/contours_bench.py [--calls 10] [--repeats 5]

Grid and timing: tools/verification_bench.py.  Kernel arm: ONE `lib.closed_contours_planes` call over all planes
(aurora_hip_closed_contours, one launch) with the output allocated beforehand, captured in a hipGraph.  Measured against, in the
same session: (a) `lib.extrema_planes` at 300 km on the same planes, the call that made the candidates, captured the same way;
(b) the floor: the time ONE read of every candidate's window (its rows and columns with the ring, 4 bytes a point) would take at
the rate aurora_hip_scores reaches on the same planes; (c) the host path with the transfer: one plane and its extrema table copied
to the host and tested by the numpy path, timed once and scaled to the 69; (d) the same call issued eagerly, and
`closed_contours()` end to end.  Before timing, one plane is checked against the numpy path byte for byte.  Not profiled: no
hardware counters were collected, so the sweeps per candidate, the LDS bank conflicts and the occupancy are not known."""
import argparse
import importlib
import json
import time

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import closed_contours, extrema, smooth  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib

mod = importlib.import_module("aurora_amd.contours")
smooth_mod = importlib.import_module("aurora_amd.smooth")
MAX_POINTS = 4096


def red_noise(g: torch.Generator, *lead) -> torch.Tensor:
    """Planes of 1e5 plus isotropic noise with a k^-3 power spectrum (amplitude k^-1.5) and a standard deviation of 1000."""
    ky = torch.fft.fftfreq(N_LAT, device="cuda")[:, None] * N_LAT
    kx = torch.fft.rfftfreq(N_LON, device="cuda")[None, :] * N_LON
    k2 = kx * kx + ky * ky
    amp = torch.where(k2 > 0, k2.clamp(min=1.0) ** -0.75, torch.zeros_like(k2))
    phase = torch.rand(*lead, N_LAT, N_LON // 2 + 1, device="cuda", generator=g) * (2 * np.pi)
    x = torch.fft.irfft2(amp * torch.exp(1j * phase), s=(N_LAT, N_LON))
    return (1e5 + 1000.0 * x / x.std(dim=(-2, -1), keepdim=True)).float()


def window_bytes(e, table, names) -> int:
    """4 bytes for every point of every candidate's window: its source rows and columns with the ring."""
    row_lo, row_count, half, _ = table
    cols = np.where(2 * mod._widest(table) + 1 >= N_LON, N_LON, 2 * mod._widest(table) + 3)
    per_row = (row_count + 2).astype(np.int64) * cols
    total = 0
    for name in names:
        rows, count = e.row[name].reshape(-1, MAX_POINTS).cpu().numpy(), e.count[name].reshape(-1).cpu().numpy()
        for r, c in zip(rows, count):
            total += int(per_row[r[:min(int(c), MAX_POINTS)]].sum())
    return 4 * total


def case(radius: float, deltas: list, e, batch, calls: int, repeats: int, shared: dict) -> dict:
    fields = planes(e.source)
    lat = batch.metadata.lat.numpy()
    table = smooth_mod.disc_table(lat, 2 * np.pi / N_LON, N_LON, True, radius)
    rows = torch.from_numpy(smooth_mod._packed(table)).cuda()
    max_words = int(mod.window_words(table, N_LON, True).max())
    T = len(deltas)
    d = torch.tensor([deltas] * N_PLANES, dtype=torch.float32, device="cuda")
    out = torch.empty(N_PLANES, T, MAX_POINTS, 2, dtype=torch.int32, device="cuda")
    kernel = lambda: lib.closed_contours_planes(fields, e.table_table, e.count_table, d, rows, max_words, True, False, 8, out=out)  # noqa: E731
    whole = lambda: closed_contours(e, deltas, radius)  # noqa: E731
    # one plane against the numpy path, and the host path with the transfer
    kernel()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x0, rows0, count0 = fields[0][0].cpu().numpy()[None], e.table_table[:1].cpu().numpy(), e.count_table[:1].cpu().numpy()
    want = mod._contours_host(x0, rows0, count0, d[:1].cpu().numpy(), table, True, False, 8)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert out[0].cpu().numpy().tobytes() == want[0].tobytes(), "the device differs from the numpy path"
    whole()
    for f in (kernel, whole):
        window_ms(f, 2)
    arms = {"kernel": captured(kernel, calls), "extrema": shared["extrema"], "scores": shared["scores"],
            "eager": lambda: window_ms(kernel, calls), "whole": lambda: window_ms(whole, calls)}
    ms = alternate(arms, repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    rate = N_PLANES * N_LAT * N_LON * 4 * 2 / med["scores"] / 1e9                    # TB/s of aurora_hip_scores on these planes
    read = window_bytes(e, table, list(e.count))
    floor = read / rate / 1e9
    counts = e.count_table.cpu().numpy()
    live = torch.arange(MAX_POINTS, device="cuda") < e.count_table[:, None]
    closed = ((out[..., 1] == 0) & live[:, None, :]).sum(dim=(0, 2)).cpu().tolist()
    return {"radius_km": radius, "deltas": deltas, "planes": N_PLANES, "grid": [N_LAT, N_LON], "candidates": int(counts.sum()),
            "candidates_per_plane": [int(counts.min()), int(counts.max())], "closed": closed, "max_rows": int(table[2].shape[1]),
            "max_words": max_words, "lds_bytes": lib.contour_lds_bytes(int(table[2].shape[1]), max_words),
            "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"], "kernel_ms_min_max": span["kernel"],
            "extrema_300km_ms": med["extrema"], "x_extrema": med["kernel"] / med["extrema"], "scores_ms": med["scores"],
            "scores_TBps": rate, "window_MB": read / 1e6, "floor_ms": floor, "x_floor": med["kernel"] / floor,
            "eager_call_ms": med["eager"], "closed_contours_call_ms": med["whole"], "host_one_plane_ms": host_ms,
            "host_scaled_ms": host_ms * N_PLANES, "host_over_kernel": host_ms * N_PLANES / med["kernel"]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} ({N_PLANES * N_LAT * N_LON * 4 / 1e6:.0f} MB)",
          flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    batch = smooth(state(lambda *lead: red_noise(g, *lead)), 100.0)
    e = extrema(batch, 300.0, kind="min", max_points=MAX_POINTS)
    fields = planes(batch)
    lat = batch.metadata.lat.numpy()
    table = smooth_mod.disc_table(lat, 2 * np.pi / N_LON, N_LON, True, 300.0)
    rows = torch.from_numpy(smooth_mod._packed(table)).cuda()
    e_out = (torch.empty(N_PLANES, N_LAT, N_LON, dtype=torch.int32, device="cuda"), torch.empty(N_PLANES, N_LAT, N_LON, device="cuda"),
             torch.empty(N_PLANES, MAX_POINTS, 2, dtype=torch.int64, device="cuda"), torch.empty(N_PLANES, dtype=torch.int32, device="cuda"))
    ws = torch.empty(lib.extrema_workspace_bytes(N_PLANES, N_LAT, N_LON), dtype=torch.uint8, device="cuda")
    find = lambda: lib.extrema_planes(fields, rows, True, False, MAX_POINTS, out=e_out, workspace=ws)  # noqa: E731
    weights = torch.from_numpy(smooth_mod._fields.latitude_weights(lat)).cuda()
    yard = lambda: lib.scores_sums(fields, fields, None, weights)  # noqa: E731
    for f in (find, yard):
        window_ms(f, 2)
    shared = {"extrema": captured(find, args.calls), "scores": captured(yard, args.calls)}
    for radius in (300.0, 600.0):
        for deltas in ([200.0], [100.0, 200.0, 400.0]):
            rec = case(radius, deltas, e, batch, args.calls, args.repeats, shared)
            print(f"R = {radius:g} km, deltas {deltas}: {rec['candidates']} candidates ({rec['candidates_per_plane']} per plane), closed "
                  f"{rec['closed']}; windows of up to {rec['max_rows'] + 2} rows x {rec['max_words']} words, {rec['lds_bytes']} bytes of "
                  f"LDS a workgroup; all planes {rec['kernel_ms']:.3f} ms (device time, median of {rec['repeats']} graph replays of "
                  f"{rec['calls_per_window']} calls) = {rec['x_extrema']:.2f} x aurora_hip_extrema at 300 km ({rec['extrema_300km_ms']:.3f} "
                  f"ms); aurora_hip_scores on the same planes {rec['scores_ms']:.3f} ms = {rec['scores_TBps']:.2f} TB/s, at which one read "
                  f"of every candidate's window ({rec['window_MB']:.1f} MB) takes {rec['floor_ms']:.4f} ms: the call is "
                  f"{rec['x_floor']:.0f} x that floor; issued eagerly {rec['eager_call_ms']:.3f} ms; closed_contours() end to end "
                  f"{rec['closed_contours_call_ms']:.3f} ms; the host path with the transfer {rec['host_one_plane_ms']:.1f} ms for one "
                  f"plane = {rec['host_scaled_ms']:.0f} ms for {N_PLANES} = {rec['host_over_kernel']:.0f} x the kernel call", flush=True)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
