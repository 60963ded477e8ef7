"""`aurora_amd.objects` on the device for 17 planes of a 0.25-degree state (721 x 1440; the 4 surface variables and the 13
levels of one atmospheric variable), at T = 1 and T = 3 thresholds, connectivity 8, wrapping in longitude.

    python tools/objects_bench.py [--calls 20] [--repeats 5]

State and timing: tools/verification_bench.py.  The fields are smooth (a k^-2.5 amplitude spectrum in both directions), so that
the objects are few and large as those of a weather field; thresholds are each plane's 0.9 (T = 1) or 0.5 / 0.9 / 0.99 (T = 3)
quantiles by count, from `field_quantiles` on the device.  Kernel arm: the ONE aurora_hip_objects call over all planes and thresholds with outputs and workspace allocated
beforehand, captured in a hipGraph.  Measured against, in the same session: (a) the time one read of the inputs plus one write
of the labels would take at the rate aurora_hip_scores reaches on the same planes (a streaming floor: the call also writes and
re-reads its 4-byte-per-point workspace several times); (b) scipy.ndimage.label on the host, the transfer of the plane counted,
ONE plane timed and scaled to the 17 (as tools/conservative_regrid_bench.py does).  Before timing, labels, count and table of
one plane are checked against the CPU path bit for bit, and two calls against each other."""
import argparse
import importlib
import json
import time

import numpy as np
import torch
from verification_bench import LEVELS, N_LAT, N_LON, SURF, alternate, captured, med_min_max, metadata, window_ms

from aurora_amd import Batch, field_quantiles, objects  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib

mod = importlib.import_module("aurora_amd.objects")       # (the package's attribute of this name is the function)
N_PLANES = len(SURF) + LEVELS


def smooth(g: torch.Generator, *lead) -> torch.Tensor:
    ki = torch.fft.fftfreq(N_LAT, device="cuda")[:, None] * N_LAT
    kj = torch.fft.rfftfreq(N_LON, device="cuda")[None, :] * N_LON
    amp = (1.0 + ki * ki + kj * kj) ** -1.25
    z = torch.randn(*lead, N_LAT, N_LON // 2 + 1, 2, device="cuda", generator=g)
    x = torch.fft.irfft2(torch.view_as_complex(z) * amp, s=(N_LAT, N_LON))
    return (280.0 + 10.0 * x / x.std()).float().contiguous()


def case(T: int, batch: Batch, calls: int, repeats: int) -> dict:
    fields = [v[:, -1] for v in (*batch.surf_vars.values(), *batch.atmos_vars.values())]
    flat = torch.cat([f.reshape(-1, N_LAT * N_LON) for f in fields])
    thr = field_quantiles(batch, (0.9,) if T == 1 else (0.5, 0.9, 0.99), kind="count").value_table   # (planes, T), on the device
    thr_host = thr.cpu().numpy()
    lat = batch.metadata.lat.numpy()
    unit = torch.from_numpy(mod.area_units(lat)).cuda()
    M = 4096
    out = (torch.empty((N_PLANES, T, N_LAT, N_LON), dtype=torch.int32, device="cuda"),
           torch.empty((N_PLANES, T), dtype=torch.int32, device="cuda"), torch.empty((N_PLANES, T, M, 10), dtype=torch.int64, device="cuda"))
    ws = torch.empty(lib.objects_workspace_bytes(N_PLANES, N_LAT, N_LON, T), dtype=torch.uint8, device="cuda")
    kernel = lambda: lib.object_labels(fields, thr, unit, False, 8, True, M, out=out, workspace=ws)  # noqa: E731
    w = torch.from_numpy(mod._fields.latitude_weights(lat)).cuda()
    yard = lambda: lib.scores_sums(fields, fields, None, w)  # noqa: E731
    named = {**{k: thr_host[i] for i, k in enumerate(SURF)}, "z": thr_host[len(SURF):]}
    whole = lambda: objects(batch, named, max_objects=M)  # noqa: E731
    first = [t.clone() for t in kernel()]
    again = kernel()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two calls differ"
    plane0 = flat[0].reshape(1, N_LAT, N_LON).cpu().numpy()
    want = mod._objects_host(plane0, thr_host[:1], mod.area_units(lat), False, 8, True, M)
    assert all(np.array_equal(a[0].cpu().numpy(), b[0]) for a, b in zip(first, want)), "the device differs from the CPU path"
    whole()
    for f in (kernel, yard, whole):
        window_ms(f, 3)
    ms = alternate({"kernel": captured(kernel, calls), "scores": captured(yard, calls), "eager": lambda: window_ms(kernel, calls),
                    "whole": lambda: window_ms(whole, calls)}, repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    from scipy import ndimage

    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        p = fields[0][0].cpu().numpy()
        for t in range(T):
            ndimage.label(p >= thr_host[0, t], structure=np.ones((3, 3)))
        host.append((time.perf_counter() - t0) * 1e3)
    n = N_LAT * N_LON
    rate = N_PLANES * n * 4 * 2 / med["scores"] / 1e9                               # TB/s of aurora_hip_scores on these planes
    floor = (N_PLANES * n * 4 + N_PLANES * T * n * 4) / rate / 1e9
    return {"T": T, "planes": N_PLANES, "grid": [N_LAT, N_LON], "connectivity": 8, "wrap": True, "max_objects": M,
            "objects_per_plane_and_threshold": first[1].float().mean(dim=0).tolist(), "workspace_MB": ws.numel() / 1e6,
            "labels_MB": out[0].numel() * 4 / 1e6, "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"],
            "kernel_ms_min_max": span["kernel"], "scores_ms": med["scores"], "scores_TBps": rate, "streaming_floor_ms": floor,
            "x_floor": med["kernel"] / floor, "eager_call_ms": med["eager"], "objects_call_ms": med["whole"],
            "scipy_one_plane_ms": min(host), "scipy_scaled_ms": min(host) * N_PLANES, "scipy_over_kernel": min(host) * N_PLANES / med["kernel"]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} ({N_PLANES * N_LAT * N_LON * 4 / 1e6:.0f} MB)",
          flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    batch = Batch({k: smooth(g, 1, 1) for k in SURF}, {}, {"z": smooth(g, 1, 1, LEVELS)}, metadata())
    for T in (1, 3):
        rec = case(T, batch, args.calls, args.repeats)
        print(f"T = {T}: mean objects per plane {rec['objects_per_plane_and_threshold']}; kernel call {rec['kernel_ms']:.3f} ms (device "
              f"time, median of {rec['repeats']} graph replays of {rec['calls_per_window']} calls; {rec['kernel_ms_min_max'][0]:.3f}-"
              f"{rec['kernel_ms_min_max'][1]:.3f}); aurora_hip_scores on the same planes {rec['scores_ms']:.3f} ms = {rec['scores_TBps']:.2f} "
              f"TB/s, at which one read of the inputs and one write of the labels take {rec['streaming_floor_ms']:.3f} ms: the call is "
              f"{rec['x_floor']:.1f} x that; issued eagerly {rec['eager_call_ms']:.3f} ms; objects() end to end {rec['objects_call_ms']:.3f} "
              f"ms; scipy.ndimage.label on the host with the transfer {rec['scipy_one_plane_ms']:.1f} ms for one plane = "
              f"{rec['scipy_scaled_ms']:.0f} ms for {N_PLANES} = {rec['scipy_over_kernel']:.0f} x the kernel call", flush=True)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
