"""`aurora_amd.field_quantiles` on the device for one 0.25-degree state (721 x 1440; 4 surface + 5 x 13 atmospheric variables =
69 planes), Q = 3 (0.5, 0.9, 0.99), kind = area and kind = count.

    python tools/field_quantiles_bench.py [--calls 10] [--repeats 5]

State and timing: tools/verification_bench.py.  The fields are red noise (5e4 plus rows with a k^-3 amplitude spectrum, as the
tests' `red_noise`): every value shares its sign and exponent, so the whole plane sits in ONE bin of the key's top byte, as a
2 m temperature in kelvin does.  A second state is CONSTANT planes: one bin in every pass, the full contention.
Kernel arm: the ONE aurora_hip_field_quantiles call over all 69 planes (`lib.field_quantile_values`: nine launches) with outputs
and workspace allocated beforehand, --calls of them per graph.  Measured against, in the same session: (a) FOUR TIMES the
time aurora_hip_scores needs to read the same planes once (`lib.scores_sums` with the planes as both operands reads each
once from memory): the floor of four read passes; (b) the rule evaluated with torch.sort on the device, in chunks of planes
(a sort needs plane-sized temporaries); (c) the numpy path on the host, the transfer of the plane counted, ONE plane timed and
scaled to the 69; (d) `field_quantiles()` end to end, issued eagerly.  Before timing, one plane of each kind is checked against
the numpy rule bit for bit, the torch evaluation against the kernel, and two calls against each other."""
import argparse
import importlib
import json
import time

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import field_quantiles  # (verification_bench has put the repository on sys.path)
from aurora_amd._fields import device_weights
from aurora_amd.engine import lib
from aurora_amd.objects import area_units

mod = importlib.import_module("aurora_amd.field_quantiles")       # (the package's attribute of this name is the function)
Q = (0.5, 0.9, 0.99)
SORT_CHUNK = 8                                                    # planes per torch.sort


def red_noise(g: torch.Generator, *lead) -> torch.Tensor:
    K = N_LON // 2 + 1
    amp = torch.zeros(K, device="cuda", dtype=torch.float64)
    amp[1:] = 500.0 * torch.arange(1, K, device="cuda", dtype=torch.float64) ** -3.0
    phase = 2 * torch.pi * torch.rand(*lead, N_LAT, K, device="cuda", dtype=torch.float64, generator=g)
    x = torch.fft.irfft(amp * torch.exp(1j * phase) * N_LON / 2, n=N_LON, dim=-1)
    return (5e4 + x).float().contiguous()


def torch_rule(flat: torch.Tensor, unit: torch.Tensor | None) -> torch.Tensor:
    """THE RULE for finite (P, n) planes by a full sort: (P, Q) float32.  unit: (n,) int64 per point, or None (count)."""
    out = []
    for p0 in range(0, flat.shape[0], SORT_CHUNK):
        x, order = torch.sort(flat[p0:p0 + SORT_CHUNK], dim=1)
        n = x.shape[1]
        if unit is None:
            cols = []
            for q in Q:
                h = float(n - 1) * q
                j = min(int(np.floor(h)), n - 1)
                a, b = x[:, j].double(), x[:, min(j + 1, n - 1)].double()
                cols.append((a + (h - j) * (b - a)).float())
            out.append(torch.stack(cols, dim=1))
        else:
            cum = torch.cumsum(unit[order], dim=1)
            W = cum[:, -1]
            target = torch.stack([torch.ceil(q * W.double()).long().clamp(min=1) for q in Q], dim=1).minimum(W[:, None])
            out.append(torch.gather(x, 1, torch.searchsorted(cum, target)))
    return torch.cat(out)


def case(name: str, batch, calls: int, repeats: int) -> dict:
    fields = planes(batch)
    lat = batch.metadata.lat.numpy()
    dev = torch.device("cuda", torch.cuda.current_device())
    unit = torch.from_numpy(area_units(lat)).cuda()
    row_w = device_weights("field_quantiles_bench", lat, dev)
    out = {k: (torch.empty((N_PLANES, len(Q)), dtype=torch.float32, device="cuda"), torch.empty(N_PLANES, dtype=torch.int64, device="cuda"),
               torch.empty(N_PLANES, dtype=torch.int64, device="cuda")) for k in mod.KINDS}
    ws = torch.empty(lib.field_quantiles_workspace_bytes(N_PLANES, len(Q)), dtype=torch.uint8, device="cuda")
    kernel = {"area": lambda: lib.field_quantile_values(fields, Q, unit, out=out["area"], workspace=ws),
              "count": lambda: lib.field_quantile_values(fields, Q, None, out=out["count"], workspace=ws)}
    reader = lambda: lib.scores_sums(fields, fields, None, row_w)  # noqa: E731
    whole = lambda: field_quantiles(batch, Q)  # noqa: E731
    flat = torch.cat([f.reshape(-1, N_LAT * N_LON) for f in fields])
    unit_points = unit[:, None].expand(N_LAT, N_LON).reshape(-1)
    plain = {"area": lambda: torch_rule(flat, unit_points), "count": lambda: torch_rule(flat, None)}

    host_ms = {}
    for kind in mod.KINDS:
        first = [t.clone() for t in kernel[kind]()]
        again = kernel[kind]()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, again)), "two calls differ"
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = mod.plane_quantiles(fields[0][0].cpu().numpy(), Q, area_units(lat) if kind == "area" else None)
            times.append((time.perf_counter() - t0) * 1e3)
        host_ms[kind] = min(times)
        assert first[0][0].cpu().numpy().tobytes() == want[0].tobytes() and (int(first[1][0]), int(first[2][0])) == want[1:], \
            f"the device differs from the numpy rule ({kind})"
        assert torch.equal(plain[kind](), first[0]), f"the torch.sort evaluation and the kernel differ ({kind})"
    assert torch.equal(whole().value_table, out["area"][0])
    for f in (*kernel.values(), reader, whole, *plain.values()):
        window_ms(f, 3)
    ms = alternate({"area": captured(kernel["area"], calls), "count": captured(kernel["count"], calls), "scores": captured(reader, calls),
                    "eager": lambda: window_ms(kernel["area"], calls), "whole": lambda: window_ms(whole, calls),
                    "sort_area": lambda: window_ms(plain["area"], 2), "sort_count": lambda: window_ms(plain["count"], 2)}, repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    gbytes = N_PLANES * N_LAT * N_LON * 4 / 1e9
    floor = 4 * med["scores"]
    return {"state": name, "planes": N_PLANES, "grid": [N_LAT, N_LON], "q": list(Q), "calls_per_window": calls, "repeats": repeats,
            "workspace_MB": ws.numel() / 1e6, "input_GB": gbytes, "area_ms": med["area"], "area_ms_min_max": span["area"],
            "count_ms": med["count"], "count_ms_min_max": span["count"], "scores_read_ms": med["scores"],
            "scores_read_TBps": gbytes / med["scores"], "four_reads_ms": floor, "area_over_four_reads": med["area"] / floor,
            "count_over_four_reads": med["count"] / floor, "eager_call_ms": med["eager"], "field_quantiles_call_ms": med["whole"],
            "torch_sort_area_ms": med["sort_area"], "torch_sort_count_ms": med["sort_count"],
            "torch_sort_over_kernel": [med["sort_area"] / med["area"], med["sort_count"] / med["count"]],
            "numpy_one_plane_ms": [host_ms["area"], host_ms["count"]],
            "numpy_scaled_ms": [host_ms["area"] * N_PLANES, host_ms["count"] * N_PLANES], "bits_equal": True}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} ({N_PLANES * N_LAT * N_LON * 4 / 1e6:.0f} MB), "
          f"q = {Q}", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, fill in (("red_noise", lambda *s: red_noise(g, *s)),
                       ("constant", lambda *s: torch.full((*s, N_LAT, N_LON), 273.15, device="cuda"))):
        rec = case(name, state(fill), args.calls, args.repeats)
        print(f"{name}: kernel call, kind = area {rec['area_ms']:.3f} ms ({rec['area_ms_min_max'][0]:.3f}-{rec['area_ms_min_max'][1]:.3f}), "
              f"kind = count {rec['count_ms']:.3f} ms ({rec['count_ms_min_max'][0]:.3f}-{rec['count_ms_min_max'][1]:.3f}) (device time, "
              f"median of {args.repeats} graph replays of {args.calls} calls); one read of the planes ({rec['input_GB']:.2f} GB) by "
              f"aurora_hip_scores {rec['scores_read_ms']:.3f} ms = {rec['scores_read_TBps']:.2f} TB/s, four of them {rec['four_reads_ms']:.3f} "
              f"ms: the call takes {rec['area_over_four_reads']:.2f} x (area) and {rec['count_over_four_reads']:.2f} x (count) that; issued "
              f"eagerly {rec['eager_call_ms']:.3f} ms; field_quantiles() end to end {rec['field_quantiles_call_ms']:.3f} ms; torch.sort "
              f"evaluation {rec['torch_sort_area_ms']:.1f} ms (area) / {rec['torch_sort_count_ms']:.1f} ms (count) = "
              f"{rec['torch_sort_over_kernel'][0]:.0f} x / {rec['torch_sort_over_kernel'][1]:.0f} x the kernel call; numpy on the host with "
              f"the transfer {rec['numpy_one_plane_ms'][0]:.0f} / {rec['numpy_one_plane_ms'][1]:.0f} ms for one plane = "
              f"{rec['numpy_scaled_ms'][0]:.0f} / {rec['numpy_scaled_ms'][1]:.0f} ms for {N_PLANES}; every bit equal", flush=True)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
