"""`Batch.regrid` on the device for an HRES-shaped batch (141 planes: 4 surface variables x 2 history steps, 5 atmospheric
variables x 13 levels x 2, 3 static variables), both directions: 0.25 -> 0.1 degrees and 0.1 -> 0.25 degrees.

    python tools/regrid_bench.py [--runs 30] [--no-host]

Device: the one aurora_hip_regrid launch over all 141 planes, timed with HIP events after warm-up, median of --runs
single-launch timings; effective GB/s = (source bytes + output bytes) / time, the bytes counted here from the shapes.  Also
the median of `Batch.regrid` end to end (tables, allocation, the launch).  Host: the SciPy path (`_interpolate`) timed on
ONE plane and multiplied by 141 -- a scaled estimate, not a run of the whole batch.  Check: device against the host path on
three planes (a surface, an atmospheric and a static one), with the bound of tests/test_gpu_regrid.py.
"""
import argparse
import json
import statistics
import sys
import time
from datetime import datetime
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from aurora_amd import Batch, Metadata  # noqa: E402
from aurora_amd.batch import _interpolate  # noqa: E402
from aurora_amd.engine import lib  # noqa: E402
from tests.test_regrid_plan import assert_matches_host, target_grid  # noqa: E402

SURF, ATMOS, STATIC, LEVELS, T = ("2t", "10u", "10v", "msl"), ("z", "u", "v", "t", "q"), ("lsm", "z", "slt"), 13, 2
N_PLANES = len(SURF) * T + len(ATMOS) * T * LEVELS + len(STATIC)


def hres_batch(res: float) -> Batch:
    lat, lon = (torch.from_numpy(x) for x in target_grid(res))
    h, w = len(lat), len(lon)
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, h, w, device="cuda", generator=g)  # noqa: E731
    md = Metadata(lat=lat, lon=lon, time=(datetime(2022, 5, 11, 12),), atmos_levels=tuple(range(50, 50 + 75 * LEVELS, 75)))
    return Batch({k: r(1, T) for k in SURF}, {k: r() for k in STATIC}, {k: r(1, T, LEVELS) for k in ATMOS}, md).to("cuda")


def events_ms(fn, runs: int) -> list[float]:
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def direction(src_res: float, dst_res: float, runs: int, host: bool) -> dict:
    b = hres_batch(src_res)
    fields = [*b.surf_vars.values(), *b.atmos_vars.values(), *b.static_vars.values()]
    lat_new, lon_new = target_grid(dst_res)
    tables = lib.regrid_plan(b.metadata.lat.cpu().numpy(), b.metadata.lon.cpu().numpy(), lat_new, lon_new)
    rows, row_w, cols, col_w = (torch.from_numpy(t).cuda() for t in tables)
    outs = [torch.empty(*v.shape[:-2], len(lat_new), len(lon_new), device="cuda") for v in fields]
    n_planes = sum(v.numel() // (v.shape[-2] * v.shape[-1]) for v in fields)
    assert n_planes == N_PLANES, n_planes
    h, w = b.spatial_shape
    bytes_src, bytes_dst = n_planes * h * w * 4, n_planes * len(lat_new) * len(lon_new) * 4
    launch = lambda: lib.regrid(fields, outs, rows, row_w, cols, col_w)  # noqa: E731
    events_ms(launch, 5)
    kernel = statistics.median(events_ms(launch, runs))
    events_ms(lambda: b.regrid(dst_res), 2)
    whole = statistics.median(events_ms(lambda: b.regrid(dst_res), max(5, runs // 3)))
    rec = {"direction": f"{src_res} -> {dst_res} deg", "planes": n_planes, "src": [h, w], "dst": [len(lat_new), len(lon_new)],
           "read_GB": bytes_src / 1e9, "written_GB": bytes_dst / 1e9, "device_ms_median": kernel, "runs": runs,
           "effective_TBps": (bytes_src + bytes_dst) / kernel / 1e9, "batch_regrid_ms_median": whole}
    if host:
        rg = b.regrid(dst_res)
        torch.cuda.synchronize()
        lat, lon = b.metadata.lat.cpu(), b.metadata.lon.cpu()
        checks = (("surf.2t[0, 1]", b.surf_vars["2t"][0, 1], rg.surf_vars["2t"][0, 1]),
                  ("atmos.t[0, 0, 7]", b.atmos_vars["t"][0, 0, 7], rg.atmos_vars["t"][0, 0, 7]),
                  ("static.z", b.static_vars["z"], rg.static_vars["z"]))
        secs = []
        for name, src, got in checks:
            t0 = time.perf_counter()
            want = _interpolate(src.cpu(), lat, lon, torch.from_numpy(lat_new), torch.from_numpy(lon_new))
            secs.append(time.perf_counter() - t0)
            assert_matches_host(got.cpu().numpy(), want.numpy(), name)
            exact = float((got.cpu() == want).float().mean())
            print(f"  check {name}: device == host path within the bound; bit-identical fraction {exact:.6f}", flush=True)
        rec["host_s_per_plane"] = min(secs)
        rec["host_s_batch_scaled"] = min(secs) * n_planes
        rec["host_note"] = f"one plane timed ({len(secs)} tries, fastest), multiplied by {n_planes}"
        rec["speedup_vs_host"] = rec["host_s_batch_scaled"] * 1e3 / kernel
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--no-host", action="store_true", help="skip the host timing and the check (e.g. under a profiler)")
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes per batch", flush=True)
    for src_res, dst_res in ((0.25, 0.1), (0.1, 0.25)):
        rec = direction(src_res, dst_res, args.runs, not args.no_host)
        line = (f"{rec['direction']}: {rec['planes']} planes {rec['src'][0]}x{rec['src'][1]} -> {rec['dst'][0]}x{rec['dst'][1]}, "
                f"{rec['read_GB']:.3f} GB read + {rec['written_GB']:.3f} GB written: kernel {rec['device_ms_median']:.3f} ms "
                f"(median of {rec['runs']}) = {rec['effective_TBps']:.2f} TB/s effective; Batch.regrid end to end "
                f"{rec['batch_regrid_ms_median']:.2f} ms")
        if "host_s_batch_scaled" in rec:
            line += (f"; host path {rec['host_s_per_plane']:.3f} s per plane x {rec['planes']} = "
                     f"{rec['host_s_batch_scaled']:.1f} s (scaled, not run)")
        print(line, flush=True)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
