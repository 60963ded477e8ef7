"""`aurora_amd.nearest_event` and `aurora_amd.object_separations` on the device for the 17 planes of tools/objects_bench.py
(721 x 1440; 4 surface variables and the 13 levels of one atmospheric variable), one threshold.  Three cases:

    objects     the objects of the smooth fields at their 0.9 quantile
    one point   ONE event per plane: every point of a plane has to reach it, the longest walk
    one point, max_km = 500   the same with the walk bounded

    python tools/nearest_event_bench.py [--calls 20] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arms: the ONE aurora_hip_nearest_event call over all planes, and the ONE
aurora_hip_object_separations call of the objects of the field moved 5 columns to the east against those maps, with outputs and
workspace allocated beforehand, each captured in a hipGraph.  Measured against, in the same session and alternating: the time
one read of the label maps plus one write of the index and key maps takes at the rate aurora_hip_scores reaches on planes of the
same size (16 bytes per point: the floor), and the two front ends issued eagerly.  Before timing, index and key of one plane and
the table of one plane are checked against the CPU path bit for bit, and two calls against each other.  What bounds a call --
the candidate reads, the fp64 keys or the tail of long walks -- is not profiled here."""
import argparse
import importlib
import json

import numpy as np
import torch
from objects_bench import N_PLANES, smooth
from verification_bench import LEVELS, N_LAT, N_LON, SURF, alternate, captured, med_min_max, metadata, window_ms

from aurora_amd import Batch, field_quantiles, nearest_event, object_separations, objects  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib

mod = importlib.import_module("aurora_amd.distances")
obj = importlib.import_module("aurora_amd.objects")
MAX_OBJECTS = 4096


def case(name: str, a, b, max_km, yard, calls: int, repeats: int) -> dict:
    la, lb = a.labels_table, b.labels_table
    lat, lon = a.lat.cpu().numpy(), a.lon.cpu().numpy()
    tables = torch.from_numpy(np.concatenate(mod.tables_of(lat, lon, True))).cuda()
    key_max = mod.key_max_of(max_km)
    lead = lb.shape[:-2]
    out = (torch.empty(lb.shape, dtype=torch.int32, device="cuda"), torch.empty(lb.shape, dtype=torch.float64, device="cuda"))
    ws = torch.empty(lib.nearest_event_workspace_bytes(int(np.prod(lead)), N_LAT, N_LON), dtype=torch.uint8, device="cuda")
    sep = (torch.empty((*lead, MAX_OBJECTS, 3), dtype=torch.int64, device="cuda"), torch.empty(lead, dtype=torch.int64, device="cuda"))
    near = lambda: lib.nearest_event_maps(lb, tables, True, key_max, out=out, workspace=ws)  # noqa: E731
    apart = lambda: lib.object_separation_table(la, out[1], out[0], a.count_table, MAX_OBJECTS, out=sep)  # noqa: E731
    first = [t.clone() for t in (*near(), *apart())]
    again = (*near(), *apart())
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
               for x, y in zip(first, again)), "two calls differ"
    index, key = mod._nearest_host(lb[:1].cpu().numpy(), *mod.tables_of(lat, lon, True), True, key_max)
    table, hausdorff = mod._separations_host(la[:1].cpu().numpy(), key, index, a.count_table[:1].cpu().numpy(), MAX_OBJECTS)
    for got, want in zip(first, (index, key, table, hausdorff)):
        assert got[:1].cpu().numpy().tobytes() == want.tobytes(), "the device differs from the CPU path"
    whole_near = lambda: nearest_event(b, max_km)  # noqa: E731
    whole_apart = lambda: object_separations(a, b, max_km)  # noqa: E731
    for f in (near, apart, yard, whole_near, whole_apart):
        window_ms(f, 3)
    ms = alternate({"nearest": captured(near, calls), "separations": captured(apart, calls), "scores": captured(yard, calls),
                    "nearest_eager": lambda: window_ms(whole_near, calls), "separations_eager": lambda: window_ms(whole_apart, calls)}, repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    n = N_LAT * N_LON
    rate = N_PLANES * n * 4 * 2 / med["scores"] / 1e9                               # TB/s of aurora_hip_scores on planes of this size
    floor = N_PLANES * n * 16 / rate / 1e9
    reached = first[0] >= 0
    return {"case": name, "planes": N_PLANES, "grid": [N_LAT, N_LON], "max_km": max_km, "events_per_plane": float((lb > 0).sum()) / N_PLANES,
            "objects_a_mean": float(a.count_table.float().mean()), "points_reached": float(reached.float().mean()),
            "largest_key": float(first[1][reached].max()) if bool(reached.any()) else None, "workspace_MB": ws.numel() / 1e6,
            "calls_per_window": calls, "repeats": repeats, "nearest_ms": med["nearest"], "nearest_ms_min_max": span["nearest"],
            "separations_ms": med["separations"], "separations_ms_min_max": span["separations"], "scores_ms": med["scores"],
            "scores_TBps": rate, "floor_ms": floor, "x_floor": med["nearest"] / floor, "nearest_event_call_ms": med["nearest_eager"],
            "object_separations_call_ms": med["separations_eager"]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON}", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    batch = Batch({k: smooth(g, 1, 1) for k in SURF}, {}, {"z": smooth(g, 1, 1, LEVELS)}, metadata())
    roll = lambda d: {k: torch.roll(v, 5, dims=-1).contiguous() for k, v in d.items()}  # noqa: E731
    moved = Batch(roll(batch.surf_vars), {}, roll(batch.atmos_vars), batch.metadata)
    thr = field_quantiles(batch, (0.9,), kind="count").value_table.cpu().numpy()
    named = {**{k: thr[i] for i, k in enumerate(SURF)}, "z": thr[len(SURF):]}
    b, a = objects(batch, named, max_objects=MAX_OBJECTS), objects(moved, named, max_objects=MAX_OBJECTS)
    # one event per plane, at a place of its own
    lone = torch.zeros_like(b.labels_table)
    for p in range(N_PLANES):
        lone[p, 0, (37 * p) % N_LAT, (211 * p) % N_LON] = 1
    count = torch.ones_like(b.count_table)
    table = torch.zeros_like(b.table_table)
    one = obj.Objects(lone, count, table, b.thresholds_table, b.lat, b.lon, b.layout, False, 8, True, MAX_OBJECTS)
    fields = [v[:, -1] for v in (*batch.surf_vars.values(), *batch.atmos_vars.values())]
    w = torch.from_numpy(obj._fields.latitude_weights(batch.metadata.lat.numpy())).cuda()
    yard = lambda: lib.scores_sums(fields, fields, None, w)  # noqa: E731
    for name, x, y, max_km in (("objects", a, b, None), ("one point", a, one, None), ("one point, max_km = 500", a, one, 500.0)):
        rec = case(name, x, y, max_km, yard, args.calls, args.repeats)
        print(f"{name}: {rec['events_per_plane']:.0f} events per plane, {100 * rec['points_reached']:.1f} % of the points reach one; "
              f"aurora_hip_nearest_event {rec['nearest_ms']:.3f} ms (device time per call, median of {rec['repeats']} graph replays of "
              f"{rec['calls_per_window']} calls; {rec['nearest_ms_min_max'][0]:.3f}-{rec['nearest_ms_min_max'][1]:.3f}); "
              f"aurora_hip_object_separations of the field moved east against it {rec['separations_ms']:.3f} ms "
              f"({rec['separations_ms_min_max'][0]:.3f}-{rec['separations_ms_min_max'][1]:.3f}); aurora_hip_scores on planes of this size "
              f"{rec['scores_ms']:.3f} ms = {rec['scores_TBps']:.2f} TB/s, at which one read of the labels plus one write of the two maps "
              f"takes {rec['floor_ms']:.3f} ms: nearest_event is {rec['x_floor']:.1f} x that; nearest_event() issued eagerly "
              f"{rec['nearest_event_call_ms']:.3f} ms, object_separations() end to end {rec['object_separations_call_ms']:.3f} ms", flush=True)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
