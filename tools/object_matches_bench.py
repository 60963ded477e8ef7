"""`aurora_amd.object_matches` on the device for the 17 planes of tools/objects_bench.py (721 x 1440; 4 surface variables and the
13 levels of one atmospheric variable), at T = 1 and T = 3 thresholds: `a` is the objects of a smooth field, `b` those of the same
field moved 5 columns to the east, so that most objects have a partner.

    python tools/object_matches_bench.py [--calls 20] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arm: the ONE aurora_hip_object_matches call over all planes and thresholds
with outputs and workspace allocated beforehand, captured in a hipGraph.  Measured against, in the same session and alternating:
(a) the time one read of both label maps takes at the rate aurora_hip_scores reaches on planes of the same size (8 bytes per
point and threshold: the floor); (b) the same table as a torch expression on the device -- torch.unique(return_counts=True) on
the packed keys of the contributing points plus an index_add_ for the units, item by item (it reads the number of pairs back:
the eager window is what it takes); (c) object_matches() issued eagerly; and, to bracket contention, the kernel on (d) ONE pair
that covers every plane (every insert on one slot) and (e) MANY pairs (a checkerboard of 8 x 8 blocks of labels 1 .. 64 against
the same shifted by 4: every chunk of 64 columns holds 16 runs).  Before timing, pairs and count of one plane are checked against
the CPU path bit for bit, and two calls against each other."""
import argparse
import importlib
import json

import numpy as np
import torch
from objects_bench import N_PLANES, smooth
from verification_bench import LEVELS, N_LAT, N_LON, SURF, alternate, captured, med_min_max, metadata, window_ms

from aurora_amd import Batch, field_quantiles, object_matches, objects  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib

mod = importlib.import_module("aurora_amd.object_matches")
obj = importlib.import_module("aurora_amd.objects")
MAX_OBJECTS, MAX_PAIRS = 4096, 4096


def torch_pairs(la: torch.Tensor, lb: torch.Tensor, unit: torch.Tensor):
    """The table of one item as a torch expression on the device: (keys, points, units)."""
    ok = (la >= 1) & (la <= MAX_OBJECTS) & (lb >= 1) & (lb <= MAX_OBJECTS)
    key = ((la.to(torch.int64) << 32) | lb.to(torch.int64))[ok]
    keys, inverse, points = torch.unique(key, return_inverse=True, return_counts=True)
    units = torch.zeros_like(keys).index_add_(0, inverse, unit[:, None].expand(N_LAT, N_LON)[ok])
    return keys, points, units


def kernel_arm(la, lb, unit, calls):
    lead = la.shape[:-2]
    out = (torch.empty((*lead, MAX_PAIRS, 4), dtype=torch.int64, device="cuda"), torch.empty(lead, dtype=torch.int32, device="cuda"))
    ws = torch.empty(lib.object_matches_workspace_bytes(int(np.prod(lead)), MAX_PAIRS), dtype=torch.uint8, device="cuda")
    call = lambda: lib.object_pairs(la, lb, unit, MAX_OBJECTS, MAX_OBJECTS, MAX_PAIRS, out=out, workspace=ws)  # noqa: E731
    window_ms(call, 3)
    return call, out, ws, captured(call, calls)


def case(T: int, batch: Batch, moved: Batch, calls: int, repeats: int) -> dict:
    thr = field_quantiles(batch, (0.9,) if T == 1 else (0.5, 0.9, 0.99), kind="count").value_table.cpu().numpy()
    named = {**{k: thr[i] for i, k in enumerate(SURF)}, "z": thr[len(SURF):]}
    a, b = objects(batch, named, max_objects=MAX_OBJECTS), objects(moved, named, max_objects=MAX_OBJECTS)
    la, lb = a.labels_table, b.labels_table
    lat = batch.metadata.lat.numpy()
    unit = torch.from_numpy(obj.area_units(lat)).cuda()
    call, out, ws, kernel = kernel_arm(la, lb, unit, calls)
    first = [t.clone() for t in call()]
    again = call()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, again)), "two calls differ"
    want = mod._pairs_host(la[:1].cpu().numpy(), lb[:1].cpu().numpy(), obj.area_units(lat), MAX_OBJECTS, MAX_OBJECTS, MAX_PAIRS)
    assert all(np.array_equal(x[:1].cpu().numpy(), y) for x, y in zip(first, want)), "the device differs from the CPU path"
    keys, points, units = torch_pairs(la[0, 0], lb[0, 0], unit)
    n0 = int(first[1][0, 0])
    assert keys.shape[0] == n0 and torch.equal(points, first[0][0, 0, :n0, 2]) and torch.equal(units, first[0][0, 0, :n0, 3])
    # contention: one pair that covers everything, and many short runs
    one = torch.ones_like(la)
    i, j = torch.meshgrid(torch.arange(N_LAT, device="cuda"), torch.arange(N_LON, device="cuda"), indexing="ij")
    board = lambda s: ((((i // 8) % 8) * 8 + ((j + s) // 8) % 8) + 1).to(torch.int32).expand_as(la).contiguous()  # noqa: E731
    many_a, many_b = board(0), board(4)
    _, one_out, _, one_pair = kernel_arm(one, one, unit, calls)
    _, many_out, _, many_pairs = kernel_arm(many_a, many_b, unit, calls)
    fields = [v[:, -1] for v in (*batch.surf_vars.values(), *batch.atmos_vars.values())]
    w = torch.from_numpy(obj._fields.latitude_weights(lat)).cuda()
    yard = lambda: lib.scores_sums(fields, fields, None, w)  # noqa: E731
    whole = lambda: object_matches(a, b, max_pairs=MAX_PAIRS)  # noqa: E731
    items = [(la[p, t], lb[p, t]) for p in range(la.shape[0]) for t in range(T)]
    expression = lambda: [torch_pairs(x, y, unit) for x, y in items]  # noqa: E731
    for f in (yard, whole, expression):
        window_ms(f, 3)
    ms = alternate({"kernel": kernel, "scores": captured(yard, calls), "one_pair": one_pair, "many_pairs": many_pairs,
                    "eager": lambda: window_ms(call, calls), "whole": lambda: window_ms(whole, calls),
                    "torch": lambda: window_ms(expression, 3)}, repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    n = N_LAT * N_LON
    rate = N_PLANES * n * 4 * 2 / med["scores"] / 1e9                               # TB/s of aurora_hip_scores on planes of this size
    floor = N_PLANES * T * n * 8 / rate / 1e9
    return {"T": T, "planes": N_PLANES, "grid": [N_LAT, N_LON], "max_objects": MAX_OBJECTS, "max_pairs": MAX_PAIRS,
            "objects_a_mean": a.count_table.float().mean(dim=0).tolist(), "objects_b_mean": b.count_table.float().mean(dim=0).tolist(),
            "pairs_mean": first[1].float().mean(dim=0).tolist(), "pairs_max": int(first[1].max()), "workspace_MB": ws.numel() / 1e6,
            "label_maps_MB": 2 * la.numel() * 4 / 1e6, "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"],
            "kernel_ms_min_max": span["kernel"], "scores_ms": med["scores"], "scores_TBps": rate, "floor_ms": floor,
            "x_floor": med["kernel"] / floor, "one_pair_ms": med["one_pair"], "many_pairs_ms": med["many_pairs"],
            "many_pairs_count": int(many_out[1].max()), "one_pair_count": int(one_out[1].max()), "eager_call_ms": med["eager"],
            "object_matches_call_ms": med["whole"], "torch_expression_ms": med["torch"], "torch_over_kernel": med["torch"] / med["kernel"]}


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
    for T in (1, 3):
        rec = case(T, batch, moved, args.calls, args.repeats)
        print(f"T = {T}: mean pairs per plane {rec['pairs_mean']} (most {rec['pairs_max']}); kernel call {rec['kernel_ms']:.3f} ms (device "
              f"time, median of {rec['repeats']} graph replays of {rec['calls_per_window']} calls; {rec['kernel_ms_min_max'][0]:.3f}-"
              f"{rec['kernel_ms_min_max'][1]:.3f}); aurora_hip_scores on planes of this size {rec['scores_ms']:.3f} ms = "
              f"{rec['scores_TBps']:.2f} TB/s, at which one read of both label maps takes {rec['floor_ms']:.3f} ms: the call is "
              f"{rec['x_floor']:.1f} x that; ONE pair covering every plane {rec['one_pair_ms']:.3f} ms, MANY pairs "
              f"({rec['many_pairs_count']} per item, 16 runs per chunk) {rec['many_pairs_ms']:.3f} ms; issued eagerly "
              f"{rec['eager_call_ms']:.3f} ms; object_matches() end to end {rec['object_matches_call_ms']:.3f} ms; the torch expression "
              f"(unique + index_add_, item by item) {rec['torch_expression_ms']:.2f} ms = {rec['torch_over_kernel']:.0f} x the kernel call",
              flush=True)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
