"""`aurora_amd.conservative_regrid` on the device: the 69-plane 0.25-degree state (721 x 1440) to 1.5 degrees (121 x 240), and a
69-plane 0.1-degree state (1801 x 3600) to 0.25 degrees (721 x 1440), beside the same rule as a torch expression.

    python tools/conservative_regrid_bench.py [--calls 10] [--repeats 5]

Grid and timing: tools/verification_bench.py.  Kernel arm: the ONE aurora_hip_conservative_regrid call
(`lib.conservative_regrid`) on a preallocated output, --calls of them per graph.  Bytes = 4 x 69 x (source points + target
points): the source read once plus the target written; TB/s = bytes / that time.  Beside it, a graph arm too,
aurora_hip_scores over 69 prediction and 69 truth planes of the 0.25-degree grid: the rate a streaming kernel of this library
reads at in this session.  The yardstick of a case is the time its bytes take at that rate; `over_yardstick` is the kernel time
over it.  Eager arm: `conservative_regrid(batch, ...)` (checks, cached tables, output allocation, the call).  Torch: the rule
as two dense weight-matrix products with finite masks in fp64 on the device (what a user would write without this kernel),
in eager windows of 2 calls.
Check: the call and `conservative_regrid()` give the same bits, the NaN pattern of the torch expression is the same, and the
largest difference to it relative to the result is reported."""
import argparse
import json

import numpy as np
import torch
from verification_bench import ATMOS, LEVELS, N_LAT, N_LON, N_PLANES, SURF, alternate, captured, med_min_max, metadata, window_ms

from aurora_amd import Batch, conservative_regrid  # (verification_bench has put the repository on sys.path)
from aurora_amd import conservative as C
from aurora_amd.batch import derive_metadata
from aurora_amd.engine import lib

CASES = {"0.25 -> 1.5": ((N_LAT, N_LON), 1.5), "0.1 -> 0.25": ((1801, 3600), 0.25)}


def state(n_lat: int, n_lon: int, seed: int) -> Batch:
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: 280.0 + 20.0 * torch.randn(*s, n_lat, n_lon, device="cuda", generator=g)  # noqa: E731
    md = derive_metadata(metadata(), lat=torch.linspace(90, -90, n_lat, dtype=torch.float64, device="cuda"),
                         lon=torch.linspace(0, 360, n_lon + 1, dtype=torch.float64, device="cuda")[:-1])
    return Batch({k: r(1, 1) for k in SURF}, {}, {k: r(1, 1, LEVELS) for k in ATMOS}, md)


def dense(axis: C.Axis, n_src: int) -> torch.Tensor:
    """The taps of an axis as a dense (n_out, n_src) fp64 matrix on the device."""
    W = np.zeros((axis.count.shape[0], n_src))
    for i, ((first, off), cnt) in enumerate(zip(axis.first, axis.count)):
        for t in range(cnt):
            W[i, (first + t) % n_src] += axis.w[off + t]
    return torch.from_numpy(W).cuda()


def torch_rule(x: torch.Tensor, Wr: torch.Tensor, Wc: torch.Tensor, need: torch.Tensor) -> torch.Tensor:
    fin = torch.isfinite(x)
    xz = torch.where(fin, x, 0.0).double()
    n, d = Wr @ xz @ Wc.T, Wr @ fin.double() @ Wc.T
    return torch.where((d > 0) & (d >= need), n / d, float("nan")).float()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes per state", flush=True)

    pred = [torch.randn(N_PLANES, N_LAT, N_LON, device="cuda")]
    truth = [torch.randn(N_PLANES, N_LAT, N_LON, device="cuda")]
    row_w = torch.ones(N_LAT, dtype=torch.float64, device="cuda")
    score = lambda: lib.scores_sums(pred, truth, None, row_w)  # noqa: E731
    scores_moved = 4 * N_LAT * N_LON * 2 * N_PLANES
    window_ms(score, 3)
    score_arm = captured(score, args.calls)

    rec = {"planes": N_PLANES, "calls_per_window": args.calls, "repeats": args.repeats, "scores_moved_GB": scores_moved / 1e9, "cases": {}}
    for name, ((n_lat, n_lon), res) in CASES.items():
        b = state(n_lat, n_lon, seed=1)
        b.surf_vars["2t"][0, 0, n_lat // 3: n_lat // 3 + 40, 100:400] = float("nan")           # a patch of land
        out_b = conservative_regrid(b, res)                                                      # (also the warm call)
        n_rows, n_cols = out_b.metadata.lat.shape[0], out_b.metadata.lon.shape[0]
        p = C.plan(b.metadata.lat.cpu().numpy(), b.metadata.lon.cpu().numpy(), out_b.metadata.lat.cpu().numpy(), out_b.metadata.lon.cpu().numpy())
        key = tuple(a.tobytes() for a in (b.metadata.lat.cpu().numpy(), b.metadata.lon.cpu().numpy(), p.lat, p.lon))
        tables = C.device_tables(p, key, torch.device("cuda", torch.cuda.current_device()))
        src = [*b.surf_vars.values(), *b.atmos_vars.values()]
        out = torch.empty(N_PLANES, n_rows, n_cols, device="cuda")
        kernel = lambda: lib.conservative_regrid(src, out, tables, 0.5)  # noqa: E731
        whole = lambda: conservative_regrid(b, res)  # noqa: E731
        Wr, Wc = dense(p.rows, n_lat), dense(p.cols, n_lon)
        need = 0.5 * torch.from_numpy(p.rows.measure[:, None] * p.cols.measure).cuda()
        plain = lambda: [torch_rule(v, Wr, Wc, need) for v in src]  # noqa: E731

        kernel()
        want = torch.cat([t.reshape(-1, n_rows, n_cols) for t in plain()])
        pub = torch.cat([t.reshape(-1, n_rows, n_cols) for t in (*out_b.surf_vars.values(), *out_b.atmos_vars.values())])
        torch.cuda.synchronize()
        assert torch.equal(torch.isnan(out), torch.isnan(want)), f"{name}: NaN pattern differs from the torch expression"
        assert torch.equal(out.nan_to_num().view(torch.int32), pub.nan_to_num().view(torch.int32)), f"{name}: call and function differ"
        ok = ~torch.isnan(out)
        worst = float(((out[ok].double() - want[ok].double()).abs() / want[ok].abs().double()).max())
        del want, pub

        for f in (kernel, whole, plain):
            window_ms(f, 2)
        ms = alternate({"kernel": captured(kernel, args.calls), "scores": score_arm, "torch": lambda: window_ms(plain, 2),
                        "call": lambda: window_ms(whole, args.calls)}, args.repeats)
        med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
        moved = 4 * N_PLANES * (n_lat * n_lon + n_rows * n_cols)
        scores_rate = scores_moved / med["scores"]                                               # bytes per ms
        yardstick_ms = moved / scores_rate
        rec["cases"][name] = c = {
            "source": [n_lat, n_lon], "target": [n_rows, n_cols], "taps_rows": [int(p.rows.count.min()), int(p.rows.count.max())],
            "taps_cols": [int(p.cols.count.min()), int(p.cols.count.max())], "moved_GB": moved / 1e9, "kernel_ms": med["kernel"],
            "kernel_ms_min_max": span["kernel"], "kernel_TBps": moved / med["kernel"] / 1e9, "scores_ms": med["scores"],
            "scores_ms_min_max": span["scores"], "scores_TBps": scores_rate / 1e9, "yardstick_ms": yardstick_ms,
            "over_yardstick": med["kernel"] / yardstick_ms, "call_ms": med["call"], "call_ms_min_max": span["call"],
            "torch_ms": med["torch"], "torch_ms_min_max": span["torch"], "torch_over_kernel": med["torch"] / med["kernel"],
            "worst_relative_difference_to_torch": worst}
        print(f"{name} ({n_lat} x {n_lon} -> {n_rows} x {n_cols}, {c['moved_GB']:.3f} GB moved): kernel call {c['kernel_ms']:.3f} ms "
              f"(device time, median of {args.repeats} graph replays of {args.calls} calls; {span['kernel'][0]:.3f}-{span['kernel'][1]:.3f}) "
              f"= {c['kernel_TBps']:.2f} TB/s; aurora_hip_scores in the same session {c['scores_TBps']:.2f} TB/s, at which these "
              f"bytes take {yardstick_ms:.3f} ms: {c['over_yardstick']:.2f} x", flush=True)
        print(f"    conservative_regrid() issued eagerly {c['call_ms']:.3f} ms per call; torch expression (two dense fp64 products) "
              f"{c['torch_ms']:.1f} ms = {c['torch_over_kernel']:.1f} x the kernel call; largest relative difference to it {worst:.2e}",
              flush=True)
        del b, out_b, src, out, Wr, Wc, need
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
