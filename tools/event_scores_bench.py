"""`aurora_amd.event_scores` on the device for one 0.25-degree state (721 x 1440; 4 surface + 5 x 13 atmospheric variables =
69 planes), T = 3 thresholds per plane, window sizes (1, 5, 9, 17, 33), beside the same integers as a torch expression.

    python tools/event_scores_bench.py [--calls 10] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arm: the ONE aurora_hip_event_scores call over all 69 planes
(`lib.event_rowsums`: two launches), --calls of them per graph.  Eager arm: `event_scores()` end to end (the call plus the
finalisation).  Read floor: the time a single read of both inputs (2 x 69 x 721 x 1440 x 4 bytes) takes at the rate
`aurora_hip_scores` reaches on this device, measured here the same way (it reads the same two inputs once).
Torch: what a user would write on the same device without this kernel -- per threshold the two masks, then per window size
F.avg_pool2d with circular longitude / zero latitude padding and divisor 1 in fp32 (counts <= 33^2 are exact), the three
squares summed per row in fp64 -- batched over all 69 planes, in eager windows: a yardstick only.
Check: the torch expression and the kernel must be equal on every integer, and the kernel repeatable.
"""
import argparse
import json

import torch
import torch.nn.functional as F
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, event_scores, field_quantiles  # (verification_bench has put the repository on sys.path)
from aurora_amd._fields import device_weights
from aurora_amd.engine import lib

SCALES = (1, 5, 9, 17, 33)
QUANTILES = (0.5, 0.9, 0.99)


def batch(seed: int, base: Batch | None = None, spread: float = 1.0) -> Batch:
    """Smooth fields (white noise box-filtered over 15 x 15 points, so that events cluster), 5e4 + O(1)."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def r(*s):
        x = torch.randn(int(torch.tensor(s).prod()), 1, N_LAT, N_LON, device="cuda", generator=g)
        x = F.avg_pool2d(F.pad(x, (7, 7, 7, 7), mode="circular"), 15, stride=1) * 15.0
        return (spread * x).reshape(*s, N_LAT, N_LON)

    return state(r, base) if base is not None else state(lambda *s: r(*s) + 5e4)


def torch_rowsums(p: torch.Tensor, t: torch.Tensor, thr: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(P, T, S, n_lat, 3) int64 and (P, n_lat) int64 for (P, n_lat, n_lon) fields and (P, T) thresholds: a plain torch
    expression, one threshold at a time (a threshold's masks and pooled planes of all 69 planes are ~1.6 GB each)."""
    ok = torch.isfinite(p) & torch.isfinite(t)
    okd = ok.double()
    out = torch.empty(p.shape[0], thr.shape[1], len(SCALES), N_LAT, 3, dtype=torch.int64, device=p.device)
    for ti in range(thr.shape[1]):
        th = thr[:, ti, None, None]
        f, o = (ok & (p >= th)).float()[:, None], (ok & (t >= th)).float()[:, None]
        for si, n in enumerate(SCALES):
            h = n // 2
            pool = lambda x: x if n == 1 else F.avg_pool2d(F.pad(F.pad(x, (h, h, 0, 0), mode="circular"), (0, 0, h, h)), n,  # noqa: E731
                                                           stride=1, divisor_override=1)
            cf, co = pool(f)[:, 0].double(), pool(o)[:, 0].double()
            out[:, ti, si, :, 0] = (((cf - co) ** 2) * okd).sum(dim=-1).long()
            out[:, ti, si, :, 1] = ((cf ** 2) * okd).sum(dim=-1).long()
            out[:, ti, si, :, 2] = ((co ** 2) * okd).sum(dim=-1).long()
    return out, ok.sum(dim=-1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} per input, T = {len(QUANTILES)}, "
          f"scales {SCALES}", flush=True)
    truth = batch(0)
    pred = batch(1, truth, spread=0.5)
    P, T = planes(pred), planes(truth)
    fq = field_quantiles(truth, QUANTILES, kind="count")       # every plane's quantiles by count, where the plane lives
    thresholds = fq.thresholds()
    thr = fq.value_table                                       # (planes, T)
    row_w = device_weights("event_scores_bench", truth.metadata.lat.numpy(), torch.device("cuda", torch.cuda.current_device()))

    kernel = lambda: lib.event_rowsums(P, T, thr, SCALES)  # noqa: E731
    whole = lambda: event_scores(pred, truth, thresholds, scales=SCALES)  # noqa: E731
    reader = lambda: lib.scores_sums(P, T, None, row_w)  # noqa: E731
    pc, tc = torch.cat([x.reshape(-1, N_LAT, N_LON) for x in P]), torch.cat([x.reshape(-1, N_LAT, N_LON) for x in T])
    plain = lambda: torch_rowsums(pc, tc, thr)  # noqa: E731

    got, again, want = kernel(), kernel(), plain()
    s = whole()
    reader()
    torch.cuda.synchronize()
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), "the kernel's tables are not repeatable"
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "the torch expression and the kernel differ"
    assert torch.equal(s.rowsums_table, got[0])
    fss = s.cpu().fss["2t"][0]
    for f in (kernel, whole, plain, reader):
        window_ms(f, 3)
    ms = alternate({"kernel": captured(kernel, args.calls), "scores": captured(reader, args.calls),
                    "torch": lambda: window_ms(plain, 2), "event_scores": lambda: window_ms(whole, args.calls)}, args.repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    gbytes = 2 * N_PLANES * N_LAT * N_LON * 4 / 1e9
    rec = {"planes": N_PLANES, "grid": [N_LAT, N_LON], "thresholds": len(QUANTILES), "scales": list(SCALES),
           "calls_per_window": args.calls, "repeats": args.repeats, "kernel_ms": med["kernel"],
           "kernel_ms_min_max": span["kernel"], "event_scores_call_ms": med["event_scores"],
           "input_GB": gbytes, "scores_read_ms": med["scores"], "scores_read_TBps": gbytes / med["scores"],
           "kernel_over_one_read": med["kernel"] / med["scores"], "torch_ms": med["torch"],
           "torch_ms_min_max": span["torch"], "kernel_over_torch": med["kernel"] / med["torch"],
           "torch_over_kernel": med["torch"] / med["kernel"], "integers_equal": True,
           "fss_2t_first_threshold": [round(float(x), 4) for x in fss[0]]}
    print(f"kernel call {rec['kernel_ms']:.3f} ms (device time, median of {args.repeats} graph replays of {args.calls} calls; "
          f"{rec['kernel_ms_min_max'][0]:.3f}-{rec['kernel_ms_min_max'][1]:.3f}); event_scores() end to end, eager "
          f"{rec['event_scores_call_ms']:.3f} ms; one read of both inputs ({gbytes:.2f} GB) at the rate of aurora_hip_scores "
          f"({rec['scores_read_TBps']:.2f} TB/s) {rec['scores_read_ms']:.3f} ms: the kernel takes {rec['kernel_over_one_read']:.1f} x "
          f"that; torch expression {rec['torch_ms']:.1f} ms ({rec['torch_ms_min_max'][0]:.1f}-{rec['torch_ms_min_max'][1]:.1f}): "
          f"kernel / torch = {rec['kernel_over_torch']:.4f} (torch / kernel = {rec['torch_over_kernel']:.1f}); every integer equal",
          flush=True)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
