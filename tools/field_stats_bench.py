"""`aurora_amd.FieldStats` on the device for a 0.25-degree state (721 x 1440; 4 surface + 5 x 13 atmospheric variables = 69
planes) with T = 2 thresholds: M = 16 ensemble members in ONE update, beside the same recurrence as plain torch.

    python tools/field_stats_bench.py [--calls 20] [--repeats 5]

State (here with B members as its batch elements) and timing: tools/verification_bench.py.  Kernel arms: the ONE
aurora_hip_field_stats_update call over all 69 planes and 16 samples (`lib.field_stats_update`: the main launch and the
one-thread launch that advances the sample index), --calls of them per graph, and a one-sample update (a roll-out step).
Bytes = planes x 721 x 1440 x (4 M + 2 (36 + 12 T)): every sample read once, the state read once and written once, counted
here from the shapes (one sample: 4 + 2 (36 + 12 T) bytes per point); TB/s = bytes / that time.  Eager arms:
`FieldStats.update(members, over="batch")` (checks, cached tables, the call) and the one-sample `update`.  Torch: the same
state advanced sample by sample with elementwise torch operations on the device (what a user would write without this
kernel), in eager windows.  Check: the integers, origin, minimum and maximum of both are equal and the sums agree to the
bound of tests/test_gpu_field_stats.py.  The share of a step is the one-sample `update` issued eagerly over the 124 ms of the
0.25-degree step.
"""
import argparse
import json

import torch
from verification_bench import ATMOS, N_LAT, N_LON, N_PLANES, STEP_MS, SURF, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, FieldStats  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib

M, T = 16, 2
THRESHOLDS = {k: [280.5, 281.5] for k in (*SURF, *ATMOS)}


def members(seed: int, B: int) -> Batch:
    g = torch.Generator(device="cuda").manual_seed(seed)
    return state(lambda *s: 280.0 + torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g), B=B)


def new_state() -> dict:
    P = N_LAT * N_LON
    return {k: torch.zeros((N_PLANES, T, P) if per_thr else (N_PLANES, P), dtype=dt, device="cuda")
            for k, (dt, per_thr) in lib.FIELD_STATS_STATE.items()}


def torch_update(s: dict, x: torch.Tensor, thr: torch.Tensor, index: int) -> None:
    """One sample x (n_planes, n_points) fp32 into the state: the recurrence of include/aurora_hip.h as elementwise torch."""
    ok = torch.isfinite(x)
    v = x.double()
    first = ok & (s["n"] == 0)
    s["origin"].copy_(torch.where(first, x, s["origin"]))
    d = torch.where(ok, v - s["origin"].double(), torch.zeros((), dtype=torch.float64, device=x.device))
    s["s1"] += d
    s["s2"] += d * d
    for ext, arg, new in (("vmin", "argmin", first | (ok & (x < s["vmin"]))), ("vmax", "argmax", first | (ok & (x > s["vmax"])))):
        s[ext].copy_(torch.where(new, x, s[ext]))
        s[arg].copy_(torch.where(new, torch.full_like(s[arg], index), s[arg]))
    ev = (x[:, None, :] >= thr[:, :, None]) & ok[:, None, :]
    s["exceed"] += ev
    s["run"].copy_(torch.where(ok[:, None, :], torch.where(ev, s["run"] + 1, torch.zeros_like(s["run"])), s["run"]))
    s["longest"].copy_(torch.maximum(s["longest"], s["run"]))
    s["n"] += ok


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="back-to-back updates per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    P = N_LAT * N_LON
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON}, {M} members, T = {T}: state "
          f"{N_PLANES * P * (36 + 12 * T) / 1e9:.2f} GB, members {N_PLANES * P * 4 * M / 1e9:.2f} GB", flush=True)
    ens = members(0, M)
    one = members(1, 1)
    samples = [[f[m:m + 1] for f in planes(ens)] for m in range(M)]
    thr = torch.tensor([[280.5, 281.5]] * N_PLANES, dtype=torch.float32, device="cuda")
    state, index = new_state(), torch.zeros(1, dtype=torch.int64, device="cuda")
    kernel = lambda: lib.field_stats_update(samples, None, None, thr, False, index, state)  # noqa: E731
    single = lambda: lib.field_stats_update([planes(one)], None, None, thr, False, index, state)  # noqa: E731
    plain_state = new_state()
    stack = torch.stack([torch.cat([f.reshape(-1, P) for f in fs]) for fs in samples])          # (M, n_planes, P): a copy

    def plain(index0=0):
        for m in range(M):
            torch_update(plain_state, stack[m], thr, index0 + m)

    kernel()
    plain()
    torch.cuda.synchronize()
    worst = 0.0
    for k in state:                                              # the check: one update of each, from a zero state
        if k in ("s1", "s2"):
            bound = 2 * (M + 1) * 2.0 ** -53 * (plain_state["s2"] if k == "s2" else (M * plain_state["s2"]).sqrt())   # sum|d| <= sqrt(n sum d^2)
            worst = max(worst, float(((state[k] - plain_state[k]).abs() / bound.clamp(min=1e-300)).max()))
        else:
            assert torch.equal(state[k], plain_state[k]), f"{k} differs from the torch recurrence"
    assert worst <= 1.0, worst
    acc = FieldStats(thresholds=THRESHOLDS)
    acc_one = FieldStats(thresholds=THRESHOLDS)
    whole = lambda: acc.update(ens, over="batch")  # noqa: E731
    whole_one = lambda: acc_one.update(one)  # noqa: E731
    for f in (kernel, single, whole, whole_one):
        window_ms(f, 3)
    ms = alternate({"kernel": captured(kernel, args.calls), "single": captured(single, args.calls),
                    "torch": lambda: window_ms(plain, 2), "update": lambda: window_ms(whole, args.calls),
                    "update_one": lambda: window_ms(whole_one, args.calls)}, args.repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    moved = N_PLANES * P * (4 * M + 2 * (36 + 12 * T))
    moved_one = N_PLANES * P * (4 + 2 * (36 + 12 * T))
    rec = {"planes": N_PLANES, "grid": [N_LAT, N_LON], "members": M, "thresholds": T, "moved_GB": moved / 1e9,
           "calls_per_window": args.calls, "repeats": args.repeats, "kernel_ms": med["kernel"],
           "kernel_ms_min_max": span["kernel"], "kernel_TBps": moved / med["kernel"] / 1e9,
           "one_sample_moved_GB": moved_one / 1e9, "one_sample_kernel_ms": med["single"],
           "one_sample_kernel_ms_min_max": span["single"], "one_sample_TBps": moved_one / med["single"] / 1e9,
           "update_call_ms": med["update"], "one_sample_update_call_ms": med["update_one"], "torch_ms": med["torch"],
           "torch_ms_min_max": span["torch"], "torch_over_kernel": med["torch"] / med["kernel"],
           "share_of_step_percent": 100 * med["update_one"] / STEP_MS, "worst_error_over_bound": worst}
    print(f"{M} members in one update: {rec['moved_GB']:.3f} GB moved: kernel call {rec['kernel_ms']:.3f} ms (device time, median of "
          f"{args.repeats} graph replays of {args.calls} calls; {rec['kernel_ms_min_max'][0]:.3f}-{rec['kernel_ms_min_max'][1]:.3f}) = "
          f"{rec['kernel_TBps']:.2f} TB/s; update(over='batch') issued eagerly {rec['update_call_ms']:.3f} ms per call; torch "
          f"recurrence {rec['torch_ms']:.1f} ms = {rec['torch_over_kernel']:.1f} x the kernel call; sums at {worst:.2e} of the bound",
          flush=True)
    print(f"one sample per update (a roll-out step): {rec['one_sample_moved_GB']:.3f} GB moved: kernel call "
          f"{rec['one_sample_kernel_ms']:.3f} ms ({rec['one_sample_kernel_ms_min_max'][0]:.3f}-{rec['one_sample_kernel_ms_min_max'][1]:.3f}) = "
          f"{rec['one_sample_TBps']:.2f} TB/s; update() end to end {rec['one_sample_update_call_ms']:.3f} ms = "
          f"{rec['share_of_step_percent']:.2f} % of a {STEP_MS:.0f} ms step", flush=True)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
