"""`aurora_amd.diagnostics` on the device for a 0.25-degree state (721 x 1440, 13 levels, B = 1) with every name asked for:
vorticity, divergence and wind speed on 13 levels and at 10 m (14 wind items) and the four vertical integrals, beside the
same quantities as a torch expression.

    python tools/diagnostics_bench.py [--calls 20] [--repeats 5]

Grid and timing: tools/verification_bench.py; the state is this bench's own (winds and humidity on real pressure levels).
Kernel arm: the ONE aurora_hip_diagnostics call (`lib.diagnostics`: the wind launch and the column launch) on preallocated
outputs, --calls of them per graph.  Bytes = 4 x 721 x 1440 x (14 x (2 + 3) + 13 x 3 + 4) planes: every input plane a group
reads once and every output written once, counted here from the shapes (u and v on levels are read by both launches and
counted twice); TB/s = bytes / that time.  Beside it, a graph arm too, aurora_hip_scores over 69 prediction and 69 truth
planes (bytes = 4 x 721 x 1440 x 138): the streaming rate a reduction kernel of this library reaches here.  Eager arm:
`diagnostics(batch, ALL)` (checks, cached tables, output allocation, the call).  Torch: the formulas of include/aurora_hip.h
as `torch.roll` expressions in fp64 on the device (what a user would write without this kernel), in eager windows.
Check: the call and `diagnostics()` give the same bits, the wind speed and the NaN pattern of the torch expression are equal,
and the largest difference of the other fields relative to the result is reported (the bound, which is relative to the terms
and not to the result, is tests/test_gpu_diagnostics.py's).
"""
import argparse
import json

import torch
from verification_bench import N_LAT, N_LON, N_PLANES as SCORE_PLANES, alternate, captured, med_min_max, metadata, window_ms

from aurora_amd import Batch, diagnostics  # (verification_bench has put the repository on sys.path)
from aurora_amd.diagnostics import NAMES, _grid, level_weights, row_table
from aurora_amd.engine import lib

LEVELS = (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)
C = len(LEVELS)
ALL = tuple(NAMES)


def state(seed: int) -> Batch:
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda off, sc, *s: off + sc * torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    return Batch({"10u": r(40, 5, 1, 1), "10v": r(-30, 5, 1, 1)}, {},
                 {"u": r(40, 5, 1, 1, C), "v": r(-30, 5, 1, 1, C), "q": (0.005 * (1 + 0.3 * r(0, 1, 1, 1, C))).abs()},
                 metadata(atmos_levels=LEVELS))


def torch_diagnostics(b: Batch, rows: torch.Tensor, L: float, w: torch.Tensor) -> dict:
    """Every name as elementwise torch in fp64 (global grid: the longitude difference wraps)."""
    A, m0, m1, m2 = (rows[:, k][:, None] for k in range(4))
    north = torch.clamp(torch.arange(N_LAT, device="cuda") - 1, min=0)
    south = torch.clamp(torch.arange(N_LAT, device="cuda") + 1, max=N_LAT - 1)
    nan = torch.full((), float("nan"), device="cuda")
    fin = lambda x: torch.where(torch.isfinite(x.float()), x.float(), nan)  # noqa: E731
    d_lon = lambda f: (torch.roll(f, -1, -1) - torch.roll(f, 1, -1)) * L  # noqa: E731
    d_lat = lambda f: m0 * f[..., north, :] + m1 * f + m2 * f[..., south, :]  # noqa: E731
    out = {}
    for prefix, (u, v) in (("", (b.atmos_vars["u"], b.atmos_vars["v"])), ("10", (b.surf_vars["10u"], b.surf_vars["10v"]))):
        u, v = u[:, -1].double(), v[:, -1].double()
        out[prefix + "ws"] = fin(torch.sqrt(u * u + v * v))
        out[prefix + "vo"] = fin(A * (d_lon(v) - d_lat(u)))
        out[prefix + "d"] = fin(A * (d_lon(u) + d_lat(v)))
    q, u, v = (b.atmos_vars[k][:, -1].double() for k in ("q", "u", "v"))
    wq = w[None, :, None, None] * q
    t, iu, iv = wq.sum(1), (wq * u).sum(1), (wq * v).sum(1)
    out.update(tcwv=fin(t), ivtu=fin(iu), ivtv=fin(iv), ivt=fin(torch.sqrt(iu * iu + iv * iv)))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    P = N_LAT * N_LON
    moved = 4 * P * ((C + 1) * (2 + 3) + C * 3 + 4)
    print(f"device: {torch.cuda.get_device_name()}; {N_LAT} x {N_LON}, {C} levels, {len(ALL)} names: {(C + 1) * 3 + 4} output planes, "
          f"{moved / 1e9:.3f} GB moved per call", flush=True)
    b = state(0)
    md = b.metadata
    lat, lon = md.lat.numpy(), md.lon.numpy()
    L, wrap = _grid(lat, lon)
    rows = torch.from_numpy(row_table(lat)).cuda()
    w = torch.from_numpy(level_weights(LEVELS)).cuda()
    ua, va, q = (b.atmos_vars[k][:, -1] for k in ("u", "v", "q"))
    us, vs = (b.surf_vars[k][:, -1] for k in ("10u", "10v"))
    new = lambda *s: torch.empty(*s, N_LAT, N_LON, device="cuda")  # noqa: E731
    outs = {k: [new(1, C), new(1)] for k in ("vo", "div", "ws")} | {k: [new(1)] for k in ("tcwv", "ivtu", "ivtv", "ivt")}
    kernel = lambda: lib.diagnostics(N_LAT, N_LON, u=[ua, us], v=[va, vs], row_table=rows, L=L, wrap=wrap, q=[q], col_u=[ua],  # noqa: E731
                                     col_v=[va], level_w=w, **outs)
    whole = lambda: diagnostics(b, ALL)  # noqa: E731
    plain = lambda: torch_diagnostics(b, rows, L, w)  # noqa: E731

    # the check: one call of each
    kernel()
    want = plain()
    got = {"ws": outs["ws"][0], "10ws": outs["ws"][1], "vo": outs["vo"][0], "10vo": outs["vo"][1], "d": outs["div"][0],
           "10d": outs["div"][1], **{k: outs[k][0] for k in ("tcwv", "ivtu", "ivtv", "ivt")}}
    pub = whole()
    torch.cuda.synchronize()
    worst = 0.0
    for k, t in got.items():
        ref = want[k].reshape(t.shape)
        assert torch.equal(torch.isnan(t), torch.isnan(ref)), f"{k}: NaN pattern differs from the torch expression"
        assert torch.equal(torch.nan_to_num(t).reshape(-1), torch.nan_to_num(getattr(pub, NAMES[k][0])[k]).reshape(-1)), k
        if k in ("ws", "10ws"):
            assert torch.equal(t, ref), f"{k} differs from the torch expression"
            continue
        ok = ~torch.isnan(t)
        worst = max(worst, float(((t[ok].double() - ref[ok].double()).abs() / ref[ok].abs().double().clamp(min=1e-300)).max()))

    pred = [torch.randn(SCORE_PLANES, N_LAT, N_LON, device="cuda")]
    truth = [torch.randn(SCORE_PLANES, N_LAT, N_LON, device="cuda")]
    row_w = torch.ones(N_LAT, dtype=torch.float64, device="cuda")
    score = lambda: lib.scores_sums(pred, truth, None, row_w)  # noqa: E731
    for f in (kernel, whole, plain, score):
        window_ms(f, 3)
    ms = alternate({"kernel": captured(kernel, args.calls), "scores": captured(score, args.calls),
                    "torch": lambda: window_ms(plain, 3), "call": lambda: window_ms(whole, args.calls)}, args.repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    scores_moved = 4 * P * 2 * SCORE_PLANES
    rec = {"grid": [N_LAT, N_LON], "levels": C, "names": len(ALL), "moved_GB": moved / 1e9, "calls_per_window": args.calls,
           "repeats": args.repeats, "kernel_ms": med["kernel"], "kernel_ms_min_max": span["kernel"],
           "kernel_TBps": moved / med["kernel"] / 1e9, "scores_moved_GB": scores_moved / 1e9, "scores_ms": med["scores"],
           "scores_ms_min_max": span["scores"], "scores_TBps": scores_moved / med["scores"] / 1e9,
           "diagnostics_call_ms": med["call"], "diagnostics_call_ms_min_max": span["call"],
           "torch_ms": med["torch"], "torch_ms_min_max": span["torch"],
           "torch_over_kernel": med["torch"] / med["kernel"], "worst_relative_difference_to_torch": worst}
    print(f"every name of a {C}-level 0.25-degree state: {rec['moved_GB']:.3f} GB moved: kernel call {rec['kernel_ms']:.3f} ms (device "
          f"time, median of {args.repeats} graph replays of {args.calls} calls; {rec['kernel_ms_min_max'][0]:.3f}-"
          f"{rec['kernel_ms_min_max'][1]:.3f}) = {rec['kernel_TBps']:.2f} TB/s; aurora_hip_scores in the same session "
          f"{rec['scores_TBps']:.2f} TB/s ({rec['scores_moved_GB']:.3f} GB in {rec['scores_ms']:.3f} ms)", flush=True)
    print(f"diagnostics() issued eagerly {rec['diagnostics_call_ms']:.3f} ms per call; torch expression (roll, fp64) "
          f"{rec['torch_ms']:.1f} ms = {rec['torch_over_kernel']:.1f} x the kernel call; largest relative difference to it "
          f"{worst:.2e}", flush=True)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
