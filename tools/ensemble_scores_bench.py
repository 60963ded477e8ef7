"""`aurora_amd.ensemble_scores` on the device for one 0.25-degree state (721 x 1440; 4 surface + 5 x 13 atmospheric variables
= 69 planes, 286 MB per member) with M = 8, 16 and 51 members, beside the same quantities as a plain torch expression.

    python tools/ensemble_scores_bench.py [--members 8 16 51] [--calls 20] [--repeats 5]

State and timing: tools/verification_bench.py.  Data: seeded on the device, truth = 101325 + 300 randn per plane,
member = truth + 0.5 + 2 randn.
Kernel arm: the ONE aurora_hip_ensemble_scores call over all 69 planes (`lib.ensemble_scores_sums`: two launches), --calls of
them per graph.  Bytes read = (M + 1) x planes x 721 x 1440 x 4, counted here from the shapes; TB/s = bytes / that time;
`x bytes / 5.0 TB/s` is that time over what the read alone would take at the rate scores.hip reaches (1.0 = bandwidth-bound
as that kernel is; above it the bucket is bound by its arithmetic).  Eager arm: `ensemble_scores()` end to end (checks,
cached tables, the call, the finalising torch operations).
Torch: what a user would write on the same device without this kernel -- fp64 differences, a finite mask, `torch.sort`
over the members for g and the ranks -- evaluated VARIABLE BY VARIABLE (13 planes at a time), and for M > 16 plane by plane,
because the (M, planes, 721, 1440) fp64 temporaries of the whole state (M = 51: 29 GB each, several alive at once) do not
fit beside the members; one evaluation per repeat.
Check: both against each other on every plane within the bound of tests/test_gpu_ensemble_scores.py (Q taken from the torch
side), and the kernel repeatable bit for bit.
"""
import argparse
import json

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, ensemble_scores  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib
from aurora_amd.scores import latitude_weights

ROOF_TBPS = 5.0                                   # what scores.hip reaches on this state (profiles/scores_bench.log)
REL = 1e-9


def batch(g: torch.Generator, base: Batch | None = None) -> Batch:
    """Seeded synthetic fields: the truth, or with `base` a member = base + 0.5 + 2 randn."""
    r = lambda *lead: torch.randn(*lead, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    return state(lambda *lead: r(*lead).mul_(300).add_(101325)) if base is None else state(lambda *lead: r(*lead).mul_(2).add_(0.5), base)


def torch_sums(x: torch.Tensor, y: torch.Tensor, w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """x (M, P, n_lat, n_lon), y (P, n_lat, n_lon) fp32 -> the eight sums (P, 8), the M + 2 counts (P, M + 2) and Q (P,) as a
    plain torch expression: fp64, masked like nansum, g and the ranks from `torch.sort` over the members."""
    M = x.shape[0]
    ok = torch.isfinite(y) & torch.isfinite(x).all(dim=0)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    W = torch.where(ok, w[:, None], zero)
    d = torch.where(ok, x.double() - y.double(), zero)
    total = lambda v: v.sum(dim=(-2, -1))  # noqa: E731
    e = d.sum(dim=0) / M
    a = d.abs().sum(dim=0) / M
    coef = (2.0 * torch.arange(1, M + 1, device=x.device, dtype=torch.float64) - M - 1).view(M, 1, 1, 1)
    g = (2.0 / M ** 2) * (coef * torch.sort(d, dim=0).values).sum(dim=0)
    v = ((d - e) ** 2).sum(dim=0) / (M - 1)
    q = (d * d).sum(dim=0) / M
    sums = torch.stack([total(ok.double()), total(W), total(W * e), total(W * e * e), total(W * e.abs()), total(W * a),
                        total(W * g), total(W * v)], dim=-1)
    below = (x < y).sum(dim=0)
    bins = torch.stack([total(ok & (below == b)) for b in range(M + 1)] + [total(ok & (x == y).any(dim=0))], dim=-1)
    return sums, bins, total(W * q)


def case(M: int, calls: int, repeats: int) -> dict:
    g = torch.Generator(device="cuda").manual_seed(M)
    truth = batch(g)
    members = [batch(g, truth) for _ in range(M)]
    w = torch.from_numpy(latitude_weights(truth.metadata.lat.numpy())).cuda()
    X, T = [planes(b) for b in members], planes(truth)
    kernel = lambda: lib.ensemble_scores_sums(X, T, w)  # noqa: E731
    whole = lambda: ensemble_scores(members, truth)  # noqa: E731
    group = 13 if M <= 16 else 1                       # planes per torch evaluation (see the module's text)

    def plain():
        out = []
        for i, t in enumerate(T):
            x, t = torch.stack([X[m][i][0] for m in range(M)]).reshape(M, -1, N_LAT, N_LON), t[0].reshape(-1, N_LAT, N_LON)
            for k in range(0, t.shape[0], group):
                out.append(torch_sums(x[:, k:k + group], t[k:k + group], w))
        return [torch.cat(c) for c in zip(*out)]

    got, again, want = kernel(), kernel(), plain()
    whole()
    torch.cuda.synchronize()
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), "the kernel's results are not repeatable"
    s, h = got[0].cpu().numpy(), got[1].cpu().numpy()
    y, yh, Q = (v.cpu().numpy() for v in want)
    assert s.shape == (N_PLANES, 8) and (s[:, 0] == y[:, 0]).all() and (h == yh).all(), "counts differ"
    worst = 0.0
    for slot, scale in ((1, y[:, 1]), (5, y[:, 5]), (2, y[:, 5]), (4, y[:, 5]), (6, 2 * y[:, 5]), (3, Q), (7, 2 * Q)):
        worst = max(worst, float(np.max(np.abs(s[:, slot] - y[:, slot]) / scale)))
    assert worst <= REL, worst
    for f in (kernel, whole):
        window_ms(f, 3)
    ms = alternate({"kernel": captured(kernel, calls), "torch": lambda: window_ms(plain, 1),
                    "scores": lambda: window_ms(whole, calls)}, repeats)
    read = (M + 1) * N_PLANES * N_LAT * N_LON * 4
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    return {"members": M, "planes": N_PLANES, "grid": [N_LAT, N_LON], "read_GB": read / 1e9, "calls_per_window": calls,
            "repeats": repeats, "kernel_ms": med["kernel"], "kernel_ms_min_max": span["kernel"],
            "kernel_TBps": read / med["kernel"] / 1e9, "roof_ms_at_5TBps": read / ROOF_TBPS / 1e9,
            "kernel_over_roof": med["kernel"] / (read / ROOF_TBPS / 1e9), "ensemble_scores_call_ms": med["scores"],
            "torch_ms": med["torch"], "torch_ms_min_max": span["torch"],
            "torch_planes_per_evaluation": group, "torch_over_kernel": med["torch"] / med["kernel"],
            "worst_error_over_bound_1e-9": worst / REL}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[8, 16, 51])
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} per member "
          f"({N_PLANES * N_LAT * N_LON * 4 / 1e6:.0f} MB)", flush=True)
    for M in args.members:
        rec = case(M, args.calls, args.repeats)
        print(f"M = {M:2d}: {rec['read_GB']:.2f} GB read: kernel call {rec['kernel_ms']:.3f} ms (device time, median of "
              f"{rec['repeats']} graph replays of {rec['calls_per_window']} calls; {rec['kernel_ms_min_max'][0]:.3f}-"
              f"{rec['kernel_ms_min_max'][1]:.3f}) = {rec['kernel_TBps']:.2f} TB/s = {rec['kernel_over_roof']:.2f} x bytes / "
              f"{ROOF_TBPS} TB/s ({rec['roof_ms_at_5TBps']:.3f} ms); ensemble_scores() end to end, eager, "
              f"{rec['ensemble_scores_call_ms']:.3f} ms; torch expression ({rec['torch_planes_per_evaluation']} planes at a "
              f"time) {rec['torch_ms']:.1f} ms = {rec['torch_over_kernel']:.0f} x the kernel call; agreement "
              f"{rec['worst_error_over_bound_1e-9']:.2e} of the 1e-9 bound, counts equal", flush=True)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
