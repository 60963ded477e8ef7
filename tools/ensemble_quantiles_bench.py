"""`aurora_amd.ensemble_quantiles` on the device for one 0.25-degree state (721 x 1440; 4 surface + 5 x 13 atmospheric variables
= 69 planes, 286 MB per member) with M = 8, 16 and 51 members and Q = 3 (q = 0.1, 0.5, 0.9), with a truth (the rank map).

    python tools/ensemble_quantiles_bench.py [--members 8 16 51] [--calls 20] [--repeats 5]

State and timing: tools/verification_bench.py.  Data: as tools/ensemble_scores_bench.py (truth = 101325 + 300 randn per plane,
member = truth + 0.5 + 2 randn, seeded on the device).
Arm 1, kernel: the ONE aurora_hip_ensemble_quantiles call over all 69 planes (`lib.ensemble_quantiles` into buffers given with
out= / rank_out=, as a roll-out would: one launch), --calls of them per graph.  Bytes = (4 (M + 1) + 4 Q + 1) x planes x 721 x
1440, counted here from the shapes.
Arm 2, front end: `ensemble_quantiles()` end to end, issued eagerly (checks, the cached plane table, the call, the outputs
allocated).
Arm 3, ensemble_scores: `aurora_hip_ensemble_scores` on the same members and truth in the same session (`lib.ensemble_scores_sums`
in a graph): it reads the same planes, sorts the same way and adds an fp64 second pass, but writes next to nothing.
Arm 4, torch: the same rule as a plain torch expression on the device -- `torch.sort` over the stacked members, two gathers,
the three fp64 operations, a finite mask, `(x < y).sum(0)` -- VARIABLE BY VARIABLE in as many planes at a time as fit in the
free memory (13, 4 or 1; 20 bytes per member value: the stack, the sorted copy, int64 indices and a mask; the planes of one
variable lie together in a batch, so more at a time would cost a copy of the ensemble first); one evaluation per repeat.
Also timed, for the expectation only: `aurora_hip_scores` (`lib.scores_sums`, a member against the truth), whose read rate R
in this session prices the written bytes: expected = ensemble_scores time + (4 Q + 1) x points / R.
Check: the kernel's maps and ranks equal the torch expression's in every bit (the data hold no zeros, whose sign
`torch.sort` does not order), and the kernel is repeatable bit for bit.
"""
import argparse
import json

import torch
from verification_bench import N_LAT, N_LON, N_PLANES, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, ensemble_quantiles  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib
from aurora_amd.quantiles import quantile_index
from aurora_amd.scores import latitude_weights

Q = (0.1, 0.5, 0.9)


def batch(g: torch.Generator, base: Batch | None = None) -> Batch:
    """Seeded synthetic fields: the truth, or with `base` a member = base + 0.5 + 2 randn."""
    r = lambda *lead: torch.randn(*lead, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    return state(lambda *lead: r(*lead).mul_(300).add_(101325)) if base is None else state(lambda *lead: r(*lead).mul_(2).add_(0.5), base)


def torch_quantiles(x: torch.Tensor, y: torch.Tensor, j, g) -> tuple[torch.Tensor, torch.Tensor]:
    """x (M, P, n_lat, n_lon), y (P, n_lat, n_lon) fp32 -> (P, Q, n_lat, n_lon) fp32 and (P, n_lat, n_lon) int8."""
    M = x.shape[0]
    s = torch.sort(x, dim=0).values
    valid = torch.isfinite(x).all(dim=0)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=x.device)
    maps = []
    for ji, gi in zip(j.tolist(), g.tolist()):
        a, b = s[ji].double(), s[min(ji + 1, M - 1)].double()
        maps.append(torch.where(valid, a + gi * (b - a), nan).float())
    rank = torch.where(valid & torch.isfinite(y), (x < y).sum(dim=0), -1).to(torch.int8)
    return torch.stack(maps, dim=1), rank


def case(M: int, calls: int, repeats: int) -> dict:
    g = torch.Generator(device="cuda").manual_seed(M)
    truth = batch(g)
    members = [batch(g, truth) for _ in range(M)]
    w = torch.from_numpy(latitude_weights(truth.metadata.lat.numpy())).cuda()
    X, T = [planes(b) for b in members], planes(truth)
    out = torch.empty(N_PLANES, len(Q), N_LAT, N_LON, device="cuda")
    rank_out = torch.empty(N_PLANES, N_LAT, N_LON, dtype=torch.int8, device="cuda")
    kernel = lambda: lib.ensemble_quantiles(X, T, Q, out=out, rank_out=rank_out)  # noqa: E731
    whole = lambda: ensemble_quantiles(members, Q, truth)  # noqa: E731
    ens = lambda: lib.ensemble_scores_sums(X, T, w)  # noqa: E731
    det = lambda: lib.scores_sums(X[0], T, None, w)  # noqa: E731
    j, gq = quantile_index(M, Q)
    free = torch.cuda.mem_get_info()[0]
    group = next(p for p in (13, 4, 1) if p == 1 or M * p * N_LAT * N_LON * 20 < 0.6 * free)

    def plain():
        res = []
        for i, v in enumerate(T):
            xi, ti = torch.stack([X[m][i][0] for m in range(M)]).reshape(M, -1, N_LAT, N_LON), v[0].reshape(-1, N_LAT, N_LON)
            for k in range(0, ti.shape[0], group):
                res.append(torch_quantiles(xi[:, k:k + group], ti[k:k + group], j, gq))
        return [torch.cat(c) for c in zip(*res)]

    kernel()
    first = (out.clone(), rank_out.clone())
    kernel()
    want = plain()
    whole()
    torch.cuda.synchronize()
    assert torch.equal(first[0].view(torch.int32), out.view(torch.int32)) and torch.equal(first[1], rank_out), "not repeatable"
    assert torch.equal(out.view(torch.int32), want[0].view(torch.int32)), "the maps differ from the torch expression"
    assert torch.equal(rank_out, want[1]), "the ranks differ from the torch expression"
    del want, first
    for f in (kernel, whole, ens, det):
        window_ms(f, 3)
    ms = alternate({"kernel": captured(kernel, calls), "front_end": lambda: window_ms(whole, calls),
                    "ensemble_scores": captured(ens, calls), "scores": captured(det, calls),
                    "torch": lambda: window_ms(plain, 1)}, repeats)
    points = N_PLANES * N_LAT * N_LON
    read, written = 4 * (M + 1) * points, (4 * len(Q) + 1) * points
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    scores_rate = 2 * 4 * points / med["scores"] / 1e9             # TB/s that aurora_hip_scores reads at in this session
    expected = med["ensemble_scores"] + written / scores_rate / 1e9
    return {"members": M, "q": list(Q), "planes": N_PLANES, "grid": [N_LAT, N_LON], "read_GB": read / 1e9,
            "written_GB": written / 1e9, "calls_per_window": calls, "repeats": repeats, "kernel_ms": med["kernel"],
            "kernel_ms_min_max": span["kernel"], "kernel_TBps": (read + written) / med["kernel"] / 1e9,
            "ensemble_quantiles_call_ms": med["front_end"], "ensemble_scores_kernel_ms": med["ensemble_scores"],
            "ensemble_scores_kernel_ms_min_max": span["ensemble_scores"], "scores_kernel_ms": med["scores"],
            "scores_read_TBps": scores_rate, "expected_ms": expected, "kernel_over_expected": med["kernel"] / expected,
            "torch_ms": med["torch"], "torch_ms_min_max": span["torch"], "torch_planes_per_evaluation": group,
            "torch_over_kernel": med["torch"] / med["kernel"], "bits_equal_torch": True}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[8, 16, 51])
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} per member "
          f"({N_PLANES * N_LAT * N_LON * 4 / 1e6:.0f} MB); q = {Q}, with a truth", flush=True)
    for M in args.members:
        r = case(M, args.calls, args.repeats)
        print(f"M = {M:2d}: {r['read_GB']:.2f} GB read, {r['written_GB']:.2f} GB written: kernel call {r['kernel_ms']:.3f} ms "
              f"(device time, median of {r['repeats']} graph replays of {r['calls_per_window']} calls; "
              f"{r['kernel_ms_min_max'][0]:.3f}-{r['kernel_ms_min_max'][1]:.3f}) = {r['kernel_TBps']:.2f} TB/s moved; "
              f"aurora_hip_ensemble_scores on the same members {r['ensemble_scores_kernel_ms']:.3f} ms, aurora_hip_scores reads "
              f"at {r['scores_read_TBps']:.2f} TB/s, so expected {r['expected_ms']:.3f} ms: the kernel takes "
              f"{r['kernel_over_expected']:.2f} x that; ensemble_quantiles() end to end, eager, "
              f"{r['ensemble_quantiles_call_ms']:.3f} ms; torch.sort expression ({r['torch_planes_per_evaluation']} planes at a "
              f"time) {r['torch_ms']:.1f} ms = {r['torch_over_kernel']:.0f} x the kernel call; maps and ranks equal the torch "
              f"expression's in every bit", flush=True)
        print(json.dumps(r), flush=True)
        del r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
