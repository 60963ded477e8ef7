"""`aurora_amd.probability_scores` on the device for one 0.25-degree state (721 x 1440; 4 surface + 5 x 13 atmospheric variables
= 69 planes, 286 MB per member) with T = 3 thresholds and M = 8, 16 and 51 members, beside the same integers as a plain torch
expression and beside aurora_hip_ensemble_scores on the same members.

    python tools/probability_scores_bench.py [--members 8 16 51] [--calls 20] [--repeats 5] [--plain-lib PATH]

Data: seeded on the device, truth = 101325 + 300 randn per plane, member = truth + 60 randn (a spread of a fifth of the
climatological deviation); thresholds 101325, 101709 and 102024 on every plane (about the 0.5, 0.9 and 0.99 quantiles of the
truth).  The share of valid points outside the two corner bins (o = 0, k = 0) and (o = 1, k = M) is printed per threshold: those
are the points that reach an LDS atomic in the kernel's ballot form.
State and timing: tools/verification_bench.py.  Kernel arm: the ONE aurora_hip_probability_scores call over all 69 planes
(`lib.probability_rows`: one launch), --calls of them per graph.  Bytes read = (M + 1) x planes x 721 x 1440 x 4, counted here
from the shapes; TB/s = bytes / that time.  Yardstick: the same bytes at the rate aurora_hip_ensemble_scores reaches on the
same members in the same session (a graph arm too): `x ensemble_scores` is this call's time over that call's time, both
reading the same bytes.
--plain-lib: a second build of the library whose kernel sends EVERY valid lane through an LDS atomic instead of taking the two
corner bins by ballot and popcount:
    AURORA_BUILD_FLAGS=-DAURORA_PROBABILITY_PLAIN_ATOMICS python -m aurora_amd.build --force, the library then copied aside
(and the default build restored).  It is called through the same plane table, checked equal, and timed alternating with the
default form.
Also `probability_scores()` end to end, issued eagerly (checks, cached tables, the call, the finalising torch operations).
Torch: what a user would write on the same device without this kernel -- a finite mask, `x >= thr` masks summed over the
members, one `scatter_add_` per threshold into the bins of each row -- evaluated VARIABLE BY VARIABLE (13 planes at a time),
and for M > 16 plane by plane; one evaluation per repeat.
Check: kernel, plain form and torch expression equal on every entry (integers), and the kernel repeatable bit for bit.
"""
import argparse
import ctypes
import json
from pathlib import Path

import torch
from verification_bench import ATMOS, N_LAT, N_LON, N_PLANES, SURF, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, probability_scores  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib
from aurora_amd.scores import latitude_weights

THRESHOLDS = (101325.0, 101709.0, 102024.0)


def batch(g: torch.Generator, base: Batch | None = None) -> Batch:
    """Seeded synthetic fields: the truth, or with `base` a member = base + 60 randn."""
    r = lambda *lead: torch.randn(*lead, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    return state(lambda *lead: r(*lead).mul_(300).add_(101325)) if base is None else state(lambda *lead: r(*lead).mul_(60), base)


def torch_rows(x: torch.Tensor, y: torch.Tensor, thr: torch.Tensor) -> torch.Tensor:
    """x (M, P, n_lat, n_lon), y (P, n_lat, n_lon) fp32, thr (P, T) -> (P, n_lat, T, 2, M + 1) int32 as a plain torch expression."""
    M, (P, n_lat, _) = x.shape[0], y.shape
    ok = torch.isfinite(y) & torch.isfinite(x).all(dim=0)
    out = torch.zeros(P, n_lat, thr.shape[1], 2 * (M + 1) + 1, dtype=torch.int32, device=x.device)
    one = torch.ones((), dtype=torch.int32, device=x.device).expand_as(y)
    for t in range(thr.shape[1]):
        th = thr[:, t, None, None]
        k, o = (x >= th).sum(dim=0), y >= th
        out[:, :, t].scatter_add_(-1, torch.where(ok, o * (M + 1) + k, 2 * (M + 1)), one)     # (the last bin: invalid points)
    return out[..., :-1].reshape(P, n_lat, thr.shape[1], 2, M + 1)


def case(M: int, calls: int, repeats: int, plain_lib) -> dict:
    g = torch.Generator(device="cuda").manual_seed(M)
    truth = batch(g)
    members = [batch(g, truth) for _ in range(M)]
    thresholds = {k: THRESHOLDS for k in (*SURF, *ATMOS)}
    thr = torch.tensor(THRESHOLDS, dtype=torch.float32, device="cuda").expand(N_PLANES, len(THRESHOLDS)).contiguous()
    w = torch.from_numpy(latitude_weights(truth.metadata.lat.numpy())).cuda()
    X, Y = [planes(b) for b in members], planes(truth)
    kernel = lambda: lib.probability_rows(X, Y, thr)  # noqa: E731
    ensemble = lambda: lib.ensemble_scores_sums(X, Y, w)  # noqa: E731
    whole = lambda: probability_scores(members, truth, thresholds)  # noqa: E731
    group = 13 if M <= 16 else 1                       # planes per torch evaluation (see the module's text)

    def plain_torch():
        out, first = [], 0
        for i, t in enumerate(Y):
            x, t = torch.stack([X[m][i][0] for m in range(M)]).reshape(M, -1, N_LAT, N_LON), t[0].reshape(-1, N_LAT, N_LON)
            for k in range(0, t.shape[0], group):
                n = min(group, t.shape[0] - k)
                out.append(torch_rows(x[:, k:k + n], t[k:k + n], thr[first + k:first + k + n]))
            first += t.shape[0]
        return torch.cat(out)

    got, again, want = kernel(), kernel(), plain_torch()
    whole(), ensemble()
    torch.cuda.synchronize()
    assert torch.equal(got, again), "the kernel's results are not repeatable"
    assert got.shape == (N_PLANES, N_LAT, len(THRESHOLDS), 2, M + 1) and torch.equal(got, want), "kernel and torch expression differ"
    counts = got.sum(dim=(0, 1), dtype=torch.int64)
    off_corner = (1 - (counts[:, 0, 0] + counts[:, 1, M]).double() / counts.sum(dim=(1, 2)).double()).tolist()
    arms = {"kernel": kernel, "ensemble": ensemble}
    if plain_lib is not None:
        pointers = lib._planes("probability_scores_bench", [(f"member {m}", fs) for m, fs in enumerate(X)] + [("truth", Y)], thr.device,
                               "thr", N_LAT, N_LON)
        table = pointers.upload()
        rows_plain = torch.empty_like(got)

        def plain():
            code = plain_lib.aurora_hip_probability_scores(table["member 0"], table["truth"], M, N_PLANES, N_LAT,
                                                           N_LON, thr.data_ptr(), len(THRESHOLDS), 0, rows_plain.data_ptr(),
                                                           torch.cuda.current_stream().cuda_stream)
            assert code == 0, plain_lib.aurora_hip_last_error()

        plain()
        torch.cuda.synchronize()
        assert torch.equal(rows_plain, got), "the plain-atomics form and the ballot form differ"
        arms["plain_atomics"] = plain
    for f in (*arms.values(), whole):
        window_ms(f, 3)
    ms = alternate({**{k: captured(f, calls) for k, f in arms.items()}, "torch": lambda: window_ms(plain_torch, 1),
                    "scores": lambda: window_ms(whole, calls)}, repeats)
    read = (M + 1) * N_PLANES * N_LAT * N_LON * 4
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    rec = {"members": M, "thresholds": len(THRESHOLDS), "planes": N_PLANES, "grid": [N_LAT, N_LON], "read_GB": read / 1e9,
           "calls_per_window": calls, "repeats": repeats, "off_corner_share_per_threshold": off_corner,
           "kernel_ms": med["kernel"], "kernel_ms_min_max": span["kernel"],
           "kernel_TBps": read / med["kernel"] / 1e9, "ensemble_scores_ms": med["ensemble"],
           "ensemble_scores_ms_min_max": span["ensemble"],
           "ensemble_scores_TBps": read / med["ensemble"] / 1e9, "kernel_over_ensemble_scores": med["kernel"] / med["ensemble"],
           "probability_scores_call_ms": med["scores"], "torch_ms": med["torch"], "torch_ms_min_max": span["torch"],
           "torch_planes_per_evaluation": group, "torch_over_kernel": med["torch"] / med["kernel"]}
    if plain_lib is not None:
        rec.update({"plain_atomics_ms": med["plain_atomics"], "plain_atomics_ms_min_max": span["plain_atomics"],
                    "plain_atomics_over_ballot": med["plain_atomics"] / med["kernel"]})
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[8, 16, 51])
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--plain-lib", type=Path, default=None, help="a build with -DAURORA_PROBABILITY_PLAIN_ATOMICS (see above)")
    args = ap.parse_args()
    plain_lib = None
    if args.plain_lib is not None:
        plain_lib = ctypes.CDLL(str(args.plain_lib))
        fn = plain_lib.aurora_hip_probability_scores
        fn.restype, fn.argtypes = lib._SIGNATURES["aurora_hip_probability_scores"]
        plain_lib.aurora_hip_last_error.restype = ctypes.c_char_p
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} per member "
          f"({N_PLANES * N_LAT * N_LON * 4 / 1e6:.0f} MB), T = {len(THRESHOLDS)}", flush=True)
    for M in args.members:
        rec = case(M, args.calls, args.repeats, plain_lib)
        share = ", ".join(f"{100 * v:.1f} %" for v in rec["off_corner_share_per_threshold"])
        line = (f"M = {M:2d}: {rec['read_GB']:.2f} GB read, off the corner bins {share}: kernel call {rec['kernel_ms']:.3f} ms "
                f"(device time, median of {rec['repeats']} graph replays of {rec['calls_per_window']} calls; "
                f"{rec['kernel_ms_min_max'][0]:.3f}-{rec['kernel_ms_min_max'][1]:.3f}) = {rec['kernel_TBps']:.2f} TB/s; "
                f"aurora_hip_ensemble_scores on the same members {rec['ensemble_scores_ms']:.3f} ms = "
                f"{rec['ensemble_scores_TBps']:.2f} TB/s: {rec['kernel_over_ensemble_scores']:.2f} x ensemble_scores; ")
        if plain_lib is not None:
            line += (f"every lane an LDS atomic {rec['plain_atomics_ms']:.3f} ms ({rec['plain_atomics_ms_min_max'][0]:.3f}-"
                     f"{rec['plain_atomics_ms_min_max'][1]:.3f}) = {rec['plain_atomics_over_ballot']:.2f} x the ballot form; ")
        line += (f"probability_scores() end to end, eager, {rec['probability_scores_call_ms']:.3f} ms; torch expression "
                 f"({rec['torch_planes_per_evaluation']} planes at a time) {rec['torch_ms']:.1f} ms = "
                 f"{rec['torch_over_kernel']:.0f} x the kernel call; kernel, plain form and torch expression equal on every entry")
        print(line, flush=True)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
