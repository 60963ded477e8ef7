"""`aurora_amd.sphere_spectra` on the device for one 0.25-degree state (721 x 1440; 4 surface + 5 x 13 atmospheric variables =
69 planes) at lmax 360, without and with a truth, beside two yardsticks measured in the same session and the same rule as a
plain torch expression.

    python tools/sphere_spectra_bench.py [--calls 10] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arm: the ONE aurora_hip_sphere_spectra call over all 69 planes
(`lib.sphere_spectra_power`: three launches), --calls of them per graph.  Eager arm: `sphere_spectra()` end to end.  Stages: the
device time of each of the three kernels of one eager call, from torch.profiler's kernel records ("not measured" where the
profiler reports none).  Bytes yardstick: one read of the planes and of the table, one write and one read of the workspace, at
the rate `aurora_hip_scores` reaches here (its two inputs over its graph-replayed call).  Arithmetic yardstick: the folded DFT
for m <= lmax (2 x rows x K x 2 (lmax + 1) per input, K = 721) and the Legendre products (2 x 2 x H x table rows per plane and
input) at the fp64 rate `aurora_hip_spectra` reaches here.  Torch: `torch.fft.rfft` and one fp64 matrix product per m against
the same table, in eager windows: a yardstick only.  Check: kernel against the torch expression relative to each plane's
largest value, and the kernel repeatable bit for bit.
"""
import argparse
import importlib
import json

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, STEP_MS, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import Batch, _fields, sphere_spectra  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib
from aurora_amd.spectra import band_weights

ss = importlib.import_module("aurora_amd.sphere_spectra")
LMAX = 360
K = N_LON // 2 + 1


def batch(seed: int, base: Batch | None = None, spread: float = 1.0) -> Batch:
    """Seeded synthetic fields about 5e4; with `base`, base + spread x noise."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: spread * torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g)  # noqa: E731
    return state(r, base) if base is not None else state(lambda *s: r(*s) + 5e4)


def torch_power(P: list, T: list | None, rows: list) -> torch.Tensor:
    """(planes, 1 or 3, lmax + 1): the rule as torch.fft.rfft and one matrix product per m (`rows`: the table's rows of each m)."""
    fields = [torch.cat([p.reshape(-1, N_LAT, N_LON) for p in x]) for x in ((P,) if T is None else (P, T))]
    F = [torch.fft.rfft(f.double(), dim=-1)[..., :LMAX + 1] / N_LON for f in fields]
    power = torch.zeros(fields[0].shape[0], 1 if T is None else 3, LMAX + 1, dtype=torch.float64, device="cuda")
    for m, Am in enumerate(rows):
        a = [torch.complex(f[:, :, m].real @ Am.T, f[:, :, m].imag @ Am.T) for f in F]
        if T is not None:
            a.append(a[0] - a[1])
        for i, alm in enumerate(a):
            power[:, i, m:] += (1.0 if m == 0 else 2.0) * (alm.real ** 2 + alm.imag ** 2)
    return power


def stage_ms(fn) -> dict:
    """Device time of the kernels of one call of `fn` by name, from torch.profiler; {} where it reports none."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        for stage in ("zonal", "legendre", "finish"):
            if f"sphere_{stage}_kernel" in e.name:
                out[stage] = out.get(stage, 0.0) + float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) / 1e3
    return out


def case(pred: Batch, truth: Batch | None, table: torch.Tensor, rows: list, rates: dict, calls: int, repeats: int) -> dict:
    P, T = planes(pred), None if truth is None else planes(truth)
    poles = ss.pole_rows(pred.metadata.lat.numpy())
    kernel = lambda: lib.sphere_spectra_power(P, T, table, LMAX, poles)  # noqa: E731
    whole = lambda: sphere_spectra(pred, truth, lmax=LMAX)  # noqa: E731
    plain = lambda: torch_power(P, T, rows)  # noqa: E731
    got, again, want = kernel(), kernel(), plain()
    whole()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "the kernel's spectra are not repeatable"
    assert bool(got[1].all()) and int(got[2].sum()) == 0
    g, y = got[0].cpu().numpy(), want.cpu().numpy()
    worst = float(np.max(np.abs(g - y)[:, :2] / np.abs(y).max(axis=-1, keepdims=True)[:, :2]))
    assert worst <= 1e-11, worst
    for f in (kernel, whole, plain):
        window_ms(f, 3)
    stages = stage_ms(kernel)
    ms = alternate({"kernel": captured(kernel, calls), "torch": lambda: window_ms(plain, 3),
                    "sphere_spectra": lambda: window_ms(whole, calls)}, repeats)
    med, span = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    n_in = 1 if truth is None else 2
    workspace = lib.sphere_spectra_workspace_bytes(N_PLANES, N_LAT, N_LON, LMAX, truth is not None)
    nbytes = n_in * N_PLANES * N_LAT * N_LON * 4 + table.numel() * 8 + 2 * workspace
    flop_zonal = 2.0 * n_in * N_PLANES * N_LAT * K * (2 * (LMAX + 1))
    flop_legendre = 2.0 * 2 * n_in * N_PLANES * N_LAT * table.shape[0]
    return {"truth": truth is not None, "planes": N_PLANES, "grid": [N_LAT, N_LON], "lmax": LMAX, "calls_per_window": calls,
            "repeats": repeats, "kernel_ms": med["kernel"], "kernel_ms_min_max": span["kernel"],
            "sphere_spectra_call_ms": med["sphere_spectra"], "share_of_step_percent": 100 * med["sphere_spectra"] / STEP_MS,
            "stage_ms": stages or "not measured", "workspace_MB": workspace / 1e6, "table_MB": table.numel() * 8 / 1e6,
            "bytes_yardstick_ms": nbytes / rates["bytes_per_ms"], "moved_GB": nbytes / 1e9,
            "zonal_GFLOP": flop_zonal / 1e9, "legendre_GFLOP": flop_legendre / 1e9,
            "arithmetic_yardstick_ms": (flop_zonal + flop_legendre) / rates["flop_per_ms"],
            "torch_ms": med["torch"], "torch_ms_min_max": span["torch"], "torch_over_kernel": med["torch"] / med["kernel"],
            "worst_difference_over_plane_max": worst}


def session_rates(pred: Batch, truth: Batch, calls: int, repeats: int) -> dict:
    """What aurora_hip_scores moves per ms and aurora_hip_spectra multiplies per ms on this device now."""
    P, T = planes(pred), planes(truth)
    lat = pred.metadata.lat.numpy()
    row_w = _fields.device_weights("bench", lat, torch.device("cuda", torch.cuda.current_device()))
    bw = torch.from_numpy(band_weights(lat, ((-90.0, 90.0),))).cuda()
    scores = lambda: lib.scores_sums(P, T, None, row_w)  # noqa: E731
    zonal = lambda: lib.spectra_power(P, T, bw)  # noqa: E731
    for f in (scores, zonal):
        window_ms(f, 3)
    ms = alternate({"scores": captured(scores, calls), "spectra": captured(zonal, calls)}, repeats)
    scores_ms, spectra_ms = med_min_max(ms["scores"])[0], med_min_max(ms["spectra"])[0]
    return {"scores_ms": scores_ms, "spectra_ms": spectra_ms, "bytes_per_ms": 2.0 * N_PLANES * N_LAT * N_LON * 4 / scores_ms,
            "flop_per_ms": 2.0 * 2 * N_PLANES * N_LAT * K * (2 * K) / spectra_ms}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON} per input, lmax {LMAX}", flush=True)
    truth = batch(0)
    pred = batch(1, truth, spread=0.02)
    rates = session_rates(pred, truth, args.calls, args.repeats)
    print(f"this session: aurora_hip_scores {rates['scores_ms']:.3f} ms = {rates['bytes_per_ms'] / 1e9:.2f} TB/s; aurora_hip_spectra "
          f"(with a truth) {rates['spectra_ms']:.3f} ms = {rates['flop_per_ms'] / 1e9:.1f} TFLOP/s fp64", flush=True)
    lat = pred.metadata.lat.numpy()
    table = _fields.tables.get(("sphere analysis", lat.tobytes(), LMAX), torch.device("cuda", torch.cuda.current_device()),
                               lambda: np.array(ss.analysis_table(lat, LMAX)), "bench")
    rows = [table[ss.row_of(LMAX, m, m):ss.row_of(LMAX, m, m) + LMAX + 1 - m] for m in range(LMAX + 1)]
    for t in (None, truth):
        rec = case(pred, t, table, rows, rates, args.calls, args.repeats)
        print(f"truth {'yes' if rec['truth'] else 'no '}: kernel call {rec['kernel_ms']:.3f} ms (device time, median of {rec['repeats']} "
              f"graph replays of {rec['calls_per_window']} calls; {rec['kernel_ms_min_max'][0]:.3f}-{rec['kernel_ms_min_max'][1]:.3f}); "
              f"stages {rec['stage_ms']}; sphere_spectra() end to end {rec['sphere_spectra_call_ms']:.3f} ms = "
              f"{rec['share_of_step_percent']:.2f} % of a {STEP_MS:.0f} ms step; bytes yardstick {rec['bytes_yardstick_ms']:.3f} ms "
              f"({rec['moved_GB']:.2f} GB); arithmetic yardstick {rec['arithmetic_yardstick_ms']:.3f} ms ({rec['zonal_GFLOP']:.0f} + "
              f"{rec['legendre_GFLOP']:.0f} GFLOP); torch expression {rec['torch_ms']:.1f} ms = {rec['torch_over_kernel']:.2f} x the kernel "
              f"call; largest difference {rec['worst_difference_over_plane_max']:.1e} of a plane's largest value", flush=True)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
