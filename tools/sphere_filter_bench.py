"""`aurora_amd.sphere_analysis`, `sphere_synthesis` and `sphere_filter` on the device for one 0.25-degree state (721 x 1440; 4
surface + 5 x 13 atmospheric variables = 69 planes) at lmax 360, beside yardsticks measured in the same session.

    python tools/sphere_filter_bench.py [--calls 5] [--repeats 5]

State and timing: tools/verification_bench.py.  Kernel arms: the ONE aurora_hip_sphere_analysis call and the ONE
aurora_hip_sphere_synthesis call over all 69 planes (`lib.sphere_analysis`, `lib.sphere_synthesis`: two launches each), --calls
of them per graph.  Filter arms: `sphere_filter(batch, lmax=360)` end to end, issued eagerly from Python and replayed from a
graph.  Yardsticks: `aurora_hip_sphere_spectra` without a truth on the same planes (graph); the same rule as a torch expression
on the device -- `torch.fft.rfft` / `irfft` and one fp64 matrix product per m each way -- in eager windows; the bytes each call
must move (planes, table, coefficients, one write and one read of the workspace) at the rate `aurora_hip_scores` reaches here.
Check: the kernels against the torch expression relative to each plane's largest value, and repeatable bit for bit.  No time is
a pass criterion."""
import argparse
import importlib
import json

import numpy as np
import torch
from verification_bench import N_LAT, N_LON, N_PLANES, STEP_MS, alternate, captured, med_min_max, planes, state, window_ms

from aurora_amd import _fields, sphere_filter  # (verification_bench has put the repository on sys.path)
from aurora_amd.engine import lib

ss = importlib.import_module("aurora_amd.sphere_spectra")
st = importlib.import_module("aurora_amd.sphere_transform")
LMAX = 360


def torch_analysis(P: list, rows: list) -> torch.Tensor:
    x = torch.cat([p.reshape(-1, N_LAT, N_LON) for p in P])
    F = torch.fft.rfft(x.double(), dim=-1)[..., :LMAX + 1] / N_LON
    a = torch.zeros(x.shape[0], LMAX + 1, LMAX + 1, dtype=torch.complex128, device="cuda")
    for m, Am in enumerate(rows):
        a[:, m, m:] = torch.complex(F[:, :, m].real @ Am.T, F[:, :, m].imag @ Am.T)
    return a


def torch_synthesis(a: torch.Tensor, rows: list) -> torch.Tensor:
    G = torch.zeros(a.shape[0], N_LAT, N_LON // 2 + 1, dtype=torch.complex128, device="cuda")
    for m, Pm in enumerate(rows):
        G[:, :, m] = torch.complex(a[:, m, m:].real @ Pm, a[:, m, m:].imag @ Pm)
    return torch.fft.irfft(G * N_LON, n=N_LON, dim=-1).float()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name()}; {N_PLANES} planes of {N_LAT} x {N_LON}, lmax {LMAX}", flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    batch = state(lambda *s: torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g) + 5e4)
    P = planes(batch)
    dev = torch.device("cuda", torch.cuda.current_device())
    lat = batch.metadata.lat.numpy()
    A = _fields.tables.get(("sphere analysis", lat.tobytes(), LMAX), dev, lambda: np.array(ss.analysis_table(lat, LMAX)), "bench")
    S = _fields.tables.get(("sphere synthesis", lat.tobytes(), LMAX), dev, lambda: np.array(st.synthesis_table(lat, LMAX)), "bench")
    span = lambda t: [t[ss.row_of(LMAX, m, m):ss.row_of(LMAX, m, m) + LMAX + 1 - m] for m in range(LMAX + 1)]  # noqa: E731
    rows_a, rows_s = span(A), span(S)
    poles = ss.pole_rows(lat)

    analysis = lambda: lib.sphere_analysis(P, A, LMAX, poles)  # noqa: E731
    coeff, valid, _ = analysis()
    synthesis = lambda: lib.sphere_synthesis(coeff, S, N_LON, valid)  # noqa: E731
    whole = lambda: sphere_filter(batch, lmax=LMAX)  # noqa: E731
    spectra = lambda: lib.sphere_spectra_power(P, None, A, LMAX, poles)  # noqa: E731
    row_w = _fields.device_weights("bench", lat, dev)
    other = planes(state(lambda *s: torch.randn(*s, N_LAT, N_LON, device="cuda", generator=g) + 5e4))
    scores = lambda: lib.scores_sums(P, other, None, row_w)  # noqa: E731
    plain = lambda: torch_synthesis(torch_analysis(P, rows_a), rows_s)  # noqa: E731

    y, again, want_a = synthesis(), synthesis(), torch_analysis(P, rows_a)
    want_y = torch_synthesis(want_a, rows_s)
    whole()
    torch.cuda.synchronize()
    assert torch.equal(y, again) and torch.equal(torch.view_as_real(coeff), torch.view_as_real(analysis()[0])), "not repeatable"
    worst_a = float((coeff - want_a).abs().max() / want_a.abs().max())
    worst_y = float(((y - want_y).abs().amax(dim=(1, 2)) / want_y.abs().amax(dim=(1, 2))).max())
    assert bool(valid.all()) and worst_a <= 1e-11 and worst_y <= 2.0 ** -22, (worst_a, worst_y)
    del want_a, want_y, again
    for f in (analysis, synthesis, whole, spectra, scores):
        window_ms(f, 3)
    window_ms(plain, 1)
    ms = alternate({"analysis": captured(analysis, args.calls), "synthesis": captured(synthesis, args.calls),
                    "filter_graph": captured(whole, args.calls), "filter_eager": lambda: window_ms(whole, args.calls),
                    "sphere_spectra": captured(spectra, args.calls), "scores": captured(scores, args.calls),
                    "torch": lambda: window_ms(plain, 1)}, args.repeats)
    med, rng = ({k: med_min_max(v)[i] for k, v in ms.items()} for i in (0, 1))
    plane_bytes, table_bytes, coeff_bytes = N_PLANES * N_LAT * N_LON * 4, A.numel() * 8, coeff.numel() * 16
    ws_a = lib.sphere_analysis_workspace_bytes(N_PLANES, N_LAT, N_LON, LMAX)
    ws_s = lib.sphere_synthesis_workspace_bytes(N_PLANES, N_LAT, N_LON, LMAX)
    rate = 2.0 * plane_bytes / med["scores"]                              # bytes per ms of aurora_hip_scores here
    moved = {"analysis": plane_bytes + table_bytes + coeff_bytes + 2 * ws_a, "synthesis": plane_bytes + table_bytes + coeff_bytes + 2 * ws_s}
    moved["filter"] = moved["analysis"] + moved["synthesis"] + 3 * coeff_bytes   # (the response: one read, one write, and the read of the copy)
    rec = {"planes": N_PLANES, "grid": [N_LAT, N_LON], "lmax": LMAX, "calls_per_window": args.calls, "repeats": args.repeats,
           "ms": med, "ms_min_max": rng, "scores_TB_per_s": rate / 1e9, "moved_GB": {k: v / 1e9 for k, v in moved.items()},
           "bytes_yardstick_ms": {k: v / rate for k, v in moved.items()}, "filter_share_of_step_percent": 100 * med["filter_eager"] / STEP_MS,
           "table_MB": table_bytes / 1e6, "coefficients_MB": coeff_bytes / 1e6, "workspace_MB": [ws_a / 1e6, ws_s / 1e6],
           "worst_coefficient_difference_over_largest": worst_a, "worst_field_difference_over_plane_max": worst_y}
    print(f"analysis {med['analysis']:.3f} ms, synthesis {med['synthesis']:.3f} ms (device time per call, median of {args.repeats} graph "
          f"replays of {args.calls} calls); sphere_filter() end to end: eager {med['filter_eager']:.3f} ms = "
          f"{rec['filter_share_of_step_percent']:.1f} % of a {STEP_MS:.0f} ms step, graph {med['filter_graph']:.3f} ms; yardsticks: "
          f"aurora_hip_sphere_spectra without a truth {med['sphere_spectra']:.3f} ms; torch expression (analysis + synthesis) "
          f"{med['torch']:.1f} ms; bytes at the {rate / 1e9:.2f} TB/s of aurora_hip_scores: analysis "
          f"{rec['bytes_yardstick_ms']['analysis']:.3f} ms, synthesis {rec['bytes_yardstick_ms']['synthesis']:.3f} ms, filter "
          f"{rec['bytes_yardstick_ms']['filter']:.3f} ms; largest difference from the torch expression: coefficients {worst_a:.1e} of the "
          f"largest, fields {worst_y:.1e} of a plane's largest value", flush=True)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
