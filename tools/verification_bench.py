"""What the eight verification benches (scores, ensemble_scores, spectra, event_scores, probability_scores, field_stats,
diagnostics, conditional_scores) share: the 0.25-degree state and the way a call is timed.  Imported by them; not a tool.

State: 721 x 1440; 4 surface + 5 x 13 atmospheric variables = 69 planes, 286 MB per input; one history entry.
Timing: a window is `calls` back-to-back calls between a HIP event pair.  A kernel arm is `calls` calls captured in a
hipGraph and replayed as ONE window (device time per call = window / calls, free of the host's enqueue time); an eager arm is
the same window issued from Python, where the host's enqueue rate counts too.  Every bench warms each eager arm with a window
of 3 calls and each graph with 2 replays, then runs its arms in a fixed order inside every repeat, so that a drift of the
device's clocks falls on all of them alike."""
import statistics
import sys
from datetime import datetime
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from aurora_amd import Batch, Metadata  # noqa: E402

SURF, ATMOS, LEVELS = ("2t", "10u", "10v", "msl"), ("z", "u", "v", "t", "q"), 13
N_LAT, N_LON = 721, 1440
N_PLANES = len(SURF) + len(ATMOS) * LEVELS
STEP_MS = 124.0                                   # the 0.25-degree forecast step


def metadata(B: int = 1, atmos_levels=tuple(range(50, 50 + 75 * LEVELS, 75))) -> Metadata:
    return Metadata(lat=torch.linspace(90, -90, N_LAT, dtype=torch.float64),
                    lon=torch.linspace(0, 360, N_LON + 1, dtype=torch.float64)[:-1],
                    time=tuple(datetime(2022, 5, 11, 12) for _ in range(B)), atmos_levels=atmos_levels)


def state(fill, base: Batch | None = None, B: int = 1) -> Batch:
    """The 69-plane state.  `fill(*lead)` makes one field of shape (*lead, N_LAT, N_LON), called once per variable in the
    order surface, atmospheric; with `base`, every field is base's plus what `fill` made."""
    def field(group, k, *lead):
        return fill(*lead) if base is None else fill(*lead) + getattr(base, group)[k]

    return Batch({k: field("surf_vars", k, B, 1) for k in SURF}, {}, {k: field("atmos_vars", k, B, 1, LEVELS) for k in ATMOS},
                 metadata(B) if base is None else base.metadata)


def planes(b: Batch) -> list[torch.Tensor]:
    return [v[:, -1] for v in (*b.surf_vars.values(), *b.atmos_vars.values())]


def window_ms(fn, calls: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def captured(fn, calls: int):
    """`calls` back-to-back calls of `fn` in one hipGraph, replayed twice to warm up: the arm that times one replay."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            fn()
    window_ms(graph.replay, 2)
    return lambda: window_ms(graph.replay, 1) / calls


def alternate(arms: dict, repeats: int) -> dict:
    """{name: [ms per call, ...]}: every arm (a callable that returns ms per call) once per repeat, in the order given."""
    ms = {k: [] for k in arms}
    for _ in range(repeats):
        for k, arm in arms.items():
            ms[k].append(arm())
    return ms


def med_min_max(ms: list) -> tuple:
    return statistics.median(ms), [min(ms), max(ms)]
