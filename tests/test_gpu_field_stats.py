"""`aurora_amd.FieldStats` on the device: aurora_hip_field_stats_update against the numpy fp64 yardstick written in
tests/test_field_stats_host.py (`yardstick`: two passes over the stacked samples; not `aurora_amd.fieldstats._update_host`,
which is code under test and is checked against the same yardstick there).

Bound (derived, not tuned; u = 2^-53).  With a point's valid samples v_1 .. v_n, origin o = fp32(v_1) and d_i = v_i - o, the
kernel and the yardstick form the SAME d_i bit for bit: v is one correctly rounded fp64 difference of fp32 values (or the
value itself), o is exact in fp64, d is one rounding of v - o.  A sum of n fp64 terms in any order is within n u sum|term| of
the exact sum, and both sides carry that:
    |s1 - s1'| <= 2 n u sum|d|
    |s2 - s2'| <= 2 (n + 1) u sum d^2      (the extra u: the yardstick rounds each d^2, the kernel's fused multiply-add does not)
n, argmin, argmax, exceed, run and longest are integers and must be equal.  origin, vmin, vmax are fp32(v): one rounding of a
correctly rounded fp64 expression on both sides, as is the derived wind speed fp32(sqrt(a^2 + b^2)) (both squares are exact in
fp64, their sum is rounded once, the fp64 square root is correctly rounded on both sides): equal bit for bit.  The data are
pressure-like (1e5 +- 300), so sums of raw values (sum v^2 ~ 1e10 n, u-relative error 1e-6 n against sum d^2 ~ 1e5 n) would
miss the s2 bound by orders of magnitude.  Every plane and every point of every case is compared."""
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, FieldStats, Metadata, rollout
from aurora_amd.engine import lib
from tests import helpers
from tests.golden_cases import CASES
from tests.test_field_stats_host import U, assert_state_matches, make_batch, variable_state, yardstick
from tests.verification_inputs import DEV, carve

pytestmark = pytest.mark.gpu
INT = ("n", "argmin", "argmax", "exceed", "run", "longest")


def samples(S, n_planes, n_lat, n_lon, seed, offset=0, scale=300.0):
    """S pressure-like samples (S, n_planes, n_lat, n_lon), each sample its own carved buffer."""
    g = torch.Generator().manual_seed(seed)
    base = 101325 + scale * torch.randn(n_planes, n_lat, n_lon, generator=g, dtype=torch.float64)
    return [carve(base + scale * torch.randn(n_planes, n_lat, n_lon, generator=g, dtype=torch.float64), offset) for _ in range(S)]


def new_state(n_planes, n_points, T):
    return {k: torch.zeros((n_planes, T, n_points) if per_thr else (n_planes, n_points), dtype=dt, device=DEV)
            for k, (dt, per_thr) in lib.FIELD_STATS_STATE.items() if T or not per_thr}


def run(xs, ref=None, second=None, thr=None, below=False, groups=None, state=None, index=None):
    """xs: S tensors (n_planes, n_lat, n_lon); second: S lists of per-plane tensors or None; calls of `groups` samples each."""
    n_planes, n_lat, n_lon = xs[0].shape
    T = 0 if thr is None else thr.shape[1]
    state = new_state(n_planes, n_lat * n_lon, T) if state is None else state
    index = torch.zeros(1, dtype=torch.int64, device=DEV) if index is None else index
    at = 0
    for g in groups or [len(xs)]:
        sec = None
        if second is not None:                                   # plane by plane: a field is one plane here
            sec = [list(second[s]) for s in range(at, at + g)]
        if second is not None:
            smp = [[xs[s][k] for k in range(n_planes)] for s in range(at, at + g)]
            rf = None if ref is None else [ref[k] for k in range(n_planes)]
        else:
            smp, rf = [[xs[s]] for s in range(at, at + g)], None if ref is None else [ref]
        lib.field_stats_update(smp, rf, sec, thr, below, index, state)
        at += g
    assert at == len(xs)
    return state, index


def host(state):
    return {k: v.cpu().numpy() for k, v in state.items()}


def assert_equal_states(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def check_against_yardstick(state, xs, ref, second, thr, below, what):
    """Every plane, every point."""
    n_planes, n_lat, n_lon = xs[0].shape
    got = host(state)
    x = np.stack([v.cpu().numpy() for v in xs]).reshape(len(xs), n_planes, -1)
    for k in range(n_planes):
        b = None
        if second is not None and second[0][k] is not None:
            b = np.stack([second[s][k].cpu().numpy().reshape(-1) for s in range(len(xs))])
        r = None if ref is None else ref[k].cpu().numpy().reshape(-1)
        y = yardstick(x[:, k], b, r, None if thr is None else list(thr[k].cpu().numpy()), below)
        assert_state_matches({name: v[k] for name, v in got.items()}, y, f"{what} plane {k}")
        if b is not None and ref is None:                        # the derived wind speed itself (origin: the first sample's)
            ws = np.sqrt(x[0, k].astype(np.float64) ** 2 + b[0].astype(np.float64) ** 2).astype(np.float32)
            assert np.isfinite(ws).all() and np.array_equal(got["origin"][k].view(np.int32), ws.view(np.int32)), (what, k, "wind speed")


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("n_planes", [1, 3])
@pytest.mark.parametrize("n_lat,n_lon", [(1, 1), (3, 5), (17, 32), (33, 130), (64, 1030)])
def test_raw_state_equals_the_yardstick(n_lat, n_lon, n_planes, offset):
    """Plain samples with two thresholds; then plane 0 as a wind speed from two components against a reference, `below`."""
    S = 9
    xs = samples(S, n_planes, n_lat, n_lon, seed=n_lat + n_lon + n_planes, offset=offset)
    if offset:
        assert xs[0].data_ptr() % 16 != 0
    thr = torch.tensor([[101325.0, 101625.0 + 10 * k] for k in range(n_planes)], dtype=torch.float32, device=DEV)
    state, index = run(xs, thr=thr)
    assert int(index) == S
    check_against_yardstick(state, xs, None, None, thr, False, f"plain {n_lat}x{n_lon} x{n_planes} +{offset}")

    bs = samples(S, 1, n_lat, n_lon, seed=7 + n_lat, offset=offset, scale=250.0)
    ref = carve(101325 + 300 * torch.randn(n_planes, n_lat, n_lon, generator=torch.Generator().manual_seed(3), dtype=torch.float64), offset)
    second = [[bs[s][0]] + [None] * (n_planes - 1) for s in range(S)]
    thr1 = torch.tensor([[100.0 * (k + 1)] for k in range(n_planes)], dtype=torch.float32, device=DEV)
    state, _ = run(xs, ref=ref, second=second, thr=thr1, below=True)
    got = host(state)
    x = np.stack([v.cpu().numpy() for v in xs]).reshape(S, n_planes, -1)
    for k in range(n_planes):
        b = np.stack([bs[s][0].cpu().numpy().reshape(-1) for s in range(S)]) if k == 0 else None
        y = yardstick(x[:, k], b, ref[k].cpu().numpy().reshape(-1), list(thr1[k].cpu().numpy()), True)
        assert_state_matches({name: v[k] for name, v in got.items()}, y, f"derived - reference {n_lat}x{n_lon} plane {k}")
    # the wind speed itself (no reference: origin is fp32(sqrt(a^2 + b^2)) of the first sample), bit for bit
    state, _ = run(xs[:2], second=second[:2])
    check_against_yardstick(state, xs[:2], None, second[:2], None, False, "wind speed")


def test_nan_land_mask_and_stray_nans():
    """A land mask that is NaN in every sample: n = 0, NaN results, arg -1.  Stray NaNs (and an infinity) in single samples
    are skipped, exactly, and do not break a run of exceedances."""
    n_lat, n_lon, S = 19, 36, 9
    b = [make_batch(n_lat, n_lon, seed=300 + s, B=1, wind=False) for s in range(S)]
    land = torch.rand(n_lat, n_lon, generator=torch.Generator().manual_seed(1)) < 0.3
    sea = (~land).nonzero().tolist()
    for s in range(S):
        b[s].surf_vars["msl"][:, -1] = 101325.0 + s                      # rising: every sample at or above 101325 ...
        b[s].surf_vars["msl"][0, -1][land] = float("nan")
    (i0, j0), (i1, j1), (i2, j2) = sea[0], sea[1], sea[2]
    b[3].surf_vars["msl"][0, -1, i0, j0] = float("nan")                  # ... so a skipped sample inside the run
    b[5].surf_vars["msl"][0, -1, i0, j0] = float("inf")
    b[0].surf_vars["msl"][0, -1, i1, j1] = float("nan")                  # the first sample missing
    b[8].surf_vars["msl"][0, -1, i2, j2] = float("-inf")                 # the last one
    acc = FieldStats(thresholds={"msl": [101325.0]})
    for x in b:
        acc.update(x.to(DEV))
    n, run_, lg = acc.count["msl"][0].cpu(), acc.state["run"][1, 0].view(n_lat, n_lon).cpu(), acc.longest_run["msl"][0, 0].cpu()
    assert (n[land] == 0).all() and (n[~land] >= 7).all()
    assert n[i0, j0] == 7 and n[i1, j1] == 8 and n[i2, j2] == 8 and int((n == 9).sum()) == len(sea) - 3
    assert lg[i0, j0] == 7 and run_[i0, j0] == 7 and lg[i1, j1] == 8 and lg[i2, j2] == 8      # skipped, not broken
    assert (acc.exceed_count["msl"][0, 0].cpu() == n).all()
    for name, q in (("mean", acc.mean), ("rms", acc.rms), ("min", acc.min), ("max", acc.max), ("std", acc.std(ddof=1))):
        v = q["msl"][0].cpu()
        assert torch.isnan(v[land]).all() and not torch.isnan(v[~land]).any(), name
    assert (acc.argmin["msl"][0].cpu()[land] == -1).all() and (acc.argmax["msl"][0].cpu()[land] == -1).all()
    assert acc.argmin["msl"][0, i1, j1] == 1 and acc.argmax["msl"][0, i2, j2] == 7 and acc.argmax["msl"][0, i0, j0] == 8
    assert torch.isnan(acc.exceed_fraction["msl"][0, 0].cpu()[land]).all()
    cpu = FieldStats(thresholds={"msl": [101325.0]})
    for x in b:
        cpu.update(x)
    for k in INT + ("origin", "vmin", "vmax"):
        assert torch.equal(acc.state[k].cpu(), cpu.state[k]), k


@pytest.mark.parametrize("below", [False, True])
def test_planted_runs(below):
    """12 samples with known runs at one point, one run at the end, a threshold equal to a value; every other point of the
    17 x 32 plane carries its own shifted copy of the sequence and is compared with the yardstick."""
    seq = torch.tensor([1, 5, 5, 0, 5, 7, 5, 5, 2, 3, 5, 5], dtype=torch.float64)
    shift = torch.arange(17 * 32, dtype=torch.float64).view(1, 17, 32) % 4          # point 0: the sequence itself
    xs = [carve(seq[s] + shift, 0) for s in range(12)]
    thr = torch.tensor([[5.0, 3.0, 6.0]], dtype=torch.float32, device=DEV)
    state, _ = run(xs, thr=thr, below=below)
    got = host(state)
    at0 = [got[k][0, :, 0].tolist() for k in ("exceed", "longest", "run")]
    if not below:
        assert at0 == [[8, 9, 1], [4, 4, 1], [2, 3, 0]]
    else:
        assert at0 == [[11, 4, 11], [6, 2, 6], [6, 0, 6]]
    check_against_yardstick(state, xs, None, None, thr, below, f"runs below={below}")


@pytest.mark.parametrize("S", [2, 5, 64])
def test_grouping_does_not_change_a_single_bit(S):
    """One call with S samples = S calls with one sample = calls with 2 + (S - 2) samples, in every state array; with a
    reference, a second operand on one plane, two thresholds, NaNs and an unaligned odd-sized grid."""
    n_planes, n_lat, n_lon = 2, 33, 61
    xs = samples(S, n_planes, n_lat, n_lon, seed=11, offset=1)
    bs = samples(S, 1, n_lat, n_lon, seed=12, offset=1)
    xs[1][0, 3, 4] = float("nan")
    xs[0][1, 0, :] = float("nan")
    ref = carve(101325 + 300 * torch.randn(n_planes, n_lat, n_lon, generator=torch.Generator().manual_seed(13), dtype=torch.float64), 3)
    second = [[None, bs[s][0]] for s in range(S)]
    thr = torch.tensor([[0.0, 300.0], [50000.0, float("nan")]], dtype=torch.float32, device=DEV)
    args = dict(ref=ref, second=second, thr=thr)
    whole, index = run(xs, **args)
    ones, _ = run(xs, groups=[1] * S, **args)
    split, _ = run(xs, groups=[2, S - 2] if S > 2 else [1, 1], **args)
    torch.cuda.synchronize()
    assert int(index) == S and int(whole["n"].max()) == S and int(whole["argmax"].max()) == S - 1
    assert_equal_states(whole, ones, "S x 1")
    assert_equal_states(whole, split, "2 + rest")
    check_against_yardstick(whole, xs, ref, second, thr, False, f"grouping S={S}")


def test_repeatable_and_independent_of_the_other_planes_and_of_alignment():
    S, n_lat, n_lon = 5, 33, 64
    a = samples(S, 3, n_lat, n_lon, seed=21)
    b = samples(S, 3, n_lat, n_lon, seed=21, offset=1)
    assert a[0].data_ptr() % 16 == 0 and b[0].data_ptr() % 16 == 4 and torch.equal(a[2], b[2])
    thr = torch.tensor([[101325.0]] * 3, dtype=torch.float32, device=DEV)
    first, _ = run(a, thr=thr)
    again, _ = run(a, thr=thr)
    unaligned, _ = run(b, thr=thr)
    assert_equal_states(first, again, "repeat")
    assert_equal_states(first, unaligned, "alignment")                 # the 16-byte and the 4-byte path: the same elements
    for k in range(3):                                                 # a plane alone = the plane among others
        single, _ = run([x[k:k + 1] for x in a], thr=thr[k:k + 1])
        for name in first:
            assert torch.equal(first[name][k:k + 1], single[name]), (k, name)


def static_batches(seed, n=4):
    return [make_batch(17, 32, seed=seed + i, B=2).to(DEV) for i in range(n)]


def copy_into(dst: Batch, src: Batch):
    for group in ("surf_vars", "atmos_vars"):
        for k, v in getattr(dst, group).items():
            v.copy_(getattr(src, group)[k])


def test_updates_are_capturable_in_a_hip_graph():
    """One captured `update` over static input buffers, replayed three times with new contents, leaves the state and the
    argmax of four eager updates: the sample index lives on the device."""
    contents = static_batches(400)
    kw = dict(thresholds={"2t": [300.0, 305.0], "10ws": [17.2]}, derived=("10ws",))
    buf = make_batch(17, 32, seed=1, B=2).to(DEV)
    eager, graphed = FieldStats(**kw), FieldStats(**kw)
    for c in contents:
        copy_into(buf, c)
        eager.update(buf)
    want = {k: v.clone() for k, v in eager.state.items()}
    copy_into(buf, contents[0])
    graphed.update(buf)                                               # the warm call: sample 0, tables uploaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.update(buf)
    for c in contents[1:]:
        copy_into(buf, c)
        graph.replay()
    torch.cuda.synchronize()
    assert_equal_states(graphed.state, want, "replay")
    assert int(graphed.state["argmax"].max()) == 3 and (graphed.count["2t"] == 4).all()
    assert torch.equal(graphed.argmax["10ws"], eager.argmax["10ws"])
    y = yardstick(np.stack([c.surf_vars["2t"][:, -1].cpu().numpy() for c in contents]), thr=[300.0, 305.0])
    st = variable_state(graphed.cpu(), "2t")
    assert_state_matches(st, y, "replayed 2t")


def test_a_cold_call_during_capture_is_refused(monkeypatch):
    # (the allocator hands the addresses of dead tensors out again, and a table that an earlier test's graph used is never
    #  evicted: an empty table cache and a warm batch that stays alive make `fresh` cold whatever ran before)
    monkeypatch.setattr(lib, "_plane_tables", type(lib._plane_tables)())
    warm = make_batch(17, 32, seed=2, B=1).to(DEV)
    acc = FieldStats().update(warm)
    fresh = make_batch(17, 32, seed=3, B=1).to(DEV)                    # addresses no call has seen
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before capturing"):
        acc.update(fresh)


def rollout_check(case_name, steps, derived):
    case = CASES[case_name]
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    model.load_state_dict(helpers.case_state_dict(model, torch.float32), strict=True)
    model = model.to(DEV).eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
    thresholds = {"2t": [280.0, 290.0]}
    dev, cpu, copies = FieldStats(thresholds, derived=derived), FieldStats(thresholds, derived=derived), []
    with torch.inference_mode():
        for pred in rollout(model, batch.to(DEV), steps=steps):
            dev.update(pred)                                           # ring-buffer views as inputs
            copies.append(pred.to("cpu"))
    for c in copies:
        cpu.update(c)
    assert [k for k, *_ in dev.layout] == [k for k, *_ in cpu.layout] and (dev.count["2t"] <= steps).all()
    got = dev.cpu()
    checked = 0
    for name, group, _, shape in got.layout:
        a, b = variable_state(got, name), variable_state(cpu, name)
        for k in INT:
            assert np.array_equal(a[k], b[k]), (name, k)
        for k in ("origin", "vmin", "vmax"):
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (name, k)
        if name in DERIVED_OF:
            x, second = (np.stack([getattr(c, group)[v][:, -1].numpy() for c in copies]) for v in DERIVED_OF[name])
        else:
            x, second = np.stack([getattr(c, group)[name][:, -1].numpy() for c in copies]), None
        y = yardstick(x, second)
        n = y["n"]
        assert np.array_equal(a["n"], n), name
        assert (np.abs(a["s1"] - b["s1"]) <= 2 * n * U * y["sum_abs_d"]).all(), (name, "s1")
        assert (np.abs(a["s2"] - b["s2"]) <= 2 * (n + 1) * U * y["s2"]).all(), (name, "s2")
        checked += int(np.prod(shape))
    assert checked == got.state["n"].shape[0]
    assert int(got.state["n"].max()) == steps and int(got.state["argmax"].max()) == steps - 1
    return got


DERIVED_OF = {"10ws": ("10u", "10v"), "ws": ("u", "v")}


def test_a_rollout_accumulated_step_by_step_equals_the_host_path():
    got = rollout_check("small_b2", 3, ("10ws", "ws"))
    assert got.mean["2t"].shape == (2, 16, 32) and got.mean["ws"].shape == (2, 4, 16, 32)


def test_nine_steps_roll_the_history_ring_over():
    rollout_check("lora_all", 9, ("10ws",))


def test_a_warm_update_allocates_less_than_a_plane_and_does_not_synchronise():
    n_lat, n_lon = 181, 360
    a = make_batch(n_lat, n_lon, seed=500, B=1).to(DEV)
    truth = make_batch(n_lat, n_lon, seed=502, B=1, wind=False).to(DEV)
    truth.surf_vars.update({"10u": a.surf_vars["10u"], "10v": a.surf_vars["10v"], "10ws": a.surf_vars["2t"]})
    truth.atmos_vars.update({"u": a.atmos_vars["u"], "v": a.atmos_vars["v"]})
    acc = FieldStats(thresholds={"2t": [300.0]}, derived=("10ws",))
    acc.update(a, minus=truth)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        acc.update(a, minus=truth)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"a warm update of {acc.state['n'].shape[0]} planes: peak allocation grows by {grown} bytes (one plane: {n_lat * n_lon * 4})")
    assert grown < n_lat * n_lon * 4
    torch.cuda.set_sync_debug_mode("error")
    try:
        mean = acc.mean                                                 # finalisation: elementwise, no read-back either
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert (acc.count["2t"] == 2).all() and mean["2t"].device == DEV


def test_device_path_argument_errors():
    """Every one raises before anything is launched: the state stays as it was."""
    good = make_batch(17, 32, seed=600).to(DEV)
    acc = FieldStats().update(good)
    before = {k: v.clone() for k, v in acc.state.items()}
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        acc.update(make_batch(17, 32, seed=601))
    mixed = make_batch(17, 32, seed=602).to(DEV)
    mixed.surf_vars["2t"] = mixed.surf_vars["2t"].cpu()
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        acc.update(mixed)
    with pytest.raises(TypeError, match="float64"):
        acc.update(good.type(torch.float64))
    tr = make_batch(17, 32, seed=603).to(DEV)
    tr.surf_vars["2t"] = tr.surf_vars["2t"].transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match="contiguous"):
        acc.update(tr)
    assert_equal_states(acc.state, before, "after refused updates")
    # the C entry point itself: -1 and a message, nothing enqueued
    xs = samples(1, 1, 3, 5, seed=1)
    state, index = run(xs)
    keep = {k: v.clone() for k, v in state.items()}
    L = lib.load()
    table = torch.tensor([xs[0].data_ptr()], dtype=torch.int64, device=DEV)
    ptrs = [state[k].data_ptr() for k in ("n", "origin", "s1", "s2", "vmin", "vmax", "argmin", "argmax")]
    call = lambda S, T, n_ptr=ptrs[0], planes=1: L.aurora_hip_field_stats_update(  # noqa: E731
        table.data_ptr(), None, None, S, planes, 15, None, T, 0, index.data_ptr(), n_ptr, *ptrs[1:], None, None, None,
        torch.cuda.current_stream().cuda_stream)
    for S, T, n_ptr, word in ((0, 0, ptrs[0], "n_samples"), (65, 0, ptrs[0], "n_samples"), (1, 9, ptrs[0], "n_thresholds"),
                              (1, -1, ptrs[0], "n_thresholds"), (1, 0, None, "null state"), (1, 2, ptrs[0], "null threshold")):
        assert call(S, T, n_ptr) == -1
        assert word in L.aurora_hip_last_error().decode()
    assert call(1, 0, planes=0) == 0                                   # n_planes = 0: a no-op
    torch.cuda.synchronize()
    assert int(index) == 1
    assert_equal_states(state, keep, "after refused calls")
    with pytest.raises(AssertionError, match="1..64 samples"):
        lib.field_stats_update([[xs[0]]] * 65, None, None, None, False, index, state)
