"""`aurora_amd.diagnostics` on the device: aurora_hip_diagnostics against the numpy fp64 yardstick written in
tests/test_diagnostics_host.py (`yardstick_wind`, `yardstick_columns`: its own row table and level weights; the CPU path of
`aurora_amd.diagnostics` is code under test and is checked against the same yardstick there).

Bound (derived there, not tuned; u = 2^-53, gamma_k = k u / (1 - k u)): two fp64 evaluations of a stencil formula in any
order, fused or not, differ by at most 2 gamma_8 S with S = |A| ((|f_e| + |f_w|) |L'| + |m0 a| + |m1 b| + |m2 c|), and the fp32
result is a correct rounding: |got - y64| <= 2 gamma_8 S + 1/2 spacing32(max(|got|, |fp32(y64)|)).  Column sums: 2 gamma_{C+2}
sum |w q u| before the fp32 rounding; ivt: |delta ivtu| + |delta ivtv| + 4 u ivt.  The wind speed is bit-equal.  Device
against CPU path: both are such evaluations, each rounded to fp32 once, so they differ by at most the same fp64 term plus one
whole spacing32.  Every plane and every point of every case is compared."""
import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, FieldStats, Metadata, diagnostics, scores
from aurora_amd.diagnostics import level_weights, row_table
from aurora_amd.engine import lib
from tests import helpers
from tests.golden_cases import CASES
from tests.test_diagnostics_host import (ALL, GRIDS, U, assert_bit_equal, assert_within, check_batch, gamma, longitude_factor,
                                         make_batch, yardstick_columns, yardstick_wind)
from tests.verification_inputs import DEV, carve

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2), (3, 5), (17, 32), (33, 130), (64, 1030)]
WIND_OUTPUTS = [("vo", "div", "ws"), ("vo",), ("div", "ws"), ("ws",), ("vo", "div")]
COLUMN_OUTPUTS = [("tcwv", "ivtu", "ivtv", "ivt"), ("tcwv",), ("ivt",), ("ivtu", "ivtv"), ("tcwv", "ivtv")]


def grid(n_lat, n_lon, wrap):
    """Descending latitudes without poles, unequal where there is room; a full circle or a regional quarter-degree strip."""
    lat = np.linspace(88.0, -88.0, n_lat)
    if n_lat > 4:
        lat[2] -= 0.3 * (lat[1] - lat[2])
    lon = np.arange(n_lon) * (360.0 / n_lon) if wrap else 10.0 + 0.25 * np.arange(n_lon)
    return lat, lon


def winds(n, n_lat, n_lon, seed, offset):
    g = torch.Generator().manual_seed(seed)
    u = carve(40 + 5 * torch.randn(n, n_lat, n_lon, generator=g, dtype=torch.float64), offset)
    v = carve(-30 + 5 * torch.randn(n, n_lat, n_lon, generator=g, dtype=torch.float64), offset)
    return u, v


def run_wind(u, v, lat, lon, wrap, outputs, offset=0):
    """One call of the wind group; the outputs asked for, each in a carved buffer filled with a canary."""
    n_lat, n_lon = u.shape[-2:]
    out = {k: carve(torch.zeros(u.shape), offset, fill=-777.0) for k in outputs}
    table = torch.from_numpy(row_table(lat)).to(DEV) if {"vo", "div"} & set(outputs) else None
    lib.diagnostics(n_lat, n_lon, u=[u], v=[v], row_table=table, L=longitude_factor(lon, wrap), wrap=wrap,
                    **{k: [t] for k, t in out.items()})
    return out


def check_wind(out, u, v, lat, lon, wrap, what):
    y = yardstick_wind(u.cpu().numpy(), v.cpu().numpy(), lat, lon, wrap)
    for k, t in out.items():
        if k == "ws":
            assert_bit_equal(t.cpu().numpy(), y["ws"], f"{what} ws")
        else:
            y64, S = y["vo" if k == "vo" else "d"]
            assert_within(t.cpu().numpy(), y64, 2 * gamma(8) * S, f"{what} {k}")


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("n_items", [1, 3])
@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("n_lat,n_lon", SHAPES)
def test_the_wind_group_equals_the_yardstick(n_lat, n_lon, wrap, n_items, offset):
    lat, lon = grid(n_lat, n_lon, wrap)
    u, v = winds(n_items, n_lat, n_lon, seed=n_lat + n_lon + n_items, offset=offset)
    if offset:
        assert u.data_ptr() % 16 != 0 and v.data_ptr() % 16 != 0
    outputs = WIND_OUTPUTS[(SHAPES.index((n_lat, n_lon)) + offset + n_items + wrap) % len(WIND_OUTPUTS)]
    out = run_wind(u, v, lat, lon, wrap, outputs, offset)
    check_wind(out, u, v, lat, lon, wrap, f"{n_lat}x{n_lon} wrap={wrap} x{n_items} +{offset} {outputs}")


def test_every_wind_output_table_is_present_and_absent_somewhere_and_one_call_is_wind_speed_alone():
    cases = {WIND_OUTPUTS[(s + o + n + w) % len(WIND_OUTPUTS)] for s in range(len(SHAPES)) for o in (0, 1, 3) for n in (1, 3) for w in (0, 1)}
    assert cases == set(WIND_OUTPUTS) and ("ws",) in cases
    for k in ("vo", "div", "ws"):
        assert any(k in c for c in cases) and any(k not in c for c in cases)
    cases = {COLUMN_OUTPUTS[(s + o + c) % len(COLUMN_OUTPUTS)] for s in range(len(SHAPES)) for o in (0, 1, 3) for c in (2, 13)}
    for k in ("tcwv", "ivtu", "ivtv", "ivt"):
        assert any(k in c for c in cases) and any(k not in c for c in cases)


def columns(B, C, n_lat, n_lon, seed, offset):
    g = torch.Generator().manual_seed(seed)
    r = lambda off, sc: off + sc * torch.randn(B, C, n_lat, n_lon, generator=g, dtype=torch.float64)  # noqa: E731
    return carve((0.005 * (1 + 0.3 * r(0, 1))).abs(), offset), carve(r(40, 5), offset), carve(r(-30, 5), offset)


def run_columns(q, u, v, levels, outputs, offset=0):
    B, C, n_lat, n_lon = q.shape
    out = {k: carve(torch.zeros(B, n_lat, n_lon), offset, fill=-777.0) for k in outputs}
    need_u, need_v = bool({"ivtu", "ivt"} & set(outputs)), bool({"ivtv", "ivt"} & set(outputs))
    lib.diagnostics(n_lat, n_lon, q=[q], col_u=[u] if need_u else None, col_v=[v] if need_v else None,
                    level_w=torch.from_numpy(level_weights(levels)).to(DEV), **{k: [t] for k, t in out.items()})
    return out


LEVELS = {2: (500, 850), 13: (1000, 50, 100, 150, 925, 200, 250, 300, 400, 500, 600, 700, 850)}


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("C", [2, 13])
@pytest.mark.parametrize("n_lat,n_lon", SHAPES)
def test_the_column_group_equals_the_yardstick(n_lat, n_lon, C, offset):
    B = 1 + (n_lat + C) % 2
    q, u, v = columns(B, C, n_lat, n_lon, seed=n_lat + C, offset=offset)
    if offset:
        assert q.data_ptr() % 16 != 0
    outputs = COLUMN_OUTPUTS[(SHAPES.index((n_lat, n_lon)) + offset + C) % len(COLUMN_OUTPUTS)]
    out = run_columns(q, u, v, LEVELS[C], outputs, offset)
    y = yardstick_columns(q.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy(), LEVELS[C])
    for k, t in out.items():
        assert_within(t.cpu().numpy(), y[k][0], y[k][1], f"{n_lat}x{n_lon} C={C} B={B} +{offset} {k}")


def test_both_groups_in_one_call_with_entries_left_out():
    """The call the public function makes: atmospheric and surface winds as items of one launch, an output asked of one of
    them only (NULL entries), and the columns."""
    n_lat, n_lon, wrap = 33, 130, True
    lat, lon = grid(n_lat, n_lon, wrap)
    ua, va = winds(4, n_lat, n_lon, seed=1, offset=1)
    us, vs = winds(1, n_lat, n_lon, seed=2, offset=3)
    q, cu, cv = columns(1, 4, n_lat, n_lon, seed=3, offset=0)
    new = lambda n: torch.full((n, n_lat, n_lon), -777.0, device=DEV)  # noqa: E731
    vo, ws_a, ws_s, ivt = new(4), new(4), new(1), new(1)
    lib.diagnostics(n_lat, n_lon, u=[ua, us], v=[va, vs], vo=[vo, None], ws=[ws_a, ws_s], row_table=torch.from_numpy(row_table(lat)).to(DEV),
                    L=longitude_factor(lon, wrap), wrap=wrap, q=[q], col_u=[cu], col_v=[cv], ivt=[ivt],
                    level_w=torch.from_numpy(level_weights((850, 1000, 500, 700))).to(DEV))
    check_wind({"vo": vo, "ws": ws_a}, ua, va, lat, lon, wrap, "atmospheric items")
    check_wind({"ws": ws_s}, us, vs, lat, lon, wrap, "surface item")
    y = yardstick_columns(q.cpu().numpy(), cu.cpu().numpy(), cv.cpu().numpy(), (850, 1000, 500, 700))
    assert_within(ivt.cpu().numpy(), *y["ivt"], "ivt beside the winds")


@pytest.mark.parametrize("n_lat,n_lon", [(33, 130), (64, 1030)])
def test_results_are_repeatable_and_depend_on_the_plane_alone(n_lat, n_lon):
    """Two calls on the same inputs, a plane alone and among others, and a plane at offset 0 and at offset 3: the same bits."""
    lat, lon = grid(n_lat, n_lon, True)
    u, v = winds(3, n_lat, n_lon, seed=9, offset=0)
    a, b = (run_wind(u, v, lat, lon, True, ("vo", "div", "ws")) for _ in range(2))
    alone = run_wind(u[1:2], v[1:2], lat, lon, True, ("vo", "div", "ws"))
    moved = run_wind(carve(u.cpu()[1:2], 3), carve(v.cpu()[1:2], 3), lat, lon, True, ("vo", "div", "ws"), offset=3)
    assert moved["vo"].data_ptr() % 16 != 0
    for k in a:
        assert_bit_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), f"twice {k}")
        assert_bit_equal(a[k][1:2].cpu().numpy(), alone[k].cpu().numpy(), f"alone {k}")
        assert_bit_equal(a[k][1:2].cpu().numpy(), moved[k].cpu().numpy(), f"offset 3 {k}")
    q, cu, cv = columns(2, 13, n_lat, n_lon, seed=10, offset=0)
    names = ("tcwv", "ivtu", "ivtv", "ivt")
    a, b = (run_columns(q, cu, cv, LEVELS[13], names) for _ in range(2))
    alone = run_columns(q[1:2], cu[1:2], cv[1:2], LEVELS[13], names)
    moved = run_columns(*(carve(t.cpu()[1:2], 3) for t in (q, cu, cv)), LEVELS[13], names, offset=3)
    for k in a:
        assert_bit_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), f"twice {k}")
        assert_bit_equal(a[k][1:2].cpu().numpy(), alone[k].cpu().numpy(), f"alone {k}")
        assert_bit_equal(a[k][1:2].cpu().numpy(), moved[k].cpu().numpy(), f"offset 3 {k}")


def assert_device_matches_host(dev: Batch, cpu: Batch, batch: Batch, wrap: bool, what: str):
    """ws bit-equal; everything else within the fp64 term of the bound plus one spacing32 (two single roundings)."""
    md = batch.metadata
    lat, lon = md.lat.double().cpu().numpy(), md.lon.double().cpu().numpy()
    last = lambda f: f[:, -1].float().cpu().numpy()  # noqa: E731
    for group in ("surf_vars", "atmos_vars"):
        assert list(getattr(dev, group)) == list(getattr(cpu, group))
        for k, t in getattr(dev, group).items():
            assert t.device == DEV and t.dtype == torch.float32 and t.shape == getattr(cpu, group)[k].shape
            got, want = t.cpu().numpy(), getattr(cpu, group)[k].numpy()
            if k in ("ws", "10ws"):
                assert_bit_equal(got, want, f"{what} {k}")
                continue
            if k in ("vo", "d", "10vo", "10d"):
                a, b = ("10u", "10v") if k.startswith("10") else ("u", "v")
                src = batch.surf_vars if k.startswith("10") else batch.atmos_vars
                bound = 2 * gamma(8) * yardstick_wind(last(src[a]), last(src[b]), lat, lon, wrap)[k[-2:] if k.endswith("vo") else "d"][1]
            else:
                bound = yardstick_columns(last(batch.atmos_vars["q"]), last(batch.atmos_vars["u"]), last(batch.atmos_vars["v"]),
                                          md.atmos_levels)[k][1]
            bound = bound[:, None]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (what, k, "NaN pattern")
            ok = ~np.isnan(got)
            with np.errstate(invalid="ignore"):
                tol = bound + np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64)
                assert (np.abs(got.astype(np.float64) - want)[ok] <= tol[ok]).all(), (what, k)


@pytest.mark.parametrize("name", list(GRIDS))
def test_the_public_function_on_the_device_equals_the_host_path_and_the_yardstick(name):
    lat, lon, wrap = GRIDS[name]
    batch = make_batch(lat, lon, seed=21)
    dev_batch = batch.to(DEV)
    d = diagnostics(dev_batch, ALL)
    assert d.metadata is dev_batch.metadata and d.static_vars["lsm"].device == DEV
    check_batch(d, batch, wrap, what=f"device, {name}")
    assert_device_matches_host(d, diagnostics(batch, ALL), batch, wrap, name)
    kept = diagnostics(dev_batch, ("10ws", "tcwv"), keep=True)         # wind speed alone, tcwv alone (no u, v read)
    assert list(kept.surf_vars) == ["2t", "10u", "10v", "10ws", "tcwv"] and list(kept.atmos_vars) == ["u", "v", "q", "t"]
    assert torch.equal(kept.surf_vars["10ws"], d.surf_vars["10ws"]) and torch.equal(kept.surf_vars["tcwv"], d.surf_vars["tcwv"])
    assert torch.equal(kept.atmos_vars["q"], dev_batch.atmos_vars["q"][:, -1:])


def test_nan_land_mask_and_pole_rows_behave_as_on_the_host():
    lat, lon, wrap = GRIDS["global descending with poles"]
    batch = make_batch(lat, lon, seed=33)
    land = torch.rand(len(lat), len(lon), generator=torch.Generator().manual_seed(1)) < 0.3
    for k in ("10u", "10v"):
        batch.surf_vars[k][:, -1, land] = float("nan")                 # a wave-model style mask on the surface wind
    batch.atmos_vars["q"][:, -1, 0, land] = float("nan")               # the lowest level under ground
    batch.atmos_vars["u"][0, -1, 2, 5, 0] = float("inf")
    d, h = diagnostics(batch.to(DEV), ALL), diagnostics(batch, ALL)
    check_batch(d, batch, wrap, what="land mask")
    assert_device_matches_host(d, h, batch, wrap, "land mask")
    assert torch.isnan(d.atmos_vars["vo"][..., [0, -1], :]).all() and torch.isnan(d.surf_vars["10d"][..., [0, -1], :]).all()
    assert torch.isnan(d.surf_vars["tcwv"][:, 0, land]).all() and torch.isfinite(d.surf_vars["tcwv"][:, 0, ~land]).all()
    assert torch.isnan(d.surf_vars["10ws"][:, 0, land]).all() and torch.isfinite(d.surf_vars["10ws"][:, 0, ~land]).all()
    assert int(torch.isnan(d.atmos_vars["ws"]).sum()) == 1 and int(torch.isnan(d.atmos_vars["d"][0, 0, 2, 5]).sum()) == 2


def test_a_golden_case_batch_on_the_device():
    """The inputs of a golden case (17 x 32, B = 2, four levels) as prediction, a shifted copy as truth: the device result as
    a `Batch` with the right shapes and metadata, equal to the host result, and food for `scores` and `FieldStats`."""
    case = CASES["small_b2"]
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    pred = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
    truth = Batch({k: v.roll(1, -1) for k, v in pred.surf_vars.items()}, pred.static_vars,
                  {k: v.roll(1, -1) for k, v in pred.atmos_vars.items()}, pred.metadata)
    names = ("vo", "d", "ws", "10ws", "10vo", "tcwv", "ivt")
    wrap = True
    dp, dt = diagnostics(pred.to(DEV), names), diagnostics(truth.to(DEV), names)
    B, C, H, W = case["B"], len(case["levels"]), case["H"], case["W"]
    assert {k: tuple(v.shape) for k, v in dp.atmos_vars.items()} == {k: (B, 1, C, H, W) for k in ("vo", "d", "ws")}
    assert {k: tuple(v.shape) for k, v in dp.surf_vars.items()} == {k: (B, 1, H, W) for k in ("10ws", "10vo", "tcwv", "ivt")}
    assert dp.metadata.time == times and dp.metadata.atmos_levels == tuple(case["levels"]) and set(dp.static_vars) == set(static)
    assert all(v.device == DEV for v in (*dp.surf_vars.values(), *dp.atmos_vars.values(), *dp.static_vars.values(), dp.metadata.lat))
    check_batch(dp, pred, wrap, names, what="golden case")
    assert_device_matches_host(dp, diagnostics(pred, names), pred, wrap, "golden case")
    s = scores(dp, dt)
    assert set(s.rmse) == set(names) and s.rmse["vo"].shape == (B, C)
    assert torch.isfinite(s.rmse["ivt"]).all() and (s.rmse["ivt"] > 0).all() and (s.count["tcwv"] > 0).all()
    acc = FieldStats().update(dp).update(dt)
    assert acc.mean["vo"].shape == (B, C, H, W) and acc.mean["vo"].device == DEV and int(acc.count["ivt"].max()) == 2


def test_the_call_is_capturable_in_a_hip_graph():
    """Captured after one warm call on the same buffers, replayed on changed input values: the bits of an eager call."""
    n_lat, n_lon, wrap = 33, 130, True
    lat, lon = grid(n_lat, n_lon, wrap)
    u, v = winds(2, n_lat, n_lon, seed=1, offset=1)
    q, cu, cv = columns(1, 4, n_lat, n_lon, seed=2, offset=0)
    new = lambda n: torch.full((n, n_lat, n_lon), -777.0, device=DEV)  # noqa: E731
    table = torch.from_numpy(row_table(lat)).to(DEV)
    level_w = torch.from_numpy(level_weights((850, 1000, 500, 700))).to(DEV)
    outs = [{k: new(2) for k in ("vo", "div", "ws")} | {k: new(1) for k in ("tcwv", "ivtu", "ivtv", "ivt")} for _ in range(2)]
    call = lambda o: lib.diagnostics(n_lat, n_lon, u=[u], v=[v], row_table=table, L=longitude_factor(lon, wrap), wrap=wrap,  # noqa: E731
                                     q=[q], col_u=[cu], col_v=[cv], level_w=level_w, **{k: [t] for k, t in o.items()})
    call(outs[0])                                                      # the warm call: the pointer table is uploaded
    call(outs[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(outs[0])
    u2, v2 = winds(2, n_lat, n_lon, seed=5, offset=0)
    q2, cu2, cv2 = columns(1, 4, n_lat, n_lon, seed=6, offset=0)
    for dst, src in ((u, u2), (v, v2), (q, q2), (cu, cu2), (cv, cv2)):
        dst.copy_(src)
    before = outs[0]["vo"].clone()
    graph.replay()
    call(outs[1])
    torch.cuda.synchronize()
    assert not torch.equal(before, outs[0]["vo"])
    for k in outs[0]:
        assert_bit_equal(outs[0][k].cpu().numpy(), outs[1][k].cpu().numpy(), f"replay {k}")
    check_wind({k: outs[0][k] for k in ("vo", "div", "ws")}, u, v, lat, lon, wrap, "replay")


def test_argument_errors_come_back_before_anything_is_enqueued():
    u, v = winds(1, 1, 8, seed=0, offset=0)                            # n_lat = 1
    canary = torch.full((1, 1, 8), -777.0, device=DEV)
    with pytest.raises(ValueError, match=r"at least 2 latitudes.*\(code -1\)"):
        lib.diagnostics(1, 8, u=[u], v=[v], ws=[canary])
    q, cu, cv = columns(1, 65, 3, 4, seed=0, offset=0)                 # C = 65
    out = torch.full((1, 3, 4), -777.0, device=DEV)
    with pytest.raises(ValueError, match=r"2\.\.64 levels, got 65.*\(code -1\)"):
        lib.diagnostics(3, 4, q=[q], tcwv=[out], level_w=torch.ones(65, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match=r"ivtu and ivt need the u plane table.*\(code -1\)"):       # a NULL u table, ivtu asked for
        lib.diagnostics(3, 4, q=[q[:, :4]], col_v=[cv[:, :4]], ivtu=[out], level_w=torch.ones(4, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert (canary == -777.0).all() and (out == -777.0).all()
    lib.diagnostics(3, 4)                                              # nothing asked for: a no-op


def test_device_errors_of_the_public_function():
    lat, lon, _ = GRIDS["regional unequal latitudes"]
    batch = make_batch(lat, lon)
    mixed = Batch(batch.surf_vars, {}, {**batch.atmos_vars, "u": batch.atmos_vars["u"].to(DEV)}, batch.metadata)
    with pytest.raises(ValueError, match="move the batch to the CPU or to one GPU first"):
        diagnostics(mixed, "vo")
    dev = batch.to(DEV)
    doubles = Batch(dev.surf_vars, {}, {**dev.atmos_vars, "v": dev.atmos_vars["v"].double()}, dev.metadata)
    with pytest.raises(TypeError, match="the device path takes float32 fields"):
        diagnostics(doubles, "ws")
    strided = Batch({**dev.surf_vars, "10u": dev.surf_vars["10u"].transpose(-1, -2).contiguous().transpose(-1, -2)}, {}, {}, dev.metadata)
    with pytest.raises(ValueError, match="not row-major contiguous"):
        diagnostics(strided, "10vo")
