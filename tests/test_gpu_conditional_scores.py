"""`aurora_amd.conditional_scores` on the device: one aurora_hip_conditional_scores call against the numpy fp64 yardstick of
tests/test_conditional_scores_host.py (`yardstick_sums`; not `aurora_amd.conditional._sums_host`, which is code under test).

Bound (derived as in tests/test_gpu_scores.py, not tuned): both sides are within N 2^-53 sum|term| of the exact sum; with
N <= 721 x 1440, 2 N 2^-53 = 2.3e-10, so the count is exact, S1, S3 and S4 agree to 1e-9 relative and S2 to 1e-9 x S4;
finalised: rmse to 1e-9 relative, mae to 2e-9 relative, bias to 2e-9 x mae.  The bin of a point comes from single correctly
rounded fp64 operations on both sides: the integers must be equal, with no tolerance.  Every plane and every bin is compared."""
import functools
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, FieldStats, Metadata, conditional_scores, rollout
from aurora_amd.engine import lib
from tests import helpers
from tests.golden_cases import CASES
from tests.test_conditional_scores_host import (GRIDS, REL, UNIT_EDGES, assert_not_trivial, assert_sums_match,
                                                check_against_yardstick, make_batches, planes, yardstick_sums)
from tests.verification_inputs import DEV, carve, weights

pytestmark = pytest.mark.gpu
EIGHT = (-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0)
NAN = float("nan")


def edge_tables(n_planes, unit):
    """(n_planes, E) float32 tables with E = 1, 3 and 8, one where a NaN-padded row stands beside a full one, and one whose
    rows are all padded."""
    rows = lambda *choices: np.array([choices[k % len(choices)] for k in range(n_planes)], dtype=np.float64) * unit  # noqa: E731
    return [rows((0.25,)), rows((-1.0, 0.0, 1.0), (-0.5, 0.5, 1.5)), rows(EIGHT), rows(UNIT_EDGES, (-0.5, 1.0, NAN, NAN)),
            rows((-0.5, 1.0, NAN, NAN, NAN))]


def call(p, t, c, s, edges: np.ndarray, by, w_dev):
    e = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float32)).to(DEV)
    out = lib.conditional_sums([p], [t], None if c is None else [c], None if s is None else [s], e, by == "pred", w_dev)
    assert out.shape == (p.shape[0], edges.shape[1] + 1, 5) and out.dtype == torch.float64 and out.device == DEV
    return out


@functools.lru_cache(maxsize=None)
def grid_inputs(n_planes, n_lat, n_lon):
    """The host planes of one grid, made and checked once for the four choices of maps (nothing writes to them)."""
    host = planes(n_planes, n_lat, n_lon, seed=n_lat + n_lon)
    assert_not_trivial(*host, weights(n_lat))
    return host


def check_tables(host, dev, n_lat, maps, what):
    """Every edge table and both `by` for one choice of maps, every plane and bin against the yardstick."""
    w = weights(n_lat)
    w_dev = torch.from_numpy(w).to(DEV)
    c_h, s_h = (host[2] if maps in ("centre", "both") else None), (host[3] if maps in ("scale", "both") else None)
    c_d, s_d = (dev[2] if c_h is not None else None), (dev[3] if s_h is not None else None)
    keep = [x.clone() for x in dev]
    for edges in edge_tables(host[0].shape[0], 1.0 if s_h is not None else 200.0):
        for by in ("truth", "pred"):
            got = call(dev[0], dev[1], c_d, s_d, edges, by, w_dev).cpu().numpy()
            for k in range(host[0].shape[0]):
                own = edges[k][~np.isnan(edges[k])]
                y = yardstick_sums(host[0][k], host[1][k], None if c_h is None else c_h[k], None if s_h is None else s_h[k],
                                   own, by, w)
                assert_sums_match(got[k, : len(own) + 1], y, f"{what} {maps} E={edges.shape[1]} {by} plane {k}")
                assert (got[k, len(own) + 1:] == 0).all()
    for x, k in zip(dev, keep):                                                  # the inputs are not modified
        assert torch.equal(x.view(torch.int32), k.view(torch.int32))


@pytest.mark.parametrize("maps", ["none", "centre", "scale", "both"])
@pytest.mark.parametrize("n_planes,n_lat,n_lon", GRIDS)
def test_raw_table_equals_the_yardstick(n_planes, n_lat, n_lon, maps):
    host = grid_inputs(n_planes, n_lat, n_lon)
    offset = 3 if (n_lat, n_lon) == (33, 90) else 0                              # planes 3 floats past a 16-byte boundary
    dev = [carve(a, offset) for a in host]
    if offset:
        assert all(x[k].data_ptr() % 16 != 0 for x in dev for k in range(n_planes))
    elif n_lon % 4 == 0:
        assert all(x[k].data_ptr() % 16 == 0 for x in dev for k in range(n_planes))
    check_tables(host, dev, n_lat, maps, f"{n_planes}x{n_lat}x{n_lon}+{offset}")


def small(seed=7, n_planes=3, n_lat=33, n_lon=64, offset=0):
    host = planes(n_planes, n_lat, n_lon, seed)
    return host, [carve(a, offset) for a in host], torch.from_numpy(weights(n_lat)).to(DEV)


def test_two_calls_agree_and_a_plane_alone_equals_it_among_three():
    for n_lat, n_lon in ((33, 64), (721, 1440)):
        host, dev, w = small(n_lat=n_lat, n_lon=n_lon)
        assert_not_trivial(*host, weights(n_lat))
        edges = np.array([UNIT_EDGES] * 3)
        whole, again = call(*dev, edges, "truth", w), call(*dev, edges, "truth", w)
        alone = torch.cat([call(*(x[k:k + 1] for x in dev), edges[k:k + 1], "truth", w) for k in range(3)])
        assert torch.equal(whole, again) and torch.equal(whole, alone)


def test_alignment_does_not_change_a_single_bit():
    host, a, w = small()
    _, b, _ = small(offset=1)
    assert_not_trivial(*host, weights(33))
    assert a[0].data_ptr() % 16 == 0 and b[0].data_ptr() % 16 == 4 and torch.equal(a[1], b[1])
    for edges in (np.array([UNIT_EDGES] * 3), np.array([EIGHT] * 3)):
        assert torch.equal(call(*a, edges, "truth", w), call(*b, edges, "truth", w))
        assert torch.equal(call(a[0], a[1], None, None, edges * 200, "pred", w), call(b[0], b[1], None, None, edges * 200, "pred", w))


@pytest.mark.parametrize("n_lat,n_lon", [(33, 64), (33, 61), (721, 1440)])
def test_a_bin_depends_on_its_own_edges_alone(n_lat, n_lon):
    """The bin [e1, e2) of a 2-edge call has the bits of that bin in a 4-edge and in an 8-edge call (three instantiations of
    the kernel); the outer bins of a 1-edge call are the tails of a finer call up to the stated summation order."""
    host, dev, w = small(n_lat=n_lat, n_lon=n_lon, n_planes=2)
    assert_not_trivial(*host, weights(n_lat))
    rows = lambda e: np.array([e] * 2)  # noqa: E731
    for maps in ((dev[2], dev[3]), (None, None)):
        unit = 1.0 if maps[0] is not None else 200.0
        two = call(dev[0], dev[1], *maps, rows((-0.5, 0.5)) * unit, "truth", w)
        four = call(dev[0], dev[1], *maps, rows(UNIT_EDGES) * unit, "truth", w)
        eight = call(dev[0], dev[1], *maps, rows(EIGHT) * unit, "truth", w)
        assert torch.equal(two[:, 1], four[:, 2]) and torch.equal(two[:, 1], eight[:, 4])
        assert torch.equal(four[:, 0, 0], eight[:, 0, 0] + eight[:, 1, 0])      # the counts of a split bin add up
        assert (two[:, 1, 0] > 0).all()
        # a 1-edge call against the tails of the 4-edge call: integers equal, the sums within the bound; and the tails are
        # the bins added in the stated order, bit for bit
        one = call(dev[0], dev[1], *maps, rows((0.5,)) * unit, "truth", w)
        above = four[:, 4] + four[:, 3]                                          # descending: the top bin first
        below = (four[:, 0] + four[:, 1]) + four[:, 2]                           # ascending
        for k in range(2):
            assert_sums_match(one[k].cpu().numpy(), torch.stack([below[k], above[k]]).cpu().numpy(), "1 edge against tails")


def batch_of(x_pred, x_truth, x_centre, x_scale, n_lat, n_lon, levels=(100, 500)):
    """Four batches over (6, n_lat, n_lon) device planes: B = 1, 'msl' with two history entries and a two-level 'z'."""
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1)[:-1],
                  time=(datetime(2023, 1, 1, 6),),
                  atmos_levels=levels)
    mk = lambda x: Batch({"msl": x[:2].view(1, 2, n_lat, n_lon)}, {}, {"z": x[2:].view(1, 2, 2, n_lat, n_lon)}, md)  # noqa: E731
    return mk(x_pred), mk(x_truth), mk(x_centre), mk(x_scale)


def test_tails_are_the_bins_in_the_stated_order_bit_for_bit():
    host, dev, _ = small(n_planes=6)
    pred, truth, centre, scale = batch_of(*dev, 33, 64)
    s = conditional_scores(pred, truth, {"msl": UNIT_EDGES, "z": (-1.0, 1.0)}, centre=centre, scale=scale)
    t = s.sums_table
    assert torch.equal(s.above_sums[:, 1], (t[:, 4] + t[:, 3]) + t[:, 2]) and torch.equal(s.below_sums[:, 2], (t[:, 0] + t[:, 1]) + t[:, 2])
    z = s.sums["z"][0]                                                           # E_v = 2 of E = 4: the padded bins add +0
    assert torch.equal(s.above_sums[1:, 0], z[:, 2] + z[:, 1]) and torch.isnan(s.rmse_above["z"][0, :, 2:]).all()
    assert ((s.count_above["msl"] + s.count_below["msl"]) == 33 * 64).all()


def test_invalid_points():
    """NaN / Inf at both row ends in every operand, a negative scale, a block of invalid rows across a workgroup's rows, a
    whole-NaN plane: exact counts, zeros and NaN scores for the empty plane, and the untouched planes keep their bits."""
    n_lat, n_lon = 40, 52
    host = [a.copy() for a in planes(4, n_lat, n_lon, seed=31)]
    w = weights(n_lat)
    assert_not_trivial(*host, w)
    clean = [carve(a) for a in host]
    w_dev = torch.from_numpy(w).to(DEV)
    edges = np.array([UNIT_EDGES] * 4)
    before = call(*clean, edges, "truth", w_dev)
    p, t, c, s = host
    p[0, 0, 0], p[0, 5, -1], t[0, 0, -1], t[0, 7, 0] = np.nan, np.inf, -np.inf, np.nan
    c[0, 9, 0], c[0, 9, -1], s[0, 11, 0], s[0, 11, -1], s[0, 13, 20] = np.nan, np.inf, np.inf, np.nan, -1.0
    t[1, 10:19] = np.nan                                                         # rows of all four waves, two turns
    p[2] = np.nan
    dev = [carve(a) for a in host]
    got = call(*dev, edges, "truth", w_dev)
    counts = got[:, :, 0].sum(dim=1).tolist()
    assert counts == [n_lat * n_lon - 9, n_lat * n_lon - 9 * n_lon, 0, n_lat * n_lon]
    assert (got[2] == 0).all() and torch.equal(got[3], before[3])
    plain = call(dev[0], dev[1], None, None, edges * 200, "truth", w_dev)
    assert plain[:, :, 0].sum(dim=1).tolist() == [n_lat * n_lon - 4, n_lat * n_lon - 9 * n_lon, 0, n_lat * n_lon]
    for k in range(4):
        assert_sums_match(got[k].cpu().numpy(), yardstick_sums(p[k], t[k], c[k], s[k], UNIT_EDGES, "truth", w), f"invalid {k}")
    x = [d[2:3] for d in dev]
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1)[:-1],
                  time=(datetime(2023, 1, 1, 6),), atmos_levels=())
    b = [Batch({"2t": v.view(1, 1, n_lat, n_lon)}, {}, {}, md) for v in x]
    empty = conditional_scores(b[0], b[1], {"2t": UNIT_EDGES}, centre=b[2], scale=b[3]).cpu()
    assert (empty.count["2t"] == 0).all() and (empty.count_above["2t"] == 0).all()
    for prop in ("rmse", "bias", "mae", "rmse_above", "bias_below", "mae_above", "fraction"):
        assert torch.isnan(getattr(empty, prop)["2t"]).all(), prop


EDGES = {"2t": UNIT_EDGES, "msl": (-0.5, 1.0), "z": np.array([[-1.0, 0.0, 1.0], [-2.0, 0.5, 2.5], [-0.25, 0.25, 3.0]])}


def assert_device_equals_host(dev_s, host_s):
    """The device front end against the CPU path at the bound of the module's text: integers equal, S1, S3, S4 and rmse to
    REL, S2 to REL x S4, mae to 2 REL and bias to 2 REL x mae; the fraction, a ratio of two sums good to REL, to 2 REL."""
    d = dev_s.cpu()
    assert d.layout == host_s.layout and torch.equal(d.edges_table.nan_to_num(), host_s.edges_table.nan_to_num())
    for a, b in ((d.sums_table, host_s.sums_table), (d.above_sums, host_s.above_sums), (d.below_sums, host_s.below_sums)):
        assert_sums_match(a.reshape(-1, 5).numpy(), b.reshape(-1, 5).numpy(), "device against host")
    for a, b in ((d.bins_table, host_s.bins_table), (d.above_table, host_s.above_table), (d.below_table, host_s.below_table)):
        assert torch.equal(a.isnan(), b.isnan())
        a, b = a.nan_to_num(), b.nan_to_num()
        fraction, bias, rmse, mae = (abs(a[..., k] - b[..., k]) for k in range(4))
        assert (rmse <= REL * b[..., 2]).all() and (mae <= 2 * REL * b[..., 3]).all()
        assert (bias <= 2 * REL * b[..., 3]).all() and (fraction <= 2 * REL * b[..., 0]).all()


@pytest.mark.parametrize("by", ["truth", "pred"])
def test_front_end_equals_the_cpu_path_and_the_yardstick(by):
    """Surface and atmospheric variables; the history slice [:, -1] is passed as a view."""
    host = make_batches(17, 32, seed=41)
    dev = [b.to(DEV) for b in host]
    for maps in ((None, None), (2, 3), (2, None), (None, 3)):
        pick = lambda bs: {"centre": None if maps[0] is None else bs[2], "scale": None if maps[1] is None else bs[3]}  # noqa: E731
        unit = 1.0 if maps[1] is not None else 200.0
        edges = {k: np.asarray(v) * unit for k, v in EDGES.items()}
        s = conditional_scores(dev[0], dev[1], edges, by=by, **pick(dev))
        assert s.rmse["2t"].device == DEV and s.rmse["z"].shape == (2, 3, 5) and s.count_above["msl"].shape == (2, 4)
        assert_device_equals_host(s, conditional_scores(host[0], host[1], edges, by=by, **pick(host)))
        check_against_yardstick(s.cpu(), host[0], host[1], pick(host)["centre"], pick(host)["scale"], edges, by, f"front end {maps}")


def test_maps_with_batch_size_one_equal_the_repeated_form_bit_for_bit():
    pred, truth, centre, scale = (b.to(DEV) for b in make_batches(33, 64, seed=42))
    one = lambda b: Batch({k: v[:1] for k, v in b.surf_vars.items()}, {}, {k: v[:1] for k, v in b.atmos_vars.items()},  # noqa: E731
                          Metadata(b.metadata.lat, b.metadata.lon, b.metadata.time[:1], b.metadata.atmos_levels))
    twice = lambda b: Batch({k: v[:1].repeat(2, 1, 1, 1) for k, v in b.surf_vars.items()}, {},  # noqa: E731
                            {k: v[:1].repeat(2, 1, 1, 1, 1) for k, v in b.atmos_vars.items()}, b.metadata)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a = conditional_scores(pred, truth, EDGES, centre=one(centre), scale=one(scale))
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 33 * 64 * 4 * 5                # (repeating the maps would take 10 planes)
    b = conditional_scores(pred, truth, EDGES, centre=twice(centre), scale=twice(scale))
    assert torch.equal(a.sums_table, b.sums_table) and torch.equal(a.bins_table.nan_to_num(), b.bins_table.nan_to_num())
    assert not torch.equal(a.sums_table, conditional_scores(pred, truth, EDGES, centre=centre, scale=scale).sums_table)


def test_conditional_scores_are_capturable_in_a_hip_graph():
    pred, truth, centre, scale = (b.to(DEV) for b in make_batches(33, 64, seed=43))
    other_pred, other_truth, _, _ = (b.to(DEV) for b in make_batches(33, 64, seed=44))
    want_first = conditional_scores(pred, truth, EDGES, centre=centre, scale=scale).cpu()   # (also the warm call)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = conditional_scores(pred, truth, EDGES, centre=centre, scale=scale)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s.sums_table.cpu(), want_first.sums_table)
    for group in ("surf_vars", "atmos_vars"):                                    # new values in the static inputs, in place
        for k in getattr(pred, group):
            getattr(pred, group)[k].copy_(getattr(other_pred, group)[k])
            getattr(truth, group)[k].copy_(getattr(other_truth, group)[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = s.cpu()
    fresh = conditional_scores(pred, truth, EDGES, centre=centre, scale=scale).cpu()
    assert not torch.equal(replayed.sums_table, want_first.sums_table)
    for f in ("sums_table", "bins_table", "above_sums", "above_table", "below_sums", "below_table"):
        a, b = getattr(replayed, f), getattr(fresh, f)
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num()), f


def test_scoring_a_rollout_step_by_step_equals_the_host_path():
    case = CASES["small_b2"]
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    model.load_state_dict(helpers.case_state_dict(model, torch.float32), strict=True)
    model = model.to(DEV).eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
    truth = batch.crop(model.patch_size)
    truth_dev = truth.to(DEV)
    stats = FieldStats().update(truth_dev, over="batch")                         # climatology maps from the input, B = 1
    centre, scale = stats.as_batch("mean"), stats.as_batch("std", ddof=1)
    edges = {k: (-1.0, 0.0, 1.0) for k in list(truth.surf_vars)[:2] + list(truth.atmos_vars)[:1]}
    got, preds = [], []
    with torch.inference_mode():
        for pred in rollout(model, batch.to(DEV), steps=2):
            got.append(conditional_scores(pred, truth_dev, edges, centre=centre, scale=scale))   # nothing is read back
            preds.append(pred)
    assert len(got) == 2
    centre_h, scale_h = centre.to("cpu"), scale.to("cpu")
    for s, pred in zip(got, preds):
        assert_device_equals_host(s, conditional_scores(pred.to("cpu"), truth, edges, centre=centre_h, scale=scale_h))
    assert not torch.equal(got[0].sums_table, got[1].sums_table) and (got[0].sums_table[..., 0].sum(dim=1) > 0).all()


def test_device_path_argument_errors():
    pred, truth, centre, _ = make_batches(17, 32, seed=45)
    e = {"2t": (0.0,)}
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        conditional_scores(pred.to(DEV), truth, e)
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        conditional_scores(pred.to(DEV), truth.to(DEV), e, centre=centre)
    with pytest.raises(TypeError, match="float64"):
        conditional_scores(pred.to(DEV), truth.to(DEV).type(torch.float64), e)
    with pytest.raises(TypeError, match="float64"):
        conditional_scores(pred.to(DEV), truth.to(DEV), e, centre=centre.to(DEV).type(torch.float64))
    tr = truth.to(DEV)
    tr.surf_vars["2t"] = tr.surf_vars["2t"].transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match="contiguous"):
        conditional_scores(pred.to(DEV), tr, e)
