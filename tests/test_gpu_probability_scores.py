"""`aurora_amd.probability_scores` on the device: one aurora_hip_probability_scores call against the numpy integer yardstick of
tests/test_probability_scores_host.py (`yardstick_rows`: one boolean mask per bin, checked there against a brute-force loop).

Every quantity is an integer, so every comparison is np.array_equal / torch.equal: there is no tolerance anywhere in this
file.  The float64 scores are compared with torch.equal too (NaN matching NaN): the finalisation is the same torch code on
exact inputs and every floating-point sum in it is a fixed tree of elementwise operations (aurora_amd/probability.py), so it
does not depend on a device's reduction order.

Inputs are those of the host file: truth y = `red_noise`, members x_m = fp32(y + red noise of amplitude 250); thresholds are
`thresholds_of` of tests/verification_inputs.py (T = 5: the data's 0.5 / 0.9 / 0.99 quantiles, one above the maximum, one NaN:
the kernel's two-register counter; T = 4: the quantiles and the NaN: its one-register counter; T = 8).  Every table test
asserts `assert_not_trivial` on its own input.

The kernel gives a wavefront a row and a 256-thread workgroup four consecutive rows; a lane takes four columns per step, by
one 16-byte load where n_lon % 4 == 0 and every plane pointer is 16-byte aligned and by four 4-byte loads otherwise; the
members are streamed four at a time."""
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, probability_scores, rollout
from aurora_amd.engine import lib
from tests import helpers
from tests.golden_cases import CASES
from tests.test_probability_scores_host import (assert_equals_yardstick, assert_not_trivial, assert_same_scores, make_ensemble,
                                                perturbed, thresholds_for, yardstick_rows)
from tests.verification_inputs import DEV, carve, quantile_thresholds, red_noise, thresholds_of

pytestmark = pytest.mark.gpu


def fields(n_planes, n_lat, n_lon, M, seed=None):
    """Truth (n_planes, n_lat, n_lon) and members (M, n_planes, n_lat, n_lon) of the module's text."""
    seed = n_lat + n_lon if seed is None else seed
    if n_lon == 1:                                                      # (red noise needs a wavenumber: a column of its own)
        y = (5e4 + 500 * np.random.default_rng(seed).standard_normal((n_planes, n_lat, 1))).astype(np.float32)
    else:
        y = red_noise((n_planes, n_lat, n_lon), seed=seed)
    return y, np.stack([perturbed(y, m) for m in range(M)])


def run(x, y, thr, below=False, offset_floats=0):
    """Host arrays through lib.probability_rows: the (n_planes, n_lat, T, 2, M + 1) table as numpy, and the device inputs."""
    xd, yd = carve(x, offset_floats), carve(y, offset_floats)
    rows = lib.probability_rows([[xd[m]] for m in range(x.shape[0])], [yd], torch.from_numpy(thr).to(DEV), below)
    assert rows.shape == (*y.shape[:2], thr.shape[1], 2, x.shape[0] + 1) and rows.dtype == torch.int32 and rows.device == DEV
    return rows.cpu().numpy(), xd, yd


def check_raw(x, y, thr, what, below=False, offset_floats=0):
    """The table of every plane against the yardstick, exactly; the inputs are left as they were."""
    rows, xd, yd = run(x, y, thr, below, offset_floats)
    assert np.array_equal(xd.cpu().numpy(), x, equal_nan=True) and np.array_equal(yd.cpu().numpy(), y, equal_nan=True)
    for k in range(y.shape[0]):
        bad = np.argwhere(rows[k] != yardstick_rows(x[:, k], y[k], thr[k], below))
        assert bad.size == 0, (what, k, len(bad), bad[:5].tolist())
    return rows, xd, yd


RAW_CASES = {   # n_planes, n_lat, n_lon, M, T, below, offset_floats
    "baseline": (3, 17, 32, 5, 5, False, 0),
    "rows_not_a_multiple_of_four_odd_n_lon_two_members": (2, 9, 45, 2, 5, False, 0),
    "one_row": (2, 1, 90, 16, 5, False, 0),
    "one_column": (1, 40, 1, 4, 5, False, 0),
    "n_lon_below_one_wave": (2, 6, 7, 3, 4, False, 0),
    "one_member_past_a_group_of_four_one_register_counter": (2, 33, 90, 17, 4, False, 0),
    "sixty_four_members_eight_thresholds": (1, 12, 130, 64, 8, False, 0),
    "fifty_one_members": (1, 20, 257, 51, 5, False, 0),
    "unaligned_planes": (2, 33, 90, 8, 5, False, 3),
    "below": (2, 33, 90, 5, 5, True, 0),
    "quarter_degree_rows": (2, 721, 1440, 4, 5, False, 0),
    "tenth_degree_row": (1, 17, 3600, 4, 5, False, 0),
}


@pytest.mark.parametrize("case", RAW_CASES)
def test_raw_tables_equal_the_yardstick(case):
    n_planes, n_lat, n_lon, M, T, below, offset = RAW_CASES[case]
    y, x = fields(n_planes, n_lat, n_lon, M)
    rows, xd, _ = check_raw(x, y, thresholds_of(y, T), case, below, offset)
    assert_not_trivial(rows, M)
    nan_slot = 3 if T == 4 else 4                                       # the NaN threshold: every point in bin (0, 0)
    assert rows[:, :, nan_slot, 0, 0].sum() == y.size and rows[:, :, nan_slot].sum() == y.size
    if T == 8:
        assert rows[..., 1, M].max() > 0 and rows[:, :, 5:].sum() == 3 * y.size           # counter bytes reach M = 64
    if offset:
        assert any(xd[m, k].data_ptr() % 16 for m in range(M) for k in range(n_planes))   # the 4-byte-load path


def test_the_vector_load_path_gives_the_integers_of_the_scalar_load_path():
    """The data of the `unaligned_planes` case with every row re-laid to 92 columns (two invalid points appended) on
    16-byte-aligned planes: the 16-byte-load path.  Equal to the yardstick on the re-laid data and, since invalid points
    count nowhere, to the table of the data as it was."""
    n_planes, n_lat, n_lon, M, T = 2, 33, 90, 8, 5
    y, x = fields(n_planes, n_lat, n_lon, M)
    thr = thresholds_of(y, T)
    y2 = np.concatenate([y, np.full((n_planes, n_lat, 2), np.nan, dtype=np.float32)], axis=-1)
    x2 = np.concatenate([x, x[..., :2]], axis=-1)
    rows, xd, yd = check_raw(x2, y2, thr, "re-laid", False, 0)
    assert all(t.data_ptr() % 16 == 0 for t in (*[xd[m, k] for m in range(M) for k in range(n_planes)], yd[0], yd[1]))
    assert_not_trivial(rows, M)
    for k in range(n_planes):
        assert np.array_equal(rows[k], yardstick_rows(x[:, k], y[k], thr[k], False))
    unaligned, _, _ = run(x, y, thr, False, 3)
    assert np.array_equal(rows, unaligned)


def test_invalid_points_as_on_the_host():
    """Single NaN / Inf at both ends of a row in member 0, in the last member and in truth, a block of invalid rows across a
    workgroup's four, a whole-NaN plane; the other planes keep their bits."""
    n_lat, n_lon, M = 21, 130, 6
    y, x = fields(4, n_lat, n_lon, M, seed=1)
    thr = thresholds_of(y, 5)
    base, _, _ = check_raw(x, y, thr, "before masking")
    assert_not_trivial(base, M)
    x[0, 0, 0, 0] = np.nan
    x[0, 0, 5, n_lon - 1] = np.inf
    x[M - 1, 0, 7, 0] = -np.inf
    x[M - 1, 0, 7, n_lon - 1] = np.nan
    y[0, n_lat - 1, 0], y[0, n_lat - 1, n_lon - 1] = np.nan, np.inf
    x[2, 1, 6:13] = np.nan                                               # rows 6..12 of plane 1: across three workgroups
    y[2, 10, :] = np.inf
    got, _, _ = check_raw(x, y, thr, "masked")
    valid = got[:, :, 0].sum(axis=(-1, -2))
    assert valid[0].sum() == n_lat * n_lon - 6 and valid[1, 6:13].tolist() == [0] * 7 and valid[2, 10] == 0
    assert valid[0, [0, 5, 7, n_lat - 1]].tolist() == [n_lon - 1, n_lon - 1, n_lon - 2, n_lon - 2]
    assert np.array_equal(got[3], base[3]) and not np.array_equal(got[0], base[0]) and not got[1, 6:13].any()
    y[3] = np.nan                                                        # a whole-NaN plane: zeros, count 0, NaN scores
    again, _, _ = check_raw(x, y, thr, "one plane all NaN")
    assert not again[3].any() and np.array_equal(again[:3], got[:3])
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1, dtype=torch.float64)[:-1],
                  time=(datetime(2023, 1, 1, 6),), atmos_levels=())
    b = lambda a: Batch({"2t": carve(a[3][None, None])}, {}, {}, md)  # noqa: E731
    s = probability_scores([b(x[m]) for m in range(M)], b(y), {"2t": thr[3, :3]}).cpu()
    assert torch.isnan(s.brier["2t"]).all() and torch.isnan(s.roc_area["2t"]).all() and torch.isnan(s.hit_rate["2t"]).all()
    assert (s.count["2t"] == 0).all() and (s.counts["2t"] == 0).all()


def test_repeatable_independent_of_the_other_planes_and_of_the_member_order():
    n_lat, n_lon, M = 70, 360, 7
    y, x = fields(3, n_lat, n_lon, M, seed=5)
    x[3, 1, 5, 100] = np.nan
    thr = thresholds_of(y, 4)
    thr_d = torch.from_numpy(thr).to(DEV)
    xd, yd = carve(x), carve(y)
    members = [[xd[m]] for m in range(M)]
    whole, again = lib.probability_rows(members, [yd], thr_d), lib.probability_rows(members, [yd], thr_d)
    single = [lib.probability_rows([[v[0][k:k + 1]] for v in members], [yd[k:k + 1]], thr_d[k:k + 1].contiguous()) for k in range(3)]
    shuffled = lib.probability_rows([members[i] for i in (4, 0, 6, 2, 1, 5, 3)], [yd], thr_d)
    torch.cuda.synchronize()
    assert torch.equal(whole, again), "two calls differ"
    assert torch.equal(whole, torch.cat(single)), "a plane alone differs from the plane within three"
    assert torch.equal(whole, shuffled), "the order of the members changes the result"
    assert np.array_equal(yd.cpu().numpy(), y) and np.array_equal(xd.cpu().numpy(), x, equal_nan=True), "an input was modified"
    assert whole[:, :, 0].sum(dim=(-1, -2, -3)).tolist() == [n_lat * n_lon - (k == 1) for k in range(3)]
    assert np.array_equal(whole[1].cpu().numpy(), yardstick_rows(x[:, 1], y[1], thr[1], False))
    assert_not_trivial(whole.cpu().numpy(), M)


@pytest.mark.parametrize("n_lat,n_lon,M,below", [(17, 32, 5, False), (33, 45, 2, True), (130, 64, 9, False)])
def test_probability_scores_of_batches_equal_the_cpu_path(n_lat, n_lon, M, below):
    """Surface and atmospheric variables through probability_scores() on device batches (history slices passed as views)
    against the same call on the host batches and against the yardstick.  Every table is equal; so is every float64 score,
    because the finalisation is the same code on exact integers and adds in fixed trees on either device."""
    members, truth = make_ensemble(n_lat, n_lon, M, seed=3)
    members[M - 1].surf_vars["2t"][1, -1, n_lat // 2, 0] = float("nan")
    thr = thresholds_for(truth)
    host = probability_scores(members, truth, thr, below=below)
    dev = probability_scores([b.to(DEV) for b in members], truth.to(DEV), thr, below=below)
    assert dev.brier["z"].device == DEV and dev.counts["2t"].device == DEV and dev.rows["z"].device == DEV
    assert dev.forecast_probability.device == DEV and dev.brier["z"].shape == (2, 3, 4) and dev.hit_rate["2t"].shape == (2, 4, M + 2)
    assert_same_scores(dev.cpu(), host)
    assert_equals_yardstick(dev, members, truth, thr, below)
    assert_not_trivial(dev.cpu().rows["2t"].numpy(), M)
    for prop in ("brier", "fair_brier", "brier_skill", "reliability", "resolution", "uncertainty", "base_rate", "roc_area",
                 "observed_frequency", "forecast_weight", "hit_rate", "false_alarm_rate", "counts", "count", "rows"):
        for k, v in getattr(dev.cpu(), prop).items():
            assert np.array_equal(v.numpy(), getattr(host, prop)[k].numpy(), equal_nan=True), (prop, k)


def test_one_batch_of_members_on_the_device_equals_the_sequence_form_and_the_cpu_path():
    members, truth = make_ensemble(33, 64, 6, seed=4, B=1)
    cat = lambda grp: {k: torch.cat([getattr(b, grp)[k] for b in members]) for k in getattr(truth, grp)}  # noqa: E731
    md = truth.metadata
    one = Batch(cat("surf_vars"), truth.static_vars, cat("atmos_vars"),
                Metadata(lat=md.lat, lon=md.lon, time=md.time * 6, atmos_levels=md.atmos_levels))
    thr = thresholds_for(truth)
    host = probability_scores(one, truth, thr)
    dev_one = probability_scores(one.to(DEV), truth.to(DEV), thr).cpu()
    dev_seq = probability_scores([b.to(DEV) for b in members], truth.to(DEV), thr).cpu()
    assert dev_one.members == 6 and dev_one.brier["z"].shape == (1, 3, 4)
    assert_same_scores(dev_one, host)
    assert_same_scores(dev_seq, host)


def test_probability_scores_are_capturable_in_a_hip_graph():
    """One warm call, then capture and replay on one stream: torch.cuda.graph captures the current stream only, and a call
    that put work on a side stream without joining it would fail the capture.  The replay on changed values in the same
    buffers equals a fresh eager call."""
    members, truth = make_ensemble(33, 64, 3, seed=7)
    members, truth = [b.to(DEV) for b in members], truth.to(DEV)
    other, _ = make_ensemble(33, 64, 3, seed=9)
    thr = {"2t": [5e4, 5e4 + 50], "z": [5e4 - 20]}
    first = probability_scores(members, truth, thr).cpu()              # (the warm call: tables and weights are uploaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = probability_scores(members, truth, thr)
    graph.replay()
    torch.cuda.synchronize()
    assert_same_scores(s.cpu(), first)
    for b, o in zip(members, other):
        for grp in ("surf_vars", "atmos_vars"):
            for k, v in getattr(b, grp).items():
                v.copy_(getattr(o, grp)[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = s.cpu()
    assert not torch.equal(replayed.rows_table, first.rows_table)
    assert_same_scores(replayed, probability_scores(members, truth, thr).cpu())


def test_the_batch_elements_of_a_rollout_are_scored_as_members():
    """A golden-case geometry: the two batch elements of a roll-out's prediction as ONE Batch of members against the first
    element of the cropped input as truth, step by step, read once at the end."""
    case = CASES["small_b2"]
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    model.load_state_dict(helpers.case_state_dict(model, torch.float32), strict=True)
    model = model.to(DEV).eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
    cropped = batch.crop(model.patch_size)
    md = cropped.metadata
    truth = Batch({k: v[:1] for k, v in cropped.surf_vars.items()}, cropped.static_vars, {k: v[:1] for k, v in cropped.atmos_vars.items()},
                  Metadata(lat=md.lat, lon=md.lon, time=md.time[:1], atmos_levels=md.atmos_levels))
    truth_dev = truth.to(DEV)
    thr = {k: quantile_thresholds(v[:, -1].numpy())[:2] for k, v in truth.surf_vars.items()}
    thr.update({k: quantile_thresholds(v[:, -1].numpy())[:1] for k, v in truth.atmos_vars.items()})
    got, preds = [], []
    with torch.inference_mode():
        for pred in rollout(model, batch.to(DEV), steps=2):
            got.append(probability_scores(pred, truth_dev, thr))        # nothing is read back in the loop
            preds.append(pred)
    got = [s.cpu() for s in got]
    for s, pred in zip(got, preds):
        assert s.members == 2 and set(s.brier) == set(pred.surf_vars) | set(pred.atmos_vars)
        host = pred.to("cpu")
        assert_same_scores(s, probability_scores(host, truth, thr))
        split = [Batch({k: v[m:m + 1] for k, v in host.surf_vars.items()}, host.static_vars,
                       {k: v[m:m + 1] for k, v in host.atmos_vars.items()}, truth.metadata) for m in range(2)]
        assert_equals_yardstick(s, split, truth, thr)
    assert not torch.equal(got[0].rows_table, got[1].rows_table)


def test_device_path_argument_errors():
    members, truth = make_ensemble(17, 32, 2, seed=12)
    thr = {"2t": [5e4]}
    dev = [b.to(DEV) for b in members]
    with pytest.raises(ValueError, match="probability_scores: .*(cpu.*cuda|cuda.*cpu)"):
        probability_scores(dev, truth, thr)
    with pytest.raises(ValueError, match="probability_scores: .*(cpu.*cuda|cuda.*cpu)"):
        probability_scores([dev[0], members[1]], truth.to(DEV), thr)
    with pytest.raises(TypeError, match="probability_scores: .*float64"):
        probability_scores([b.type(torch.float64) for b in dev], truth.to(DEV).type(torch.float64), thr)
    tr = truth.to(DEV)
    tr.surf_vars["2t"] = tr.surf_vars["2t"].transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match="probability_scores: .*contiguous"):
        probability_scores(dev, tr, thr)
