"""`aurora_amd.event_scores` on the device: one aurora_hip_event_scores call against the numpy integer yardstick of
tests/test_event_scores_host.py (`yardstick_rowsums`: explicit np.roll / shifted sums, checked there against a brute-force
loop and scipy's uniform_filter).

Every quantity is an integer, so every comparison is np.array_equal / torch.equal: there is no tolerance anywhere in this
file.  The float64 scores are compared with torch.equal too (NaN matching NaN): the finalisation is the same torch code on
exact inputs and its row reduction is a fixed tree of elementwise operations (aurora_amd/events.py), so it does not depend on
a device's reduction order.

Test fields are `red_noise` (mean 5e4, a k^-3 spectrum), so events cluster; thresholds are the data's own 0.5 / 0.9 / 0.99
quantiles, one above the maximum and one NaN (T = 5: the kernel's two-register form), or the quantiles and the NaN alone
(T = 4: its one-register form).

The kernel's tile is 256 - 2 h_max centre columns (h_max: half the largest window) by 128 centre rows:
`test_raw_tables_equal_the_yardstick[tile_and_segment_seams_*]` sits one above and one below both with h_max = 2 (252 columns).

The call needs no workspace, so the guard half of the workspace test is replaced by the assertion that
aurora_hip_event_scores_workspace_bytes is 0 and that the call runs with a NULL workspace."""
import ctypes
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, event_scores, rollout
from aurora_amd.engine import lib
from tests import helpers
from tests.golden_cases import CASES
from tests.test_event_scores_host import assert_equals_yardstick, thresholds_for, yardstick_rowsums
from tests.verification_inputs import DEV, carve, quantile_thresholds, red_noise, red_noise_batch, thresholds_of

pytestmark = pytest.mark.gpu


def check_raw(p, t, thr, scales, what, below=False, offset_floats=0, planes=None):
    """(n_planes, n_lat, n_lon) host arrays through lib.event_rowsums; the planes in `planes` (default: all) against the
    yardstick, exactly."""
    n_planes, n_lat, n_lon = p.shape
    pd, td = carve(p, offset_floats), carve(t, offset_floats)
    rowsums, valid = lib.event_rowsums([pd], [td], torch.from_numpy(thr).to(DEV), scales, below)
    assert rowsums.shape == (n_planes, thr.shape[1], len(scales), n_lat, 3) and rowsums.dtype == torch.int64
    assert valid.shape == (n_planes, n_lat) and valid.dtype == torch.int64 and rowsums.device == DEV
    rowsums, valid = rowsums.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(pd.cpu().numpy(), p, equal_nan=True) and np.array_equal(td.cpu().numpy(), t, equal_nan=True)
    for k in range(n_planes) if planes is None else planes:
        want, want_valid = yardstick_rowsums(p[k], t[k], thr[k], scales, below)
        assert np.array_equal(valid[k], want_valid), (what, k)
        bad = np.argwhere(rowsums[k] != want)
        assert bad.size == 0, (what, k, len(bad), bad[:5].tolist())
    return rowsums, valid


RAW_CASES = {
    "baseline": (3, 17, 32, (1, 3, 5), 5, False, 0),
    "odd_n_lon_whole_circle": (2, 9, 45, (1, 3, 45), 5, False, 0),
    "window_taller_than_plane_max_n": (2, 3, 64, (1, 9, 63), 5, False, 0),
    "one_row": (2, 1, 90, (1, 5), 5, False, 0),
    "one_column": (1, 40, 1, (1,), 5, False, 0),
    "quarter_degree": (2, 721, 1440, (1, 5, 9, 17, 33), 5, False, 0),
    "tenth_degree_row": (1, 17, 3600, (1, 33), 5, False, 0),
    "eight_scales_eight_thresholds": (2, 70, 257, (1, 3, 5, 7, 9, 11, 13, 63), 8, False, 0),
    "three_floats_past_16_bytes": (2, 33, 90, (1, 5, 9), 5, False, 3),
    "below": (2, 33, 90, (1, 5, 9), 5, True, 0),
    "tile_and_segment_seams_above": (1, 129, 253, (1, 5), 4, False, 0),
    "tile_and_segment_seams_below": (1, 127, 251, (1, 5), 4, False, 0),
    "one_register_form_two_tiles": (2, 40, 300, (1, 3, 33), 4, True, 1),
}


@pytest.mark.parametrize("case", RAW_CASES)
def test_raw_tables_equal_the_yardstick(case):
    n_planes, n_lat, n_lon, scales, T, below, offset = RAW_CASES[case]
    p = red_noise((n_planes, n_lat, n_lon), seed=n_lat + n_lon)
    t = red_noise((n_planes, n_lat, n_lon), seed=n_lat + n_lon + 1)
    if n_lon == 1:                                                      # (red noise needs a wavenumber: a column of its own)
        g = np.random.default_rng(7)
        p, t = (5e4 + 500 * g.standard_normal((n_planes, n_lat, 1))).astype(np.float32), (5e4 + 500 * g.standard_normal((n_planes, n_lat, 1))).astype(np.float32)
    rowsums, _ = check_raw(p, t, thresholds_of(t, T), scales, case, below, offset)
    assert rowsums[:, 0].any() and not rowsums[:, 3 if T == 4 else 4].any()   # events at the median; none at the NaN threshold


def test_invalid_points_as_on_the_host():
    """Single NaN / Inf at a tile corner and at both ends of a row (where the wrap applies), a block of invalid rows across the
    row-segment seam (between rows 127 and 128), a whole-NaN plane; the other planes keep their bits."""
    n_lat, n_lon, scales = 140, 300, (1, 5, 9)                          # h_max = 4: tiles of 248 columns, segments of 128 rows
    p, t = red_noise((4, n_lat, n_lon), seed=1), red_noise((4, n_lat, n_lon), seed=2)
    thr = thresholds_of(t, 5)
    base, base_valid = check_raw(p, t, thr, scales, "before masking")
    p[0, 0, 0] = np.nan
    p[0, 5, n_lon - 1] = np.inf
    t[0, 127, 247], t[0, 128, 248] = -np.inf, np.nan                    # the corner between four tiles / segments
    t[0, n_lat - 1, 0] = np.nan
    p[1, 125:132] = np.nan                                              # a block of rows straddling the segment seam
    t[2, 60, :] = np.inf
    got, valid = check_raw(p, t, thr, scales, "masked")
    assert valid[0].sum() == n_lat * n_lon - 5 and valid[1, 125:132].tolist() == [0] * 7 and valid[2, 60] == 0
    assert np.array_equal(got[3], base[3]) and np.array_equal(valid[3], base_valid[3])
    assert not np.array_equal(got[0], base[0]) and not got[1, :, :, 125:132].any()
    p[3] = np.nan                                                       # a whole-NaN plane: zeros, valid 0, FSS NaN
    again, valid = check_raw(p, t, thr, scales, "one plane all NaN")
    assert not again[3].any() and not valid[3].any() and np.array_equal(again[:3], got[:3])
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1, dtype=torch.float64)[:-1],
                  time=(datetime(2023, 1, 1, 6),), atmos_levels=())
    b = lambda a: Batch({"2t": carve(a[3][None, None])}, {}, {}, md)  # noqa: E731
    s = event_scores(b(p), b(t), {"2t": thr[3, :3]}, scales=scales).cpu()
    assert torch.isnan(s.fss["2t"]).all() and (s.count["2t"] == 0).all() and (s.hits["2t"] == 0).all()


def assert_same_scores(a, b):
    for f in ("rowsums_table", "valid_table", "counts_table"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    for f in ("fss_table", "rates_table"):                              # float64, NaN matching NaN: equal, not close
        assert np.array_equal(getattr(a, f).numpy(), getattr(b, f).numpy(), equal_nan=True), f


@pytest.mark.parametrize("n_lat,n_lon,scales,below", [(17, 32, (1, 3, 5), False), (33, 45, (3, 9), True), (130, 64, (1, 7, 63), False)])
def test_event_scores_of_a_batch_equal_the_cpu_path(n_lat, n_lon, scales, below):
    """Surface and atmospheric variables through event_scores() on device batches (history slices passed as views) against the
    same call on the host batches and against the yardstick.  Every table is equal; so is every float64 score, because the
    finalisation adds the rows in a fixed tree of elementwise operations on either device."""
    pred, truth = red_noise_batch(n_lat, n_lon, seed=3), red_noise_batch(n_lat, n_lon, seed=4)
    pred.surf_vars["2t"][1, -1, n_lat // 2, 0] = float("nan")
    thr = thresholds_for(pred, truth)
    host = event_scores(pred, truth, thr, scales=scales, below=below)
    dev = event_scores(pred.to(DEV), truth.to(DEV), thr, scales=scales, below=below)
    assert dev.fss["z"].device == DEV and dev.hits["2t"].device == DEV and dev.scales == host.scales
    assert dev.fss["z"].shape == (2, 3, 3, len(dev.scales)) and dev.csi["2t"].shape == (2, 3)
    assert_same_scores(dev.cpu(), host)
    assert_equals_yardstick(dev, pred, truth, thr, below)
    assert {k: v.tolist() for k, v in dev.cpu().count.items()} == {k: v.tolist() for k, v in host.count.items()}


def test_repeatable_independent_of_the_other_planes_and_of_alignment():
    n_lat, n_lon, scales = 70, 1440, (1, 5, 9, 17, 33)
    p, t = red_noise((7, n_lat, n_lon), seed=5), red_noise((7, n_lat, n_lon), seed=6)
    p[2, 5, 100] = np.nan
    thr = torch.from_numpy(thresholds_of(t, 4)).to(DEV)
    pd, td = carve(p), carve(t)
    po, to = carve(p, 1), carve(t, 1)                                # the same values one float (4 bytes) further on
    assert pd.data_ptr() % 16 == 0 and po.data_ptr() % 16 == 4
    whole, again = lib.event_rowsums([pd], [td], thr, scales), lib.event_rowsums([pd], [td], thr, scales)
    single = [lib.event_rowsums([pd[k:k + 1]], [td[k:k + 1]], thr[k:k + 1].contiguous(), scales) for k in range(7)]
    shifted = lib.event_rowsums([po], [to], thr, scales)
    torch.cuda.synchronize()
    for i in (0, 1):
        assert torch.equal(whole[i], again[i]), "two calls differ"
        assert torch.equal(whole[i], torch.cat([s[i] for s in single])), "a plane alone differs from the plane within seven"
        assert torch.equal(whole[i], shifted[i]), "pointer alignment changes the result"
    assert whole[1].sum(dim=1).tolist() == [n_lat * n_lon - (k == 2) for k in range(7)]
    want, _ = yardstick_rowsums(p[2], t[2], thr[2].cpu().numpy(), scales, False)
    assert np.array_equal(whole[0][2].cpu().numpy(), want)


def test_event_scores_are_capturable_in_a_hip_graph():
    pred, truth = (b.to(DEV) for b in (red_noise_batch(33, 64, seed=7), red_noise_batch(33, 64, seed=8)))
    other = red_noise_batch(33, 64, seed=9).to(DEV)
    thr = {"2t": [5e4, 5e4 + 50], "z": [5e4 - 20]}
    first = event_scores(pred, truth, thr, scales=(1, 5)).cpu()        # (the warm call: tables and weights are uploaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = event_scores(pred, truth, thr, scales=(1, 5))
    graph.replay()
    torch.cuda.synchronize()
    assert_same_scores(s.cpu(), first)
    for grp in ("surf_vars", "atmos_vars"):
        for k, v in getattr(pred, grp).items():
            v.copy_(getattr(other, grp)[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = s.cpu()
    assert not torch.equal(replayed.rowsums_table, first.rowsums_table)
    assert_same_scores(replayed, event_scores(pred, truth, thr, scales=(1, 5)).cpu())


def test_the_call_needs_no_workspace():
    """The design has no workspace: the size function is 0 for every argument and the C call runs with a NULL workspace of 0
    bytes; output tables that held 0xA5 bytes come back right (the call clears them itself) and their neighbours are
    untouched."""
    n, n_lat, n_lon, scales = 3, 45, 90, (1, 3, 9)
    p, t = red_noise((n, n_lat, n_lon), seed=10), red_noise((n, n_lat, n_lon), seed=11)
    thr = thresholds_of(t, 5)
    assert lib.event_scores_workspace_bytes(n, n_lat, n_lon, 5, 3) == 0 and lib.event_scores_workspace_bytes(69, 721, 1440, 8, 8) == 0
    pd, td, thr_d = carve(p), carve(t), torch.from_numpy(thr).to(DEV)
    want = lib.event_rowsums([pd], [td], thr_d, scales)
    n_rs, n_v, guard = n * 5 * 3 * n_lat * 3, n * n_lat, 1 << 13
    buf = torch.full(((n_rs + n_v + 2 * guard) * 8,), 0xA5, dtype=torch.uint8, device=DEV)
    words = buf.view(torch.int64)
    rs, vd = words[guard:guard + n_rs], words[guard + n_rs:guard + n_rs + n_v]
    ptrs = torch.tensor([x[k].data_ptr() for x in (pd, td) for k in range(n)], dtype=torch.int64).to(DEV)
    L = lib.load()
    sc = (ctypes.c_int32 * 3)(*scales)
    code = L.aurora_hip_event_scores(ptrs.data_ptr(), ptrs.data_ptr() + 8 * n, n, n_lat, n_lon, thr_d.data_ptr(), 5, sc, 3, 0,
                                     rs.data_ptr(), vd.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream)
    assert code == 0, L.aurora_hip_last_error()
    torch.cuda.synchronize()
    assert torch.equal(rs.view(n, 5, 3, n_lat, 3), want[0]) and torch.equal(vd.view(n, n_lat), want[1])
    assert (buf[:guard * 8] == 0xA5).all() and (buf[(guard + n_rs + n_v) * 8:] == 0xA5).all(), "the call wrote outside its tables"


def test_a_rollout_is_scored_step_by_step_and_read_once():
    case = CASES["small_b2"]
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    model.load_state_dict(helpers.case_state_dict(model, torch.float32), strict=True)
    model = model.to(DEV).eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
    truth = batch.crop(model.patch_size)
    truth_dev = truth.to(DEV)
    n_lon = truth.metadata.lon.shape[0]
    scales = tuple(n for n in (1, 3, 5) if n <= n_lon)
    thr = {k: quantile_thresholds(v[:, -1].numpy())[:2] for k, v in truth.surf_vars.items()}
    thr.update({k: quantile_thresholds(v[:, -1].numpy())[:1] for k, v in truth.atmos_vars.items()})
    got, preds = [], []
    with torch.inference_mode():
        for pred in rollout(model, batch.to(DEV), steps=3):
            got.append(event_scores(pred, truth_dev, thr, scales=scales))   # nothing is read back in the loop
            preds.append(pred)
    got = [s.cpu() for s in got]
    for s, pred in zip(got, preds):
        assert set(s.fss) == set(pred.surf_vars) | set(pred.atmos_vars)
        assert_equals_yardstick(s, pred, truth, thr)
        assert_same_scores(s, event_scores(pred.to("cpu"), truth, thr, scales=scales))
    assert not torch.equal(got[0].rowsums_table, got[1].rowsums_table)


def test_device_path_argument_errors():
    pred, truth = red_noise_batch(17, 32, seed=12), red_noise_batch(17, 32, seed=13)
    thr = {"2t": [5e4]}
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        event_scores(pred.to(DEV), truth, thr)
    with pytest.raises(TypeError, match="float64"):
        event_scores(pred.to(DEV).type(torch.float64), truth.to(DEV).type(torch.float64), thr)
    tr = truth.to(DEV)
    tr.surf_vars["2t"] = tr.surf_vars["2t"].transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match="contiguous"):
        event_scores(pred.to(DEV), tr, thr)
