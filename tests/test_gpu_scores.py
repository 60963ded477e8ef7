"""`aurora_amd.scores` on the device: one aurora_hip_scores call against a numpy fp64 yardstick written in the tests.

Yardstick: `tests.test_scores_host.yardstick_sums` -- the table of include/aurora_hip.h in numpy fp64, not
`aurora_amd.scores._sums_host` (code under test, checked against the same yardstick in tests/test_scores_host.py).

Bound (derived, not tuned): a sum of N fp64 terms in any order is within N 2^-53 sum|term| of the exact sum, and both sides
carry that, so with N = 721 x 1440 (2 N 2^-53 = 2.3e-10) the nonnegative slots 1, 3, 4, 6, 7 must agree to 1e-9 relative,
the signed slots 2 and 5 to 1e-9 x the sum of their absolute terms (slot 4 bounds slot 2, sqrt(S6 S7) bounds slot 5), and
slot 0 exactly.  The terms themselves differ by a few 2^-53 relative (the kernel fuses some multiply-adds), far inside.
Every plane of every case is compared.

Finalised scores inherit it: rmse = sqrt(S3 / S1) to 1e-9 relative (two 1e-9 ratios under a square root), mae to 2e-9
relative, bias to 2e-9 x mae absolute (|S2 error| <= 1e-9 S4, and S1's 1e-9 acts on |bias| <= mae), acc to 3e-9 absolute
(numerator 1e-9 of the denominator, denominator 1e-9 relative with |acc| <= 1, and the roundings of the division)."""
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, rollout, scores
from aurora_amd.engine import lib
from aurora_amd.scores import latitude_weights
from tests import helpers
from tests.golden_cases import CASES
from tests.test_scores_host import yardstick_sums
from tests.verification_inputs import DEV, carve, cos_weights, randn_batch, weights

pytestmark = pytest.mark.gpu
REL = 1e-9


def fields(n_planes, n_lat, n_lon, seed, offset_floats=0):
    """Seeded pressure-like data, d small against p: p = 101325 + 300 randn, t = p + 2 randn + 0.5, c = 101325 + 100 randn,
    each carved `offset_floats` past the start of its buffer."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(n_planes, n_lat, n_lon, generator=g, dtype=torch.float64)  # noqa: E731
    p = 101325 + 300 * r()
    return [carve(v, offset_floats) for v in (p, p + 2 * r() + 0.5, 101325 + 100 * r())]


def assert_sums_match(got: np.ndarray, want: np.ndarray, what: str):
    """got / want: (8,) sums of one plane, the bound of the module's text."""
    print(f"{what}: got {got.tolist()} want {want.tolist()}")
    assert got[0] == want[0], (what, "count", got[0], want[0])
    for s in (1, 3, 4, 6, 7):
        assert abs(got[s] - want[s]) <= REL * want[s], (what, s, got[s], want[s])
    assert abs(got[2] - want[2]) <= REL * want[4], (what, 2, got[2], want[2])
    assert abs(got[5] - want[5]) <= REL * np.sqrt(want[6] * want[7]), (what, 5, got[5], want[5])


def check_raw(p, t, c, n_lat, what):
    w = weights(n_lat)
    w_dev = torch.from_numpy(w).to(DEV)
    for clim in (None, c):
        keep = [x.clone() for x in (p, t, c)]
        got = lib.scores_sums([p], [t], None if clim is None else [clim], w_dev)
        assert got.shape == (p.shape[0], 8) and got.dtype == torch.float64 and got.device == DEV
        got = got.cpu().numpy()
        for x, k in zip((p, t, c), keep):
            assert torch.equal(x, k) or (torch.equal(x.isnan(), k.isnan()) and torch.equal(x.nan_to_num(), k.nan_to_num()))
        for k in range(p.shape[0]):
            want = yardstick_sums(p[k].cpu().numpy(), t[k].cpu().numpy(), None if clim is None else clim[k].cpu().numpy(), w)
            assert_sums_match(got[k], want, f"{what} clim={clim is not None} plane {k}")
        if clim is None:
            assert (got[:, 5:] == 0).all()


@pytest.mark.parametrize("n_planes,n_lat,n_lon,offset", [
    (4, 17, 32, 0),         # the toy batch
    (3, 721, 1440, 0),      # 0.25 degrees
    (5, 33, 61, 0),         # odd n_lon: rows are not 16-byte aligned, a partial last quad
    (3, 33, 64, 1),         # planes one float past a 16-byte boundary
    (3, 720, 1440, 3),      # the cropped grid, unaligned
    (2, 1, 37, 0), (2, 19, 1, 0), (1, 1, 1, 0),
])
def test_raw_sums_equal_the_yardstick(n_planes, n_lat, n_lon, offset):
    p, t, c = fields(n_planes, n_lat, n_lon, seed=n_lat + n_lon, offset_floats=offset)
    if offset:
        assert p.data_ptr() % 16 != 0
    check_raw(p, t, c, n_lat, f"{n_planes}x{n_lat}x{n_lon}+{offset}")


def test_alignment_does_not_change_a_single_bit():
    """The same values behind aligned and unaligned plane pointers: the 16-byte and the 4-byte path add the same elements in
    the same order."""
    w = torch.from_numpy(weights(33)).to(DEV)
    a = fields(3, 33, 64, seed=5)
    b = fields(3, 33, 64, seed=5, offset_floats=1)
    assert a[0].data_ptr() % 16 == 0 and b[0].data_ptr() % 16 == 4 and torch.equal(a[1], b[1])
    assert torch.equal(lib.scores_sums([a[0]], [a[1]], [a[2]], w), lib.scores_sums([b[0]], [b[1]], [b[2]], w))


def test_nan_land_mask_and_stray_nans_count_exactly():
    """The wave model's pattern: NaN over one land mask in pred and truth alike, plus stray NaNs in one of them; a plane
    that is NaN everywhere gives count 0 and zero sums."""
    n_lat, n_lon = 73, 144
    p, t, c = fields(4, n_lat, n_lon, seed=21)
    g = torch.Generator().manual_seed(22)
    land = (torch.rand(n_lat, n_lon, generator=g) < 0.3).to(DEV)
    p[:, land] = float("nan")
    t[:, land] = float("nan")
    sea = (~land).nonzero()
    for k, (where, n) in enumerate(((p, 5), (t, 7), (c, 3))):
        for i, j in sea[10 * k: 10 * k + n].tolist():
            where[k, i, j] = float("nan") if k != 1 else float("inf")
    p[3] = float("nan")
    n_sea = int((~land).sum())
    w = torch.from_numpy(weights(n_lat)).to(DEV)
    with_clim = lib.scores_sums([p], [t], [c], w).cpu().numpy()
    without = lib.scores_sums([p], [t], None, w).cpu().numpy()
    assert with_clim[:, 0].tolist() == [n_sea - 5, n_sea - 7, n_sea - 3, 0]
    assert without[:, 0].tolist() == [n_sea - 5, n_sea - 7, n_sea, 0]
    assert (with_clim[3] == 0).all() and (without[3] == 0).all()
    check_raw(p, t, c, n_lat, "land mask")


def batches(n_lat, n_lon, seed, B=2, levels=(100, 500, 850)):
    truth = randn_batch(n_lat, n_lon, seed=seed, B=B, offset=280.0, scale=15.0, levels=levels)
    err = randn_batch(n_lat, n_lon, seed=seed + 1, B=B, offset=0.3, scale=1.5, levels=levels)
    clim = randn_batch(n_lat, n_lon, seed=seed + 2, B=B, offset=280.0, scale=5.0, levels=levels)
    pred = Batch({k: v + err.surf_vars[k] for k, v in truth.surf_vars.items()}, truth.static_vars,
                 {k: v + err.atmos_vars[k] for k, v in truth.atmos_vars.items()}, truth.metadata)
    return pred, truth, clim


def assert_scores_match_yardstick(s, pred, truth, clim, what):
    """Finalised scores of every plane against the yardstick's sums (bounds: the module's text)."""
    s = s.cpu()
    w = cos_weights(pred.metadata.lat.double().cpu().numpy())
    n = 0
    for grp in ("surf_vars", "atmos_vars"):
        for k, v in getattr(pred, grp).items():
            pk, tk = v[:, -1].cpu().numpy(), getattr(truth, grp)[k][:, -1].cpu().numpy()
            ck = None if clim is None else getattr(clim, grp)[k][:, -1].cpu().numpy()
            lead = pk.shape[:-2]
            assert tuple(s.rmse[k].shape) == lead
            for idx in np.ndindex(*lead):
                y = yardstick_sums(pk[idx], tk[idx], None if ck is None else ck[idx], w)
                assert_sums_match(s.sums[k][idx].numpy(), y, f"{what} {k}{idx}")
                rmse, bias, mae = np.sqrt(y[3] / y[1]), y[2] / y[1], y[4] / y[1]
                assert int(s.count[k][idx]) == y[0]
                assert abs(float(s.rmse[k][idx]) - rmse) <= REL * rmse, (what, k, idx)
                assert abs(float(s.mae[k][idx]) - mae) <= 2 * REL * mae, (what, k, idx)
                assert abs(float(s.bias[k][idx]) - bias) <= 2 * REL * mae, (what, k, idx)
                if ck is not None:
                    assert abs(float(s.acc[k][idx]) - y[5] / np.sqrt(y[6] * y[7])) <= 3 * REL, (what, k, idx)
                n += 1
    assert n == s.table.shape[0]


@pytest.mark.parametrize("n_lat,n_lon", [(17, 32), (33, 61)])
def test_scores_of_a_batch_equal_the_yardstick(n_lat, n_lon):
    pred, truth, clim = batches(n_lat, n_lon, seed=30)
    for c in (None, clim):
        s = scores(pred.to(DEV), truth.to(DEV), None if c is None else c.to(DEV))
        assert s.rmse["2t"].device == DEV and s.rmse["2t"].dtype == torch.float64 and (s.acc is None) == (c is None)
        assert_scores_match_yardstick(s, pred, truth, c, f"{n_lat}x{n_lon}")


def test_scores_at_a_quarter_degree_equal_the_yardstick():
    """721 x 1440, B = 1, one surface variable and a two-level one; the history slice [:, -1] is passed as a view."""
    md = Metadata(lat=torch.linspace(90, -90, 721, dtype=torch.float64), lon=torch.linspace(0, 360, 1441)[:-1],
                  time=(datetime(2023, 1, 1, 6),), atmos_levels=(500, 850))
    p, t, c = fields(6, 721, 1440, seed=40)
    mk = lambda x: Batch({"msl": x[:2].view(1, 2, 721, 1440)}, {}, {"z": x[2:].view(1, 2, 2, 721, 1440)}, md)  # noqa: E731
    pred, truth, clim = mk(p), mk(t), mk(c)
    s = scores(pred, truth, clim)
    assert s.rmse["msl"].shape == (1,) and s.rmse["z"].shape == (1, 2)
    assert_scores_match_yardstick(s, pred, truth, clim, "0.25 degrees")


def test_repeatable_bit_for_bit_and_independent_of_the_other_planes():
    """Two calls give identical sums; a 69-plane 0.25-degree batch gives, plane for plane, what its planes give one at a
    time (the reduction tree of a plane does not depend on how many planes ride along)."""
    n = 69
    g = torch.Generator(device=DEV).manual_seed(50)
    p = 101325 + 300 * torch.randn(n, 721, 1440, device=DEV, generator=g)
    t = p + 2 * torch.randn(n, 721, 1440, device=DEV, generator=g)
    c = 101325 + 100 * torch.randn(n, 721, 1440, device=DEV, generator=g)
    p[7, 100:200, 300:500] = float("nan")
    w = torch.from_numpy(weights(721)).to(DEV)
    for clim in (None, c):
        args = lambda sl=slice(None): ([p[sl]], [t[sl]], None if clim is None else [clim[sl]], w)  # noqa: E731
        whole = lib.scores_sums(*args())
        again = lib.scores_sums(*args())
        single = torch.cat([lib.scores_sums(*args(slice(k, k + 1))) for k in range(n)])
        torch.cuda.synchronize()
        assert torch.equal(whole, again)
        assert torch.equal(whole, single)
        assert whole[7, 0] == 721 * 1440 - 100 * 200 and (whole[:7, 0] == 721 * 1440).all()


def test_scores_are_capturable_in_a_hip_graph():
    pred, truth, clim = (b.to(DEV) for b in batches(33, 64, seed=60))
    other_pred, other_truth, _ = (b.to(DEV) for b in batches(33, 64, seed=70))
    want_first = scores(pred, truth, clim).cpu()                   # (also the warm call: tables and weights are uploaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = scores(pred, truth, clim)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s.table.cpu(), want_first.table)
    for k in pred.surf_vars:                                       # new values in the static inputs, in place
        pred.surf_vars[k].copy_(other_pred.surf_vars[k])
        truth.surf_vars[k].copy_(other_truth.surf_vars[k])
    for k in pred.atmos_vars:
        pred.atmos_vars[k].copy_(other_pred.atmos_vars[k])
        truth.atmos_vars[k].copy_(other_truth.atmos_vars[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = s.table.cpu()
    assert not torch.equal(replayed, want_first.table)
    assert torch.equal(replayed, scores(pred, truth, clim).table.cpu())
    assert_scores_match_yardstick(s, pred, truth, clim, "replay")


def test_a_cold_call_during_capture_is_refused(monkeypatch):
    """A capture cannot replay the upload of the plane-pointer table, so a call on tensors no earlier call has seen must
    refuse while the stream is capturing (checked with the capture query patched: nothing is captured here)."""
    pred, truth, _ = (b.to(DEV) for b in batches(17, 32, seed=80))
    w = torch.from_numpy(weights(17)).to(DEV)
    p, t = pred.surf_vars["2t"].clone(), truth.surf_vars["2t"].clone()     # addresses no call has seen
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before capturing"):
        lib.scores_sums([p], [t], None, w)


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
    got, preds = [], []
    with torch.inference_mode():
        for pred in rollout(model, batch.to(DEV), steps=3):
            got.append(scores(pred, truth_dev, truth_dev))         # nothing is read back in the loop
            preds.append(pred)
    got = [s.cpu() for s in got]
    assert len(got) == 3
    for s, pred in zip(got, preds):
        host = scores(pred.to("cpu"), truth, truth)
        assert list(s.rmse) == list(host.rmse) and set(s.rmse) == set(pred.surf_vars) | set(pred.atmos_vars)
        assert torch.equal(s.table[:, 0], host.table[:, 0])
        # both sides within the module's bound of the exact sums -> the finalised columns within twice that
        for col, name in ((8, "rmse"), (10, "mae")):
            np.testing.assert_allclose(s.table[:, col], host.table[:, col], rtol=4 * REL, atol=0, err_msg=name)
        assert (abs(s.table[:, 9] - host.table[:, 9]) <= 4 * REL * host.table[:, 10]).all()
        assert torch.isnan(s.table[:, 11]).all() and torch.isnan(host.table[:, 11]).all()    # truth as its own climatology
    assert not torch.equal(got[0].table, got[1].table)


def test_a_warm_call_allocates_less_than_a_plane_and_does_not_synchronise():
    n_lat, n_lon = 721, 1440
    p, t, c = fields(8, n_lat, n_lon, seed=90)
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1)[:-1],
                  time=(datetime(2023, 1, 1, 6),), atmos_levels=(1, 2, 3, 4, 5, 6))
    mk = lambda x: Batch({"2t": x[:2].view(1, 2, n_lat, n_lon)}, {}, {"z": x[2:].view(1, 1, 6, n_lat, n_lon)}, md)  # noqa: E731
    pred, truth, clim = mk(p), mk(t), mk(c)
    before = [x.clone() for x in (p, t, c)]
    scores(pred, truth, clim)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s = scores(pred, truth, clim)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"a warm scores() call of 7 planes: peak allocation grows by {grown} bytes (one plane: {n_lat * n_lon * 4})")
    assert grown < n_lat * n_lon * 4
    for x, k in zip((p, t, c), before):
        assert torch.equal(x, k)
    assert s.count["z"].shape == (1, 6)


def test_device_path_argument_errors():
    pred, truth, _ = batches(17, 32, seed=100)
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        scores(pred.to(DEV), truth)
    with pytest.raises(TypeError, match="float64"):
        scores(pred.to(DEV).type(torch.float64), truth.to(DEV).type(torch.float64))
    with pytest.raises(TypeError, match="float64"):
        scores(pred.to(DEV), truth.to(DEV).type(torch.float64))
    tr = truth.to(DEV)
    tr.surf_vars["2t"] = tr.surf_vars["2t"].transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match="contiguous"):
        scores(pred.to(DEV), tr)
    np.testing.assert_allclose(latitude_weights(np.linspace(90, -90, 17)), weights(17), rtol=1e-14, atol=1e-18)
