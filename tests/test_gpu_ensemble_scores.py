"""`aurora_amd.ensemble_scores` on the device: one aurora_hip_ensemble_scores call against a numpy fp64 yardstick written
in the tests.

Yardstick: `tests.test_ensemble_scores_host.yardstick_ensemble` -- the table of include/aurora_hip.h in numpy fp64 with the
PAIRWISE form of g, not `aurora_amd.ensemble._ensemble_sums_host` (code under test, checked against the same yardstick in
tests/test_ensemble_scores_host.py).

Bound (derived, not tuned).  The count, the histogram and the ties: exactly.  A sum of N fp64 terms in any order is within
N 2^-53 sum|term| of the exact sum, both sides carry that, and with N <= 721 x 1440 (2 N 2^-53 = 2.3e-10) the project's
figure is REL = 1e-9 (tests/test_gpu_scores.py).  The per-point terms differ between kernel and yardstick by a few
M^2 2^-53 <= 5e-13 of a (the sorted against the pairwise form of g, 1 / M as a factor instead of a divisor, fused
multiply-adds), or of q = (sum_m d_m^2) / M for the squared terms: far inside.  With |e| <= a, g <= 2 a, e^2 <= q and
v <= 2 q (M >= 2), and Q = sum w q from the yardstick:
    S1, S5 to REL relative;  S2, S4 to REL S5;  S6 to REL 2 S5;  S3 to REL Q;  S7 to REL 2 Q.
Every plane of every case is compared.  The data make the bound bite: members = truth + 0.5 + 2 randn on a pressure-like
101325 +- 300 field in fp32, so that sums of raw values (1e5 against differences of 2: five digits, 1e-11 x 1e5 / 2 of
them lost at 2^-53 -- and all of them in fp32) or an fp32 accumulator (2^-24 = 6e-8 per term) miss it by orders of magnitude.

Finalised scores inherit it (a_bar = S5 / S1, q_bar = Q / S1): bias and mae to 2 REL a_bar absolute (the numerator to
REL S5, and S1's REL acting on a value <= a_bar); crps = (S5 - S6 / 2) / S1 to 4 REL a_bar (S5 to REL S5, S6 / 2 to REL S5,
and S1's REL on a value <= 2 a_bar); fair_crps to 6 REL a_bar (the factor M / (M - 1) <= 2 on the S6 term); rmse and
spread through the square root: u = S3 / S1 is known to du = 2 REL q_bar (u <= q_bar) and u = S7 / S1 to du = 4 REL q_bar
(u <= 2 q_bar), and |sqrt(u') - sqrt(u)| <= min(sqrt(du), du / sqrt(u)).
(`assert_ensemble_sums_match` and `assert_finalised_match` of tests/test_ensemble_scores_host.py hold these.)"""
from datetime import datetime

import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, ensemble_scores, rollout
from aurora_amd.engine import lib
from tests import helpers
from tests.golden_cases import CASES
from tests.test_ensemble_scores_host import (REL, assert_batch_matches_yardstick, assert_ensemble_sums_match, lagged,
                                             pressure_ensemble, yardstick_ensemble)
from tests.verification_inputs import DEV, carve, weights

pytestmark = pytest.mark.gpu


def check_raw(x, t, what, offset=0):
    """x (M, n_planes, n_lat, n_lon), t (n_planes, n_lat, n_lon) on the host: one call, every plane against the yardstick."""
    M, n_planes, n_lat, _ = x.shape
    w = weights(n_lat)
    xd, td = [carve(x[m], offset) for m in range(M)], carve(t, offset)
    if offset and x.shape[-1] % 4 == 0:
        assert td.data_ptr() % 16 != 0
    sums, hist = lib.ensemble_scores_sums([[v] for v in xd], [td], torch.from_numpy(w).to(DEV))
    assert sums.shape == (n_planes, 8) and sums.dtype == torch.float64 and sums.device == DEV
    assert hist.shape == (n_planes, M + 2) and hist.dtype == torch.int64 and hist.device == DEV
    sums, hist = sums.cpu().numpy(), hist.cpu().numpy()
    for m in range(M):                                            # the inputs are not modified
        assert torch.equal(xd[m].cpu().nan_to_num(1.5, 2.5, 3.5), x[m].nan_to_num(1.5, 2.5, 3.5))
    for k in range(n_planes):
        want = yardstick_ensemble(x[:, k].numpy(), t[k].numpy(), w)
        assert_ensemble_sums_match(sums[k], hist[k], want, f"{what} plane {k}")
    return sums, hist


GRIDS = [
    (2, 17, 32, 0),         # the toy batch
    (3, 33, 61, 0),         # odd n_lon: rows are not 16-byte aligned, a partial last quad, a partial last wave
    (2, 33, 64, 1),         # planes one float past a 16-byte boundary
    (2, 1, 37, 0),          # one row
    (1, 19, 1, 0),          # one column
]


@pytest.mark.parametrize("M", (2, 3, 4, 8, 12, 16, 17, 32, 51, 64))       # every bucket full and padded
@pytest.mark.parametrize("n_planes,n_lat,n_lon,offset", GRIDS)
def test_raw_sums_equal_the_yardstick(M, n_planes, n_lat, n_lon, offset):
    x, t = pressure_ensemble(M, n_planes, n_lat, n_lon, seed=100 * M + n_lat + n_lon)
    check_raw(x, t, f"M={M} {n_planes}x{n_lat}x{n_lon}+{offset}", offset)


@pytest.mark.parametrize("M,offset", [(2, 0), (3, 3), (8, 0), (17, 0), (51, 0), (64, 1)])
def test_raw_sums_at_a_quarter_degree_equal_the_yardstick(M, offset):
    """721 x 1440 (N at the limit REL was derived for); with an offset the cropped 720-row grid, unaligned.  Two planes for
    the small ensembles, one for the large ones (the yardstick's pairwise g takes M^2 passes over a plane on the host)."""
    n_lat, n_planes = 720 if offset else 721, 2 if M <= 8 else 1
    x, t = pressure_ensemble(M, n_planes, n_lat, 1440, seed=7 * M)
    check_raw(x, t, f"M={M} {n_planes}x{n_lat}x1440+{offset}", offset)


def test_alignment_does_not_change_a_single_bit():
    """The same values behind aligned and unaligned plane pointers (the buckets with 16-byte loads, and one without)."""
    w = torch.from_numpy(weights(33)).to(DEV)
    for M in (3, 8, 13, 40):
        x, t = pressure_ensemble(M, 3, 33, 64, seed=5 + M)
        a = lib.ensemble_scores_sums([[carve(x[m])] for m in range(M)], [carve(t)], w)
        xb, tb = [carve(x[m], 1) for m in range(M)], carve(t, 1)
        assert tb.data_ptr() % 16 == 4
        b = lib.ensemble_scores_sums([[v] for v in xb], [tb], w)
        # one member unaligned is enough to leave the 16-byte path
        c = lib.ensemble_scores_sums([[carve(x[m], int(m == M - 1))] for m in range(M)], [carve(t)], w)
        for other in (b, c):
            assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1]), M


@pytest.mark.parametrize("M", (3, 11, 33))
def test_nan_land_mask_and_stray_nans_count_exactly(M):
    """The wave model's pattern: NaN over one land mask in every member and in truth, plus stray NaN / inf in single
    members and in truth; a plane that is NaN everywhere in one member gives zeros throughout."""
    n_lat, n_lon = 73, 144
    x, t = pressure_ensemble(M, 4, n_lat, n_lon, seed=21 + M)
    g = torch.Generator().manual_seed(22)
    land = torch.rand(n_lat, n_lon, generator=g) < 0.3
    x[:, :, land] = float("nan")
    t[:, land] = float("nan")
    sea = (~land).nonzero()
    for i, j in sea[:5].tolist():
        x[0, 0, i, j] = float("nan")
    for i, j in sea[10:17].tolist():
        x[M - 1, 1, i, j] = float("inf")
    for i, j in sea[14:20].tolist():                              # (three of them the points above)
        x[1, 1, i, j] = float("-inf")
    for i, j in sea[30:33].tolist():
        t[2, i, j] = float("nan")
    x[M // 2, 3] = float("nan")
    n_sea = int((~land).sum())
    sums, hist = check_raw(x, t, f"land mask M={M}")
    assert sums[:, 0].tolist() == [n_sea - 5, n_sea - 10, n_sea - 3, 0]
    assert (sums[3] == 0).all() and (hist[3] == 0).all()
    assert hist[:, :M + 1].sum(axis=1).tolist() == sums[:, 0].tolist()


def test_ties_and_bounded_variables():
    """A variable clamped at zero: members and truth sit on the bound together, counted as ties and ranked by `<`."""
    M = 9
    x, t = pressure_ensemble(M, 2, 33, 61, seed=77)
    x, t = (x - 101325.0).clamp(min=0.0) / 100, (t - 101325.0).clamp(min=0.0) / 100
    sums, hist = check_raw(x, t, "clamped")
    assert (hist[:, M + 1] > 100).all() and (hist[:, 0] > hist[:, 1]).all()


@pytest.mark.parametrize("M", (5, 20))
def test_scores_of_batches_equal_the_yardstick_and_the_host_path(M):
    members, truth = lagged(M, n_lat=33, n_lon=61, seed=30)
    s = ensemble_scores([b.to(DEV) for b in members], truth.to(DEV))
    assert s.crps["2t"].device == DEV and s.crps["2t"].dtype == torch.float64 and s.rank_hist["z"].dtype == torch.int64
    assert s.rank_hist["z"].shape == (2, 3, M + 1) and s.members == M
    assert_batch_matches_yardstick(s, members, truth, f"batches M={M}")
    host, dev = ensemble_scores(members, truth), s.cpu()
    assert torch.equal(dev.hist, host.hist) and torch.equal(dev.table[:, 0], host.table[:, 0]) and dev.layout == host.layout
    # both within the bound of the exact sums -> within twice the bound of each other
    S5 = host.table[:, 5]
    for col, scale in ((1, host.table[:, 1]), (5, S5), (2, S5), (4, S5), (6, 2 * S5)):
        assert ((dev.table[:, col] - host.table[:, col]).abs() <= 2 * REL * scale).all(), col
    a_bar = S5 / host.table[:, 1]
    for col in (9, 10, 11, 12):                                   # bias, mae, crps, fair_crps
        assert ((dev.table[:, col] - host.table[:, col]).abs() <= 12 * REL * a_bar).all(), col


def test_one_batch_of_members_on_the_device():
    members, truth = lagged(6, seed=35, B=1)
    cat = lambda d: {k: torch.cat([getattr(b, d)[k] for b in members]).to(DEV) for k in getattr(truth, d)}  # noqa: E731
    md = truth.metadata
    one = Batch(cat("surf_vars"), {}, cat("atmos_vars"), Metadata(md.lat, md.lon, tuple(md.time[0] for _ in range(6)),
                                                                   md.atmos_levels))
    a = ensemble_scores(one, truth.to(DEV))
    b = ensemble_scores([m.to(DEV) for m in members], truth.to(DEV))
    assert torch.equal(a.table, b.table) and torch.equal(a.hist, b.hist) and a.crps["z"].shape == (1, 3)
    assert_batch_matches_yardstick(a, members, truth, "one batch")


def test_repeatable_bit_for_bit_and_independent_of_the_other_planes():
    """Two calls give identical results; a many-plane 0.25-degree call gives, plane for plane, what its planes give one at a
    time (the reduction tree of a plane does not depend on how many planes ride along)."""
    n = 6
    g = torch.Generator(device=DEV).manual_seed(50)
    t = 101325 + 300 * torch.randn(n, 721, 1440, device=DEV, generator=g)
    w = torch.from_numpy(weights(721)).to(DEV)
    for M in (4, 10, 51):
        x = [t + 0.5 + 2 * torch.randn(n, 721, 1440, device=DEV, generator=g) for _ in range(M)]
        x[M - 1][2, 100:200, 300:500] = float("nan")
        args = lambda sl=slice(None): ([[v[sl]] for v in x], [t[sl]], w)  # noqa: E731
        whole, again = lib.ensemble_scores_sums(*args()), lib.ensemble_scores_sums(*args())
        single = [lib.ensemble_scores_sums(*args(slice(k, k + 1))) for k in range(n)]
        torch.cuda.synchronize()
        for i in (0, 1):
            assert torch.equal(whole[i], again[i]), M
            assert torch.equal(whole[i], torch.cat([s[i] for s in single])), M
        assert whole[0][2, 0] == 721 * 1440 - 100 * 200 and whole[0][0, 0] == 721 * 1440
        assert (whole[1][:, :M + 1].sum(dim=1) == whole[0][:, 0]).all()
        del x


def test_member_order_changes_only_what_is_added_in_member_order():
    M = 17
    x, t = pressure_ensemble(M, 3, 33, 61, seed=60)
    w = torch.from_numpy(weights(33)).to(DEV)
    xd, td = [carve(x[m]) for m in range(M)], carve(t)
    a = lib.ensemble_scores_sums([[v] for v in xd], [td], w)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(1)).tolist()
    b = lib.ensemble_scores_sums([[xd[m]] for m in perm], [td], w)
    assert torch.equal(a[1], b[1])
    for s in (0, 1, 5, 6):                                        # formed from the sorted members: bit for bit
        assert torch.equal(a[0][:, s], b[0][:, s]), s
    Q = a[0][:, 7] * (M - 1) / M + a[0][:, 3]                     # q = v (M - 1) / M + e^2
    for s, scale in ((2, a[0][:, 5]), (4, a[0][:, 5]), (3, Q), (7, 2 * Q)):   # e is added in member order
        assert ((a[0][:, s] - b[0][:, s]).abs() <= 2 * REL * scale).all(), s


def test_scores_are_capturable_in_a_hip_graph():
    M = 6
    members, truth = lagged(M, n_lat=33, n_lon=64, seed=60)
    other, other_truth = lagged(M, n_lat=33, n_lon=64, seed=70)
    members, truth = [b.to(DEV) for b in members], truth.to(DEV)
    want_first = ensemble_scores(members, truth).cpu()            # (also the warm call: tables and weights are uploaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = ensemble_scores(members, truth)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s.table.cpu(), want_first.table) and torch.equal(s.hist.cpu(), want_first.hist)
    for dst, src in zip(members + [truth], other + [other_truth]):   # new values in the static inputs, in place
        for grp in ("surf_vars", "atmos_vars"):
            for k, v in getattr(dst, grp).items():
                v.copy_(getattr(src, grp)[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = s.cpu()
    assert not torch.equal(replayed.table, want_first.table) and not torch.equal(replayed.hist, want_first.hist)
    eager = ensemble_scores(members, truth).cpu()
    assert torch.equal(replayed.table, eager.table) and torch.equal(replayed.hist, eager.hist)
    assert_batch_matches_yardstick(replayed, other, other_truth, "replay")


def test_a_cold_call_during_capture_is_refused(monkeypatch):
    x, t = pressure_ensemble(2, 1, 17, 32, seed=80)
    w = torch.from_numpy(weights(17)).to(DEV)
    xd, td = [carve(x[m]).clone() for m in range(2)], carve(t).clone()     # addresses no call has seen
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before capturing"):
        lib.ensemble_scores_sums([[v] for v in xd], [td], w)


def test_scoring_a_rollout_of_four_members_step_by_step():
    """A small model rolls out B = 4 perturbed states as one batch; every step is scored as a 4-member ensemble against a
    shifted copy of the first member, nothing is read back in the loop, and the host path agrees."""
    case = CASES["small_b2"]
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    model.load_state_dict(helpers.case_state_dict(model, torch.float32), strict=True)
    model = model.to(DEV).eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    g = torch.Generator().manual_seed(3)
    four = lambda d: {k: v.float()[:1] * (1 + 1e-3 * torch.randn(4, *[1] * (v.dim() - 1), generator=g))  # noqa: E731
                      for k, v in d.items()}
    batch = Batch(four(surf), {k: v.float() for k, v in static.items()}, four(atmos),
                  Metadata(lat.float(), lon.float(), tuple(times[0] for _ in range(4)), tuple(case["levels"])))
    got, preds, truths = [], [], []
    with torch.inference_mode():
        for pred in rollout(model, batch.to(DEV), steps=3):
            truth = Batch({k: v[:1] + 0.25 for k, v in pred.surf_vars.items()}, {},
                          {k: v[:1] * 1.001 for k, v in pred.atmos_vars.items()},
                          Metadata(pred.metadata.lat, pred.metadata.lon, pred.metadata.time[:1], pred.metadata.atmos_levels))
            got.append(ensemble_scores(pred, truth))               # ONE batch: its four elements are the members
            preds.append(pred)
            truths.append(truth)
    got = [s.cpu() for s in got]
    assert len(got) == 3 and not torch.equal(got[0].table, got[1].table)
    for s, pred, truth in zip(got, preds, truths):
        assert s.members == 4 and set(s.crps) == set(pred.surf_vars) | set(pred.atmos_vars)
        assert s.rank_hist[next(iter(pred.atmos_vars))].shape == (1, len(case["levels"]), 5)
        host = ensemble_scores(pred.to("cpu"), truth.to("cpu"))
        assert torch.equal(s.hist, host.hist) and torch.equal(s.table[:, 0], host.table[:, 0])
        S5 = host.table[:, 5]
        for col, scale in ((1, host.table[:, 1]), (5, S5), (2, S5), (4, S5), (6, 2 * S5)):
            assert ((s.table[:, col] - host.table[:, col]).abs() <= 2 * REL * scale).all(), col
        single = [Batch({k: v[m:m + 1] for k, v in pred.surf_vars.items()}, {},
                        {k: v[m:m + 1] for k, v in pred.atmos_vars.items()}, truth.metadata).to("cpu") for m in range(4)]
        assert_batch_matches_yardstick(s, single, truth.to("cpu"), "roll-out")


def test_a_warm_call_allocates_less_than_a_plane_and_does_not_synchronise():
    n_lat, n_lon, M = 721, 1440, 5
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1)[:-1],
                  time=(datetime(2023, 1, 1, 6),), atmos_levels=(1, 2, 3))
    g = torch.Generator(device=DEV).manual_seed(90)
    mk = lambda: Batch({"2t": 280 + torch.randn(1, 2, n_lat, n_lon, device=DEV, generator=g)}, {},  # noqa: E731
                       {"z": 280 + torch.randn(1, 1, 3, n_lat, n_lon, device=DEV, generator=g)}, md)
    truth, members = mk(), [mk() for _ in range(M)]
    ensemble_scores(members, truth)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s = ensemble_scores(members, truth)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"a warm ensemble_scores() call of 4 planes x {M} members: peak allocation grows by {grown} bytes "
          f"(one plane: {n_lat * n_lon * 4})")
    assert grown < n_lat * n_lon * 4
    assert s.count["z"].shape == (1, 3) and int(s.count["2t"][0]) == n_lat * n_lon


def test_device_path_argument_errors():
    members, truth = lagged(3, seed=100)
    dev = [b.to(DEV) for b in members]
    with pytest.raises(ValueError, match="members and truth are on.*(cpu.*cuda|cuda.*cpu)"):
        ensemble_scores(dev, truth)
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        ensemble_scores([dev[0], members[1], dev[2]], truth.to(DEV))
    with pytest.raises(TypeError, match=r"members\[1\] variable '2t' is torch.float64"):
        ensemble_scores([dev[0], dev[1].type(torch.float64), dev[2]], truth.to(DEV))
    with pytest.raises(TypeError, match="truth variable '2t' is torch.float64"):
        ensemble_scores(dev, truth.to(DEV).type(torch.float64))
    bad = members[2].to(DEV)
    bad.atmos_vars["z"] = bad.atmos_vars["z"].transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match=r"members\[2\] variable 'z' are not row-major contiguous"):
        ensemble_scores([dev[0], dev[1], bad], truth.to(DEV))
