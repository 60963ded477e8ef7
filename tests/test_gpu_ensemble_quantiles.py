"""`aurora_amd.ensemble_quantiles` on the device: one aurora_hip_ensemble_quantiles call against the yardstick of
tests/test_ensemble_quantiles_host.py (`yardstick_quantiles`: the rule in numpy, the order through `np.lexsort`, the three
fp64 operations one by one), in EVERY BIT: the rule fixes each rounding, so there is no tolerance here.  NaN positions must be
the same; NaN payloads are not compared."""
from datetime import datetime

import numpy as np
import pytest
import torch

from aurora_amd import Batch, Metadata, ensemble_quantiles
from aurora_amd.engine import lib
from tests.test_ensemble_quantiles_host import Q8, assert_same_bits, special_values, yardstick_quantiles
from tests.test_ensemble_scores_host import lagged, pressure_ensemble
from tests.verification_inputs import DEV, carve, weights

pytestmark = pytest.mark.gpu


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_raw(x, t, q, what, offset=0):
    """x (M, n_planes, n_lat, n_lon), t (n_planes, n_lat, n_lon) or None on the host: one call, every plane against the
    yardstick; the inputs are not modified."""
    M, n_planes, n_lat, n_lon = x.shape
    xd = [carve(x[m], offset) for m in range(M)]
    td = None if t is None else carve(t, offset)
    if offset and n_lon % 4 == 0:
        assert xd[0].data_ptr() % 16 != 0
    maps, rank = lib.ensemble_quantiles([[v] for v in xd], None if td is None else [td], q)
    assert maps.shape == (n_planes, len(q), n_lat, n_lon) and maps.dtype == torch.float32 and maps.device == DEV
    assert (rank is None) == (t is None)
    maps = maps.cpu().numpy()
    for m in range(M):
        assert same_bits(xd[m].cpu(), x[m]), f"{what}: member {m} was modified"
    for k in range(n_planes):
        want, want_rank = yardstick_quantiles(x[:, k].numpy(), q, None if t is None else t[k].numpy())
        assert_same_bits(maps[k], want, f"{what} plane {k}")
        if t is not None:
            assert rank.shape == (n_planes, n_lat, n_lon) and rank.dtype == torch.int8
            assert np.array_equal(rank[k].cpu().numpy(), want_rank), f"{what} plane {k}: rank"
    return maps, None if rank is None else rank.cpu().numpy()


GRIDS = [
    (2, 17, 32, 0),         # the toy batch
    (3, 33, 61, 0),         # odd n_lon: a partial last quad, output planes after the first not 16-byte aligned
    (2, 33, 64, 1),         # inputs one float past a 16-byte boundary
    (2, 1, 37, 0),          # one row
    (1, 19, 1, 0),          # one column
]


@pytest.mark.parametrize("M", (2, 3, 4, 8, 12, 16, 17, 32, 51, 64))       # every bucket full and padded
@pytest.mark.parametrize("n_planes,n_lat,n_lon,offset", GRIDS)
def test_raw_maps_equal_the_yardstick(M, n_planes, n_lat, n_lon, offset):
    x, t = pressure_ensemble(M, n_planes, n_lat, n_lon, seed=100 * M + n_lat + n_lon)
    what = f"M={M} {n_planes}x{n_lat}x{n_lon}+{offset}"
    with_truth, _ = check_raw(x, t, Q8, what + " truth", offset)
    without, _ = check_raw(x, None, Q8, what, offset)
    assert np.array_equal(with_truth.view(np.int32), without.view(np.int32))


@pytest.mark.parametrize("M", (8, 51))
def test_alignment_does_not_change_a_single_bit(M):
    """The same values behind aligned and unaligned input pointers, into an aligned output and through out= into one carved
    one float past a 16-byte boundary (and a rank map one byte past a 4-byte boundary)."""
    x, t = pressure_ensemble(M, 3, 33, 64, seed=5 + M)
    results = []
    for offset in (0, 1):
        xd, td = [[carve(x[m], offset)] for m in range(M)], [carve(t, offset)]
        assert td[0].data_ptr() % 16 == 4 * offset
        results.append(lib.ensemble_quantiles(xd, td, Q8))
        assert results[-1][0].data_ptr() % 16 == 0
        out = torch.full((1 + 3 * 8 * 33 * 64,), -7.0, device=DEV)[1:].view(3, 8, 33, 64)
        rank_out = torch.full((1 + 3 * 33 * 64,), -7, dtype=torch.int8, device=DEV)[1:].view(3, 33, 64)
        assert out.data_ptr() % 16 == 4 and rank_out.data_ptr() % 4 == 1
        got = lib.ensemble_quantiles(xd, td, Q8, out=out, rank_out=rank_out)
        assert got[0] is out and got[1] is rank_out
        results.append(got)
    for maps, rank in results[1:]:
        assert same_bits(maps, results[0][0]) and torch.equal(rank, results[0][1])
    # one unaligned member is enough to leave the 16-byte path
    mixed = lib.ensemble_quantiles([[carve(x[m], int(m == M - 1))] for m in range(M)], [carve(t)], Q8)
    assert same_bits(mixed[0], results[0][0]) and torch.equal(mixed[1], results[0][1])
    assert_same_bits(results[0][0][1].cpu().numpy(), yardstick_quantiles(x[:, 1].numpy(), Q8)[0], f"M={M}")


def test_one_plane_at_a_quarter_degree_equals_the_yardstick():
    x, t = pressure_ensemble(17, 1, 721, 1440, seed=7 * 17)
    check_raw(x, t, (0.1, 0.5, 0.9), "M=17 1x721x1440")


@pytest.mark.parametrize("M", (3, 11, 33))
def test_special_values_on_the_device(M):
    """NaN land mask and stray NaN / Inf; a variable clamped at zero with signed zeros; the rank map counts to the rank
    histogram of aurora_hip_ensemble_scores."""
    clean, x, t, bad = special_values(M, seed=1)
    maps, rank = check_raw(torch.from_numpy(x), torch.from_numpy(t), Q8, f"special M={M}")
    assert np.array_equal(np.isnan(maps), np.broadcast_to(bad[:, None], maps.shape))
    want, _ = check_raw(torch.from_numpy(clean), None, Q8, f"clean M={M}")
    keep = np.broadcast_to(~bad[:, None], maps.shape)
    assert np.array_equal(maps[keep].view(np.int32), want[keep].view(np.int32))
    assert np.array_equal(rank == -1, bad | ~np.isfinite(t))
    _, hist = lib.ensemble_scores_sums([[carve(x[m])] for m in range(M)], [carve(t)], torch.from_numpy(weights(33)).to(DEV))
    hist = hist.cpu().numpy()
    for k in range(2):
        assert np.array_equal(np.bincount(rank[k][rank[k] >= 0], minlength=M + 1), hist[k, :M + 1]), k
    # signed zeros
    z = (torch.from_numpy(clean) - 101325.0).clamp(min=0.0) / 100
    g = torch.Generator().manual_seed(5)
    z[(z == 0) & (torch.rand(z.shape, generator=g) < 0.5)] = -0.0
    assert int((torch.signbit(z) & (z == 0)).sum()) > 100
    zy = (torch.from_numpy(t) - 101325.0).nan_to_num(0.0, 0.0, 0.0).clamp(min=0.0) / 100
    a, ra = check_raw(z, zy, Q8, f"zeros M={M}")
    b, rb = check_raw(z.flip(0), zy, Q8, f"zeros, members reversed, M={M}")
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(ra, rb)


def test_repeatable_and_independent_of_the_other_planes_and_of_member_order():
    M = 13
    x, t = pressure_ensemble(M, 3, 33, 61, seed=50)
    xd, td = [carve(x[m]) for m in range(M)], carve(t)
    args = lambda sl=slice(None), order=range(M): ([[xd[m][sl]] for m in order], [td[sl]], Q8)  # noqa: E731
    whole, again = lib.ensemble_quantiles(*args()), lib.ensemble_quantiles(*args())
    single = [lib.ensemble_quantiles(*args(slice(k, k + 1))) for k in range(3)]
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(1)).tolist()
    permuted = lib.ensemble_quantiles(*args(order=perm))
    for other in (again, permuted, tuple(torch.cat([s[i] for s in single]) for i in (0, 1))):
        assert same_bits(whole[0], other[0]) and torch.equal(whole[1], other[1])


def one_batch_of(members, truth):
    cat = lambda d: {k: torch.cat([getattr(b, d)[k] for b in members]) for k in getattr(truth, d)}  # noqa: E731
    md = truth.metadata
    return Batch(cat("surf_vars"), truth.static_vars, cat("atmos_vars"),
                 Metadata(md.lat, md.lon, tuple(md.time[0] for _ in members), md.atmos_levels))


@pytest.mark.parametrize("form,M", (("sequence", 5), ("one batch", 6)))
@pytest.mark.parametrize("with_truth", (False, True))
def test_batches_on_the_device_equal_the_host_path(form, M, with_truth):
    members, truth = lagged(M, n_lat=33, n_lon=61, seed=30, B=2 if form == "sequence" else 1)
    members[1].surf_vars["2t"][0, -1, 3, 4:9] = float("nan")
    host_members = members if form == "sequence" else one_batch_of(members, truth)
    dev_members = [b.to(DEV) for b in members] if form == "sequence" else host_members.to(DEV)
    host = ensemble_quantiles(host_members, Q8, truth if with_truth else None)
    dev = ensemble_quantiles(dev_members, Q8, truth.to(DEV) if with_truth else None)
    assert dev.maps.device == DEV and dev.quantile["z"].device == DEV and dev.layout == host.layout and dev.members == M
    assert dev.quantile["z"].shape == (host.maps.shape[0] // 5, 3, 8, 33, 61) and dev.q == host.q
    got = dev.cpu()
    assert_same_bits(got.maps.numpy(), host.maps.numpy(), form)
    if with_truth:
        assert dev.rank["2t"].dtype == torch.int8 and torch.equal(got.ranks, host.ranks)
    else:
        assert got.ranks is None
    med = dev.as_batch(0.5)
    assert med.surf_vars["2t"].device == DEV and med.surf_vars["2t"].shape == (host.maps.shape[0] // 5, 1, 33, 61)
    assert len(med.metadata.time) == med.surf_vars["2t"].shape[0]


def test_a_warm_call_is_capturable_in_a_hip_graph():
    M = 6
    members, truth = lagged(M, n_lat=33, n_lon=64, seed=60)
    other, other_truth = lagged(M, n_lat=33, n_lon=64, seed=70)
    members, truth = [b.to(DEV) for b in members], truth.to(DEV)
    first = ensemble_quantiles(members, Q8, truth).cpu()           # (also the warm call: the plane table is uploaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eq = ensemble_quantiles(members, Q8, truth)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(eq.maps.cpu(), first.maps) and torch.equal(eq.ranks.cpu(), first.ranks)
    for dst, src in zip(members + [truth], other + [other_truth]):   # new values in the static inputs, in place
        for grp in ("surf_vars", "atmos_vars"):
            for k, v in getattr(dst, grp).items():
                v.copy_(getattr(src, grp)[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = eq.cpu()
    assert not torch.equal(replayed.maps, first.maps) and not torch.equal(replayed.ranks, first.ranks)
    eager = ensemble_quantiles(members, Q8, truth).cpu()
    assert same_bits(replayed.maps, eager.maps) and torch.equal(replayed.ranks, eager.ranks)
    host = ensemble_quantiles(other, Q8, other_truth)
    assert_same_bits(replayed.maps.numpy(), host.maps.numpy(), "replay")


def test_a_cold_call_during_capture_is_refused(monkeypatch):
    x, _ = pressure_ensemble(2, 1, 17, 32, seed=80)
    xd = [carve(x[m]).clone() for m in range(2)]                   # addresses no call has seen
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before capturing a graph \\(the plane-pointer table"):
        lib.ensemble_quantiles([[v] for v in xd], None, (0.5,))


def test_a_warm_call_allocates_its_outputs_alone_and_does_not_synchronise():
    n_lat, n_lon, M = 721, 1440, 5
    md = Metadata(lat=torch.linspace(90, -90, n_lat, dtype=torch.float64), lon=torch.linspace(0, 360, n_lon + 1)[:-1],
                  time=(datetime(2023, 1, 1, 6),), atmos_levels=(1, 2, 3))
    g = torch.Generator(device=DEV).manual_seed(90)
    mk = lambda: Batch({"2t": 280 + torch.randn(1, 2, n_lat, n_lon, device=DEV, generator=g)}, {},  # noqa: E731
                       {"z": 280 + torch.randn(1, 1, 3, n_lat, n_lon, device=DEV, generator=g)}, md)
    truth, members = mk(), [mk() for _ in range(M)]
    ensemble_quantiles(members, truth=truth)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eq = ensemble_quantiles(members, truth=truth)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    outputs = 4 * 3 * n_lat * n_lon * 4 + 4 * n_lat * n_lon
    # torch's caching allocator hands out a cached block whole unless the remainder exceeds 1 MiB, and counts the block: each
    # of the two outputs may be charged up to 1 MiB more than its size.  Still less than one plane (4.15 MB) of anything else.
    slack = 2 * (1 << 20)
    print(f"a warm ensemble_quantiles() call of 4 planes x {M} members, Q = 3: peak allocation grows by {grown} bytes "
          f"(its outputs: {outputs}; one plane: {n_lat * n_lon * 4})")
    assert slack < n_lat * n_lon * 4 and grown <= outputs + slack
    assert eq.quantile["z"].shape == (1, 3, 3, n_lat, n_lon) and int((eq.rank["2t"] >= 0).sum()) == n_lat * n_lon


def test_device_path_argument_errors():
    members, truth = lagged(3, seed=100)
    dev = [b.to(DEV) for b in members]
    with pytest.raises(ValueError, match="the fields of members and truth are on.*(cpu.*cuda|cuda.*cpu)"):
        ensemble_quantiles(dev, truth=truth)
    with pytest.raises(ValueError, match="the fields of members are on.*(cpu.*cuda|cuda.*cpu)"):
        ensemble_quantiles([dev[0], members[1], dev[2]])
    with pytest.raises(TypeError, match=r"members\[1\] variable '2t' is torch.float64"):
        ensemble_quantiles([dev[0], dev[1].type(torch.float64), dev[2]])
    with pytest.raises(TypeError, match="truth variable '2t' is torch.float64"):
        ensemble_quantiles(dev, truth=truth.to(DEV).type(torch.float64))
    bad = members[2].to(DEV)
    bad.atmos_vars["z"] = bad.atmos_vars["z"].transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match=r"members\[2\] variable 'z' are not row-major contiguous"):
        ensemble_quantiles([dev[0], dev[1], bad])
    # the C entry point: code -1 with a message, before any launch
    L = lib.load()
    err, f = L.aurora_hip_last_error, L.aurora_hip_ensemble_quantiles
    q = torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64)
    x = torch.zeros(8, 17, 32, device=DEV)
    table = torch.tensor([x[m].data_ptr() for m in range(8)], dtype=torch.int64, device=DEV)
    out, rank = torch.empty(1, 3, 17, 32, device=DEV), torch.empty(1, 17, 32, dtype=torch.int8, device=DEV)
    call = lambda M, n_q, truth, r: f(table.data_ptr(), truth, M, 1, 17, 32, q.data_ptr(), n_q, out.data_ptr(), r, None)  # noqa: E731
    for M in (1, 65):
        assert call(M, 3, None, None) == -1 and b"n_members" in err(), M
    for n_q in (0, 9):
        assert call(7, n_q, None, None) == -1 and b"n_q" in err(), n_q
    assert call(7, 3, table.data_ptr() + 56, None) == -1 and b"rank" in err()
    assert call(7, 3, table.data_ptr() + 56, rank.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (out == 0).all() and (rank == 0).all()
