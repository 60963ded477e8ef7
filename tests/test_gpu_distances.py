"""aurora_hip_nearest_event and aurora_hip_object_separations (aurora_amd/csrc/nearest_event.hip) against the CPU path of
aurora_amd.nearest_event / object_separations, which tests/test_distances_host.py pins to a brute force: index, key, table and
hausdorff_bits are equal bit for bit, dtype included, and so is everything finalised from them (THE RULE: aurora_amd/distances.py)."""
import dataclasses
import functools
import importlib

import numpy as np
import pytest
import torch

from aurora_amd import _fields, nearest_event, object_separations, objects
from aurora_amd.engine import lib
from tests.test_distances_host import lats, lons, objects_on, sprinkle
from tests.test_gpu_object_matches import carve
from tests.test_objects_host import batch_of, patterns
from tests.verification_inputs import DEV, red_noise

pytestmark = pytest.mark.gpu
mod = importlib.import_module("aurora_amd.distances")


def grid(H, W, wrap):
    return (lats(H), lons(W, True), True) if wrap else (lats(H, "up"), lons(W, False), False)


def host(labels, la, H, W, wrap, max_km=None, max_objects=8):
    """The CPU path on (..., H, W) label maps: (index, key) of `labels`, then (table, hausdorff) of `la` against them."""
    lat, lon, wrap = grid(H, W, wrap)
    index, key = mod._nearest_host(labels, *mod.tables_of(lat, lon, wrap), wrap, mod.key_max_of(max_km))
    count = la.reshape(*la.shape[:-2], -1).max(axis=-1).clip(min=0).astype(np.int32)
    return (index, key, *mod._separations_host(la, key, index, count, max_objects))


def device(labels, la, H, W, wrap, max_km=None, max_objects=8, offset=0, **kw):
    """lib.nearest_event_maps and lib.object_separation_table on device copies of the same maps, as host arrays."""
    lat, lon, wrap = grid(H, W, wrap)
    tables = torch.from_numpy(np.concatenate(mod.tables_of(lat, lon, wrap))).to(DEV)
    index, key = lib.nearest_event_maps(carve(labels, offset), tables, wrap, mod.key_max_of(max_km), **kw)
    count = torch.from_numpy(la.reshape(*la.shape[:-2], -1).max(axis=-1).clip(min=0).astype(np.int32)).to(DEV)
    table, hausdorff = lib.object_separation_table(carve(la, offset), key, index, count, max_objects)
    return tuple(t.cpu().numpy() for t in (index, key, table, hausdorff))


def assert_same(got, want):
    for g, w, what in zip(got, want, ("index", "key", "table", "hausdorff")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, np.argwhere(g != w)[:5])


@functools.lru_cache(maxsize=None)
def maps(H, W, n=2, T=2, seed=1):
    """Two (n, T, H, W) stacks of labels in -1 .. 9, events at a few percent of the points; item 0 of the first has none."""
    b = np.stack([sprinkle(H, W, 0.03, seed=seed + k) for k in range(n * T)]).reshape(n, T, H, W)
    a = np.stack([sprinkle(H, W, 0.05, seed=seed + 100 + k) * 3 for k in range(n * T)]).reshape(n, T, H, W).astype(np.int32)
    b[0, 0] = np.minimum(b[0, 0], 0)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


def same_results(x, y):
    """Every table and every finalised property of two ObjectSeparations and their NearestEvents, NaN equal to NaN."""
    same = lambda p, q: p.dtype == q.dtype and p.shape == q.shape and torch.equal(p.isnan(), q.isnan()) and torch.equal(p.nan_to_num(), q.nan_to_num())  # noqa: E731
    flat = lambda d: {k: v.cpu().double() if v.dtype == torch.bool else v.cpu() for k, v in d.items()}  # noqa: E731
    assert x.table_table.dtype == torch.int64 and x.nearest.index_table.dtype == torch.int32 and x.nearest.key_table.dtype == torch.float64
    pairs = [(getattr(x, w), getattr(y, w), w) for w in ("table", "hausdorff_bits", "distance_km", "nearest_b", "a_lat", "a_lon", "b_lat",
                                                        "b_lon", "hausdorff_km")]
    pairs += [(getattr(x.nearest, w), getattr(y.nearest, w), w) for w in ("index", "key", "label", "distance_km")]
    pairs += [(x.matched(f), y.matched(f), "matched") for f in (0.0, 500.0)]
    for p, q, what in pairs:
        p, q = flat(p), flat(q)
        assert p.keys() == q.keys()
        for k in p:
            assert same(p[k], q[k]), (what, k)


# ---- through objects: the whole chain on the device against the whole chain on the host ------------------------------------------
@pytest.mark.parametrize("name", ("seam", "band", "comb", "serpentine", "rings", "special"))
def test_patterns_through_objects_equal_the_cpu_chain(name):
    plane = np.asarray(patterns()[name], dtype=np.float32)
    thr = {"x": [0.5, 1.5]}
    ba, bb = batch_of(plane[None]), batch_of(np.roll(plane, 2, axis=1)[None])
    for kw, max_km in ((dict(max_objects=64, wrap=True), None), (dict(max_objects=3, wrap=False), 2000.0)):
        on_host = object_separations(objects(ba, thr, **kw), objects(bb, thr, **kw), max_km)
        on_device = object_separations(objects(ba.to(DEV), thr, **kw), objects(bb.to(DEV), thr, **kw), max_km)
        assert on_device.table_table.device.type == "cuda" and on_device.nearest.key_table.device.type == "cuda"
        same_results(on_device, on_host)
        same_results(on_device.cpu(), on_host)


# ---- label maps fed straight to the kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (1, 2, 63, 64, 65, 127, 128, 129, 257))
@pytest.mark.parametrize("H", (1, 2, 40))
def test_widths_and_heights(H, W):
    la, lb = maps(H, W)
    for wrap in (True, False):
        assert_same(device(lb, la, H, W, wrap), host(lb, la, H, W, wrap))
    assert_same(device(lb, la, H, W, True, max_km=1500.0, max_objects=2), host(lb, la, H, W, True, max_km=1500.0, max_objects=2))
    # dense maps: long runs of events, and every point an event
    dense = (np.indices((H, W)).sum(0) % 5 > 0).astype(np.int32)[None]
    assert_same(device(dense, 1 - dense, H, W, True), host(dense, 1 - dense, H, W, True))
    assert_same(device(np.ones_like(dense), dense, H, W, False), host(np.ones_like(dense), dense, H, W, False))


@pytest.mark.parametrize("offset", (0, 1, 3))
def test_alignment_does_not_matter(offset):
    la, lb = maps(33, 70)
    assert_same(device(lb, la, 33, 70, True, offset=offset), host(lb, la, 33, 70, True))


@pytest.mark.parametrize("T", (1, 8))
def test_threshold_counts(T):
    la, lb = maps(33, 70, n=3, T=T)
    assert_same(device(lb, la, 33, 70, True), host(lb, la, 33, 70, True))


def test_a_plane_without_events():
    la, lb = maps(40, 130)
    got = device(np.zeros_like(lb), la, 40, 130, True)
    assert (got[0] == -1).all() and np.isinf(got[1]).all() and (got[3] == 0x7FF0000000000000).all()
    assert_same(got, host(np.zeros_like(lb), la, 40, 130, True))


@pytest.mark.parametrize("max_km", (None, 500.0))
@pytest.mark.parametrize("corner", ((0, 0), (180, 359)))
def test_one_event_in_a_corner_of_a_one_degree_grid(corner, max_km):
    # the longest walk: every point of the plane must reach the one event, 180 rows away at the most; a stop rule that cut a
    # winner would leave -1 or +inf behind
    one = np.zeros((1, 181, 360), np.int32)
    one[0][corner] = 4
    everywhere = np.ones((1, 181, 360), np.int32)
    for wrap in (True, False):
        got, want = device(one, everywhere, 181, 360, wrap, max_km), host(one, everywhere, 181, 360, wrap, max_km)
        assert_same(got, want)
        if max_km is None:
            assert (got[0] == corner[0] * 360 + corner[1]).all()
        else:
            assert (got[0] >= 0).sum() > 10 and (got[0] < 0).sum() > 60000 and got[3][0] == 0x7FF0000000000000


def test_a_quarter_degree_plane_at_its_0_9_quantile():
    plane = red_noise((1, 721, 1440), seed=11)
    thr = {"x": [float(np.quantile(plane, 0.9))]}
    a = objects(batch_of(plane).to(DEV), thr, wrap=True)
    b = objects(batch_of(np.roll(plane, 40, axis=-1)).to(DEV), thr, wrap=True)
    on_device = object_separations(a, b)
    on_host = object_separations(a.cpu(), b.cpu())                                  # the numpy path on the same label maps
    print("objects:", a.count_table.tolist(), b.count_table.tolist(), "hausdorff_km:", on_host.hausdorff_km["x"].tolist())
    assert int(a.count_table.min()) > 0
    same_results(on_device, on_host)


def test_independence_of_the_other_items():
    la, lb = maps(40, 130, n=7, T=1)
    alone, among, last = device(lb[6:], la[6:], 40, 130, True), device(lb[4:], la[4:], 40, 130, True), device(lb, la, 40, 130, True)
    for x, y, z in zip(alone, among, last):
        assert x[0].tobytes() == y[2].tobytes() == z[6].tobytes()


def test_two_calls_give_identical_bytes():
    la, lb = maps(40, 257, n=3)
    first, second = device(lb, la, 40, 257, True), device(lb, la, 40, 257, True)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()


def test_a_small_workspace_is_refused_and_nothing_is_written():
    la, lb = maps(40, 64)
    out = (torch.full((2, 2, 40, 64), -7, dtype=torch.int32, device=DEV), torch.full((2, 2, 40, 64), -7.0, dtype=torch.float64, device=DEV))
    need = lib.nearest_event_workspace_bytes(4, 40, 64)
    assert need == 4 * 40 * 64 * 2 + 4 * 40 * 4 + 4 * 8
    with pytest.raises(ValueError, match="workspace"):
        device(lb, la, 40, 64, True, out=out, workspace=torch.empty(need - 8, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out)
    got = device(lb, la, 40, 64, True, out=out, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
    assert_same(got, host(lb, la, 40, 64, True))


def to_device(o):
    return dataclasses.replace(o, **{f: getattr(o, f).to(DEV) for f in ("labels_table", "count_table", "table_table", "thresholds_table", "lat", "lon")})


def test_capture_in_a_hip_graph():
    la, lb = maps(33, 70, n=3)
    other_a, other_b = maps(33, 70, n=3, seed=9)
    lat, lon, _ = grid(33, 70, True)
    a = to_device(objects_on(la, lat, lon, True, max_objects=8))
    b = dataclasses.replace(to_device(objects_on(lb, lat, lon, True, max_objects=8)), lat=a.lat, lon=a.lon)   # one copy per grid, as `objects` keeps
    object_separations(a, b, 3000.0)                                              # the warm call: the tables are uploaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = object_separations(a, b, 3000.0)
    a.labels_table.copy_(torch.from_numpy(other_a))
    b.labels_table.copy_(torch.from_numpy(other_b))
    a.count_table.copy_(torch.from_numpy(other_a.reshape(3, 2, -1).max(axis=-1).clip(min=0).astype(np.int32)))
    for t in (s.table_table, s.hausdorff_table, s.nearest.index_table):
        t.fill_(-5)
    graph.replay()
    torch.cuda.synchronize()
    want = object_separations(objects_on(other_a, lat, lon, True, max_objects=8), objects_on(other_b, lat, lon, True, max_objects=8), 3000.0)
    for x, y in ((s.table_table, want.table_table), (s.hausdorff_table, want.hausdorff_table), (s.nearest.index_table, want.nearest.index_table),
                 (s.nearest.key_table, want.nearest.key_table)):
        assert x.cpu().numpy().tobytes() == y.numpy().tobytes()
    with pytest.MonkeyPatch.context() as mp:                                       # a cold call during capture is refused
        mp.setattr(mod._fields, "tables", _fields.DeviceTables(capturing=lambda: True))
        with pytest.raises(RuntimeError, match="nearest_event: call once .* before capturing a graph"):
            nearest_event(b)
