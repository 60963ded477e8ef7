"""aurora_hip_object_matches (aurora_amd/csrc/object_matches.hip) against the CPU path of aurora_amd.object_matches, which
tests/test_object_matches_host.py pins to a dict loop: pairs and count are equal bit for bit, dtype included, and so is
everything finalised from them (THE RULE: aurora_amd/object_matches.py)."""
import dataclasses
import functools
import importlib

import numpy as np
import pytest
import torch

from aurora_amd import object_matches, objects
from aurora_amd.engine import lib
from tests.test_object_matches_host import hand_maps, objects_of, stripes
from tests.test_objects_host import batch_of, lat_of, patterns
from tests.verification_inputs import DEV, red_noise

pytestmark = pytest.mark.gpu
mod = importlib.import_module("aurora_amd.object_matches")
obj = importlib.import_module("aurora_amd.objects")


def carve(labels: np.ndarray, offset: int = 0) -> torch.Tensor:
    """A device copy of int32 label maps carved out of a flat buffer `offset` int32 past its aligned start.  The buffer is
    filled with 1, a label that would contribute were it read as a point."""
    flat = torch.ones(offset + labels.size, dtype=torch.int32)
    flat[offset:] = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).reshape(-1)
    return flat.to(DEV)[offset:].view(labels.shape)


def unit_of(H: int) -> np.ndarray:
    return obj.area_units(lat_of(H))


def host(la, lb, max_a=8, max_b=8, max_pairs=64):
    return mod._pairs_host(np.asarray(la, np.int32), np.asarray(lb, np.int32), unit_of(la.shape[-2]), max_a, max_b, max_pairs)


def device(la, lb, max_a=8, max_b=8, max_pairs=64, offset=0, **kw):
    """lib.object_pairs on device copies of (..., H, W) label maps, as host arrays."""
    unit = torch.from_numpy(unit_of(la.shape[-2])).to(DEV)
    out = lib.object_pairs(carve(la, offset), carve(lb, offset), unit, max_a, max_b, max_pairs, **kw)
    return tuple(t.cpu().numpy() for t in out)


def assert_same(got, want):
    for g, w, what in zip(got, want, ("pairs", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, g, w)


@functools.lru_cache(maxsize=None)
def maps(H, W, n=2, T=2, seed=1):
    """Two (n, T, H, W) stacks of labels in -1 .. 9 (8 and 9 are past the tables of the default max_objects = 8): `a` in runs of
    about seven columns, which cross the 64-column chunks, `b` in blocks of three by two; item 0 of `b` is white noise."""
    g = np.random.default_rng(seed + 7 * H + W)
    a = np.repeat(g.integers(-1, 10, (n, T, H, W // 7 + 1), dtype=np.int32), 7, axis=-1)[..., :W]
    b = np.repeat(np.repeat(g.integers(-1, 10, (n, T, H // 2 + 1, W // 3 + 1), dtype=np.int32), 2, axis=-2), 3, axis=-1)[..., :H, :W]
    b[0, 0] = g.integers(-1, 10, (H, W), dtype=np.int32)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


def same_matches(x, y):
    """Every table and every finalised property of two results (finalised where each lives), NaN equal to NaN."""
    same = lambda p, q: p.dtype == q.dtype and p.shape == q.shape and torch.equal(p.isnan(), q.isnan()) and torch.equal(p.nan_to_num(), q.nan_to_num())  # noqa: E731
    flat = lambda d: {k: v.cpu().double() if v.dtype == torch.bool else v.cpu() for k, v in d.items()}  # noqa: E731
    assert x.pairs_table.dtype == torch.int64 and x.count_table.dtype == torch.int32
    for what in ("pairs", "count", "overflow", "truncated", "intersection", "iou", "fraction_of_a", "fraction_of_b", "distance_km",
                 "best_b", "best_b_fraction", "best_a", "best_a_fraction"):
        p, q = flat(getattr(x, what)), flat(getattr(y, what))
        assert p.keys() == q.keys()
        for k in p:
            assert same(p[k], q[k]), (what, k)
    for f in (0.0, 0.5):
        for k in x.matched_a(f):
            assert torch.equal(x.matched_a(f)[k].cpu(), y.matched_a(f)[k].cpu()) and torch.equal(x.matched_b(f)[k].cpu(), y.matched_b(f)[k].cpu())
        sx, sy = x.summary(f), y.summary(f)
        for what in sx:
            p, q = flat(sx[what]), flat(sy[what])
            for k in p:
                assert same(p[k], q[k]), ("summary", what, k)


# ---- through objects: the whole chain on the device against the whole chain on the host ------------------------------------------
@pytest.mark.parametrize("name", sorted(patterns()))
def test_patterns_through_objects_equal_the_cpu_chain(name):
    plane = np.asarray(patterns()[name], dtype=np.float32)
    thr = {"x": [0.5, 1.5]}
    ba, bb = batch_of(plane[None]), batch_of(np.roll(plane, 1, axis=1)[None])
    kw = dict(max_objects=64, connectivity=8, wrap=True)
    on_host = object_matches(objects(ba, thr, **kw), objects(bb, thr, **kw), max_pairs=128)
    on_device = object_matches(objects(ba.to(DEV), thr, **kw), objects(bb.to(DEV), thr, **kw), max_pairs=128)
    assert on_device.pairs_table.device.type == "cuda"
    same_matches(on_device, on_host)
    same_matches(on_device.cpu(), on_host)


@pytest.mark.parametrize("name", sorted(hand_maps()))
def test_hand_drawn_maps_equal_the_cpu_path(name):
    la, lb = (np.asarray(x)[None, None] for x in hand_maps()[name])
    assert_same(device(la, lb, 64, 64, 64), host(la, lb, 64, 64, 64))
    assert_same(device(la, lb, 2, 3, 64), host(la, lb, 2, 3, 64))


def test_object_matches_finalised_on_the_device_equals_the_cpu_object():
    la, lb = maps(40, 130, n=3)
    a, b = objects_of(la, max_objects=8), objects_of(lb, max_objects=6)
    to = lambda o: dataclasses.replace(o, **{f: getattr(o, f).to(DEV) for f in ("labels_table", "count_table", "table_table", "thresholds_table", "lat", "lon")})  # noqa: E731
    on_host, on_device = object_matches(a, b, max_pairs=64), object_matches(to(a), to(b), max_pairs=64)
    assert int(on_host.count_table.min()) > 10 and on_device.iou["x"].device.type == "cuda"
    same_matches(on_device, on_host)
    with pytest.raises(ValueError, match="object_matches: a is on cpu and b on cuda:0; move both"):
        object_matches(a, to(b))


# ---- label maps fed straight to the kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (1, 2, 63, 64, 65, 130, 257))
@pytest.mark.parametrize("H", (1, 2, 40))
def test_widths_and_heights(H, W):
    la, lb = maps(H, W)
    assert_same(device(la, lb), host(la, lb))
    assert_same(device(la, lb, 5, 9, 45), host(la, lb, 5, 9, 45))
    # one run per row that is open at every chunk boundary, against columns
    rows, cols = np.indices((H, W))
    ra, cb = (rows % 8 + 1).astype(np.int32)[None], (cols % 8 + 1).astype(np.int32)[None]
    assert_same(device(ra, cb), host(ra, cb))


@pytest.mark.parametrize("offset", (0, 1, 3))
def test_alignment_does_not_matter(offset):
    la, lb = maps(40, 64)
    assert_same(device(la, lb, offset=offset), host(la, lb))
    la, lb = maps(33, 70)
    assert_same(device(la, lb, offset=offset), host(la, lb))


@pytest.mark.parametrize("T", (1, 5, 8))
def test_threshold_counts(T):
    la, lb = maps(33, 70, n=3, T=T)
    assert_same(device(la, lb), host(la, lb))


def home_slots(ka, kb, log2c):
    """The home slot of include/aurora_hip.h, in numpy uint64 (the product wraps modulo 2^64)."""
    key = (ka.astype(np.uint64) << np.uint64(32)) | kb.astype(np.uint64)
    with np.errstate(over="ignore"):
        return (key * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - log2c)


def test_keys_that_collide_at_the_end_of_the_table_wrap_around():
    ka, kb = (x.reshape(-1) for x in np.indices((200, 200)) + 1)
    at_end = np.flatnonzero(home_slots(ka, kb, 7) >= 126)[:48]                      # max_pairs = 64: C = 128
    assert at_end.shape[0] == 48 >= 40
    la, lb = np.zeros((1, 4, 16), np.int32), np.zeros((1, 4, 16), np.int32)
    la.reshape(-1)[:48], lb.reshape(-1)[:48] = ka[at_end], kb[at_end]               # one point each
    want = host(la, lb, 256, 256, 64)
    assert want[1][0] == 48
    assert_same(device(la, lb, 256, 256, 64), want)
    assert_same(device(la, lb, 256, 256, 48), host(la, lb, 256, 256, 48))
    over = device(la, lb, 256, 256, 47)
    assert over[1][0] == -1 and not over[0].any()


@pytest.mark.parametrize("max_pairs", (640, 639, 256))
def test_stripes_fit_exactly_and_overflow_writes_nothing_past_the_table(max_pairs):
    la, lb = (x[None] for x in stripes())
    want = host(la, lb, 64, 64, max_pairs)
    size = max_pairs * 4
    buffer = torch.full((size + 64,), -77, dtype=torch.int64, device=DEV)
    count = torch.full((1 + 16,), -77, dtype=torch.int32, device=DEV)
    out = (buffer[:size].view(1, max_pairs, 4), count[:1])
    assert_same(device(la, lb, 64, 64, max_pairs, out=out), want)
    assert (buffer[size:] == -77).all() and (count[1:] == -77).all()
    if max_pairs == 640:
        assert want[1][0] == 640 and (want[0][0, :, 2] == 4).all()
    else:                                                                           # 639: too many keys; 256: C = 512 < 640, the hash fills up
        assert want[1][0] == -1 and int(count[0]) == -1 and not buffer[:size].any()


@pytest.mark.parametrize("shape", [(40, 257), (721, 1440)])
def test_one_pair_that_covers_the_plane(shape):
    la, lb = np.full((1, *shape), 3, np.int32), np.full((1, *shape), 2, np.int32)
    pairs, count = device(la, lb)
    assert count[0] == 1 and pairs[0, 0].tolist() == [3, 2, shape[0] * shape[1], int(unit_of(shape[0]).sum()) * shape[1]]
    assert not pairs[0, 1:].any()
    assert_same((pairs, count), host(la, lb))


def test_a_quarter_degree_plane_against_itself_shifted():
    plane = red_noise((1, 721, 1440), seed=11)
    thr = {"x": np.quantile(plane, [0.5, 0.9, 0.99]).astype(np.float32).tolist()}
    a = objects(batch_of(plane).to(DEV), thr, wrap=True)
    b = objects(batch_of(np.roll(plane, 5, axis=-1)).to(DEV), thr, wrap=True)
    on_device = object_matches(a, b, max_pairs=8192)
    on_host = object_matches(a.cpu(), b.cpu(), max_pairs=8192)                      # the numpy path on the same label maps
    print("objects:", a.count_table.tolist(), b.count_table.tolist(), "pairs:", on_host.count_table.tolist())
    assert int(on_host.count_table.max()) > 0
    same_matches(on_device, on_host)
    small = object_matches(a, b, max_pairs=2)                                       # C = 64 against many more keys
    same_matches(small, object_matches(a.cpu(), b.cpu(), max_pairs=2))


def test_independence_of_the_other_items():
    la, lb = maps(40, 130, n=7, T=1)
    alone, among, last = device(la[6:], lb[6:]), device(la[4:], lb[4:]), device(la, lb)
    for x, y, z in zip(alone, among, last):
        assert x[0].tobytes() == y[2].tobytes() == z[6].tobytes()


def test_two_calls_give_identical_bytes():
    la, lb = maps(40, 257, n=3)
    first, second = device(la, lb), device(la, lb)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()


def test_a_small_workspace_is_refused_and_nothing_is_written():
    la, lb = maps(40, 64)
    out = (torch.full((2, 2, 64, 4), -7, dtype=torch.int64, device=DEV), torch.full((2, 2), -7, dtype=torch.int32, device=DEV))
    need = lib.object_matches_workspace_bytes(4, 64)
    assert need == 4 * (3 * 128 + 1) * 8
    with pytest.raises(ValueError, match="workspace"):
        device(la, lb, out=out, workspace=torch.empty(need - 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="max_pairs"):
        device(la, lb, max_pairs=8193, out=(torch.full((2, 2, 8193, 4), -7, dtype=torch.int64, device=DEV), out[1]))
    with pytest.raises(AssertionError, match="pairs must be a contiguous"):
        device(la, lb, out=(out[0][:, :, :32], out[1]))
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out)
    device(la, lb, out=out, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
    assert_same(tuple(t.cpu().numpy() for t in out), host(la, lb))


def test_capture_in_a_hip_graph():
    la, lb = maps(33, 70, n=3)
    other_a, other_b = maps(33, 70, n=3, seed=9)
    da, db, unit = carve(la), carve(lb), torch.from_numpy(unit_of(33)).to(DEV)      # uploaded beforehand
    out = (torch.empty((3, 2, 64, 4), dtype=torch.int64, device=DEV), torch.empty((3, 2), dtype=torch.int32, device=DEV))
    ws = torch.empty(lib.object_matches_workspace_bytes(6, 64), dtype=torch.uint8, device=DEV)
    lib.object_pairs(da, db, unit, 8, 8, 64, out=out, workspace=ws)                 # the warm call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.object_pairs(da, db, unit, 8, 8, 64, out=out, workspace=ws)
    da.copy_(torch.from_numpy(other_a))
    db.copy_(torch.from_numpy(other_b))
    for t in out:
        t.fill_(-5)
    graph.replay()
    torch.cuda.synchronize()
    replayed = tuple(t.cpu().numpy() for t in out)
    assert_same(replayed, device(other_a, other_b))
    assert_same(replayed, host(other_a, other_b))
