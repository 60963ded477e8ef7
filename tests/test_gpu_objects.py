"""aurora_hip_objects (aurora_amd/csrc/objects.hip) against the CPU path of aurora_amd.objects, which tests/test_objects_host.py
pins to a flood fill: labels, count and table are equal bit for bit (THE RULE: aurora_amd/objects.py)."""
import functools
import importlib

import numpy as np
import pytest
import torch

from aurora_amd import Batch, diagnostics, objects
from aurora_amd import _fields
from aurora_amd.engine import lib
from tests.test_objects_host import lat_of, patterns
from tests.verification_inputs import DEV, carve, red_noise, red_noise_batch, thresholds_of

pytestmark = pytest.mark.gpu
mod = importlib.import_module("aurora_amd.objects")


def host(planes: np.ndarray, thr: np.ndarray, below=False, connectivity=8, wrap=False, max_objects=64):
    """The CPU path on (n, H, W) planes and (n, T) thresholds."""
    return mod._objects_host(planes, np.asarray(thr, dtype=np.float32), mod.area_units(lat_of(planes.shape[1])), below, connectivity,
                             wrap, max_objects)


def device(planes, thr, below=False, connectivity=8, wrap=False, max_objects=64, offset=0, **kw):
    """lib.object_labels on device copies of the same planes (a list of tensors or one array), as host arrays."""
    fields = planes if isinstance(planes, list) else [carve(np.array(planes), offset, fill=np.nan)]
    n_lat = fields[0].shape[-2]
    unit = torch.from_numpy(mod.area_units(lat_of(n_lat))).to(DEV)
    out = lib.object_labels(fields, torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float32)).to(DEV), unit, below, connectivity,
                            wrap, max_objects, **kw)
    return tuple(t.cpu().numpy() for t in out)


def assert_same(got, want):
    for g, w, what in zip(got, want, ("labels", "count", "table")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what


@functools.lru_cache(maxsize=None)
def noise(H, W, n=2, seed=1):
    planes = red_noise((n, H, W), seed=seed + 7 * H + W)
    planes.setflags(write=False)
    return planes


# ---- the smallest cases first ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(patterns()))
def test_patterns_equal_the_cpu_path(name):
    plane = patterns()[name][None]
    thr = np.array([[0.5, np.nan]], dtype=np.float32)
    for connectivity in (4, 8):
        for wrap in (False, True):
            for below in ((False, True) if name in ("ties", "special") else (False,)):
                kw = dict(below=below, connectivity=connectivity, wrap=wrap)
                assert_same(device(plane, thr, **kw), host(plane, thr, **kw))


@pytest.mark.parametrize("W", (1, 2, 63, 64, 65, 130, 257))
@pytest.mark.parametrize("H", (1, 2, 40))
def test_widths_and_heights(H, W):
    planes = noise(H, W)
    thr = thresholds_of(planes, 5)
    for connectivity, wrap in ((8, True), (4, False)):
        assert_same(device(planes, thr, connectivity=connectivity, wrap=wrap), host(planes, thr, connectivity=connectivity, wrap=wrap))
    # long runs that are open at every chunk boundary, and a full row
    wide = np.ones((1, H, W), dtype=np.float32)
    wide[0, :, W // 2] = 0
    wide[0, -1] = 1
    assert_same(device(wide, [[0.5]], wrap=True), host(wide, [[0.5]], wrap=True))


@pytest.mark.parametrize("offset", (0, 1, 3))
def test_alignment_does_not_matter(offset):
    planes = noise(40, 64)
    thr = thresholds_of(planes, 5)
    assert_same(device(planes, thr, wrap=True, offset=offset), host(planes, thr, wrap=True))


@pytest.mark.parametrize("T", (1, 5, 8))
def test_threshold_counts(T):
    planes = noise(33, 70, n=3)
    thr = thresholds_of(planes, 8)[:, :1] if T == 1 else thresholds_of(planes, T)
    assert_same(device(planes, thr, wrap=True), host(planes, thr, wrap=True))
    assert_same(device(planes, thr, below=True, connectivity=4), host(planes, thr, below=True, connectivity=4))


def test_a_quarter_degree_plane():
    plane = red_noise((1, 721, 1440), seed=11)
    thr = thresholds_of(plane, 4)[:, :3]                                            # the 0.5 / 0.9 / 0.99 quantiles
    got, want = device(plane, thr, wrap=True, max_objects=4096), host(plane, thr, wrap=True, max_objects=4096)
    print("objects per threshold:", want[1].tolist())
    assert_same(got, want)


def test_independence_of_the_other_planes():
    planes = noise(40, 130, n=7)
    thr = thresholds_of(planes, 5)
    alone = device(planes[6:], thr[6:], wrap=True)
    among = device(planes[4:], thr[4:], wrap=True)
    last = device(planes, thr, wrap=True)
    for a, b, c in zip(alone, among, last):
        assert a[0].tobytes() == b[2].tobytes() == c[6].tobytes()


def test_two_calls_give_identical_bytes():
    planes = noise(40, 257, n=3)
    thr = thresholds_of(planes, 5)
    first, second = device(planes, thr, wrap=True), device(planes, thr, wrap=True)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


def test_max_objects_below_the_count_writes_nothing_past_the_table():
    planes = noise(40, 130)
    thr = thresholds_of(planes, 5)
    want = host(planes, thr, wrap=True, max_objects=3)
    assert (want[1] > 3).any()
    n, T = thr.shape
    size = n * T * 3 * 10
    buffer = torch.full((size + 64,), -77, dtype=torch.int64, device=DEV)
    out = (torch.empty((n, T, 40, 130), dtype=torch.int32, device=DEV), torch.empty((n, T), dtype=torch.int32, device=DEV),
           buffer[:size].view(n, T, 3, 10))
    assert_same(device(planes, thr, wrap=True, max_objects=3, out=out), want)
    assert (buffer[size:] == -77).all()
    assert np.array_equal(out[1].cpu().numpy() > 3, want[1] > 3)                    # truncated


def test_a_small_workspace_is_refused_and_nothing_is_written():
    planes = noise(40, 64)
    thr = thresholds_of(planes, 5)
    n, T = thr.shape
    out = (torch.full((n, T, 40, 64), -7, dtype=torch.int32, device=DEV), torch.full((n, T), -7, dtype=torch.int32, device=DEV),
           torch.full((n, T, 8, 10), -7, dtype=torch.int64, device=DEV))
    need = lib.objects_workspace_bytes(n, 40, 64, T)
    assert need == (n * T * (40 * 64 + 40) * 4 + 7) // 8 * 8
    with pytest.raises(ValueError, match="workspace"):
        device(planes, thr, max_objects=8, out=out, workspace=torch.empty(need - 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="connectivity"):
        device(planes, thr, max_objects=8, out=out, connectivity=5)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out)
    device(planes, thr, max_objects=8, out=out, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
    assert_same(tuple(t.cpu().numpy() for t in out), host(planes, thr, max_objects=8))


# ---- the front end ---------------------------------------------------------------------------------------------------------------
def same_objects(a, b):
    """Every table and every finalised property of two results (finalised where each lives), NaN equal to NaN."""
    same = lambda x, y: x.dtype == y.dtype and torch.equal(x.isnan(), y.isnan()) and torch.equal(x.nan_to_num(), y.nan_to_num())  # noqa: E731
    for what in ("labels", "count", "table", "truncated", "points", "area", "centroid_row", "centroid_col", "centroid_lat",
                 "centroid_lon", "peak", "peak_row", "peak_col", "peak_lat", "peak_lon", "bbox"):
        x, y = ({k: v.cpu().double() if v.dtype == torch.bool else v.cpu() for k, v in getattr(r, what).items()} for r in (a, b))
        assert x.keys() == y.keys()
        for k in x:
            assert same(x[k], y[k]), (what, k)


def test_capture_in_a_hip_graph():
    b = red_noise_batch(33, 70, seed=2, B=1).to(DEV)
    other = red_noise_batch(33, 70, seed=3, B=1)
    thr = {"2t": [float(np.quantile(b.surf_vars["2t"].cpu().numpy(), 0.8))], "z": [5e4, 5.02e4]}
    objects(b, thr, max_objects=32)                                                # the warm call: tables are uploaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = objects(b, thr, max_objects=32)
    for k in ("2t", "msl"):
        b.surf_vars[k].copy_(other.surf_vars[k])
    b.atmos_vars["z"].copy_(other.atmos_vars["z"])
    graph.replay()
    torch.cuda.synchronize()
    same_objects(o, objects(other, thr, max_objects=32))
    with pytest.MonkeyPatch.context() as mp:                                       # a cold call during capture is refused
        mp.setattr(mod._fields, "tables", _fields.DeviceTables(capturing=lambda: True))
        with pytest.raises(RuntimeError, match="objects: call once .* before capturing a graph"):
            objects(b, thr, max_objects=32)


def test_end_to_end_on_derived_fields():
    g = torch.Generator().manual_seed(4)
    base = red_noise_batch(33, 70, seed=5, B=2, levels=(300, 500, 700, 850))
    field = lambda *s, scale=1.0, off=0.0: (off + scale * torch.randn(*s, 33, 70, generator=g)).float()  # noqa: E731
    q = (0.004 * torch.rand(2, 2, 4, 33, 70, generator=g)).float()
    pred = Batch({"10u": field(2, 2, scale=9), "10v": field(2, 2, scale=9)}, {},
                 {"u": field(2, 2, 4, scale=15, off=8), "v": field(2, 2, 4, scale=15), "q": q}, base.metadata)
    thr = {"ivt": [250.0, 500.0], "10ws": [15.0]}
    on_host = objects(diagnostics(pred, ("ivt", "10ws")), thr)
    on_device = objects(diagnostics(pred.to(DEV), ("ivt", "10ws")), thr)
    assert on_device.labels["ivt"].device.type == "cuda" and int(on_host.count_table.sum()) > 0
    same_objects(on_device, on_host)
    assert torch.equal(on_device.cpu().table["ivt"], on_host.table["ivt"])
