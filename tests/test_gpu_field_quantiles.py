"""aurora_hip_field_quantiles (aurora_amd/csrc/field_quantiles.hip) against the CPU path of aurora_amd.field_quantiles, which
tests/test_field_quantiles_host.py pins to numpy and to a plain-Python inverted CDF: values, valid and total are equal bit for
bit in both kinds (THE RULE: aurora_amd/field_quantiles.py)."""
import functools
import importlib

import numpy as np
import pytest
import torch

from aurora_amd import _fields, field_quantiles
from aurora_amd.engine import lib
from aurora_amd.objects import area_units
from tests.test_field_quantiles_host import Q3, Q8, cases, lat_of
from tests.verification_inputs import DEV, carve, red_noise, red_noise_batch

pytestmark = pytest.mark.gpu
mod = importlib.import_module("aurora_amd.field_quantiles")
KINDS = ("area", "count")


def unit_of(n_lat, kind):
    return area_units(lat_of(n_lat)) if kind == "area" else None


def host(planes: np.ndarray, q, kind):
    """The CPU path on (n, H, W) planes."""
    return mod._quantiles_host(planes, q, unit_of(planes.shape[1], kind))


def device(planes, q, kind, offset=0, **kw):
    """lib.field_quantile_values on device copies of the same planes (a list of tensors or one array), as host arrays."""
    fields = planes if isinstance(planes, list) else [carve(np.array(planes), offset, fill=np.nan)]
    unit = unit_of(fields[0].shape[-2], kind)
    out = lib.field_quantile_values(fields, q, None if unit is None else torch.from_numpy(unit).to(DEV), **kw)
    return tuple(t.cpu().numpy() for t in out)


def assert_same(got, want):
    for g, w, what in zip(got, want, ("values", "valid", "total")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, g, w)


def check(planes, q=Q3, **kw):
    for kind in KINDS:
        assert_same(device(planes, q, kind, **kw), host(planes, q, kind))


@functools.lru_cache(maxsize=None)
def noise(H, W, n=2, seed=1):
    planes = red_noise((n, H, W), seed=seed + 7 * H + W)
    planes.setflags(write=False)
    return planes


def from_keys(keys: np.ndarray) -> np.ndarray:
    """The float32 values whose keys K are `keys` (uint32): the inverse of `objects.value_keys`."""
    k = keys.astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


# ---- the smallest cases first ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases()))
def test_cases_equal_the_cpu_path(name):
    plane = cases()[name][None]
    for q in (Q3, Q8, (0.5,), (0.0, 1.0)):
        check(plane, q)


@pytest.mark.parametrize("W", (1, 2, 3, 4, 63, 64, 65, 257))
@pytest.mark.parametrize("H", (1, 2, 40))
def test_widths_and_heights(H, W):
    planes = noise(H, W).copy()
    planes[1].reshape(-1)[::5] = np.nan
    check(planes)
    check(planes, Q8)


@pytest.mark.parametrize("byte", (0, 1, 2, 3))
def test_one_byte_of_the_key_discriminates(byte):
    """Keys that differ in byte `byte` alone (0: the top one): that pass is the only one that tells the points apart."""
    g = np.random.default_rng(byte)
    base = np.uint32(0xc2a5f03c) & ~np.uint32(0xff << (24 - 8 * byte))      # (finite whatever a lower byte holds)
    for spread in (256, 3):
        digits = g.integers(0, spread, (2, 33, 70)).astype(np.uint32) * np.uint32(256 // spread)
        if byte == 0:                                                       # the top bytes 0x40 .. 0xbf: finite, both signs
            digits = np.uint32(0x40) + digits % np.uint32(0x80)
        planes = from_keys(base | (digits << np.uint32(24 - 8 * byte)))
        assert np.isfinite(planes).all()
        check(planes)
        check(planes, Q8)


def test_every_byte_position_at_once():
    g = np.random.default_rng(9)
    keys = np.uint32(0xc2000000) + (g.integers(0, 4, (2, 33, 70)).astype(np.uint32) * np.uint32(0x00400000)) \
        + (g.integers(0, 256, (2, 33, 70)).astype(np.uint32) << np.uint32(8)) + g.integers(0, 2, (2, 33, 70)).astype(np.uint32)
    check(from_keys(keys), Q8)


def test_halves_and_a_constant_plane():
    halves = np.ones((1, 40, 130), dtype=np.float32)                      # j and hi of q = 0.5 are in different pass-0 bins
    halves[0, :, ::2] = -1.0
    check(halves, (0.5,))
    check(halves, Q8)
    check(np.full((2, 40, 257), 273.15, dtype=np.float32), Q8)            # one bin, full contention, in every pass
    zeros = np.zeros((1, 40, 65), dtype=np.float32)
    zeros[0, ::2] = -0.0
    check(zeros, (0.0, 0.49, 0.5, 0.51, 1.0))


def test_invalid_points():
    planes = noise(40, 65, n=3).copy()
    planes[0] = np.nan                                                     # all NaN
    planes[1] = np.nan
    planes[1, 17, 33] = 5e4                                                # one valid point
    g = np.random.default_rng(2)
    scattered = planes[2].reshape(-1)
    scattered[g.integers(0, scattered.size, 300)] = np.nan
    scattered[g.integers(0, scattered.size, 100)] = np.inf
    scattered[g.integers(0, scattered.size, 100)] = -np.inf
    for q in (Q3, (0.0, 1.0), (0.5,)):
        check(planes, q)
    poles = noise(40, 64).copy()                                           # every valid point on a pole row: W = 0
    poles[:, 1:-1] = np.nan
    got = device(poles, Q3, "area")
    assert np.isnan(got[0]).all() and got[1].tolist() == [128, 128] and got[2].tolist() == [0, 0]
    check(poles)


def test_ties_across_the_target():
    plane = np.full((1, 40, 63), 2.0, dtype=np.float32)
    plane[0, :3], plane[0, -3:] = 1.0, 3.0
    check(plane, Q8)
    check(plane, (0.07, 0.08, 0.92, 0.93))


@pytest.mark.parametrize("Q", (1, 8))
def test_numbers_of_q(Q):
    q = Q8[:Q]
    check(noise(33, 70, n=3), q)


@pytest.mark.parametrize("offset", (1, 3))
def test_alignment_does_not_matter(offset):
    planes = noise(40, 64)
    for kind in KINDS:
        aligned, shifted = device(planes, Q3, kind), device(planes, Q3, kind, offset=offset)
        assert_same(shifted, aligned)
        assert_same(shifted, host(planes, Q3, kind))


def test_independence_of_the_other_planes():
    planes = noise(40, 130, n=7)
    for kind in KINDS:
        alone, among, last = device(planes[6:], Q3, kind), device(planes[4:], Q3, kind), device(planes, Q3, kind)
        for a, b, c in zip(alone, among, last):
            assert a[0].tobytes() == b[2].tobytes() == c[6].tobytes()


def test_two_calls_give_identical_bytes():
    planes = noise(40, 257, n=3)
    for kind in KINDS:
        first, second = device(planes, Q8, kind), device(planes, Q8, kind)
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()


def test_a_quarter_degree_plane():
    plane = red_noise((1, 721, 1440), seed=11)
    for kind in KINDS:
        got, want = device(plane, Q3, kind), host(plane, Q3, kind)
        print(kind, want[0].tolist(), want[1].tolist(), want[2].tolist())
        assert_same(got, want)


def test_a_small_workspace_is_refused_and_nothing_is_written():
    planes = noise(40, 64)
    need = lib.field_quantiles_workspace_bytes(2, 3)
    out = (torch.full((2, 3), -7.0, dtype=torch.float32, device=DEV), torch.full((2,), -7, dtype=torch.int64, device=DEV),
           torch.full((2,), -7, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="workspace"):
        device(planes, Q3, "area", out=out, workspace=torch.empty(need - 8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="not in"):
        device(planes, (0.5, 1.5, 0.1), "area", out=out)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out)
    guard = torch.full((need + 512,), 0x5a, dtype=torch.uint8, device=DEV)     # nothing is written past the workspace
    device(planes, Q3, "area", out=out, workspace=guard[:need])
    assert_same(tuple(t.cpu().numpy() for t in out), host(planes, Q3, "area"))
    assert bool((guard[need:] == 0x5a).all())


# ---- the front end ---------------------------------------------------------------------------------------------------------------
def same_quantiles(a, b):
    for what in ("value", "valid", "total"):
        x, y = getattr(a.cpu(), what), getattr(b.cpu(), what)
        assert x.keys() == y.keys()
        for k in x:
            assert x[k].dtype == y[k].dtype and x[k].numpy().tobytes() == y[k].numpy().tobytes(), (what, k)


def test_the_front_end_equals_the_cpu_front_end():
    b = red_noise_batch(33, 70, seed=2, B=2)
    for kind in KINDS:
        on_device, on_host = field_quantiles(b.to(DEV), Q3, kind=kind), field_quantiles(b, Q3, kind=kind)
        assert on_device.value["z"].device.type == "cuda" and on_device.value["z"].shape == (2, 3, 3)
        same_quantiles(on_device, on_host)
        for name, t in on_device.thresholds(1).items():
            assert np.array_equal(t, on_host.thresholds(1)[name])
    with pytest.raises(TypeError, match="field_quantiles: batch variable '2t' is torch.float64; the device path takes float32"):
        field_quantiles(red_noise_batch(9, 12, dtype=torch.float64).to(DEV))


def test_capture_in_a_hip_graph():
    b = red_noise_batch(33, 70, seed=2, B=1).to(DEV)
    other = red_noise_batch(33, 70, seed=3, B=1)
    for kind in KINDS:
        field_quantiles(b, Q3, kind=kind)                                          # the warm call: tables are uploaded
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fq = field_quantiles(b, Q3, kind=kind)
        kept = {k: v.clone() for k, v in {**b.surf_vars, **b.atmos_vars}.items()}
        for k in ("2t", "msl"):
            b.surf_vars[k].copy_(other.surf_vars[k])
        b.atmos_vars["z"].copy_(other.atmos_vars["z"])
        graph.replay()
        torch.cuda.synchronize()
        same_quantiles(fq, field_quantiles(other, Q3, kind=kind))
        for k, v in kept.items():
            (b.surf_vars if k in b.surf_vars else b.atmos_vars)[k].copy_(v)
    with pytest.MonkeyPatch.context() as mp:                                       # a cold call during capture is refused
        mp.setattr(mod._fields, "tables", _fields.DeviceTables(capturing=lambda: True))
        with pytest.raises(RuntimeError, match="field_quantiles: call once .* before capturing a graph"):
            field_quantiles(b, Q3)
